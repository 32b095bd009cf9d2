// What the entries that summarise stored weight sets on the device share (npbnn_importance.hip: npbnn_predict_sets_summary;
// npbnn_support.hip: npbnn_predict_sets_support): the replay of the sets into an accumulator, the flag word's bits, the launch shape of
// the streaming kernels and the HIP-event timer behind NPBNN_FI_TIMING.  Not part of the ABI.
#pragma once
#include "npbnn_ctx.hip.h"

#include <climits>
#include <cstdlib>
#include <cstring>

namespace npbnn_api {

constexpr int kFiThreads = 256;
constexpr int kFiMaxBlocks = 2048;                 // memory-bound kernels: grid-stride beyond this many workgroups

constexpr int kFlagBadRow = 1;                     // permutation index outside [0, n_rows)
constexpr int kFlagNaN = 2;                        // a prediction is NaN
constexpr int kFlagBadLabel = 4;                   // a label outside [0, C)

inline unsigned grid_for(long long items) {
    long long b = (items + kFiThreads - 1) / kFiThreads;
    if (b < 1) b = 1;
    if (b > kFiMaxBlocks) b = kFiMaxBlocks;
    return (unsigned)b;
}

// HIP events around the parts of a call, when NPBNN_FI_TIMING is set (tools/time_feature_importance.py, tools/time_posterior_threshold.py)
struct FiTimer {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool on = false;
    FiTimer() {
        const char* e = getenv("NPBNN_FI_TIMING");
        on = e && *e && strcmp(e, "0") != 0;
        if (on)
            for (hipEvent_t& x : ev)
                if (hipEventCreate(&x) != hipSuccess) on = false;
    }
    FiTimer(const FiTimer&) = delete;
    FiTimer& operator=(const FiTimer&) = delete;
    ~FiTimer() {
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
    }
    void mark(int i, hipStream_t s) { if (on) (void)hipEventRecord(ev[i], s); }
    // nanoseconds between marks a and b (both reached: the stream was synchronised)
    int ns(int a, int b) {
        float ms = 0.f;
        if (!on || hipEventElapsedTime(&ms, ev[a], ev[b]) != hipSuccess) return 0;
        const double v = (double)ms * 1e6;
        return v > (double)INT_MAX ? INT_MAX : (int)v;
    }
};

// What replay_sets_accumulate folds a group's float32 values into
enum { kReplayVotes = 0, kReplaySums = 1, kReplayLppd = 2, kReplayUncertainty = 3 };

constexpr int kLppdAcc = 5;                        // float64 accumulators per row of kReplayLppd, each an array [n_rows]

// The extra pointers of kReplayLppd (npbnn_lppd.hip), all on the device.  The accumulator d_acc is [kLppdAcc][n_rows]: the running
// maximum m of the row's log-likelihoods, sum exp(ll - m), K (the row's ll under the first set), sum (ll - K), sum (ll - K)^2.
struct ReplayLppd {
    int lik_kind = 0;                 // NPBNN_LIK_CATEGORICAL or NPBNN_LIK_GAUSS
    const int* labels = nullptr;      // [n_rows] (categorical)
    const float* targets = nullptr;   // [n_rows][C] (Gaussian)
    const double* lconst = nullptr;   // [n_sets][C] -0.5 log(2 pi) - log(sigma) (Gaussian)
    const double* isigma = nullptr;   // [n_sets][C] 1 / sigma (Gaussian)
    double* part = nullptr;           // [n_sets][n_wg]: every workgroup's sum of its rows' ll under a set
    int n_wg = 0;                     // workgroups of the accumulate launch: grid_for(n_rows)
};

// What kReplayUncertainty (npbnn_uncertainty.hip) needs beside the accumulator d_acc, which is [C + 1][n_rows] for the softmax output (sum of
// the sets' probabilities per class, then the sum of their entropies) and [3 or 4][T][n_rows] for regression (K = the first set's mean,
// sum (mu - K), sum (mu - K)^2, and under NPBNN_OUT_SOFTPLUS_HALF sum sigma^2).
struct ReplayUncertainty {
    int out_kind = 0;                 // NPBNN_OUT_SOFTMAX, NPBNN_OUT_IDENTITY or NPBNN_OUT_SOFTPLUS_HALF
    int n_wg = 0;                     // workgroups of the accumulate launch: grid_for(n_rows)
};

// The n_sets weight sets against the resident matrix `which`, group after group as npbnn_predict_sets replays them (sets that share
// their slopes travel together, the float32 retry), each group's float32 predictions folded into d_acc before the next group
// overwrites them: kReplayVotes uint32 votes [n_rows][C] (d_acc read as unsigned), kReplaySums float64 sums [n_rows][C], in set order;
// kReplayLppd (with `lppd`, and apply_out_fn 0: the values are the pre-output ones) the per-row log-likelihood accumulators above;
// kReplayUncertainty (with `unc`, apply_out_fn 0 likewise) the accumulators of the uncertainty decomposition above.  d_acc
// (n_rows x C doubles, kLppdAcc x n_rows, or as ReplayUncertainty says) and the flag word d_flag are the caller's, zeroed by it in stream order before the call;
// kFlagNaN (and kFlagBadLabel, kReplayLppd) is raised there.  `who` names the entry in error messages.  Leaves the pass and accumulation
// times in ctx->fi_ns[1], [2] (NPBNN_FI_TIMING).  Defined in npbnn_importance.hip.
int replay_sets_accumulate(npbnn_ctx* ctx, const char* who, const double* W_sets, const double* act_prm_sets, int n_sets, int which, int apply_out_fn,
                           int mode, double* d_acc, int* d_flag, const ReplayLppd* lppd = nullptr, const ReplayUncertainty* unc = nullptr);

// lppd_accumulate_kernel over a group's values y [g][n_rows][C], the sets s0 .. s0 + g - 1.  Defined in npbnn_lppd.hip.
void launch_lppd_accumulate(hipStream_t st, const float* y, int g, int s0, long long n_rows, int C, double* d_acc, const ReplayLppd& a, int* d_flag);

// The accumulate kernel of a.out_kind over a group's values y [g][n_rows][n_out], the sets s0 .. s0 + g - 1.  Defined in npbnn_uncertainty.hip.
void launch_uncertainty_accumulate(hipStream_t st, const float* y, int g, int s0, long long n_rows, int n_out, double* d_acc, const ReplayUncertainty& a,
                                   int* d_flag);

}  // namespace npbnn_api
