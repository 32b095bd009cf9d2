// What the entries that run stored weight sets over a resident table share (npbnn_capi.hip: npbnn_predict_sets; npbnn_importance.hip:
// npbnn_predict_sets_summary; npbnn_support.hip; npbnn_lppd.hip; npbnn_uncertainty.hip; npbnn_calibration.hip; npbnn_pdp.hip, route 2;
// and through npbnn_stack.hip.h npbnn_hpd.hip, npbnn_convergence.hip, npbnn_predictive.hip):
// the replay of the sets group after group (replay_sets, npbnn_sets.hip) and the host helpers it is built from, the flag word's bits,
// the launch shape of the streaming kernels, the HIP-event timer behind NPBNN_FI_TIMING, the fixed-order workgroup sum and the host
// tail that adds its partials, and the host scaffold of an entry: open_sets_table (the checks before the device is touched; every
// entry but npbnn_predict_sets), finish_sets_entry (the tail of the five entries that end in a final kernel and a flag word),
// check_sigma_sets and PointOuts (npbnn_lppd.hip, npbnn_uncertainty.hip, npbnn_calibration.hip).  The device code those three fold
// with - the softmax fold, softplus, the label check - is in npbnn_fold.hip.h, which has a rule on contraction of its own; the kStack*
// limits, the tile and the stack of the column kernels are in npbnn_stack.hip.h.  Nothing here belongs to a single entry.  Not part of the ABI.
#pragma once
#include "npbnn_ctx.hip.h"

#include <climits>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

namespace npbnn_api {

constexpr int kFiThreads = 256;
constexpr int kFiWaves = kFiThreads / 64;
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

// ---- device helpers (this header is compiled under each unit's default fp contraction, whatever pragma follows the include: only
// helpers with no product feeding a sum live here)

// The sum of v over a workgroup of kFiThreads threads in a fixed order: lanes by shuffles, then the waves in wave order through
// lds [kFiWaves].  Every thread of the workgroup calls it; thread 0 returns the sum.
__device__ inline double block_sum(double v, double* lds) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                 // (lds may still be read from the previous call)
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    double s = lds[0];
    for (int w = 1; w < kFiWaves; ++w) s += lds[w];
    return s;
}

// the maximum of a row of C float32 values, widened; nan: one of them is NaN.  VEC: C is a multiple of 4, the row is read as float4.
template <bool VEC>
__device__ inline double row_max(const float* __restrict__ row, int C, bool& nan) {
    double mx = -INFINITY;
    if (VEC) {
        for (int k = 0; k < C; k += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + k);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                nan = nan || (v[q] != v[q]);
                mx = fmax(mx, (double)v[q]);
            }
        }
    } else {
        for (int k = 0; k < C; ++k) {
            const float v = row[k];
            nan = nan || (v != v);
            mx = fmax(mx, (double)v);
        }
    }
    return mx;
}

// ---- host helpers of a replay (npbnn_sets.hip)

// room for n elements, and for one vector access when n is 0
template <class T>
int dev_alloc(npbnn_ctx* ctx, DevBuf<T>& b, size_t n) {
    return b.reserve(ctx, n ? n : 16 / sizeof(T));
}

// How many of the sets s0, s0 + 1, ... share set s0's activation slopes [n_sets][n_act] (all of them when there are none), cap at most:
// they travel together in one streaming read of X.
int slope_group_len(const double* act_prm_sets, int n_act, int s0, int n_sets, int cap);

// set s0's slopes (zeros when there are none) into ctx->net.act_prm
void load_group_slopes(npbnn_ctx* ctx, const double* act_prm_sets, int n_act, int s0);

// make_params turned into a prediction pass of packed weight images: no labels or targets, no likelihood, float32 values into y_out -
// pre-output ones unless apply_out_fn
EvalParams predict_params(npbnn_ctx* ctx, const Dataset& d, float* y_out, int apply_out_fn);

// The sets s0 .. s0 + g - 1 and their float32 predictions y [g][n_rows][C] on the device; the pass that wrote them is complete.
struct SetGroup {
    int s0, g;
    const float* y;
};
// What an entry does with a group: returns an NPBNN_* code; may enqueue on ctx->stream.
using SetSink = std::function<int(const SetGroup&)>;

// The n_sets weight sets against the resident matrix `which`, group after group: sets that share their slopes travel together, up to
// kMaxCand per streaming read of X and as many as the launch plan carries (weight-streamed path: up to kWideMaxCand where the pass is
// the fused one, else one), and a group whose layer-0 weights leave the fp16 range repeats on the float32 path - on the
// weight-streamed path only the set that left it, alone; the sets before it are delivered as computed and a fresh group follows it.  Without y_stack every group writes to ctx->d_y, so `sink` has to be
// through with (or have enqueued its reads of) the values when it returns; with y_stack, [n_sets][n_rows][C] on the device, group s0
// writes to its place in it.  `sink` (may be empty) runs once per group, after the group's pass has succeeded: never for an attempt
// that is retried.  `who` names the entry in error messages.  Leaves the time of the passes (weight packing included) and of the sinks
// in ctx->fi_ns[1], [2] (NPBNN_FI_TIMING), and the passes it launched and the most sets one carried in ctx->replay_passes, replay_max_group.
int replay_sets(npbnn_ctx* ctx, const char* who, const double* W_sets, const double* act_prm_sets, int n_sets, int which, int apply_out_fn,
                float* y_stack, const SetSink& sink);

// A group's predictions y [g][n_rows][C] folded into d_acc [n_rows][C]: mode 0 uint32 votes (d_acc read as unsigned), mode 1 float64
// sums in set order.  d_acc and the flag word are zeroed by the caller in stream order; kFlagNaN is raised there.  Defined next to its
// kernels in npbnn_importance.hip.
void launch_summary_accumulate(hipStream_t st, const float* y, int g, long long n_rows, int C, int mode, double* d_acc, int* d_flag);

// The end of an entry on ctx->stream: the flag word into *flags and the partials d_part [n_q][n_wg] back, the stream
// synchronised, and each quantity's partials added in workgroup order into (*totals)[n_q].
int fetch_flags_and_totals(npbnn_ctx* ctx, const int* d_flag, const double* d_part, size_t n_q, int n_wg, int* flags, std::vector<double>* totals);

// ---- the scaffold of an entry over stored sets: plain functions and one struct, called in sequence by the entry

// The resident table an entry runs over, and the launch shape of its streaming kernels.
struct SetsTable {
    Dataset* d = nullptr;
    long long n_rows = 0;
    hipStream_t st = nullptr;
    int n_wg = 0;                      // grid_for(n_rows)
};
// The checks every entry makes before it touches the device - `which` is 0 or 1, npbnn_set_arch was called, the table is there
// (check_dataset_for_lik with NPBNN_LIK_NONE) - then hipSetDevice, and *t filled.  Launches nothing.
int open_sets_table(npbnn_ctx* ctx, const char* who, int which, SetsTable* t);

// NPBNN_E_ARG unless every entry of sigma_sets [n_sets][T] is positive and finite
int check_sigma_sets(npbnn_ctx* ctx, const char* who, const double* sigma_sets, int n_sets, int T);

// The per-row outputs of an entry that the caller may leave out: one device buffer, a slice per output that is wanted.
struct PointOuts {
    struct Slot { double* host; size_t off, len; bool on; };
    // registers an output of n values (four at most) and returns its slot; always: the kernels write it whether the caller takes it or not
    int add(double* host_out, size_t n, bool always = false) {
        s[count] = Slot{host_out, total, n, host_out || always};
        if (s[count].on) total += n;
        return count++;
    }
    int reserve(npbnn_ctx* ctx) { return buf.reserve(ctx, total); }
    // the slot's place on the device, or nullptr when it has none
    double* dev(int i) const { return s[i].on ? buf.get() + s[i].off : nullptr; }
    // enqueues the copies of the outputs the caller gave
    int copy_out(npbnn_ctx* ctx, hipStream_t st) const;

    Slot s[4] = {};
    size_t total = 0;
    int count = 0;
    DevBuf<double> buf;
};

// The tail of an entry whose final kernel has been enqueued, in this order: hipGetLastError, tm.mark(1), fetch_flags_and_totals
// (d_part [n_q][n_wg] into (*totals)[n_q]; n_q may be 0), the time between the marks 0 and 1 into *ns_slot, the refusal of a NaN
// prediction, and with n_classes > 0 that of a label outside [0, n_classes).  The time is stored before the refusals.
int finish_sets_entry(npbnn_ctx* ctx, const char* who, FiTimer& tm, const int* d_flag, const double* d_part, size_t n_q, int n_wg, int* ns_slot,
                      int n_classes, std::vector<double>* totals);

}  // namespace npbnn_api
