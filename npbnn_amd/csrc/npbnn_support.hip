// Confidence thresholds and Bayes-factor support on the device (include/npbnn_hip.h: npbnn_predict_sets_support): what
// get_posterior_threshold's sweep of 99 thresholds (np_bnn/BNN_lib.py:640-671, one get_accuracy_threshold with a cross-tabulation per
// threshold, :627-637), CalcTP / CalcFP / CalcTP_BF / CalcFP_BF (:305-337) and turn_low_pp_instances_to_nan (:674-679) ask of the summary
// over the stored samples, in one pass over the accumulator npbnn_predict_sets_summary's replay leaves in HBM
// (replay_sets with launch_summary_accumulate, npbnn_sets.hip.h: the two entries share both, so their quotients are the same bits).
//
// support_final_kernel, one thread per row as summary_final_kernel: q[k] = (double)acc[k] / n_sets, k* the first class holding the
// largest q, p = q[k*].  The row then counts once in cube[b][label][k*], b = the number of thresholds strictly below p (bisection
// over the caller's ascending float64 thresholds: `t < p` in float64, nothing recomputed), and - with prior summaries - once in
// bf_table[b'][k* == label], b' = the number of Bayes-factor thresholds strictly below (p / (1e-10 + 1 - p)) / (r / (1e-10 + 1 - r)),
// r = prior[row][k*], in CalcTP_BF's order of operations.  Every threshold's accuracy, retained share and confusion table are suffix sums
// of the cube over b.  Counts are integer atomics only: the tables do not depend on the order of arrival.
//
// LDS budget: kSupportLdsBytes = 52 KiB per 256-thread workgroup - 40 KiB of uint32 cube cells (10240: 99 thresholds + 1 bins x 10 x 10
// classes = 10000 fit), 4 KiB for up to 512 thresholds, 4 KiB for up to 512 Bayes-factor thresholds and 4 KiB + 8 B for their 513 x 2
// cells.  Three such workgroups fit a compute unit's 160 KiB: 12 waves per CU, each lane with its row's C loads in flight, which is
// what a kernel that reads n_rows x C accumulators once needs to keep HBM busy (summary_final_kernel runs at the same 256 threads and
// 16 KiB).  The launch asks only for what the call uses (dynamic LDS), so the usual case - 4 classes - takes 7 KiB and is bound by
// waves, not LDS.  A workgroup zeroes and flushes its cells once, so the grid is capped at three workgroups per CU when the cube is
// counted in LDS: one global 64-bit atomic per non-zero cell and workgroup.  A cube over the budget is counted by global atomics
// straight away; more than 512 thresholds are searched in global memory.
#include "npbnn_sets.hip.h"

#include <cmath>

namespace npbnn_api {

namespace {

constexpr int kSupportLdsCells = 10240;            // uint32 cube cells counted in LDS (40 KiB)
constexpr int kSupportLdsThresholds = 512;         // thresholds (and Bayes-factor thresholds) staged in LDS (4 KiB each)
constexpr int kSupportWgPerCu = 3;                 // workgroups of the full budget a compute unit's 160 KiB holds

// the number of entries of the ascending array t[0 .. n) strictly below v (0 for a NaN v)
__device__ inline int count_below(const double* t, int n, double v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct SupportArgs {
    long long n_rows;
    int C;
    double n_sets;
    const long long* labels;
    const double* thresholds;        // [n_thresholds] ascending
    int n_thresholds;
    const double* prior;             // [n_rows][C] or nullptr
    const double* bf_thresholds;     // [n_bf] ascending
    int n_bf;
    int has_cutoff;
    double cutoff;
    double* summary;                 // [n_rows][C] or nullptr
    unsigned char* keep;             // [n_rows] or nullptr
    unsigned long long* cube;        // [n_thresholds + 1][C][C]
    unsigned long long* bf_table;    // [n_bf + 1][2] or nullptr
    int lds_cube, lds_thr, lds_bf;   // count the cube / stage the thresholds / stage and count the Bayes-factor side in LDS
    int* flag;
};

template <class ACC>
__global__ __launch_bounds__(kFiThreads) void support_final_kernel(const ACC* __restrict__ acc, SupportArgs a) {
    extern __shared__ double lds_support[];
    // layout: [thresholds | bf thresholds | cube cells | bf cells], the doubles first (alignment)
    double* s_thr = lds_support;
    double* s_bft = s_thr + (a.lds_thr ? a.n_thresholds : 0);
    unsigned* s_cube = reinterpret_cast<unsigned*>(s_bft + (a.lds_bf ? a.n_bf : 0));
    const int C = a.C, cells = (a.n_thresholds + 1) * C * C, bf_cells = a.prior ? (a.n_bf + 1) * 2 : 0;
    unsigned* s_bf = s_cube + (a.lds_cube ? cells : 0);
    if (a.lds_thr)
        for (int i = threadIdx.x; i < a.n_thresholds; i += kFiThreads) s_thr[i] = a.thresholds[i];
    if (a.lds_bf) {
        for (int i = threadIdx.x; i < a.n_bf; i += kFiThreads) s_bft[i] = a.bf_thresholds[i];
        for (int i = threadIdx.x; i < bf_cells; i += kFiThreads) s_bf[i] = 0u;
    }
    if (a.lds_cube)
        for (int i = threadIdx.x; i < cells; i += kFiThreads) s_cube[i] = 0u;
    __syncthreads();
    const double* thr = a.lds_thr ? s_thr : a.thresholds;
    const double* bft = a.lds_bf ? s_bft : a.bf_thresholds;
    bool bad = false;
    for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < a.n_rows; r += (long long)gridDim.x * kFiThreads) {
        double best = 0.0;
        int bk = -1;
        for (int k = 0; k < C; ++k) {
            const double q = (double)acc[r * C + k] / a.n_sets;
            if (bk < 0 || q > best) { best = q; bk = k; }
        }
        const bool kept = !a.has_cutoff || best > a.cutoff;
        if (a.keep) a.keep[r] = kept ? 1 : 0;
        if (a.summary) {
            const double nan = __builtin_nan("");
            for (int k = 0; k < C; ++k) a.summary[r * C + k] = kept ? (double)acc[r * C + k] / a.n_sets : nan;
        }
        const long long lab = a.labels[r];
        if (lab < 0 || lab >= C) { bad = true; continue; }
        const int b = count_below(thr, a.n_thresholds, best);
        const int cell = (b * C + (int)lab) * C + bk;
        if (a.lds_cube) atomicAdd(&s_cube[cell], 1u);
        else atomicAdd(&a.cube[cell], 1ull);
        if (a.prior) {
            const double pr = a.prior[r * C + bk];
            const double bf = (best / (1e-10 + 1 - best)) / (pr / (1e-10 + 1 - pr));
            const int bcell = count_below(bft, a.n_bf, bf) * 2 + (bk == (int)lab ? 1 : 0);
            if (a.lds_bf) atomicAdd(&s_bf[bcell], 1u);
            else atomicAdd(&a.bf_table[bcell], 1ull);
        }
    }
    if (bad) atomicOr(a.flag, kFlagBadLabel);
    __syncthreads();
    if (a.lds_cube)
        for (int i = threadIdx.x; i < cells; i += kFiThreads) {
            const unsigned n = s_cube[i];
            if (n) atomicAdd(&a.cube[i], (unsigned long long)n);
        }
    if (a.lds_bf)
        for (int i = threadIdx.x; i < bf_cells; i += kFiThreads) {
            const unsigned n = s_bf[i];
            if (n) atomicAdd(&a.bf_table[i], (unsigned long long)n);
        }
}

// ascending (equal neighbours allowed) and free of NaN
bool ascending(const double* t, int n) {
    for (int i = 0; i < n; ++i)
        if (std::isnan(t[i]) || (i > 0 && t[i] < t[i - 1])) return false;
    return true;
}

}  // namespace

}  // namespace npbnn_api

using namespace npbnn_api;

extern "C" int npbnn_predict_sets_support(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which, int apply_out_fn,
                                          int mode, const int64_t* labels, const double* thresholds, int32_t n_thresholds, const double* prior_summary,
                                          const double* bf_thresholds, int32_t n_bf, const double* cutoff, int64_t* out_cube, int64_t* out_bf,
                                          double* out_summary, uint8_t* out_keep) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (!W_sets || n_sets < 1 || !labels || !out_cube || n_thresholds < 0 || (n_thresholds > 0 && !thresholds) || n_bf < 0)
        return fail(ctx, NPBNN_E_ARG, "predict_sets_support: bad arguments");
    if ((prior_summary != nullptr) != (out_bf != nullptr) || (!prior_summary && n_bf > 0) || (n_bf > 0 && !bf_thresholds))
        return fail(ctx, NPBNN_E_ARG, "predict_sets_support: prior_summary, bf_thresholds and out_bf go together");
    if (mode != 0 && mode != 1) return fail(ctx, NPBNN_E_ARG, "predict_sets_support: mode must be 0 (votes) or 1 (mean), got %d", mode);
    if (!ascending(thresholds, n_thresholds)) return fail(ctx, NPBNN_E_ARG, "predict_sets_support: the thresholds are not ascending (or one is NaN)");
    if (!ascending(bf_thresholds, n_bf)) return fail(ctx, NPBNN_E_ARG, "predict_sets_support: the Bayes-factor thresholds are not ascending (or one is NaN)");
    if (cutoff && std::isnan(*cutoff)) return fail(ctx, NPBNN_E_ARG, "predict_sets_support: the cutoff is NaN");
    SetsTable tb;
    int rc = open_sets_table(ctx, "predict_sets_support", which, &tb);
    if (rc) return rc;
    const int C = ctx->net.n_out;
    const long long n_rows = tb.n_rows;
    const size_t per_set = (size_t)n_rows * C;
    const long long cells_ll = (long long)(n_thresholds + 1) * C * C;
    if (cells_ll > (1ll << 28)) return fail(ctx, NPBNN_E_ARG, "predict_sets_support: %d thresholds x %d x %d classes is too large a table", n_thresholds, C, C);
    const size_t cells = (size_t)cells_ll, bf_cells = prior_summary ? (size_t)(n_bf + 1) * 2 : 0;
    hipStream_t st = tb.st;
    // accumulators, the summary, the keep mask, both tables, the labels, the thresholds [thresholds | bf thresholds], the prior, the flag word
    DevBuf<double> d_acc, d_summary, d_thr, d_prior;
    DevBuf<unsigned char> d_keep;
    DevBuf<unsigned long long> d_tables;
    DevBuf<long long> d_labels;
    DevBuf<int> d_flag;
    if ((rc = d_acc.reserve(ctx, per_set))) return rc;
    if ((rc = d_flag.reserve(ctx, 4))) return rc;
    if ((rc = d_tables.reserve(ctx, cells + bf_cells))) return rc;
    if ((rc = d_labels.reserve(ctx, (size_t)n_rows))) return rc;
    if ((rc = d_thr.reserve(ctx, (size_t)n_thresholds + (size_t)n_bf + 1))) return rc;
    if (out_summary && (rc = d_summary.reserve(ctx, per_set))) return rc;
    if (out_keep && (rc = d_keep.reserve(ctx, (size_t)n_rows))) return rc;
    if (prior_summary) {
        if ((rc = d_prior.reserve(ctx, per_set))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(d_prior, prior_summary, per_set * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_labels, labels, (size_t)n_rows * sizeof(long long), hipMemcpyHostToDevice, st));
    if (n_thresholds) HIP_TRY(ctx, hipMemcpyAsync(d_thr, thresholds, (size_t)n_thresholds * sizeof(double), hipMemcpyHostToDevice, st));
    if (n_bf) HIP_TRY(ctx, hipMemcpyAsync(d_thr.get() + n_thresholds, bf_thresholds, (size_t)n_bf * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(d_tables, 0, (cells + bf_cells) * sizeof(unsigned long long), st));
    HIP_TRY(ctx, hipMemsetAsync(d_acc, 0, per_set * sizeof(double), st));
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(int), st));
    rc = replay_sets(ctx, "predict_sets_support", W_sets, act_prm_sets, n_sets, which, apply_out_fn, nullptr, [&](const SetGroup& grp) {
        launch_summary_accumulate(st, grp.y, grp.g, n_rows, C, mode, d_acc.get(), d_flag.get());
        return NPBNN_OK;
    });
    if (rc) return rc;

    SupportArgs a;
    a.n_rows = n_rows;
    a.C = C;
    a.n_sets = (double)n_sets;
    a.labels = d_labels.get();
    a.thresholds = d_thr.get();
    a.n_thresholds = n_thresholds;
    a.prior = prior_summary ? d_prior.get() : nullptr;
    a.bf_thresholds = d_thr.get() + n_thresholds;
    a.n_bf = n_bf;
    a.has_cutoff = cutoff ? 1 : 0;
    a.cutoff = cutoff ? *cutoff : 0.0;
    a.summary = out_summary ? d_summary.get() : nullptr;
    a.keep = out_keep ? d_keep.get() : nullptr;
    a.cube = d_tables.get();
    a.bf_table = prior_summary ? d_tables.get() + cells : nullptr;
    a.lds_cube = cells <= (size_t)kSupportLdsCells ? 1 : 0;
    a.lds_thr = n_thresholds <= kSupportLdsThresholds ? 1 : 0;
    a.lds_bf = (prior_summary && n_bf <= kSupportLdsThresholds) ? 1 : 0;
    a.flag = d_flag.get();
    const size_t lds = (a.lds_thr ? (size_t)n_thresholds : 0) * sizeof(double) + (a.lds_bf ? (size_t)n_bf : 0) * sizeof(double) +
                       (a.lds_cube ? cells : 0) * sizeof(unsigned) + (a.lds_bf ? bf_cells : 0) * sizeof(unsigned);
    unsigned grid = grid_for(n_rows);
    const unsigned cap = (unsigned)(kSupportWgPerCu * (ctx->n_cu > 0 ? ctx->n_cu : 256));
    if (a.lds_cube && grid > cap) grid = cap;      // (a workgroup zeroes and flushes its cells once: no more of them than run at a time)
    FiTimer tm;
    tm.mark(0, st);
    if (mode == 0)
        hipLaunchKernelGGL(support_final_kernel<unsigned>, dim3(grid), dim3(kFiThreads), lds, st, (const unsigned*)reinterpret_cast<unsigned*>(d_acc.get()), a);
    else
        hipLaunchKernelGGL(support_final_kernel<double>, dim3(grid), dim3(kFiThreads), lds, st, (const double*)d_acc.get(), a);
    std::vector<double> none;                      // (no floating-point partials: the tables are integers)
    if ((rc = finish_sets_entry(ctx, "predict_sets_support", tm, d_flag.get(), nullptr, 0, 0, &ctx->fi_ns[4], C, &none))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_cube, d_tables, cells * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (out_bf) HIP_TRY(ctx, hipMemcpyAsync(out_bf, d_tables.get() + cells, bf_cells * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (out_summary) HIP_TRY(ctx, hipMemcpyAsync(out_summary, d_summary, per_set * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out_keep) HIP_TRY(ctx, hipMemcpyAsync(out_keep, d_keep, (size_t)n_rows, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return NPBNN_OK;
}
