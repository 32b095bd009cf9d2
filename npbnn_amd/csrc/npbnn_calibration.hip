// Posterior calibration of stored weight sets on the device (include/npbnn_hip.h: npbnn_predict_sets_calibration): whether the
// probabilities the posterior mean reports can be believed, checked against the labels or targets of the resident table.  With z_s a
// set's pre-output values of a row and S sets, float64 throughout:
//   softmax output (SoftMax, np_bnn/BNN_lib.py:166), m = (1/S) sum_s softmax(z_s), B bins:
//     k* = the first argmax of m;  confidence = m[k*];  correct = (k* == label);  brier = sum_k (m_k - [k == label])^2;
//     nll = -log m[label] (+inf when m[label] is 0);  bin = min(B - 1, floor(confidence B));
//     the reliability table count[B], sum_confidence[B], n_correct[B], and the totals of brier, nll and correct over the rows;
//   regression (RegressTransform :174: mu = z, sigma the caller's per set; RegressTransformError :177: mu = z[:T],
//   sigma = softplus(z[T:])), y the row's target, per (row, target):
//     pit = (1/S) sum_s Phi((y - mu_s) / sigma_s), Phi(u) = 0.5 erfc(-u / sqrt 2): the probability integral transform under the
//     posterior predictive mixture;  mean = K + (1/S) sum_s (mu_s - K), K the first set's mu;  sq_err = (y - mean)^2;
//     pit_hist[T][B] (bin = min(B - 1, floor(pit B))), covered[T][n_levels] (|pit - 0.5| <= level / 2: y lies inside the mixture's
//     central interval of that level), and the totals of sq_err and pit per target.
//
// The sets replay through replay_sets (npbnn_sets.hip.h) with apply_out_fn = 0: a group's d_y holds the float32 pre-output values.
// The accumulate kernels, one thread per row, take each set of the group in set order and widen the row's values to float64 before
// any exp, log or erfc.  Softmax: softmax_mean_accumulate_kernel<ENTROPY = false> (npbnn_fold.hip.h), the kernel
// npbnn_uncertainty.hip folds with, without its entropy term: sum_s softmax(z_s)_k onto [C][n_rows].  Regression:
// [3][T][n_rows], K, sum (mu - K) and sum Phi.  No sum is reassociated and no product fused into a sum (fp contract off), so a set
// folded alone and a set folded as the second of a group leave the same bits.
// The final kernels, one thread per row, write the pointwise values and each row's bin to device arrays.  The integer tables are
// counted per workgroup in LDS and added to the table in HBM with integer atomics (exact in any order).  The floating-point sums -
// the totals, and sum_confidence bin after bin with the bins on the outside - are per-workgroup partials (lanes by shuffles, the
// waves in wave order through LDS) the host adds in workgroup order.  No floating-point atomics; the grid depends on n_rows alone, so
// neither the grouping of the sets nor scheduling changes a bit.
#include "npbnn_fold.hip.h"

#include <cmath>
#include <vector>

// (no product is fused into a sum anywhere in this unit: see above)
#pragma clang fp contract(off)

namespace npbnn_api {

namespace {

constexpr int kCalMaxBins = 64;
constexpr int kCalMaxLevels = 16;

typedef float f32x2 __attribute__((ext_vector_type(2)));

// the coverage levels of a call, by value in the kernel's arguments
struct CalLevels {
    int n = 0;
    double half[kCalMaxLevels];       // level / 2
};

// Phi((y - mu) / sigma), the standard normal distribution function as 0.5 erfc(-u / sqrt 2)
__device__ inline double cal_phi(double y, double mu, double sigma) {
    const double u = (y - mu) / sigma;
    return 0.5 * erfc(-u / 1.4142135623730951);
}

// Target t of row r under the group's sets (mu[j], sg[j], set order) onto its accumulators K, sum (mu - K), sum Phi at
// [0 | 1 | 2][T][n_rows]; yt the row's target.
__device__ inline void cal_fold_target(int t, int T, const double (&mu)[kMaxCand], const double (&sg)[kMaxCand], double yt, int g, int s0, long long r,
                                       long long n_rows, double* __restrict__ acc, bool& nan) {
    const long long tn = (long long)T * n_rows;
    double* p = acc + (long long)t * n_rows + r;
    double K = 0.0, s1 = 0.0, sp = 0.0;
    if (s0 > 0) { K = p[0]; s1 = p[tn]; sp = p[2 * tn]; }
#pragma unroll
    for (int j = 0; j < kMaxCand; ++j) {
        if (j >= g) continue;
        if (s0 + j == 0) K = mu[j];
        else s1 += mu[j] - K;
        const double phi = cal_phi(yt, mu[j], sg[j]);
        nan = nan || (mu[j] != mu[j]) || (phi != phi);
        sp += phi;
    }
    p[0] = K; p[tn] = s1; p[2 * tn] = sp;
}

// Regression.  y [g][n_rows][n_out]; SP: NPBNN_OUT_SOFTPLUS_HALF (n_out = 2 T, the sigma of target t is softplus of output T + t), else
// identity (n_out = T, the sigma of set s and target t is sigma[s][t]).  targets [n_rows][T] as the device keeps them (float32).
// VEC: n_out is a multiple of 4.  Without SP the means are read as float4.  With SP T is even and the boundary between means and
// sigmas may lie inside a float4 (T = 2), so the row is read in aligned pairs: the means of targets t, t + 1 and their sigmas' values
// at T + t, T + t + 1.
template <bool SP, bool VEC>
__global__ __launch_bounds__(kFiThreads) void cal_regress_accumulate_kernel(const float* __restrict__ y, int g, int s0, long long n_rows, int n_out,
                                                                            const float* __restrict__ targets, const double* __restrict__ sigma,
                                                                            double* __restrict__ acc, int* __restrict__ flag) {
    bool nan = false;
    const long long per_set = n_rows * n_out;
    const int T = SP ? n_out / 2 : n_out;
    constexpr int W = VEC ? (SP ? 2 : 4) : 1;          // targets per read
    for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads) {
        const float* row = y + r * n_out;
        const float* trow = targets + r * T;
        for (int t = 0; t < T; t += W) {
            float vm[kMaxCand][W], vs[kMaxCand][W];
#pragma unroll
            for (int j = 0; j < kMaxCand; ++j) {
#pragma unroll
                for (int q = 0; q < W; ++q) vm[j][q] = vs[j][q] = 0.f;
                if (j >= g) continue;
                const float* pr = row + (long long)j * per_set;
                if (W == 4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(pr + t);
#pragma unroll
                    for (int q = 0; q < W; ++q) vm[j][q] = v[q];
                } else if (W == 2) {
                    const f32x2 v = *reinterpret_cast<const f32x2*>(pr + t);
                    const f32x2 s = *reinterpret_cast<const f32x2*>(pr + T + t);
#pragma unroll
                    for (int q = 0; q < W; ++q) { vm[j][q] = v[q]; vs[j][q] = s[q]; }
                } else {
                    vm[j][0] = pr[t];
                    if (SP) vs[j][0] = pr[T + t];
                }
            }
#pragma unroll
            for (int q = 0; q < W; ++q) {
                double mu[kMaxCand], sg[kMaxCand];
#pragma unroll
                for (int j = 0; j < kMaxCand; ++j) {
                    mu[j] = (double)vm[j][q];
                    sg[j] = 1.0;
                    if (j >= g) continue;
                    if (SP) {
                        nan = nan || (vs[j][q] != vs[j][q]);
                        sg[j] = softplus_f64((double)vs[j][q]);
                    } else {
                        sg[j] = sigma[(long long)(s0 + j) * T + t + q];
                    }
                }
                cal_fold_target(t + q, T, mu, sg, (double)trow[t + q], g, s0, r, n_rows, acc, nan);
            }
        }
    }
    if (nan) atomicOr(flag, kFlagNaN);
}

// Softmax output.  Per row: predicted class, confidence, brier, nll (each [n_rows], always written) and the row's bin; the tables
// counts [2][B] (count, n_correct; zeroed by the caller), and the workgroup's partials part[3 + B][gridDim.x]: the totals of brier, nll
// and correct, then sum_confidence bin after bin.
__global__ __launch_bounds__(kFiThreads) void cal_softmax_final_kernel(const double* __restrict__ acc, const int* __restrict__ labels, long long n_rows, int C,
                                                                       int n_sets, int B, long long* __restrict__ out_pred, double* __restrict__ out_conf,
                                                                       double* __restrict__ out_brier, double* __restrict__ out_nll, int* __restrict__ bins,
                                                                       unsigned long long* __restrict__ counts, double* __restrict__ part,
                                                                       int* __restrict__ flag) {
    __shared__ double red[kFiWaves];
    __shared__ unsigned int hist[2 * kCalMaxBins];
    for (int i = threadIdx.x; i < 2 * B; i += kFiThreads) hist[i] = 0u;
    __syncthreads();
    const double S = (double)n_sets;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    bool nan = false;
    for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads) {
        const int lab = labels[r];
        int best = 0;
        double conf = -1.0, br = 0.0, ml = 0.0;
        for (int k = 0; k < C; ++k) {
            const double m = acc[(long long)k * n_rows + r] / S;
            nan = nan || (m != m);
            if (m > conf) { conf = m; best = k; }      // (strictly larger: the first class among equal ones)
            const double d = m - (k == lab ? 1.0 : 0.0);
            br += d * d;
            if (k == lab) ml = m;
        }
        const double nl = -log(ml);                    // (+inf when the label's mean probability is 0: a value, not an error)
        const int ok = best == lab ? 1 : 0;
        int b = (int)floor(conf * (double)B);
        b = b < 0 ? 0 : (b > B - 1 ? B - 1 : b);
        out_pred[r] = best;
        out_conf[r] = conf;
        out_brier[r] = br;
        out_nll[r] = nl;
        bins[r] = b;
        atomicAdd(&hist[b], 1u);
        if (ok) atomicAdd(&hist[B + b], 1u);
        t0 += br;
        t1 += nl;
        t2 += (double)ok;
    }
    if (nan) atomicOr(flag, kFlagNaN);
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * B; i += kFiThreads)
        if (hist[i]) atomicAdd(&counts[i], (unsigned long long)hist[i]);
    const double a0 = block_sum(t0, red), a1 = block_sum(t1, red), a2 = block_sum(t2, red);
    const long long w = (long long)gridDim.x;
    if (threadIdx.x == 0) {
        part[blockIdx.x] = a0;
        part[w + blockIdx.x] = a1;
        part[2 * w + blockIdx.x] = a2;
    }
    // sum_confidence: bin by bin, so that a thread keeps one running sum whatever B is (its rows' values were written by itself)
    for (int b = 0; b < B; ++b) {
        double sc = 0.0;
        for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads)
            if (bins[r] == b) sc += out_conf[r];
        const double a = block_sum(sc, red);
        if (threadIdx.x == 0) part[(3 + b) * w + blockIdx.x] = a;
    }
}

// Regression.  pit, mean, sq_err [n_rows][T] (always written); counts [T][B + L] (pit_hist, then covered per level; zeroed by the
// caller), and the workgroup's partials part[2][T][gridDim.x]: the totals of sq_err and of pit per target.  Target by target, so that a
// thread keeps two running totals whatever T is.
__global__ __launch_bounds__(kFiThreads) void cal_regress_final_kernel(const double* __restrict__ acc, const float* __restrict__ targets, long long n_rows, int T,
                                                                       int n_sets, int B, CalLevels lv, double* __restrict__ out_pit,
                                                                       double* __restrict__ out_mean, double* __restrict__ out_sq,
                                                                       unsigned long long* __restrict__ counts, double* __restrict__ part,
                                                                       int* __restrict__ flag) {
    __shared__ double red[kFiWaves];
    __shared__ unsigned int hist[kCalMaxBins + kCalMaxLevels];
    const double S = (double)n_sets;
    const long long tn = (long long)T * n_rows;
    const int n_cnt = B + lv.n;
    bool nan = false;
    for (int t = 0; t < T; ++t) {
        __syncthreads();                               // (the previous target's counts have left hist)
        for (int i = threadIdx.x; i < n_cnt; i += kFiThreads) hist[i] = 0u;
        __syncthreads();
        double t0 = 0.0, t1 = 0.0;
        for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads) {
            const double* p = acc + (long long)t * n_rows + r;
            const double K = p[0], s1 = p[tn], sp = p[2 * tn];
            const double pit = sp / S;
            const double mean = K + s1 / S;
            const double d = (double)targets[r * T + t] - mean;
            const double sq = d * d;
            nan = nan || (pit != pit) || (mean != mean);
            out_pit[r * T + t] = pit;
            out_mean[r * T + t] = mean;
            out_sq[r * T + t] = sq;
            int b = (int)floor(pit * (double)B);
            b = b < 0 ? 0 : (b > B - 1 ? B - 1 : b);
            atomicAdd(&hist[b], 1u);
            const double off = fabs(pit - 0.5);
            for (int l = 0; l < lv.n; ++l)
                if (off <= lv.half[l]) atomicAdd(&hist[B + l], 1u);
            t0 += sq;
            t1 += pit;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n_cnt; i += kFiThreads)
            if (hist[i]) atomicAdd(&counts[(long long)t * n_cnt + i], (unsigned long long)hist[i]);
        const double a0 = block_sum(t0, red), a1 = block_sum(t1, red);
        if (threadIdx.x == 0) {
            const long long w = (long long)gridDim.x;
            part[(0 * T + t) * w + blockIdx.x] = a0;
            part[(1 * T + t) * w + blockIdx.x] = a1;
        }
    }
    if (nan) atomicOr(flag, kFlagNaN);
}

// The accumulate kernel of out_kind over a group's values y [g][n_rows][n_out], the sets s0 .. s0 + g - 1, on n_wg workgroups.  The
// accumulator d_acc is [C][n_rows] for the softmax output and [3][T][n_rows] for regression (above).
void calibration_accumulate(hipStream_t st, const float* y, int g, int s0, long long n_rows, int n_out, const float* targets, const double* d_sigma,
                            double* d_acc, int out_kind, int n_wg, int* d_flag) {
    const dim3 grid((unsigned)n_wg), block(kFiThreads);
    const bool vec = n_out % 4 == 0;
    if (out_kind == NPBNN_OUT_SOFTMAX) {
        launch_softmax_mean_accumulate<false>(st, y, g, s0, n_rows, n_out, d_acc, n_wg, d_flag);
    } else if (out_kind == NPBNN_OUT_SOFTPLUS_HALF) {
        if (vec) hipLaunchKernelGGL((cal_regress_accumulate_kernel<true, true>), grid, block, 0, st, y, g, s0, n_rows, n_out, targets, d_sigma, d_acc, d_flag);
        else hipLaunchKernelGGL((cal_regress_accumulate_kernel<true, false>), grid, block, 0, st, y, g, s0, n_rows, n_out, targets, d_sigma, d_acc, d_flag);
    } else {
        if (vec) hipLaunchKernelGGL((cal_regress_accumulate_kernel<false, true>), grid, block, 0, st, y, g, s0, n_rows, n_out, targets, d_sigma, d_acc, d_flag);
        else hipLaunchKernelGGL((cal_regress_accumulate_kernel<false, false>), grid, block, 0, st, y, g, s0, n_rows, n_out, targets, d_sigma, d_acc, d_flag);
    }
}

}  // namespace

}  // namespace npbnn_api

using namespace npbnn_api;

extern "C" int npbnn_predict_sets_calibration(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which,
                                              const double* sigma_sets, int32_t n_bins, const double* levels, int32_t n_levels, double* out_point0,
                                              double* out_point1, double* out_point2, int64_t* out_pred, int64_t* out_counts, double* out_bin_sums,
                                              double* out_totals) {
    const char* who = "predict_sets_calibration";
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    ctx->fi_ns[1] = ctx->fi_ns[2] = ctx->calibration_ns = 0;       // (a call that is refused has launched nothing)
    if (!W_sets || n_sets < 1 || !out_totals || !out_counts) return fail(ctx, NPBNN_E_ARG, "%s: bad arguments", who);
    if (n_bins < 1 || n_bins > kCalMaxBins) return fail(ctx, NPBNN_E_ARG, "%s: n_bins must lie in 1..%d, got %d", who, kCalMaxBins, n_bins);
    if (n_levels < 0 || n_levels > kCalMaxLevels || (n_levels > 0 && !levels))
        return fail(ctx, NPBNN_E_ARG, "%s: n_levels must lie in 0..%d (with levels given), got %d", who, kCalMaxLevels, n_levels);
    CalLevels lv;
    for (int l = 0; l < kCalMaxLevels; ++l) lv.half[l] = 0.0;
    for (int l = 0; l < n_levels; ++l) {
        if (!(levels[l] > 0.0 && levels[l] < 1.0)) return fail(ctx, NPBNN_E_ARG, "%s: level %d is %g; every level lies strictly inside (0, 1)", who, l, levels[l]);
        lv.half[l] = levels[l] / 2.0;
    }
    SetsTable tb;
    int rc = open_sets_table(ctx, who, which, &tb);
    if (rc) return rc;
    const int n_out = ctx->net.n_out;
    const int kind = ctx->arch.out_kind;
    const bool softmax = kind == NPBNN_OUT_SOFTMAX, sp = kind == NPBNN_OUT_SOFTPLUS_HALF;
    if (sp && n_out % 2 != 0)
        return fail(ctx, NPBNN_E_ARG, "%s: NPBNN_OUT_SOFTPLUS_HALF splits the outputs into means and sigmas, and %d is odd", who, n_out);
    const int T = softmax ? 1 : (sp ? n_out / 2 : n_out);            // columns of the per-row quantities
    if (softmax) {
        lv.n = 0;                                                   // (the levels belong to regression)
        if (!out_bin_sums) return fail(ctx, NPBNN_E_ARG, "%s: out_bin_sums is required under the softmax output", who);
        if (sigma_sets) return fail(ctx, NPBNN_E_ARG, "%s: sigma_sets goes with NPBNN_OUT_IDENTITY and with nothing else", who);
    } else {
        lv.n = n_levels;
        if (out_bin_sums) return fail(ctx, NPBNN_E_ARG, "%s: out_bin_sums belongs to the softmax output (it must be NULL under regression)", who);
        if (out_pred) return fail(ctx, NPBNN_E_ARG, "%s: out_pred belongs to the softmax output (it must be NULL under regression)", who);
        if (sp && sigma_sets) return fail(ctx, NPBNN_E_ARG, "%s: NPBNN_OUT_SOFTPLUS_HALF predicts its sigma: sigma_sets must be NULL", who);
        if (!sp && !sigma_sets) return fail(ctx, NPBNN_E_ARG, "%s: NPBNN_OUT_IDENTITY needs sigma_sets [n_sets][n_targets]", who);
    }
    Dataset& d = *tb.d;
    if (softmax && !d.labels) return fail(ctx, NPBNN_E_STATE, "%s: no labels on this data set (npbnn_set_labels_i64)", who);
    if (!softmax) {
        if (!d.targets) return fail(ctx, NPBNN_E_STATE, "%s: no targets on this data set (npbnn_set_targets_f64)", who);
        if (d.k != T) return fail(ctx, NPBNN_E_ARG, "%s: targets have %d columns, the network predicts %d", who, d.k, T);
        if (!sp && (rc = check_sigma_sets(ctx, who, sigma_sets, n_sets, T))) return rc;
    }
    const long long n_rows = tb.n_rows;
    hipStream_t st = tb.st;
    const int n_wg = tb.n_wg;
    const size_t n_acc = softmax ? (size_t)n_out * n_rows : (size_t)3 * T * n_rows;
    const size_t n_col = (size_t)n_rows * T;
    const size_t n_cnt = softmax ? (size_t)2 * n_bins : (size_t)T * (n_bins + n_levels);
    const size_t n_q = softmax ? (size_t)3 + n_bins : (size_t)2 * T;       // float sums that come back as per-workgroup partials
    // (the final kernels write all three pointwise arrays; those the caller gave come back)
    PointOuts po;
    const int o0 = po.add(out_point0, n_col, true), o1 = po.add(out_point1, n_col, true), o2 = po.add(out_point2, n_col, true);
    // accumulators, the pointwise results (po), predicted class and bin per row, the tables, the partials, the sigmas, the flag word
    DevBuf<double> d_acc, d_part, d_sig;
    DevBuf<long long> d_pred;
    DevBuf<unsigned long long> d_cnt;
    DevBuf<int> d_bin, d_flag;
    if ((rc = d_acc.reserve(ctx, n_acc))) return rc;
    if ((rc = d_flag.reserve(ctx, 4))) return rc;
    if ((rc = d_part.reserve(ctx, n_q * n_wg))) return rc;
    if ((rc = po.reserve(ctx))) return rc;
    if ((rc = d_cnt.reserve(ctx, n_cnt))) return rc;
    if (softmax && (rc = d_pred.reserve(ctx, (size_t)n_rows))) return rc;
    if (softmax && (rc = d_bin.reserve(ctx, (size_t)n_rows))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(int), st));
    HIP_TRY(ctx, hipMemsetAsync(d_cnt, 0, n_cnt * sizeof(unsigned long long), st));
    if (softmax) {
        if ((rc = check_labels_on_device(ctx, who, d.labels.get(), n_rows, n_out, d_flag.get()))) return rc;
    } else if (!sp) {
        // (the sets' sigmas go to the device once per call: a group reads its rows of them)
        if ((rc = d_sig.reserve(ctx, (size_t)n_sets * T))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(d_sig, sigma_sets, (size_t)n_sets * T * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));                     // (sigma_sets is pageable memory of the caller's)
    }
    // (the first set of a row writes every accumulator: d_acc needs no zeroing)
    rc = replay_sets(ctx, who, W_sets, act_prm_sets, n_sets, which, 0, nullptr, [&](const SetGroup& grp) {
        calibration_accumulate(st, grp.y, grp.g, grp.s0, n_rows, n_out, softmax ? nullptr : (const float*)d.targets.get(), d_sig.get(), d_acc.get(), kind,
                               n_wg, d_flag.get());
        return NPBNN_OK;
    });
    if (rc) return rc;
    FiTimer tm;
    tm.mark(0, st);
    const dim3 grid((unsigned)n_wg), block(kFiThreads);
    if (softmax)
        hipLaunchKernelGGL(cal_softmax_final_kernel, grid, block, 0, st, (const double*)d_acc.get(), (const int*)d.labels.get(), n_rows, n_out, (int)n_sets,
                           (int)n_bins, d_pred.get(), po.dev(o0), po.dev(o1), po.dev(o2), d_bin.get(), d_cnt.get(), d_part.get(), d_flag.get());
    else
        hipLaunchKernelGGL(cal_regress_final_kernel, grid, block, 0, st, (const double*)d_acc.get(), (const float*)d.targets.get(), n_rows, T, (int)n_sets,
                           (int)n_bins, lv, po.dev(o0), po.dev(o1), po.dev(o2), d_cnt.get(), d_part.get(), d_flag.get());
    std::vector<double> sums;
    // (the labels were checked before the replay and the final kernels raise no label flag: 0 classes)
    if ((rc = finish_sets_entry(ctx, who, tm, d_flag.get(), d_part.get(), n_q, n_wg, &ctx->calibration_ns, 0, &sums))) return rc;
    if (softmax) {
        memcpy(out_totals, sums.data(), 3 * sizeof(double));
        memcpy(out_bin_sums, sums.data() + 3, (size_t)n_bins * sizeof(double));
    } else {
        memcpy(out_totals, sums.data(), (size_t)2 * T * sizeof(double));
    }
    static_assert(sizeof(unsigned long long) == sizeof(int64_t) && sizeof(long long) == sizeof(int64_t), "the tables are copied as they are");
    HIP_TRY(ctx, hipMemcpyAsync(out_counts, d_cnt, n_cnt * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if ((rc = po.copy_out(ctx, st))) return rc;
    if (out_pred) HIP_TRY(ctx, hipMemcpyAsync(out_pred, d_pred, (size_t)n_rows * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return NPBNN_OK;
}
