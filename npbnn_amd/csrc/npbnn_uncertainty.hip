// Posterior uncertainty decomposition of stored weight sets on the device (include/npbnn_hip.h: npbnn_predict_sets_uncertainty): the
// uncertainty of a prediction split into the part the data cannot remove (aleatoric) and the part that comes from the posterior over
// the weights (epistemic).  With z_s a set's pre-output values of a row and S sets:
//   softmax output (SoftMax, np_bnn/BNN_lib.py:166), p_s = softmax(z_s):
//     mean_prob_k = (1/S) sum_s p_sk;  predictive entropy = -sum_k m_k log m_k of that mean (a term with m_k = 0 is 0);
//     expected entropy = (1/S) sum_s H(p_s), H(p_s) = lse(z_s) - sum_k p_sk z_sk;  mutual information = max(0, predictive - expected);
//   regression (RegressTransform :174: mu = z; RegressTransformError :177: mu = z[:T], sigma = softplus(z[T:])):
//     mean_t = mean_s mu_st;  epistemic_t = var_s mu_st (ddof 0);  aleatoric_t = mean_s sigma_st^2 (RegressTransformError only: the
//     sigma of RegressTransform is the caller's);  total = epistemic + aleatoric.
//
// The sets replay through replay_sets (npbnn_sets.hip.h), the driver all stored-sets entries share, with apply_out_fn = 0: a group's d_y
// holds the float32 pre-output values.  The accumulate kernels, one thread per row, take each set of the group in set order and widen
// the row's values to float64 before any exp or log.  Softmax: softmax_mean_accumulate_kernel<ENTROPY = true> (npbnn_fold.hip.h),
// accumulators [C + 1][n_rows]: sum_s p_sk per class, then sum_s H_s.  Regression: per (target, row)
// K = the first set's mu, sum (mu - K), sum (mu - K)^2 (the variance does not cancel when the mean is large and the spread tiny), and
// for RegressTransformError sum sigma^2: [3 or 4][T][n_rows].  Every array is [n_rows] long per class or target, so a thread per row
// reads and writes it coalesced.  No sum is reassociated and no product fused into a sum (fp contract off), so a set folded alone and a
// set folded as the second of a group leave the same bits.
// The final kernels, one thread per row, turn the accumulators into the outputs and into per-workgroup partials of every per-row
// quantity's total: lanes by shuffles, the waves in wave order through LDS, and the host adds the workgroups in order.  No
// floating-point atomics; the grid depends on n_rows alone, so neither the grouping of the sets nor scheduling changes a bit.
#include "npbnn_fold.hip.h"

#include <cmath>
#include <vector>

// (no product is fused into a sum anywhere in this unit: see above)
#pragma clang fp contract(off)

namespace npbnn_api {

namespace {

// One output o of a row under the group's sets (v[j], set order) onto its accumulators.  o < T (always, without SP): the mean of
// target o - K, sum (mu - K), sum (mu - K)^2 at [0 | 1 | 2][T][n_rows]; o >= T: the sigma of target o - T - sum softplus(z)^2 at
// [3][T][n_rows].
template <bool SP>
__device__ inline void unc_fold_output(int o, int T, const float (&v)[kMaxCand], int g, int s0, long long r, long long n_rows, double* __restrict__ acc,
                                       bool& nan) {
    const long long tn = (long long)T * n_rows;
    if (!SP || o < T) {
        double* p = acc + (long long)o * n_rows + r;
        double K = 0.0, s1 = 0.0, s2 = 0.0;
        if (s0 > 0) { K = p[0]; s1 = p[tn]; s2 = p[2 * tn]; }
#pragma unroll
        for (int j = 0; j < kMaxCand; ++j) {
            if (j >= g) continue;
            nan = nan || (v[j] != v[j]);
            const double mu = (double)v[j];
            if (s0 + j == 0) {
                K = mu;
            } else {
                const double d = mu - K;
                s1 += d;
                s2 += d * d;
            }
        }
        p[0] = K; p[tn] = s1; p[2 * tn] = s2;
    } else {
        double* p = acc + 3 * tn + (long long)(o - T) * n_rows + r;
        double sg = s0 > 0 ? p[0] : 0.0;
#pragma unroll
        for (int j = 0; j < kMaxCand; ++j) {
            if (j >= g) continue;
            nan = nan || (v[j] != v[j]);
            const double s = softplus_f64((double)v[j]);
            sg += s * s;
        }
        p[0] = sg;
    }
}

// Regression.  y [g][n_rows][n_out]; SP: NPBNN_OUT_SOFTPLUS_HALF (n_out = 2 T), else identity (n_out = T).  VEC: n_out is a multiple
// of 4, rows are read as float4 - with SP the boundary between means and sigmas may lie inside a vector (T = 2), so every element
// finds its side by its own index.
template <bool SP, bool VEC>
__global__ __launch_bounds__(kFiThreads) void unc_regress_accumulate_kernel(const float* __restrict__ y, int g, int s0, long long n_rows, int n_out,
                                                                            double* __restrict__ acc, int* __restrict__ flag) {
    bool nan = false;
    const long long per_set = n_rows * n_out;
    const int T = SP ? n_out / 2 : n_out;
    for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads) {
        const float* row = y + r * n_out;
        if (VEC) {
            for (int k = 0; k < n_out; k += 4) {
                f32x4 w[kMaxCand];
#pragma unroll
                for (int j = 0; j < kMaxCand; ++j) w[j] = j < g ? *reinterpret_cast<const f32x4*>(row + (long long)j * per_set + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v[kMaxCand];
#pragma unroll
                    for (int j = 0; j < kMaxCand; ++j) v[j] = w[j][q];
                    unc_fold_output<SP>(k + q, T, v, g, s0, r, n_rows, acc, nan);
                }
            }
        } else {
            for (int k = 0; k < n_out; ++k) {
                float v[kMaxCand];
#pragma unroll
                for (int j = 0; j < kMaxCand; ++j) v[j] = j < g ? row[(long long)j * per_set + k] : 0.f;
                unc_fold_output<SP>(k, T, v, g, s0, r, n_rows, acc, nan);
            }
        }
    }
    if (nan) atomicOr(flag, kFlagNaN);
}

// Softmax output: mean_prob [n_rows][C], predictive entropy, expected entropy and mutual information [n_rows] (each may be nullptr) and
// the workgroup's partials of the three per-row quantities' totals, part[3][gridDim.x]
__global__ __launch_bounds__(kFiThreads) void unc_softmax_final_kernel(const double* __restrict__ acc, long long n_rows, int C, int n_sets,
                                                                       double* __restrict__ out_mean, double* __restrict__ out_pred, double* __restrict__ out_exp,
                                                                       double* __restrict__ out_mi, double* __restrict__ part, int* __restrict__ flag) {
    __shared__ double red[kFiWaves];
    const double S = (double)n_sets;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    bool nan = false;
    for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads) {
        double pe = 0.0;
        for (int k = 0; k < C; ++k) {
            const double m = acc[(long long)k * n_rows + r] / S;
            if (out_mean) out_mean[r * C + k] = m;
            if (m > 0.0) pe -= m * log(m);
        }
        const double ee = acc[(long long)C * n_rows + r] / S;
        const double mi = n_sets > 1 ? fmax(0.0, pe - ee) : 0.0;
        nan = nan || (pe != pe) || (ee != ee);
        if (out_pred) out_pred[r] = pe;
        if (out_exp) out_exp[r] = ee;
        if (out_mi) out_mi[r] = mi;
        t0 += pe;
        t1 += ee;
        t2 += mi;
    }
    if (nan) atomicOr(flag, kFlagNaN);
    const double a0 = block_sum(t0, red), a1 = block_sum(t1, red), a2 = block_sum(t2, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = a0;
        part[gridDim.x + blockIdx.x] = a1;
        part[2 * gridDim.x + blockIdx.x] = a2;
    }
}

// Regression: mean, total, aleatoric and epistemic variance [n_rows][T] (each may be nullptr; total and aleatoric only with SP) and the
// workgroup's partials of their totals per target, part[4][T][gridDim.x] (without SP the total's and the aleatoric rows are 0).
// Target by target, so that a thread keeps three running totals whatever T is.
template <bool SP>
__global__ __launch_bounds__(kFiThreads) void unc_regress_final_kernel(const double* __restrict__ acc, long long n_rows, int T, int n_sets,
                                                                       double* __restrict__ out_mean, double* __restrict__ out_total, double* __restrict__ out_alea,
                                                                       double* __restrict__ out_epi, double* __restrict__ part, int* __restrict__ flag) {
    __shared__ double red[kFiWaves];
    const double S = (double)n_sets;
    const long long tn = (long long)T * n_rows;
    bool nan = false;
    for (int t = 0; t < T; ++t) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
        for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads) {
            const double* p = acc + (long long)t * n_rows + r;
            const double K = p[0], s1 = p[tn], s2 = p[2 * tn];
            const double mean = K + s1 / S;
            const double ev = n_sets > 1 ? fmax(0.0, (s2 - s1 * s1 / S) / S) : 0.0;
            const double av = SP ? p[3 * tn] / S : 0.0;
            nan = nan || (mean != mean) || (ev != ev) || (av != av);
            if (out_mean) out_mean[r * T + t] = mean;
            if (out_epi) out_epi[r * T + t] = ev;
            if (SP && out_alea) out_alea[r * T + t] = av;
            if (SP && out_total) out_total[r * T + t] = ev + av;
            t0 += mean;
            t1 += av;
            t2 += ev;
        }
        const double a0 = block_sum(t0, red), a1 = block_sum(t1, red), a2 = block_sum(t2, red);
        if (threadIdx.x == 0) {
            const long long w = (long long)gridDim.x;
            part[(0 * T + t) * w + blockIdx.x] = a0;
            part[(1 * T + t) * w + blockIdx.x] = SP ? a2 + a1 : 0.0;
            part[(2 * T + t) * w + blockIdx.x] = a1;
            part[(3 * T + t) * w + blockIdx.x] = a2;
        }
    }
    if (nan) atomicOr(flag, kFlagNaN);
}

// The accumulate kernel of out_kind over a group's values y [g][n_rows][n_out], the sets s0 .. s0 + g - 1, on n_wg workgroups.  The
// accumulator d_acc is [C + 1][n_rows] for the softmax output and [3 or 4][T][n_rows] for regression (above).
void uncertainty_accumulate(hipStream_t st, const float* y, int g, int s0, long long n_rows, int n_out, double* d_acc, int out_kind, int n_wg,
                            int* d_flag) {
    const dim3 grid((unsigned)n_wg), block(kFiThreads);
    const bool vec = n_out % 4 == 0;
    if (out_kind == NPBNN_OUT_SOFTMAX) {
        launch_softmax_mean_accumulate<true>(st, y, g, s0, n_rows, n_out, d_acc, n_wg, d_flag);
    } else if (out_kind == NPBNN_OUT_SOFTPLUS_HALF) {
        if (vec) hipLaunchKernelGGL((unc_regress_accumulate_kernel<true, true>), grid, block, 0, st, y, g, s0, n_rows, n_out, d_acc, d_flag);
        else hipLaunchKernelGGL((unc_regress_accumulate_kernel<true, false>), grid, block, 0, st, y, g, s0, n_rows, n_out, d_acc, d_flag);
    } else {
        if (vec) hipLaunchKernelGGL((unc_regress_accumulate_kernel<false, true>), grid, block, 0, st, y, g, s0, n_rows, n_out, d_acc, d_flag);
        else hipLaunchKernelGGL((unc_regress_accumulate_kernel<false, false>), grid, block, 0, st, y, g, s0, n_rows, n_out, d_acc, d_flag);
    }
}

}  // namespace

}  // namespace npbnn_api

using namespace npbnn_api;

extern "C" int npbnn_predict_sets_uncertainty(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which,
                                              double* out_mean, double* out_total, double* out_aleatoric, double* out_epistemic, double* out_totals) {
    const char* who = "predict_sets_uncertainty";
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    ctx->fi_ns[1] = ctx->fi_ns[2] = ctx->fi_ns[6] = 0;       // (a call that is refused has launched nothing)
    if (!W_sets || n_sets < 1 || !out_totals) return fail(ctx, NPBNN_E_ARG, "%s: bad arguments", who);
    SetsTable tb;
    int rc = open_sets_table(ctx, who, which, &tb);
    if (rc) return rc;
    const int n_out = ctx->net.n_out;
    const int kind = ctx->arch.out_kind;
    const bool softmax = kind == NPBNN_OUT_SOFTMAX, sp = kind == NPBNN_OUT_SOFTPLUS_HALF;
    if (sp && n_out % 2 != 0)
        return fail(ctx, NPBNN_E_ARG, "%s: NPBNN_OUT_SOFTPLUS_HALF splits the outputs into means and sigmas, and %d is odd", who, n_out);
    if (kind == NPBNN_OUT_IDENTITY && (out_total || out_aleatoric))
        return fail(ctx, NPBNN_E_ARG, "%s: the identity output predicts no sigma: the aleatoric and the total variance are the "
                    "caller's to add (out_total and out_aleatoric must be NULL)", who);
    const long long n_rows = tb.n_rows;
    hipStream_t st = tb.st;
    const int n_wg = tb.n_wg;
    const int T = softmax ? 1 : (sp ? n_out / 2 : n_out);            // columns of the per-row quantities
    const size_t n_acc = softmax ? (size_t)(n_out + 1) * n_rows : (size_t)(sp ? 4 : 3) * T * n_rows;
    const size_t n_mean = (size_t)n_rows * (softmax ? n_out : T), n_col = (size_t)n_rows * T;
    const size_t n_q = softmax ? 3 : (size_t)4 * T;                  // float sums that come back as per-workgroup partials
    PointOuts po;
    const int o_mean = po.add(out_mean, n_mean), o_total = po.add(out_total, n_col), o_alea = po.add(out_aleatoric, n_col),
              o_epi = po.add(out_epistemic, n_col);
    // accumulators, the pointwise results (po), the partials, the flag word
    DevBuf<double> d_acc, d_part;
    DevBuf<int> d_flag;
    if ((rc = d_acc.reserve(ctx, n_acc))) return rc;
    if ((rc = d_flag.reserve(ctx, 4))) return rc;
    if ((rc = d_part.reserve(ctx, n_q * n_wg))) return rc;
    if ((rc = po.reserve(ctx))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(int), st));
    // (the first set of a row writes every accumulator: d_acc needs no zeroing)
    rc = replay_sets(ctx, who, W_sets, act_prm_sets, n_sets, which, 0, nullptr, [&](const SetGroup& grp) {
        uncertainty_accumulate(st, grp.y, grp.g, grp.s0, n_rows, n_out, d_acc.get(), kind, n_wg, d_flag.get());
        return NPBNN_OK;
    });
    if (rc) return rc;
    FiTimer tm;
    tm.mark(0, st);
    const dim3 grid((unsigned)n_wg), block(kFiThreads);
    if (softmax)
        hipLaunchKernelGGL(unc_softmax_final_kernel, grid, block, 0, st, (const double*)d_acc.get(), n_rows, n_out, (int)n_sets, po.dev(o_mean), po.dev(o_total),
                           po.dev(o_alea), po.dev(o_epi), d_part.get(), d_flag.get());
    else if (sp)
        hipLaunchKernelGGL(unc_regress_final_kernel<true>, grid, block, 0, st, (const double*)d_acc.get(), n_rows, T, (int)n_sets, po.dev(o_mean),
                           po.dev(o_total), po.dev(o_alea), po.dev(o_epi), d_part.get(), d_flag.get());
    else
        hipLaunchKernelGGL(unc_regress_final_kernel<false>, grid, block, 0, st, (const double*)d_acc.get(), n_rows, T, (int)n_sets, po.dev(o_mean),
                           po.dev(o_total), po.dev(o_alea), po.dev(o_epi), d_part.get(), d_flag.get());
    std::vector<double> totals;
    if ((rc = finish_sets_entry(ctx, who, tm, d_flag.get(), d_part.get(), n_q, n_wg, &ctx->fi_ns[6], 0, &totals))) return rc;
    memcpy(out_totals, totals.data(), totals.size() * sizeof(double));
    if ((rc = po.copy_out(ctx, st))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return NPBNN_OK;
}
