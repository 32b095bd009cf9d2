// Log pointwise predictive density and WAIC of stored weight sets on the device (include/npbnn_hip.h: npbnn_predict_sets_lppd).  The
// per-row terms are the summands of calc_likelihood (np_bnn/BNN_lib.py:121, log(prediction[i, label_i])) and of
// calc_likelihood_regression (:131, norm.logpdf(y, mu, sigma)), unweighted and untempered: ll[s][i], summed over the target columns for
// regression.  From that [S][N] matrix, which is never built:
//   lppd_i = logsumexp_s ll[s][i] - log S,  mean_ll_i = mean_s ll[s][i],  p_waic_i = var_s ll[s][i] (ddof 1),  ll_sample[s] = sum_i ll[s][i].
//
// The sets replay through replay_sets (npbnn_sets.hip.h), the entries' shared driver, with apply_out_fn = 0: a group's d_y holds the
// float32 pre-output values (logits, or the means of identity-output regression).  lppd_accumulate_kernel, one thread per row, takes
// each set of the group in set order, widens the row's C values to float64 and forms ll - categorical as z[label] - (max + log sum
// exp(z - max)), never log(softmax): a probability that underflows in float32 stays a finite log - then updates the row's five float64
// accumulators [kLppdAcc][n_rows]: running maximum m, sum exp(ll - m) (rescaled when m moves), K = the row's ll under the first set, and
// the sums of (ll - K) and (ll - K)^2 (the variance does not cancel when |ll| is large and its spread tiny).  The row is read twice
// (maximum, then the sum of exponentials; the second read hits the cache), so no class count needs a register array or scratch.
// Per-sample totals without floating-point atomics: a thread adds its rows' ll per set in row order, a wave reduces by shuffles, the
// workgroup's four waves through LDS in wave order, and one float64 partial goes to part[set][workgroup]; the host adds a set's partials
// in workgroup order.  The grid depends on n_rows alone, so neither the grouping of the sets nor scheduling changes a bit.
// lppd_final_kernel, one thread per row, turns the accumulators into lppd_i, mean_ll_i, p_waic_i and per-workgroup partials of their
// totals, reduced the same way.
#include "npbnn_fold.hip.h"

#include <cmath>
#include <vector>

namespace npbnn_api {

namespace {

constexpr int kLppdAcc = 5;                        // float64 accumulators per row, each an array [n_rows]

// What lppd_accumulate_kernel needs beside a group's values, all on the device.  The accumulator acc is [kLppdAcc][n_rows]: the running
// maximum m of the row's log-likelihoods, sum exp(ll - m), K (the row's ll under the first set), sum (ll - K), sum (ll - K)^2.
struct LppdArgs {
    int lik_kind = 0;                 // NPBNN_LIK_CATEGORICAL or NPBNN_LIK_GAUSS
    const int* labels = nullptr;      // [n_rows] (categorical)
    const float* targets = nullptr;   // [n_rows][C] (Gaussian)
    const double* lconst = nullptr;   // [n_sets][C] -0.5 log(2 pi) - log(sigma) (Gaussian)
    const double* isigma = nullptr;   // [n_sets][C] 1 / sigma (Gaussian)
    double* part = nullptr;           // [n_sets][n_wg]: every workgroup's sum of its rows' ll under a set
    int n_wg = 0;                     // workgroups of the accumulate launch: grid_for(n_rows)
};

// GAUSS: the likelihood is Gaussian (else categorical).  VEC: C is a multiple of 4, rows are read as float4.
template <bool GAUSS, bool VEC>
__global__ __launch_bounds__(kFiThreads) void lppd_accumulate_kernel(const float* __restrict__ y, int g, int s0, long long n_rows, int C,
                                                                     double* __restrict__ acc, LppdArgs a, int* __restrict__ flag) {
    __shared__ double red[kFiWaves];
    bool nan = false, bad = false;
    const long long per_set = n_rows * C;
    double tot[kMaxCand];
#pragma unroll
    for (int j = 0; j < kMaxCand; ++j) tot[j] = 0.0;
    double* acc_m = acc;
    double* acc_e = acc + n_rows;
    double* acc_k = acc + 2 * n_rows;
    double* acc_s = acc + 3 * n_rows;
    double* acc_q = acc + 4 * n_rows;
    for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads) {
        int lab = 0;
        if (!GAUSS) {
            lab = a.labels[r];
            if (lab < 0 || lab >= C) { bad = true; continue; }
        }
        double m = 0.0, e = 0.0, K = 0.0, s1 = 0.0, s2 = 0.0;
        if (s0 > 0) { m = acc_m[r]; e = acc_e[r]; K = acc_k[r]; s1 = acc_s[r]; s2 = acc_q[r]; }
#pragma unroll
        for (int j = 0; j < kMaxCand; ++j) {
            if (j >= g) break;
            const float* row = y + (long long)j * per_set + r * C;
            double ll;
            if (GAUSS) {
                const float* t = a.targets + r * C;
                const double* lc = a.lconst + (long long)(s0 + j) * C;
                const double* is = a.isigma + (long long)(s0 + j) * C;
                ll = 0.0;
                if (VEC) {
                    for (int k = 0; k < C; k += 4) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(row + k);
                        const f32x4 tv = *reinterpret_cast<const f32x4*>(t + k);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            nan = nan || (v[q] != v[q]);
                            const double u = ((double)tv[q] - (double)v[q]) * is[k + q];
                            ll += lc[k + q] - 0.5 * u * u;
                        }
                    }
                } else {
                    for (int k = 0; k < C; ++k) {
                        const float v = row[k];
                        nan = nan || (v != v);
                        const double u = ((double)t[k] - (double)v) * is[k];
                        ll += lc[k] - 0.5 * u * u;
                    }
                }
            } else {
                const double mx = row_max<VEC>(row, C, nan);
                ll = (double)row[lab] - (mx + log(row_sum_exp<VEC>(row, C, mx)));
            }
            nan = nan || (ll != ll);
            tot[j] += ll;
            if (s0 + j == 0) {
                m = ll; e = 1.0; K = ll; s1 = 0.0; s2 = 0.0;
            } else {
                if (ll > m) { e = e * exp(m - ll) + 1.0; m = ll; }
                else e += exp(ll - m);
                const double dl = ll - K;
                s1 += dl;
                s2 += dl * dl;
            }
        }
        acc_m[r] = m; acc_e[r] = e; acc_k[r] = K; acc_s[r] = s1; acc_q[r] = s2;
    }
    if (nan) atomicOr(flag, kFlagNaN);
    if (bad) atomicOr(flag, kFlagBadLabel);
#pragma unroll
    for (int j = 0; j < kMaxCand; ++j) {
        if (j >= g) break;                            // (g is uniform: every thread takes the same reductions)
        const double s = block_sum(tot[j], red);
        if (threadIdx.x == 0) a.part[(long long)(s0 + j) * a.n_wg + blockIdx.x] = s;
    }
}

// lppd_i, mean_ll_i, p_waic_i (each output array may be nullptr) and the workgroup's partials of their totals, part[3][gridDim.x]
__global__ __launch_bounds__(kFiThreads) void lppd_final_kernel(const double* __restrict__ acc, long long n_rows, int n_sets, double* __restrict__ out_lppd,
                                                                double* __restrict__ out_mean, double* __restrict__ out_pwaic, double* __restrict__ part) {
    __shared__ double red[kFiWaves];
    const double S = (double)n_sets, log_s = log(S);
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads) {
        const double m = acc[r], e = acc[n_rows + r], K = acc[2 * n_rows + r], s1 = acc[3 * n_rows + r], s2 = acc[4 * n_rows + r];
        const double lp = m + log(e) - log_s;
        const double mean = K + s1 / S;
        double pw = 0.0;
        if (n_sets > 1) pw = fmax(0.0, (s2 - s1 * s1 / S) / (S - 1.0));
        if (out_lppd) out_lppd[r] = lp;
        if (out_mean) out_mean[r] = mean;
        if (out_pwaic) out_pwaic[r] = pw;
        t0 += lp;
        t1 += mean;
        t2 += pw;
    }
    const double a0 = block_sum(t0, red), a1 = block_sum(t1, red), a2 = block_sum(t2, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = a0;
        part[gridDim.x + blockIdx.x] = a1;
        part[2 * gridDim.x + blockIdx.x] = a2;
    }
}

// lppd_accumulate_kernel over a group's values y [g][n_rows][C], the sets s0 .. s0 + g - 1
void lppd_accumulate(hipStream_t st, const float* y, int g, int s0, long long n_rows, int C, double* d_acc, const LppdArgs& a, int* d_flag) {
    const dim3 grid((unsigned)a.n_wg), block(kFiThreads);
    const bool vec = C % 4 == 0;
    if (a.lik_kind == NPBNN_LIK_GAUSS) {
        if (vec) hipLaunchKernelGGL((lppd_accumulate_kernel<true, true>), grid, block, 0, st, y, g, s0, n_rows, C, d_acc, a, d_flag);
        else hipLaunchKernelGGL((lppd_accumulate_kernel<true, false>), grid, block, 0, st, y, g, s0, n_rows, C, d_acc, a, d_flag);
    } else {
        if (vec) hipLaunchKernelGGL((lppd_accumulate_kernel<false, true>), grid, block, 0, st, y, g, s0, n_rows, C, d_acc, a, d_flag);
        else hipLaunchKernelGGL((lppd_accumulate_kernel<false, false>), grid, block, 0, st, y, g, s0, n_rows, C, d_acc, a, d_flag);
    }
}

}  // namespace

}  // namespace npbnn_api

using namespace npbnn_api;

extern "C" int npbnn_predict_sets_lppd(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which, int lik_kind,
                                       const double* sigma_sets, double* out_lppd_i, double* out_mean_ll_i, double* out_pwaic_i,
                                       double* out_ll_sample, double* out_totals) {
    const char* who = "predict_sets_lppd";
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    ctx->fi_ns[1] = ctx->fi_ns[2] = ctx->fi_ns[5] = 0;       // (a call that is refused has launched nothing)
    if (!W_sets || n_sets < 1 || !out_totals) return fail(ctx, NPBNN_E_ARG, "%s: bad arguments", who);
    if (lik_kind == NPBNN_LIK_GAUSS_PRED_SIGMA || lik_kind == NPBNN_LIK_POISSON || lik_kind == NPBNN_LIK_NEGBIN || lik_kind == NPBNN_LIK_NEGBIN2D ||
        lik_kind == NPBNN_LIK_NEGBIN_BASE10)
        return fail(ctx, NPBNN_E_ARG, "%s: predicted-sigma regression and the count likelihoods are out of scope (likelihood kind %d); "
                    "NPBNN_LIK_CATEGORICAL and NPBNN_LIK_GAUSS are served", who, lik_kind);
    if (lik_kind != NPBNN_LIK_CATEGORICAL && lik_kind != NPBNN_LIK_GAUSS)
        return fail(ctx, NPBNN_E_ARG, "%s: lik_kind must be NPBNN_LIK_CATEGORICAL or NPBNN_LIK_GAUSS, got %d", who, lik_kind);
    const bool gauss = lik_kind == NPBNN_LIK_GAUSS;
    if (gauss != (sigma_sets != nullptr)) return fail(ctx, NPBNN_E_ARG, "%s: sigma_sets goes with NPBNN_LIK_GAUSS and with nothing else", who);
    SetsTable tb;
    int rc = open_sets_table(ctx, who, which, &tb);
    if (rc) return rc;
    const int C = ctx->net.n_out;
    if (ctx->arch.out_kind != (gauss ? NPBNN_OUT_IDENTITY : NPBNN_OUT_SOFTMAX))
        return fail(ctx, NPBNN_E_ARG, "%s: the %s likelihood goes with the %s output function", who, gauss ? "Gaussian" : "categorical",
                    gauss ? "identity" : "softmax");
    Dataset& d = *tb.d;
    if (!gauss && !d.labels) return fail(ctx, NPBNN_E_STATE, "%s: no labels on this data set (npbnn_set_labels_i64)", who);
    if (gauss) {
        if (!d.targets) return fail(ctx, NPBNN_E_STATE, "%s: no targets on this data set (npbnn_set_targets_f64)", who);
        if (d.k != C) return fail(ctx, NPBNN_E_ARG, "%s: targets have %d columns, the network %d outputs", who, d.k, C);
        if ((rc = check_sigma_sets(ctx, who, sigma_sets, n_sets, C))) return rc;
    }
    const long long n_rows = tb.n_rows;
    hipStream_t st = tb.st;
    const int n_wg = tb.n_wg;
    PointOuts po;
    const int o_lppd = po.add(out_lppd_i, (size_t)n_rows), o_mean = po.add(out_mean_ll_i, (size_t)n_rows), o_pw = po.add(out_pwaic_i, (size_t)n_rows);
    // accumulators, the pointwise results (po), the partials [n_sets][n_wg] | [3][n_wg], the sigma terms [lconst | isigma], the flag word
    DevBuf<double> d_acc, d_part, d_sig;
    DevBuf<int> d_flag;
    if ((rc = d_acc.reserve(ctx, (size_t)kLppdAcc * n_rows))) return rc;
    if ((rc = d_flag.reserve(ctx, 4))) return rc;
    if ((rc = d_part.reserve(ctx, (size_t)(n_sets + 3) * n_wg))) return rc;
    if ((rc = po.reserve(ctx))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(int), st));
    LppdArgs a;
    a.lik_kind = lik_kind;
    a.part = d_part.get();
    a.n_wg = n_wg;
    std::vector<double> h_sig;
    if (gauss) {
        const size_t n = (size_t)n_sets * C;
        h_sig.resize(2 * n);
        const double half_log_2pi = 0.5 * log(2.0 * M_PI);
        for (size_t i = 0; i < n; ++i) {
            h_sig[i] = -half_log_2pi - log(sigma_sets[i]);
            h_sig[n + i] = 1.0 / sigma_sets[i];
        }
        if ((rc = d_sig.reserve(ctx, 2 * n))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(d_sig, h_sig.data(), 2 * n * sizeof(double), hipMemcpyHostToDevice, st));
        a.targets = d.targets.get();
        a.lconst = d_sig.get();
        a.isigma = d_sig.get() + n;
    } else {
        a.labels = d.labels.get();
        if ((rc = check_labels_on_device(ctx, who, d.labels.get(), n_rows, C, d_flag.get()))) return rc;
    }
    // (the first set of a row writes every accumulator: d_acc needs no zeroing)
    rc = replay_sets(ctx, who, W_sets, act_prm_sets, n_sets, which, 0, nullptr, [&](const SetGroup& grp) {
        lppd_accumulate(st, grp.y, grp.g, grp.s0, n_rows, C, d_acc.get(), a, d_flag.get());
        return NPBNN_OK;
    });
    if (rc) return rc;
    FiTimer tm;
    tm.mark(0, st);
    double* d_tot = d_part.get() + (size_t)n_sets * n_wg;
    hipLaunchKernelGGL(lppd_final_kernel, dim3((unsigned)n_wg), dim3(kFiThreads), 0, st, (const double*)d_acc.get(), n_rows, (int)n_sets, po.dev(o_lppd),
                       po.dev(o_mean), po.dev(o_pw), d_tot);
    std::vector<double> sums;          // every set's ll total, then the three totals
    if ((rc = finish_sets_entry(ctx, who, tm, d_flag.get(), d_part.get(), (size_t)n_sets + 3, n_wg, &ctx->fi_ns[5], C, &sums))) return rc;
    if (out_ll_sample) memcpy(out_ll_sample, sums.data(), (size_t)n_sets * sizeof(double));
    memcpy(out_totals, sums.data() + n_sets, 3 * sizeof(double));
    if ((rc = po.copy_out(ctx, st))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return NPBNN_OK;
}
