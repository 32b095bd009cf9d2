// Pareto-smoothed importance-sampling leave-one-out cross-validation of stored samples (include/npbnn_hip.h: npbnn_op_psis has the
// definition, npbnn_predict_sets_loo the entry; Vehtari, Gelman, Gabry 2017; Vehtari et al. 2024; the fit of the generalized Pareto
// distribution is Zhang and Stephens 2009 with the weakly informative prior of loo / ArviZ).
//
// psis_kernel is a column kernel over a sample stack (npbnn_stack.hip.h: tile rule, loader, launch): a workgroup takes its tile of
// adjacent columns of log-likelihoods into LDS as columns of P = next power of two >= S values (padded with +inf, pitch P + 1) and
// sorts each ascending by a bitonic network.  Sorting ll sorts the log ratios x = min(ll) - ll the other way round, so the tail - the
// x above the cut - is the column's first n entries, and nothing but the sorted column is needed: one wave per column finds the cut
// and n, holds the n <= 384 tail values t_j in registers (six a lane), runs one wave_sum per candidate b_q (49 at most), folds the
// weights w_q with a lane per candidate, and evaluates the smoothed log weight of a tail entry where it is used, in the two passes of
// each log-sum-exp (maximum, then sum).  Everything after the load is float64 with contraction off; no scratch, no atomics but the
// flag; lanes stride over the column and the wave adds by the fixed butterfly, so the bits of a column's results depend on its values
// alone.  The network is this unit's own copy of hpd_kernel's (npbnn_hpd.hip): that kernel's three builds were left untouched.
//
// npbnn_predict_sets_loo replays the sets through replay_sets with apply_out_fn = 0; its sink, loo_log_lik_kernel, writes every
// group's ll[s][i] - lppd_accumulate_kernel's expressions in its term order (npbnn_lppd.hip) - into a float64 device matrix [S][N] and
// the per-sample totals as per-workgroup partials, as that kernel does.  One launch of psis_kernel<double> reads the matrix once.
#include "npbnn_fold.hip.h"
#include "npbnn_stack.hip.h"

#include <cfloat>
#include <cmath>
#include <vector>

namespace npbnn_api {

namespace {

constexpr int kFlagNotFinite = 8;                  // a log-likelihood is NaN or infinite (beside the kFlag* of npbnn_sets.hip.h)
constexpr int kPsisMaxTail = 384;                  // M = ceil(min(S / 5, 3 sqrt(S))) at S = kStackMaxSamples
constexpr int kPsisTailPerLane = kPsisMaxTail / 64;
constexpr int kPsisMinTail = 4;                    // a tail of this many values or fewer is not fitted
static_assert(9LL * kStackMaxSamples <= (long long)kPsisMaxTail * kPsisMaxTail, "3 sqrt(S) tail values fit the lanes' registers");

struct PsisParams {
    const void* values;       // values[s * col_stride + c]: log-likelihoods
    long long n_cols, col_stride;
    int S, P, log2P, M, tile, log2tile;
    double log_min;           // log(DBL_MIN)
    double* elpd;
    double* lppd;
    double* k;
    int* flag;                // kFlagNotFinite: a value is not finite
};

// PSIS-LOO of one sorted column col[0] <= ... <= col[S - 1], by one wave: elpd_loo_i, lppd_i, k in every lane
template <class T>
__device__ inline void psis_column(const T* col, int S, int M, double log_min, int lane, double& elpd, double& lppd, double& khat) {
#pragma clang fp contract(off)
    const double c0 = (double)col[0];                              // min ll = -max(-ll): x_s = c0 - ll_s, the largest at s = 0
    const double cut = fmax(c0 - (double)col[M], log_min), ecut = exp(cut);
    int cnt = 0;
    for (int s = lane; s < M; s += 64) cnt += (c0 - (double)col[s]) > cut ? 1 : 0;
    const int n = wave_all(cnt, [](int a, int b) { return a + b; });     // the tail: s < n; ascending, its j-th value (from 0) is s = n - 1 - j
    double k = INFINITY, sigma = 0.0;
    if (n > kPsisMinTail) {                                        // (uniform over the wave)
        const double dn = (double)n;
        double t[kPsisTailPerLane];
#pragma unroll
        for (int r = 0; r < kPsisTailPerLane; ++r) {
            const int j = lane + 64 * r;
            t[r] = j < n ? exp(c0 - (double)col[n - 1 - j]) - ecut : 0.0;      // (a 0 adds log1p(0) = 0 to a sum)
        }
        const int m = 30 + (int)floor(sqrt(dn));
        const double t_quart = exp(c0 - (double)col[n - (int)floor(dn / 4.0 + 0.5)]) - ecut;     // t[floor(n / 4 + 0.5) - 1]
        const double t_top = exp(c0 - (double)col[0]) - ecut;                                    // t[n - 1]
        double bq = 0.0, kq = 0.0;                                 // lane q - 1 keeps b_q and k_q
        for (int q = 0; q < m; ++q) {
            const double b = (1.0 - sqrt((double)m / ((double)(q + 1) - 0.5))) / (3.0 * t_quart) + 1.0 / t_top;
            double part = 0.0;
#pragma unroll
            for (int r = 0; r < kPsisTailPerLane; ++r) {
                if (64 * r >= n) break;                            // (uniform; the registers past the tail hold 0 and would add 0)
                part += log1p(-b * t[r]);
            }
            const double kk = wave_sum(part) / dn;
            if (lane == q) { bq = b; kq = kk; }
        }
        const bool act = lane < m;
        const double Lq = act ? dn * (log(-bq / kq) - kq - 1.0) : 0.0;
        double den = 0.0;
        for (int r = 0; r < m; ++r) den += exp(__shfl(Lq, r) - Lq);
        double w = act ? 1.0 / den : 0.0;
        if (!(w >= 10.0 * DBL_EPSILON)) w = 0.0;
        w /= wave_sum(w);
        const double b = wave_sum(bq * w);
        double part = 0.0;
#pragma unroll
        for (int r = 0; r < kPsisTailPerLane; ++r) {
            if (64 * r >= n) break;
            part += log1p(-b * t[r]);
        }
        const double kp = wave_sum(part) / dn;
        sigma = -kp / b;
        k = (dn * kp + 5.0) / (dn + 10.0);
    }
    // the log weight of entry s: smoothed inside a fitted tail, x_s elsewhere
    auto lw_at = [&](int s) -> double {
        if (n <= kPsisMinTail || s >= n) return c0 - (double)col[s];
        const double l1 = log1p(-(((double)(n - s) - 0.5) / (double)n));
        const double q = (k == 0.0 ? -sigma * l1 : sigma * expm1(-k * l1) / k) + ecut;
        return fmin(log(q), 0.0);
    };
    double m_w = -INFINITY, m_a = -INFINITY;
    for (int s = lane; s < S; s += 64) {
        const double lw = lw_at(s);
        m_w = fmax(m_w, lw);
        m_a = fmax(m_a, lw + (double)col[s]);
    }
    m_w = wave_max(m_w);
    m_a = wave_max(m_a);
    const double top = (double)col[S - 1];
    double s_w = 0.0, s_a = 0.0, s_p = 0.0;
    for (int s = lane; s < S; s += 64) {
        const double lw = lw_at(s), ll = (double)col[s];
        s_w += exp(lw - m_w);
        s_a += exp((lw + ll) - m_a);
        s_p += exp(ll - top);
    }
    s_w = wave_sum(s_w);
    s_a = wave_sum(s_a);
    s_p = wave_sum(s_p);
    elpd = (m_a + log(s_a)) - (m_w + log(s_w));
    lppd = (top + log(s_p)) - log((double)S);
    khat = k;
}

template <class T>
__global__ __launch_bounds__(kStackThreads) void psis_kernel(PsisParams p) {
    extern __shared__ __align__(16) unsigned char psis_lds[];
    T* sh = reinterpret_cast<T*>(psis_lds);
    const int pitch = p.P + 1;
    const long long c0 = (long long)blockIdx.x * p.tile;
    const int tc = (int)min((long long)p.tile, p.n_cols - c0);

    // ---- the tile into LDS columns; +inf past S
    if (load_stack_tile<1, true, true>(sh, static_cast<const T*>(p.values), (const T*)nullptr, p.col_stride, p.S, p.P, (T)INFINITY, p.tile,
                                       p.log2tile, tc, pitch, [c0](int c) { return c0 + c; }))
        atomicOr(p.flag, kFlagNotFinite);

    // ---- bitonic sort of every column, ascending (P >= 2: S >= 2)
    const int log2half = p.log2P - 1;
    const int n_pairs = tc << log2half;
    for (int k = 2; k <= p.P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < n_pairs; t += kStackThreads) {
                const int c = t >> log2half, q = t & ((1 << log2half) - 1);
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
                T* col = sh + c * pitch;
                const T a = col[i], b = col[i + j];
                if ((a > b) == ((i & k) == 0)) {
                    col[i] = b;
                    col[i + j] = a;
                }
            }
        }
    }
    __syncthreads();

    // ---- per column (one wave each)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < tc; c += kStackWaves) {
        double elpd, lppd, khat;
        psis_column(sh + c * pitch, p.S, p.M, p.log_min, lane, elpd, lppd, khat);
        if (lane == 0) {
            p.elpd[c0 + c] = elpd;
            p.lppd[c0 + c] = lppd;
            p.k[c0 + c] = khat;
        }
    }
}

// psis_kernel over n_cols columns of the device array `values` (T = float or double); elpd / lppd / k device arrays [n_cols].  The
// kernel is enqueued on `stream`; it raises kFlagNotFinite in `flag` (zeroed by the caller in stream order): the caller reads it.
template <class T>
int launch_psis(npbnn_ctx* ctx, hipStream_t stream, const void* values, long long S, long long n_cols, long long col_stride, double* elpd,
                double* lppd, double* k, int* flag) {
    PsisParams p{};
    p.values = values;
    p.n_cols = n_cols;
    p.col_stride = col_stride;
    p.S = (int)S;
    for (p.P = 1; p.P < S; p.P *= 2) ++p.log2P;       // (the smallest power of two >= S)
    p.M = (int)ceil(fmin((double)S / 5.0, 3.0 * sqrt((double)S)));
    p.log_min = log(DBL_MIN);
    p.elpd = elpd;
    p.lppd = lppd;
    p.k = k;
    p.flag = flag;
    return launch_stack_kernel(ctx, stream, reinterpret_cast<const void*>(psis_kernel<T>), nullptr, (size_t)(p.P + 1) * sizeof(T), p);
}

int check_psis_samples(npbnn_ctx* ctx, const char* who, long long S) {
    if (S < 2) return fail(ctx, NPBNN_E_ARG, "%s: %lld samples, leave-one-out importance sampling needs at least 2", who, S);
    if (S > kStackMaxSamples) return fail(ctx, NPBNN_E_ARG, "%s: %lld samples, at most %d", who, S, kStackMaxSamples);
    return NPBNN_OK;
}

// What loo_log_lik_kernel needs beside a group's values, all on the device (LppdArgs of npbnn_lppd.hip, and the matrix)
struct LooArgs {
    const int* labels = nullptr;      // [n_rows] (categorical)
    const float* targets = nullptr;   // [n_rows][C] (Gaussian)
    const double* lconst = nullptr;   // [n_sets][C] -0.5 log(2 pi) - log(sigma) (Gaussian)
    const double* isigma = nullptr;   // [n_sets][C] 1 / sigma (Gaussian)
    double* part = nullptr;           // [n_sets][n_wg]: every workgroup's sum of its rows' ll under a set
    double* ll = nullptr;             // [n_sets][n_rows]
    int n_wg = 0;
};

// A group's values y [g][n_rows][C] into ll[s0 + j][r], one thread per row: lppd_accumulate_kernel's terms in its order, its label
// and NaN checks, and its per-sample partials.  GAUSS: the likelihood is Gaussian (else categorical).  VEC: C is a multiple of 4.
template <bool GAUSS, bool VEC>
__global__ __launch_bounds__(kFiThreads) void loo_log_lik_kernel(const float* __restrict__ y, int g, int s0, long long n_rows, int C, LooArgs a,
                                                                 int* __restrict__ flag) {
    __shared__ double red[kFiWaves];
    bool nan = false, bad = false;
    const long long per_set = n_rows * C;
    double tot[kMaxCand];
#pragma unroll
    for (int j = 0; j < kMaxCand; ++j) tot[j] = 0.0;
    for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads) {
        int lab = 0;
        if (!GAUSS) {
            lab = a.labels[r];
            if (lab < 0 || lab >= C) { bad = true; continue; }
        }
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
            a.ll[(long long)(s0 + j) * n_rows + r] = ll;
        }
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

void loo_log_lik(hipStream_t st, bool gauss, const float* y, int g, int s0, long long n_rows, int C, const LooArgs& a, int* d_flag) {
    const dim3 grid((unsigned)a.n_wg), block(kFiThreads);
    const bool vec = C % 4 == 0;
    if (gauss) {
        if (vec) hipLaunchKernelGGL((loo_log_lik_kernel<true, true>), grid, block, 0, st, y, g, s0, n_rows, C, a, d_flag);
        else hipLaunchKernelGGL((loo_log_lik_kernel<true, false>), grid, block, 0, st, y, g, s0, n_rows, C, a, d_flag);
    } else {
        if (vec) hipLaunchKernelGGL((loo_log_lik_kernel<false, true>), grid, block, 0, st, y, g, s0, n_rows, C, a, d_flag);
        else hipLaunchKernelGGL((loo_log_lik_kernel<false, false>), grid, block, 0, st, y, g, s0, n_rows, C, a, d_flag);
    }
}

}  // namespace

}  // namespace npbnn_api

using namespace npbnn_api;

extern "C" int npbnn_op_psis(int device, const void* values, int value_type, int64_t n_samples, int64_t n_cols, int64_t col_stride,
                             double* out_elpd, double* out_lppd, double* out_k) {
    const char* who = "op_psis";
    StackInput in(value_type);
    if (!values || !out_elpd || !out_lppd || !out_k || n_cols < 0 || col_stride < n_cols || !in.ok())
        return fail(nullptr, NPBNN_E_ARG, "%s: bad arguments", who);
    int rc = check_psis_samples(nullptr, who, n_samples);
    if (rc) return rc;
    if (n_cols == 0) return NPBNN_OK;
    HIP_TRY(nullptr, hipSetDevice(device));
    DevBuf<double> d_res;
    DevBuf<int> d_flag;
    if ((rc = in.upload(values, n_samples, n_cols, col_stride))) return rc;
    if ((rc = dev_alloc(nullptr, d_res, 3 * (size_t)n_cols))) return rc;
    if ((rc = dev_alloc(nullptr, d_flag, 1))) return rc;
    HIP_TRY(nullptr, hipMemset(d_flag.get(), 0, sizeof(int)));
    double* elpd = d_res.get();
    double* lppd = elpd + n_cols;
    double* k = lppd + n_cols;
    if (in.f32()) rc = launch_psis<float>(nullptr, nullptr, in.buf.get(), n_samples, n_cols, col_stride, elpd, lppd, k, d_flag.get());
    else rc = launch_psis<double>(nullptr, nullptr, in.buf.get(), n_samples, n_cols, col_stride, elpd, lppd, k, d_flag.get());
    if (rc) return rc;
    int bad = 0;
    HIP_TRY(nullptr, hipMemcpy(&bad, d_flag.get(), sizeof(int), hipMemcpyDeviceToHost));
    if (bad) return fail(nullptr, NPBNN_E_ARG, "%s: a value is NaN or infinite", who);
    HIP_TRY(nullptr, hipMemcpy(out_elpd, elpd, (size_t)n_cols * 8, hipMemcpyDeviceToHost));
    HIP_TRY(nullptr, hipMemcpy(out_lppd, lppd, (size_t)n_cols * 8, hipMemcpyDeviceToHost));
    HIP_TRY(nullptr, hipMemcpy(out_k, k, (size_t)n_cols * 8, hipMemcpyDeviceToHost));
    return NPBNN_OK;
}

extern "C" int npbnn_predict_sets_loo(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which, int lik_kind,
                                      const double* sigma_sets, double* out_elpd, double* out_lppd, double* out_k, double* out_log_lik_sample,
                                      double* out_log_lik) {
    const char* who = "predict_sets_loo";
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    ctx->fi_ns[1] = ctx->fi_ns[2] = ctx->loo_ns = 0;         // (a call that is refused has launched nothing)
    if (!W_sets || !out_elpd || !out_lppd || !out_k) return fail(ctx, NPBNN_E_ARG, "%s: bad arguments", who);
    if (lik_kind == NPBNN_LIK_GAUSS_PRED_SIGMA || lik_kind == NPBNN_LIK_POISSON || lik_kind == NPBNN_LIK_NEGBIN || lik_kind == NPBNN_LIK_NEGBIN2D ||
        lik_kind == NPBNN_LIK_NEGBIN_BASE10)
        return fail(ctx, NPBNN_E_ARG, "%s: predicted-sigma regression and the count likelihoods are out of scope (likelihood kind %d); "
                    "NPBNN_LIK_CATEGORICAL and NPBNN_LIK_GAUSS are served", who, lik_kind);
    if (lik_kind != NPBNN_LIK_CATEGORICAL && lik_kind != NPBNN_LIK_GAUSS)
        return fail(ctx, NPBNN_E_ARG, "%s: lik_kind must be NPBNN_LIK_CATEGORICAL or NPBNN_LIK_GAUSS, got %d", who, lik_kind);
    const bool gauss = lik_kind == NPBNN_LIK_GAUSS;
    if (gauss != (sigma_sets != nullptr)) return fail(ctx, NPBNN_E_ARG, "%s: sigma_sets goes with NPBNN_LIK_GAUSS and with nothing else", who);
    int rc = check_psis_samples(ctx, who, n_sets);
    if (rc) return rc;
    SetsTable tb;
    if ((rc = open_sets_table(ctx, who, which, &tb))) return rc;
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
    if ((rc = check_stack_budget(ctx, who, n_sets, n_rows, 1, sizeof(double), "float64"))) return rc;
    hipStream_t st = tb.st;
    const int n_wg = tb.n_wg;
    // the matrix [n_sets][n_rows], the three pointwise results, the partials [n_sets][n_wg], the sigma terms [lconst | isigma], the flag word
    DevBuf<double> d_ll, d_res, d_part, d_sig;
    DevBuf<int> d_flag;
    if ((rc = dev_alloc(ctx, d_ll, (size_t)n_sets * n_rows))) return rc;
    if ((rc = dev_alloc(ctx, d_res, 3 * (size_t)n_rows))) return rc;
    if ((rc = dev_alloc(ctx, d_part, (size_t)n_sets * n_wg))) return rc;
    if ((rc = dev_alloc(ctx, d_flag, 4))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_flag.get(), 0, sizeof(int), st));
    LooArgs a;
    a.part = d_part.get();
    a.ll = d_ll.get();
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
        if ((rc = dev_alloc(ctx, d_sig, 2 * n))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(d_sig.get(), h_sig.data(), 2 * n * sizeof(double), hipMemcpyHostToDevice, st));
        a.targets = d.targets.get();
        a.lconst = d_sig.get();
        a.isigma = d_sig.get() + n;
    } else {
        a.labels = d.labels.get();
        if ((rc = check_labels_on_device(ctx, who, d.labels.get(), n_rows, C, d_flag.get()))) return rc;
    }
    rc = replay_sets(ctx, who, W_sets, act_prm_sets, n_sets, which, 0, nullptr, [&](const SetGroup& grp) {
        loo_log_lik(st, gauss, grp.y, grp.g, grp.s0, n_rows, C, a, d_flag.get());
        return NPBNN_OK;
    });
    if (rc) return rc;
    FiTimer tm;
    tm.mark(0, st);
    double* elpd = d_res.get();
    double* lppd = elpd + n_rows;
    double* k = lppd + n_rows;
    if ((rc = launch_psis<double>(ctx, st, d_ll.get(), n_sets, n_rows, n_rows, elpd, lppd, k, d_flag.get()))) return rc;
    tm.mark(1, st);
    int flags = 0;
    std::vector<double> sums;          // every set's ll total
    if ((rc = fetch_flags_and_totals(ctx, d_flag.get(), d_part.get(), (size_t)n_sets, n_wg, &flags, &sums))) return rc;
    ctx->loo_ns = tm.ns(0, 1);
    if (flags & kFlagNaN) return fail(ctx, NPBNN_E_ARG, "%s: a prediction is NaN", who);
    if (flags & kFlagBadLabel) return fail(ctx, NPBNN_E_ARG, "%s: a label lies outside [0, %d)", who, C);
    if (flags & kFlagNotFinite) return fail(ctx, NPBNN_E_ARG, "%s: a log-likelihood is not finite", who);
    if (out_log_lik_sample) memcpy(out_log_lik_sample, sums.data(), (size_t)n_sets * sizeof(double));
    HIP_TRY(ctx, hipMemcpyAsync(out_elpd, elpd, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_lppd, lppd, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_k, k, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out_log_lik) HIP_TRY(ctx, hipMemcpyAsync(out_log_lik, d_ll.get(), (size_t)n_sets * n_rows * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return NPBNN_OK;
}
