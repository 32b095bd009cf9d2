// Convergence diagnostics in function space (include/npbnn_hip.h: npbnn_op_convergence, npbnn_predict_sets_convergence): split R-hat
// and effective sample size of every column of a sample stack.  A column is M chains of N draws, chain-major (sample s = j * N + t);
// each chain gives two split chains of n = N / 2 draws, its first n and its last n (the middle draw of an odd N is dropped), m = 2 M
// in all.  Per split chain k: mu_k, d = x - mu_k, acov_k(t) = (1/n) sum_{i < n - t} d_i d_{i+t}, s2_k = acov_k(0) n / (n - 1).  Over
// them: W = mean s2_k, Bn = sum (mu_k - mean mu)^2 / (m - 1), varp = W (n - 1) / n + Bn, rhat = sqrt(varp / W),
// rho(t) = 1 - (W - mean_k acov_k(t)) / varp; ess = m n / tau from Geyer's initial monotone sequence of pair sums P_k = rho(2k) +
// rho(2k + 1) (the header has the whole definition).  The reference has no counterpart: it leaves convergence to a trace viewer on
// the logged weights.
//
// convergence_kernel is a stack column kernel (npbnn_stack.hip.h: the tile rule, the loader, the wave sum and the launch it shares
// with hpd_kernel and the mixture kernels): a workgroup takes a tile of adjacent columns and keeps it in LDS in the input's type,
// column pitch S | 1 (odd, against bank conflicts).  Each wave then takes one column at a time.  Pass 1: the split chains' means, one after the other, into the wave's
// LDS slots; pass 2: the centred sums, d formed on the fly from the LDS copy - never sum x^2 - n mu^2.  A lag's sum over all split
// chains is one scan: the lanes stride over the flat index (split chain, i) and a fixed xor butterfly leaves the same bits in every
// lane, so the stop and monotone decisions are wave-uniform.  Lags are scanned in pairs as the sequence asks for them: a column whose
// sequence stops early never pays for the later lags.  All arithmetic is float64, no product is fused into a sum (fp contract off),
// no floating-point atomics, no scratch.  The grid depends on the column count alone.
//
// npbnn_predict_sets_convergence replays the stored sets through replay_into_stack (npbnn_stack.hip.h) into a float32 device stack
// [S][rows][C], as npbnn_predict_sets_hpd does; one launch of convergence_kernel reads it once, and convergence_summary_kernel, one
// workgroup per output, reduces rhat and ess over the rows in a fixed order.
#include "npbnn_stack.hip.h"

#include <cmath>

#pragma clang fp contract(off)

namespace npbnn_api {

namespace {

constexpr int kConvMaxChains = 64;
constexpr int kConvMinDraws = 8;

struct ConvParams {
    const void* values;       // values[s * col_stride + c]
    long long n_cols, col_stride;
    int S, M, N, n, tile, log2tile;
    double* rhat;
    double* ess;
    int* flag;                // bit 0: a value is not finite
};

// where split chain k begins in a column
__device__ inline int split_start(int k, int N, int n) { return (k >> 1) * N + ((k & 1) ? N - n : 0); }

// sum over the split chains k < m and i < n - t of d_{k,i} d_{k,i+t}, t < n
template <class T>
__device__ inline double lag_sum(const T* col, const double* mu, int m, int N, int n, int t, int lane) {
    const int len = n - t;
    int k = 0, i = lane;
    while (i >= len) { i -= len; ++k; }
    double s = 0.0;
    while (k < m) {
        const T* x = col + split_start(k, N, n) + i;
        const double mk = mu[k];
        s += ((double)x[0] - mk) * ((double)x[t] - mk);
        i += 64;
        while (i >= len) { i -= len; ++k; }
    }
    return wave_sum(s);
}

template <class T>
__global__ __launch_bounds__(kStackThreads) void convergence_kernel(ConvParams p) {
    extern __shared__ __align__(16) unsigned char conv_lds[];
    __shared__ double mu_lds[kStackWaves][2 * kConvMaxChains];
    T* sh = reinterpret_cast<T*>(conv_lds);
    const int pitch = p.S | 1;
    const long long c0 = (long long)blockIdx.x * p.tile;
    const int tc = (int)min((long long)p.tile, p.n_cols - c0);

    // ---- the tile into LDS columns
    const bool bad = load_stack_tile<1, false, true>(sh, static_cast<const T*>(p.values), (const T*)nullptr, p.col_stride, p.S, p.S, (T)0, p.tile,
                                                     p.log2tile, tc, pitch, [c0](int c) { return c0 + c; });
    if (bad) atomicOr(p.flag, 1);
    // (a tile with a value that is not finite has no result: the call fails)
    if (__syncthreads_or(bad)) return;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = p.N, n = p.n, m = 2 * p.M;
    const double dn = (double)n, dm = (double)m;
    double* mu = mu_lds[wave];
    for (int c = wave; c < tc; c += kStackWaves) {
        const T* col = sh + c * pitch;
        // pass 1: the split chains' means
        double mu_sum = 0.0;
        for (int k = 0; k < m; ++k) {
            const T* x = col + split_start(k, N, n);
            double s = 0.0;
            for (int i = lane; i < n; i += 64) s += (double)x[i];
            const double mk = wave_sum(s) / dn;
            mu[k] = mk;                                // (every lane holds the same bits and reads back what it wrote itself)
            mu_sum += mk;
        }
        const double mu_all = mu_sum / dm;
        // pass 2: s2_k of every split chain and the spread of the means
        double w_sum = 0.0, b_sum = 0.0;
        for (int k = 0; k < m; ++k) {
            const T* x = col + split_start(k, N, n);
            const double mk = mu[k];
            double s = 0.0;
            for (int i = lane; i < n; i += 64) {
                const double d = (double)x[i] - mk;
                s += d * d;
            }
            w_sum += wave_sum(s) / dn * dn / (dn - 1.0);
            const double e = mk - mu_all;
            b_sum += e * e;
        }
        const double W = w_sum / dm;
        double rhat = NAN, ess = NAN;
        if (W != 0.0) {
            const double Bn = b_sum / (dm - 1.0);
            const double varp = W * (dn - 1.0) / dn + Bn;
            rhat = sqrt(varp / W);
            // rho(t), t >= 1, from one scan
            auto rho = [&](int t) { return 1.0 - (W - lag_sum(col, mu, m, N, n, t, lane) / dn / dm) / varp; };
            double prev = 1.0 + rho(1);
            double sum = prev;
            for (int k = 1; 2 * k + 1 <= n - 1; ++k) {
                const double r0 = rho(2 * k);
                double P = r0 + rho(2 * k + 1);
                if (P < 0.0) break;
                P = fmin(P, prev);
                sum += P;
                prev = P;
            }
            const double tau = fmax(-1.0 + 2.0 * sum, 1.0 / log10(dm * dn));
            ess = dm * dn / tau;
        }
        if (lane == 0) {
            p.rhat[c0 + c] = rhat;
            p.ess[c0 + c] = ess;
        }
    }
}

// Output o of [n_rows][C] columns, one workgroup each: out[o] = {max rhat, min ess, columns with rhat > threshold, constant columns
// (rhat is NaN)}.  NaNs take no part in max / min; both are NaN when every column is constant.
__global__ __launch_bounds__(kFiThreads) void convergence_summary_kernel(const double* __restrict__ rhat, const double* __restrict__ ess, long long n_rows,
                                                                         int C, double threshold, double* __restrict__ out) {
    __shared__ double red[4][kFiWaves];
    const int o = blockIdx.x;
    double mx = -INFINITY, mn = INFINITY, above = 0.0, constant = 0.0;
    for (long long r = threadIdx.x; r < n_rows; r += kFiThreads) {
        const double a = rhat[r * C + o], e = ess[r * C + o];
        if (a != a) constant += 1.0;
        else {
            mx = fmax(mx, a);
            if (a > threshold) above += 1.0;
        }
        if (e == e) mn = fmin(mn, e);
    }
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmax(mx, __shfl_xor(mx, off));
        mn = fmin(mn, __shfl_xor(mn, off));
        above += __shfl_xor(above, off);
        constant += __shfl_xor(constant, off);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = mx; red[1][wave] = mn; red[2][wave] = above; red[3][wave] = constant; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kFiWaves; ++w) {
            mx = fmax(mx, red[0][w]);
            mn = fmin(mn, red[1][w]);
            above += red[2][w];
            constant += red[3][w];
        }
        out[4 * o + 0] = mx == -INFINITY ? NAN : mx;
        out[4 * o + 1] = mn == INFINITY ? NAN : mn;
        out[4 * o + 2] = above;
        out[4 * o + 3] = constant;
    }
}

// the limits of a column, or an error through fail(ctx, ...)
int convergence_shape(npbnn_ctx* ctx, const char* who, long long M, long long N) {
    if (M < 1 || M > kConvMaxChains) return fail(ctx, NPBNN_E_ARG, "%s: %lld chains, 1 to %d", who, M, kConvMaxChains);
    if (N < kConvMinDraws) return fail(ctx, NPBNN_E_ARG, "%s: %lld draws per chain, at least %d", who, N, kConvMinDraws);
    if (M * N > kStackMaxSamples) return fail(ctx, NPBNN_E_ARG, "%s: %lld samples, at most %d", who, M * N, kStackMaxSamples);
    return NPBNN_OK;
}

// convergence_kernel over n_cols columns of the device array `values` (T = float or double); rhat / ess device arrays [n_cols].  The
// kernel is enqueued on `stream` and `flag` (zeroed here) raised when a value is not finite; the caller synchronises and reads it.
template <class T>
int launch_convergence(npbnn_ctx* ctx, hipStream_t stream, const void* values, int M, int N, long long n_cols, long long col_stride, double* rhat,
                       double* ess, int* flag) {
    ConvParams p{};
    p.values = values;
    p.n_cols = n_cols;
    p.col_stride = col_stride;
    p.M = M;
    p.N = N;
    p.S = M * N;
    p.n = N / 2;
    p.rhat = rhat;
    p.ess = ess;
    p.flag = flag;
    HIP_TRY(ctx, hipMemsetAsync(flag, 0, sizeof(int), stream));
    return launch_stack_kernel(ctx, stream, reinterpret_cast<const void*>(convergence_kernel<T>), nullptr, (size_t)(p.S | 1) * sizeof(T), p);
}

}  // namespace

}  // namespace npbnn_api

using namespace npbnn_api;

extern "C" int npbnn_op_convergence(int device, const void* values, int value_type, int32_t n_chains, int32_t n_draws, int64_t n_cols,
                                    int64_t col_stride, double* out_rhat, double* out_ess) {
    StackInput in(value_type);
    if (!values || !out_rhat || !out_ess || n_cols < 0 || col_stride < n_cols || !in.ok())
        return fail(nullptr, NPBNN_E_ARG, "op_convergence: bad arguments");
    int rc = convergence_shape(nullptr, "op_convergence", n_chains, n_draws);
    if (rc) return rc;
    if (n_cols == 0) return NPBNN_OK;
    HIP_TRY(nullptr, hipSetDevice(device));
    DevBuf<double> d_res;
    DevBuf<int> d_flag;
    if ((rc = in.upload(values, (int64_t)n_chains * n_draws, n_cols, col_stride))) return rc;
    if ((rc = dev_alloc(nullptr, d_res, 2 * (size_t)n_cols))) return rc;
    if ((rc = dev_alloc(nullptr, d_flag, 1))) return rc;
    double* rhat = d_res.get();
    double* ess = rhat + n_cols;
    if (in.f32()) rc = launch_convergence<float>(nullptr, nullptr, in.buf.get(), n_chains, n_draws, n_cols, col_stride, rhat, ess, d_flag.get());
    else rc = launch_convergence<double>(nullptr, nullptr, in.buf.get(), n_chains, n_draws, n_cols, col_stride, rhat, ess, d_flag.get());
    if (rc) return rc;
    int bad = 0;
    HIP_TRY(nullptr, hipMemcpy(&bad, d_flag.get(), sizeof(int), hipMemcpyDeviceToHost));
    if (bad) return fail(nullptr, NPBNN_E_ARG, "op_convergence: a value is NaN or infinite");
    HIP_TRY(nullptr, hipMemcpy(out_rhat, rhat, (size_t)n_cols * 8, hipMemcpyDeviceToHost));
    HIP_TRY(nullptr, hipMemcpy(out_ess, ess, (size_t)n_cols * 8, hipMemcpyDeviceToHost));
    return NPBNN_OK;
}

extern "C" int npbnn_predict_sets_convergence(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int32_t n_chains,
                                              int which, int apply_out_fn, double rhat_threshold, double* out_rhat, double* out_ess,
                                              double* out_summary) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    ctx->fi_ns[1] = ctx->fi_ns[2] = ctx->fi_ns[7] = 0;       // (a call that is refused has launched nothing)
    if (!W_sets || !out_summary || n_sets < 1 || n_chains < 1) return fail(ctx, NPBNN_E_ARG, "predict_sets_convergence: bad arguments");
    if (rhat_threshold != rhat_threshold) return fail(ctx, NPBNN_E_ARG, "predict_sets_convergence: the threshold is NaN");
    if (n_sets % n_chains != 0)
        return fail(ctx, NPBNN_E_ARG, "predict_sets_convergence: %d sets do not divide into %d chains of equal length", n_sets, n_chains);
    int rc = convergence_shape(ctx, "predict_sets_convergence", n_chains, n_sets / n_chains);
    if (rc) return rc;
    SetsTable tb;
    if ((rc = open_sets_table(ctx, "predict_sets_convergence", which, &tb))) return rc;
    const int C = ctx->net.n_out;
    const long long n_rows = tb.n_rows;
    const size_t per_set = (size_t)n_rows * C;
    hipStream_t st = tb.st;
    DevBuf<float> stack;
    DevBuf<double> d_res;
    DevBuf<int> d_flag;
    if ((rc = replay_into_stack(ctx, "predict_sets_convergence", W_sets, act_prm_sets, n_sets, which, apply_out_fn, tb, &stack))) return rc;
    if ((rc = dev_alloc(ctx, d_res, 2 * per_set + 4 * (size_t)C))) return rc;
    if ((rc = dev_alloc(ctx, d_flag, 1))) return rc;
    double* rhat = d_res.get();
    double* ess = rhat + per_set;
    double* summary = ess + per_set;
    FiTimer tm;
    tm.mark(0, st);
    if ((rc = launch_convergence<float>(ctx, st, stack.get(), n_chains, n_sets / n_chains, (long long)per_set, (long long)per_set, rhat, ess, d_flag.get())))
        return rc;
    hipLaunchKernelGGL(convergence_summary_kernel, dim3((unsigned)C), dim3(kFiThreads), 0, st, (const double*)rhat, (const double*)ess, n_rows, C,
                       rhat_threshold, summary);
    HIP_TRY(ctx, hipGetLastError());
    tm.mark(1, st);
    int bad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, d_flag.get(), sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_summary, summary, 4 * (size_t)C * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out_rhat) HIP_TRY(ctx, hipMemcpyAsync(out_rhat, rhat, per_set * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out_ess) HIP_TRY(ctx, hipMemcpyAsync(out_ess, ess, per_set * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->fi_ns[7] = tm.ns(0, 1);
    if (bad) return fail(ctx, NPBNN_E_ARG, "predict_sets_convergence: a prediction is NaN or infinite");
    return NPBNN_OK;
}
