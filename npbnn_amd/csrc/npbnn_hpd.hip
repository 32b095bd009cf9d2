// Highest-posterior-density intervals (include/npbnn_hip.h): calcHPD of np_bnn/BNN_lib.py:286-302 over many columns at once.
//
// calcHPD sorts one vector of S values, takes nIn = round(level * S) of them (round half to even: nearbyint under the default
// rounding mode) and returns the first window d[k] .. d[k + nIn - 1] of smallest width (a later window replaces the best only when
// strictly narrower).  hpd_kernel gives each workgroup a tile of TC adjacent columns (the tile rule, the loader and the launch are
// the stack column kernels' shared ones, npbnn_stack.hip.h): the tile goes into LDS as TC columns of P = next power of two >= S
// values (padded with +inf, column pitch P + 1 against bank conflicts) and is sorted there by a bitonic network.
// Each wave then scans the windows of its columns - widths in W, the input's type for npbnn_op_hpd and float64 for the float32
// stack of npbnn_predict_sets_hpd - and a shuffle reduction picks the smallest width, the smallest k among equal ones.  The mean
// (float64 sum in a fixed order) comes from the same LDS copy.  No atomics but the non-finite flag, no scratch.
//
// npbnn_predict_sets_hpd replays the stored sets through replay_into_stack (npbnn_stack.hip.h), each group writing its float32
// predictions straight into a device stack [S][rows][C]; one launch of hpd_kernel then reads the stack once.
#include "npbnn_stack.hip.h"

#include <cmath>

namespace npbnn_api {

namespace {

struct HpdParams {
    const void* values;       // values[s * col_stride + c]
    long long n_cols, col_stride;
    int S, P, log2P, n_in, tile, log2tile;
    double* lo;
    double* hi;
    double* mean;             // or nullptr
    int* flag;                // bit 0: a value is not finite
};

template <class T, class W>
__global__ __launch_bounds__(kStackThreads) void hpd_kernel(HpdParams p) {
    extern __shared__ __align__(16) unsigned char hpd_lds[];
    T* sh = reinterpret_cast<T*>(hpd_lds);
    const int pitch = p.P + 1;
    const long long c0 = (long long)blockIdx.x * p.tile;
    const int tc = (int)min((long long)p.tile, p.n_cols - c0);

    // ---- the tile into LDS columns; +inf past S
    if (load_stack_tile<1, true, true>(sh, static_cast<const T*>(p.values), (const T*)nullptr, p.col_stride, p.S, p.P, (T)INFINITY, p.tile,
                                       p.log2tile, tc, pitch, [c0](int c) { return c0 + c; }))
        atomicOr(p.flag, 1);

    // ---- bitonic sort of every column, ascending
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

    // ---- per column (one wave each): the first narrowest window, and the mean
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = p.S - p.n_in + 1;
    for (int c = wave; c < tc; c += kStackWaves) {
        const T* col = sh + c * pitch;
        W best = (W)0;
        int bk = -1;
        for (int k = lane; k < m; k += 64) {
            const W w = (W)col[k + p.n_in - 1] - (W)col[k];
            if (bk < 0 || w < best) { best = w; bk = k; }
        }
        double sum = 0.0;
        if (p.mean)
            for (int s = lane; s < p.S; s += 64) sum += (double)col[s];
        for (int off = 32; off > 0; off >>= 1) {
            const W ob = __shfl_xor(best, off);
            const int ok = __shfl_xor(bk, off);
            if (ok >= 0 && (bk < 0 || ob < best || (ob == best && ok < bk))) { best = ob; bk = ok; }
        }
        sum = wave_sum(sum);
        if (lane == 0) {
            p.lo[c0 + c] = (double)col[bk];
            p.hi[c0 + c] = (double)col[bk + p.n_in - 1];
            if (p.mean) p.mean[c0 + c] = sum / (double)p.S;
        }
    }
}

// nIn of calcHPD, or an error through fail(ctx, ...)
int hpd_window(npbnn_ctx* ctx, const char* who, long long S, double level, int* n_in) {
    if (!(level > 0.0 && level < 1.0)) return fail(ctx, NPBNN_E_ARG, "%s: level %g outside (0, 1)", who, level);
    if (S > kStackMaxSamples) return fail(ctx, NPBNN_E_ARG, "%s: %lld samples, at most %d", who, S, kStackMaxSamples);
    const double r = nearbyint(level * (double)S);
    if (r < 2.0) return fail(ctx, NPBNN_E_ARG, "%s: too little data to calculate marginal parameters (round(%g * %lld) < 2)", who, level, S);
    *n_in = (int)r;
    return NPBNN_OK;
}

// hpd_kernel over n_cols columns of the device array `values` (T = float or double, widths in W); lo / hi / mean device arrays
// [n_cols].  The kernel is enqueued on `stream` and `flag` (zeroed here) raised when a value is not finite: the caller reads it.
template <class T, class W>
int launch_hpd(npbnn_ctx* ctx, hipStream_t stream, const void* values, long long S, long long n_cols, long long col_stride, int n_in, double* lo,
               double* hi, double* mean, int* flag) {
    HpdParams p{};
    p.values = values;
    p.n_cols = n_cols;
    p.col_stride = col_stride;
    p.S = (int)S;
    for (p.P = 1; p.P < S; p.P *= 2) ++p.log2P;       // (the smallest power of two >= S)
    p.n_in = n_in;
    p.lo = lo;
    p.hi = hi;
    p.mean = mean;
    p.flag = flag;
    HIP_TRY(ctx, hipMemsetAsync(flag, 0, sizeof(int), stream));
    return launch_stack_kernel(ctx, stream, reinterpret_cast<const void*>(hpd_kernel<T, W>), nullptr, (size_t)(p.P + 1) * sizeof(T), p);
}

}  // namespace

}  // namespace npbnn_api

using namespace npbnn_api;

extern "C" int npbnn_op_hpd(int device, const void* values, int value_type, int64_t n_samples, int64_t n_cols, int64_t col_stride,
                            double level, double* out_lo, double* out_hi) {
    StackInput in(value_type);
    if (!values || !out_lo || !out_hi || n_cols < 0 || col_stride < n_cols || n_samples < 1 || !in.ok())
        return fail(nullptr, NPBNN_E_ARG, "op_hpd: bad arguments");
    int n_in = 0;
    int rc = hpd_window(nullptr, "op_hpd", n_samples, level, &n_in);
    if (rc) return rc;
    if (n_cols == 0) return NPBNN_OK;
    HIP_TRY(nullptr, hipSetDevice(device));
    DevBuf<double> d_res;
    DevBuf<int> d_flag;
    if ((rc = in.upload(values, n_samples, n_cols, col_stride))) return rc;
    if ((rc = dev_alloc(nullptr, d_res, 2 * (size_t)n_cols))) return rc;
    if ((rc = dev_alloc(nullptr, d_flag, 1))) return rc;
    double* lo = d_res.get();
    double* hi = lo + n_cols;
    if (in.f32()) rc = launch_hpd<float, float>(nullptr, nullptr, in.buf.get(), n_samples, n_cols, col_stride, n_in, lo, hi, nullptr, d_flag.get());
    else rc = launch_hpd<double, double>(nullptr, nullptr, in.buf.get(), n_samples, n_cols, col_stride, n_in, lo, hi, nullptr, d_flag.get());
    if (rc) return rc;
    int bad = 0;
    HIP_TRY(nullptr, hipMemcpy(&bad, d_flag.get(), sizeof(int), hipMemcpyDeviceToHost));
    if (bad) return fail(nullptr, NPBNN_E_ARG, "op_hpd: a value is NaN or infinite");
    HIP_TRY(nullptr, hipMemcpy(out_lo, lo, (size_t)n_cols * 8, hipMemcpyDeviceToHost));
    HIP_TRY(nullptr, hipMemcpy(out_hi, hi, (size_t)n_cols * 8, hipMemcpyDeviceToHost));
    return NPBNN_OK;
}

extern "C" int npbnn_predict_sets_hpd(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which,
                                      int apply_out_fn, double level, double* out_mean, double* out_lo, double* out_hi) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (!W_sets || !out_mean || !out_lo || !out_hi || n_sets < 1) return fail(ctx, NPBNN_E_ARG, "predict_sets_hpd: bad arguments");
    SetsTable tb;
    int n_in = 0;
    int rc = open_sets_table(ctx, "predict_sets_hpd", which, &tb);
    if (rc || (rc = hpd_window(ctx, "predict_sets_hpd", n_sets, level, &n_in))) return rc;
    const size_t per_set = (size_t)tb.n_rows * ctx->net.n_out;
    DevBuf<float> stack;
    DevBuf<double> d_res;
    DevBuf<int> d_flag;
    if ((rc = replay_into_stack(ctx, "predict_sets_hpd", W_sets, act_prm_sets, n_sets, which, apply_out_fn, tb, &stack))) return rc;
    if ((rc = dev_alloc(ctx, d_res, 3 * per_set))) return rc;
    if ((rc = dev_alloc(ctx, d_flag, 1))) return rc;
    // bounds from the float32 values with float64 widths: upstream's calcHPD on the float64 array npbnn_predict_sets returns
    double* lo = d_res.get();
    double* hi = lo + per_set;
    double* mean = hi + per_set;
    rc = launch_hpd<float, double>(ctx, ctx->stream, stack.get(), n_sets, (long long)per_set, (long long)per_set, n_in, lo, hi, mean, d_flag.get());
    if (rc) return rc;
    int bad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, d_flag.get(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (bad) return fail(ctx, NPBNN_E_ARG, "predict_sets_hpd: a value is NaN or infinite");
    HIP_TRY(ctx, hipMemcpyAsync(out_lo, lo, per_set * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out_hi, hi, per_set * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out_mean, mean, per_set * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NPBNN_OK;
}
