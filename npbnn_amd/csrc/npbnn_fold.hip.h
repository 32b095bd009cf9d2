// What the entries that fold a group's float32 pre-output values into float64 per-row accumulators share (npbnn_lppd.hip,
// npbnn_uncertainty.hip, npbnn_calibration.hip): softplus and sum exp(z - max) in float64, the fold of the softmax probabilities (with
// or without the entropy term), and the check of the labels before anything is launched.  The moment folds and the regression row
// loaders stay in their units: they differ in what they accumulate and in how they read.  Not part of the ABI.
//
// Floating-point contraction.  A header is compiled under the including unit's default contraction, whatever pragma follows the
// include (npbnn_sets.hip.h), and npbnn_lppd.hip leaves contraction on: its Gaussian term is fused today and stays so.  A file-scope
// pragma here would reach it.  So every function of this header in which a product feeds a sum carries
// `#pragma clang fp contract(off)` as the first statement of its body; the pragma holds through inlining (the entropy term compiles
// to a multiply and an add from a unit at the default setting, to one fused multiply-add without it).  A function without such a
// product needs none.
#pragma once
#include "npbnn_sets.hip.h"

namespace npbnn_api {

// softplus as np.logaddexp(0, z) (RegressTransformError): max(z, 0) + log1p(exp(-|z|))
__device__ inline double softplus_f64(double z) { return fmax(z, 0.0) + log1p(exp(-fabs(z))); }

// sum_k exp(z[k] - mx), in class order
template <bool VEC>
__device__ inline double row_sum_exp(const float* __restrict__ row, int C, double mx) {
    double s = 0.0;
    if (VEC) {
        for (int k = 0; k < C; k += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + k);
#pragma unroll
            for (int q = 0; q < 4; ++q) s += exp((double)v[q] - mx);
        }
    } else {
        for (int k = 0; k < C; ++k) s += exp((double)row[k] - mx);
    }
    return s;
}

// Softmax output: the probabilities of a group's sets onto the per-class sums, one thread per row, the sets in set order.
// y [g][n_rows][C]; acc [C][n_rows]: sum_s softmax(z_s)_k, and with ENTROPY one row more, acc[C][n_rows]: sum_s H(p_s),
// H = lse(z) - sum_k p_k z_k = log(sum) - sum exp(z - max) (z - max) / sum, never log(softmax): a probability that underflows
// contributes 0.  The row is read for its maximum, again for sum exp(z - max), and a third time class by class, adding
// exp(z - max) / sum to the class's accumulator: no class count needs a register array or scratch (the later reads hit the cache).
// No sum is reassociated and no product fused into a sum, so a set folded alone and a set folded as the second of a group leave the
// same bits.  VEC: C is a multiple of 4, rows are read as float4.
template <bool ENTROPY, bool VEC>
__global__ __launch_bounds__(kFiThreads) void softmax_mean_accumulate_kernel(const float* __restrict__ y, int g, int s0, long long n_rows, int C,
                                                                             double* __restrict__ acc, int* __restrict__ flag) {
#pragma clang fp contract(off)
    bool nan = false;
    const long long per_set = n_rows * C;
    for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads) {
        double mx[kMaxCand], se[kMaxCand];
        double h = 0.0;
        if (ENTROPY) h = s0 > 0 ? acc[(long long)C * n_rows + r] : 0.0;
#pragma unroll
        for (int j = 0; j < kMaxCand; ++j) {
            mx[j] = 0.0;
            se[j] = 1.0;
            if (j >= g) continue;
            const float* row = y + (long long)j * per_set + r * C;
            const double m = row_max<VEC>(row, C, nan);
            double e;                                 // sum exp(z - m), in class order
            if (ENTROPY) {
                double ez = 0.0;                      // sum exp(z - m) (z - m), in class order
                e = 0.0;
                if (VEC) {
                    for (int k = 0; k < C; k += 4) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(row + k);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const double d = (double)v[q] - m, x = exp(d);
                            e += x;
                            ez += x * d;
                        }
                    }
                } else {
                    for (int k = 0; k < C; ++k) {
                        const double d = (double)row[k] - m, x = exp(d);
                        e += x;
                        ez += x * d;
                    }
                }
                const double hs = log(e) - ez / e;    // lse(z) - sum_k p_k z_k, both shifted by m
                nan = nan || (hs != hs);
                h += hs;
            } else {
                e = row_sum_exp<VEC>(row, C, m);
                nan = nan || (e != e);
            }
            mx[j] = m;
            se[j] = e;
        }
        if (ENTROPY) acc[(long long)C * n_rows + r] = h;
        // class by class: the group's probabilities onto the class's sum, in set order
        if (VEC) {
            for (int k = 0; k < C; k += 4) {
                double a[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] = s0 > 0 ? acc[(long long)(k + q) * n_rows + r] : 0.0;
#pragma unroll
                for (int j = 0; j < kMaxCand; ++j) {
                    if (j >= g) continue;
                    const f32x4 v = *reinterpret_cast<const f32x4*>(y + (long long)j * per_set + r * C + k);
#pragma unroll
                    for (int q = 0; q < 4; ++q) a[q] += exp((double)v[q] - mx[j]) / se[j];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[(long long)(k + q) * n_rows + r] = a[q];
            }
        } else {
            for (int k = 0; k < C; ++k) {
                double a = s0 > 0 ? acc[(long long)k * n_rows + r] : 0.0;
#pragma unroll
                for (int j = 0; j < kMaxCand; ++j) {
                    if (j >= g) continue;
                    a += exp((double)y[(long long)j * per_set + r * C + k] - mx[j]) / se[j];
                }
                acc[(long long)k * n_rows + r] = a;
            }
        }
    }
    if (nan) atomicOr(flag, kFlagNaN);
}

// softmax_mean_accumulate_kernel over a group's values y [g][n_rows][C], the sets s0 .. s0 + g - 1, on n_wg workgroups.  ENTROPY is a
// template argument, so that a unit builds the two kernels it launches and not the other unit's.
template <bool ENTROPY>
inline void launch_softmax_mean_accumulate(hipStream_t st, const float* y, int g, int s0, long long n_rows, int C, double* d_acc, int n_wg, int* d_flag) {
    const dim3 grid((unsigned)n_wg), block(kFiThreads);
    if (C % 4 == 0) hipLaunchKernelGGL((softmax_mean_accumulate_kernel<ENTROPY, true>), grid, block, 0, st, y, g, s0, n_rows, C, d_acc, d_flag);
    else hipLaunchKernelGGL((softmax_mean_accumulate_kernel<ENTROPY, false>), grid, block, 0, st, y, g, s0, n_rows, C, d_acc, d_flag);
}

// labels outside [0, C): found before any evaluation is launched
static __global__ __launch_bounds__(kFiThreads) void label_check_kernel(const int* __restrict__ labels, long long n_rows, int C, int* __restrict__ flag) {
    bool bad = false;
    for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads) {
        const int v = labels[r];
        if (v < 0 || v >= C) bad = true;
    }
    if (bad) atomicOr(flag, kFlagBadLabel);
}

// label_check_kernel on ctx->stream and its answer: NPBNN_E_ARG when a label lies outside [0, C).  d_flag is the entry's flag word,
// zeroed in stream order; the stream is synchronised.
inline int check_labels_on_device(npbnn_ctx* ctx, const char* who, const int* d_labels, long long n_rows, int C, int* d_flag) {
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(label_check_kernel, dim3(grid_for(n_rows)), dim3(kFiThreads), 0, st, d_labels, n_rows, C, d_flag);
    HIP_TRY(ctx, hipGetLastError());
    int bad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (bad) return fail(ctx, NPBNN_E_ARG, "%s: a label lies outside [0, %d)", who, C);
    return NPBNN_OK;
}

}  // namespace npbnn_api
