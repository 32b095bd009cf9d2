// What the column kernels over a sample stack [S][n_cols] share (npbnn_hpd.hip, npbnn_convergence.hip, npbnn_predictive.hip): the tile
// rule (npbnn_stack_plan.h), the wave reductions, the loader of a tile into LDS, the launch, the owner of an npbnn_op_* input and the
// replay of stored sets into a device stack.  The flag word is the caller's: the launch only enqueues, the caller reads the word and
// refuses.  Compiled under each unit's default contraction, as npbnn_sets.hip.h is: no product feeds a sum here.  Not part of the ABI.
#pragma once
#include "npbnn_sets.hip.h"
#include "npbnn_stack_plan.h"

namespace npbnn_api {

// f over v of every lane of the wave by a fixed xor butterfly: the same bits in every lane
template <class T, class F>
__device__ inline T wave_all(T v, F f) {
    for (int off = 32; off > 0; off >>= 1) v = f(v, __shfl_xor(v, off));
    return v;
}
__device__ inline double wave_sum(double v) { return wave_all(v, [](double a, double b) { return a + b; }); }
__device__ inline double wave_min(double v) { return wave_all(v, [](double a, double b) { return fmin(a, b); }); }
__device__ inline double wave_max(double v) { return wave_all(v, [](double a, double b) { return fmax(a, b); }); }
__device__ inline int wave_or(int v) { return wave_all(v, [](int a, int b) { return a | b; }); }

// The workgroup's tile of tc <= tile columns into LDS, sample row by sample row (a row of the tile is one coalesced read where its
// columns are adjacent): sh[c * pitch + s] = g[s * col_stride + at(c)] for s < S, and with PAD `pad` for S <= s < fill and in the
// columns past tc (fill == S without it).  PLANES == 2: g2's values likewise, behind the tile's first plane.  Returns whether a value
// this thread loaded is not finite, looked at with CHECK only.  Every thread of the workgroup calls it; no barrier.
template <int PLANES, bool PAD, bool CHECK, class T, class At>
__device__ inline bool load_stack_tile(T* sh, const T* g, const T* g2, long long col_stride, int S, int fill, T pad, int tile, int log2tile,
                                       int tc, int pitch, At at) {
    T* sh2 = sh + (long long)tile * pitch;
    bool bad = false;
    for (int i = threadIdx.x; i < (fill << log2tile); i += kStackThreads) {
        const int s = i >> log2tile, c = i & (tile - 1);
        const bool in = c < tc && (!PAD || s < S);
        if (!PAD && !in) continue;
        T v = pad;
        if (in) {
            const long long j = (long long)s * col_stride + at(c);
            v = g[j];
            if (CHECK && !isfinite(v)) bad = true;
            if (PLANES == 2) sh2[c * pitch + s] = g2[j];
        }
        sh[c * pitch + s] = v;
    }
    return bad;
}

// One kernel over the p.n_cols columns of p, enqueued on `stream`: the tile by the plan for columns of col_bytes staged bytes (into
// p.tile, p.log2tile); `staged` where the tile goes into LDS, `unstaged` where a single column does not (nullptr from HPD and
// convergence, whose widest column fits).
static_assert((kStackMaxSamples + 1) * 8 <= kMixMaxLds, "one plane of kStackMaxSamples float64 values and its pitch fits");
template <class P>
int launch_stack_kernel(npbnn_ctx* ctx, hipStream_t stream, const void* staged, const void* unstaged, size_t col_bytes, P p) {
    const npbnn_stack_tile t = npbnn_stack_tile_of((long long)col_bytes, p.n_cols, kMixMaxLds);
    p.tile = t.tile;
    p.log2tile = t.log2tile;
    const void* fn = t.staged ? staged : unstaged;
    if (t.lds_bytes > 0) HIP_TRY(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds_bytes));
    void* args[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel(fn, dim3((unsigned)t.blocks), dim3(kStackThreads), args, (size_t)t.lds_bytes, stream));
    HIP_TRY(ctx, hipGetLastError());
    return NPBNN_OK;
}

// The values of an npbnn_op_* call on the device: n_samples rows of col_stride float32 or float64 values, the last one n_cols long.
struct StackInput {
    explicit StackInput(int value_type) : type(value_type) {}
    bool ok() const { return type == NPBNN_VALUE_F64 || type == NPBNN_VALUE_F32; }
    bool f32() const { return type == NPBNN_VALUE_F32; }
    int upload(const void* values, int64_t n_samples, int64_t n_cols, int64_t col_stride) {
        const size_t bytes = ((size_t)(n_samples - 1) * (size_t)col_stride + (size_t)n_cols) * (f32() ? 4 : 8);
        if (int rc = dev_alloc(nullptr, buf, (bytes + 7) / 8)) return rc;      // (rounded up to whole doubles)
        HIP_TRY(nullptr, hipMemcpy(buf.get(), values, bytes, hipMemcpyHostToDevice));
        return NPBNN_OK;
    }
    int type;
    DevBuf<double> buf;
};

// NPBNN_E_NOMEM through fail(ctx, ...) when a device array [n_sets][n_rows][C] of elem_bytes-wide `type` values is over the byte
// budget of a stack (1 GiB, or NPBNN_HPD_STACK_BYTES from the environment); the message names the largest row count that fits.
int check_stack_budget(npbnn_ctx* ctx, const char* who, int n_sets, long long n_rows, int C, size_t elem_bytes = sizeof(float),
                       const char* type = "float32");

// The sets replayed (replay_sets) into *stack, [n_sets][t.n_rows][outputs] float32 on the device, allocated here.  NPBNN_E_NOMEM
// through fail(ctx, ...) before anything is allocated when the stack is over its byte budget (check_stack_budget, npbnn_sets.hip:
// 1 GiB, or NPBNN_HPD_STACK_BYTES from the environment); the message names the largest row count that fits.
int replay_into_stack(npbnn_ctx* ctx, const char* who, const double* W_sets, const double* act_prm_sets, int n_sets, int which, int apply_out_fn,
                      const SetsTable& t, DevBuf<float>* stack);

}  // namespace npbnn_api
