// Partial dependence (npbnn_predict_pdp, include/npbnn_hip.h): per grid point and row, the prediction averaged over the stored weight
// sets, with the focal feature columns set to the grid point's values.
//
// Route 1, the grid-batched kernel (networks on the LDS-resident path whose layers are narrow enough): with the focal columns at
// constants v_g, layer 0's pre-activation is X_base W0^T + b0 + sum_f v_g[f] W0[:, f], X_base being X with those columns at 0.  The
// product depends on the set but not on the grid point, so pdp_kernel computes it once per row and set - one read of X per launch
// for every grid point - and each grid point adds its shifted bias (pdp_prep_kernel: float64 sums from the float64 weights, rounded
// once) before the later layers and the output function run in registers.  One thread per row, one workgroup per 256 rows: a row's
// sums over the sets are added in a fixed order by the thread that owns it, so the result is deterministic without atomics.
//
// Route 2, per grid point: the grid values (and data_transform's columns) go into col_override, which the weight pack folds into
// layer 0's bias; the evaluation kernels of npbnn_predict_sets run once per (grid point, group of sets) on either path, and
// pdp_add_kernel adds their predictions into the same accumulator.
//
// Accumulated local effects (npbnn_predict_ale) share both routes: the bin edges take the grid points' place, and a row is evaluated at
// the two edges of its own bin only.  Route 1 (ale_kernel) is pdp_kernel's layer 0 followed by two runs of the later layers per row
// and set; route 2 (ale_pick_kernel) picks each pass's predictions by bin.  Either way the differences are added per (bin, output)
// over a workgroup's rows in row order, then over the workgroups in a fixed order (ale_reduce_kernel), in float64 and without atomics.
//
// Route 1's layer-0 stage, the later layers and the entries' shared host steps (pdp_layer0, pdp_dense, pdp_forward, plan_route,
// upload_sets, Route1Kernel) are in npbnn_route1.hip.h, which npbnn_saliency.hip and npbnn_shapley.hip include too.  The preparation
// of route 1's float32 blocks (pdp_prep_kernel, prepare_route1) is below, for all of them.
#include "npbnn_route1.hip.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace npbnn_api {

namespace {

constexpr size_t kPdpAccBytes = 512ull << 20;    // device budget of the float32 accumulator [grid points][rows][outputs]: larger grids
                                                 // run in chunks of grid points, each chunk one more read of X per set group

// grid point g for set S (and, recursively, the sets after it): shifted bias, later layers, output function, summed into ys
template <int S, int H0P, int NS>
__device__ __forceinline__ void pdp_grid_sets(const PdpParams& p, const float (&z0)[NS][H0P], int g, const float* stail, float (&ys)[kPdpTail]) {
    if constexpr (S < NS) {
        if (S < p.n_set) {
            const float* b = p.bias + ((size_t)(p.set0 + S) * p.n_grid + p.g0 + g) * H0P;
            float h[H0P];
#pragma unroll
            for (int k = 0; k < H0P; ++k) h[k] = z0[S][k] + b[k];
            float y[kPdpTail];
            pdp_forward<H0P>(p, h, stail + (size_t)S * p.tail_floats, p.slopes + (size_t)(p.set0 + S) * kMaxLayers, y);
#pragma unroll
            for (int c = 0; c < kPdpTail; ++c) ys[c] += y[c];
            pdp_grid_sets<S + 1>(p, z0, g, stail, ys);
        }
    }
}

// grid (ceil(n_rows / 256)), block 256, dynamic LDS Fp H0P + n_set tail_floats floats.  NS: sets of one launch whose layer-0 sums a
// thread keeps in registers (NS H0P = 64 floats).
template <int H0P, int NS>
__global__ __launch_bounds__(kPdpRows) void pdp_kernel(const PdpParams p) {
    extern __shared__ float4 pdp_lds[];
    float* stail = reinterpret_cast<float*>(pdp_lds) + (size_t)p.Fp * H0P;
    const int tid = threadIdx.x;
    const long long row = (long long)blockIdx.x * kPdpRows + tid;
    const bool live = row < p.n_rows;
    for (int i = tid; i < p.n_set * p.tail_floats; i += kPdpRows) stail[i] = p.tail[(size_t)p.set0 * p.tail_floats + i];

    float z0[NS][H0P];
    pdp_layer0<0>(p, z0, live, row);
    __syncthreads();      // (the tails of every set are in LDS)
    if (!live) return;

    for (int g = 0; g < p.n_g; ++g) {
        float ys[kPdpTail];
#pragma unroll
        for (int c = 0; c < kPdpTail; ++c) ys[c] = 0.f;
        pdp_grid_sets<0>(p, z0, g, stail, ys);
        float* a = p.acc + ((size_t)g * p.n_rows + row) * p.C;
#pragma unroll
        for (int c = 0; c < kPdpTail; ++c)
            if (c < p.C) a[c] = p.accumulate ? a[c] + ys[c] : ys[c];
    }
}

// grid (n_sets), block 256: a set's float64 weights -> route 1's float32 blocks.  co_all [n_grid][F]: per grid point the constant of
// every overridden column (NaN = the data); the overridden columns are the same for every grid point.
__global__ __launch_bounds__(256) void pdp_prep_kernel(const PdpPrep q, const double* W, const double* co_all, float* w0t, float* bias,
                                                       float* tail) {
    const int s = blockIdx.x;
    const double* w = W + (size_t)s * q.wn;
    const int in0 = q.F + q.hb0;
    float* dw = w0t + (size_t)s * q.Fp * q.H0P;
    for (int i = threadIdx.x; i < q.Fp * q.H0P; i += blockDim.x) {
        const int f = i / q.H0P, h = i % q.H0P;
        float v = 0.f;
        if (f < q.F && h < q.H0 && __builtin_isnan(co_all[f])) v = (float)w[(size_t)h * in0 + q.hb0 + f];
        dw[i] = v;
    }
    float* db = bias + (size_t)s * q.n_grid * q.H0P;
    for (int i = threadIdx.x; i < q.n_grid * q.H0P; i += blockDim.x) {
        const int g = i / q.H0P, h = i % q.H0P;
        double a = 0.0;
        if (h < q.H0) {
            const double* wr = w + (size_t)h * in0;
            const double* co = co_all + (size_t)g * q.F;
            if (q.hb0) a = wr[0];
            for (int f = 0; f < q.F; ++f)
                if (!__builtin_isnan(co[f])) a += co[f] * wr[q.hb0 + f];
        }
        db[i] = (float)a;
    }
    float* dt = tail + (size_t)s * q.tail_floats;
    for (int l = 1; l < q.n_layers; ++l) {
        const int n_out = q.l_out[l], inp = q.t_inp[l], hb = q.l_hb[l], stride = q.l_in[l] + hb, r4 = (n_out + 3) & ~3;
        const double* wl = w + q.l_woff[l];
        for (int i = threadIdx.x; i < r4 + n_out * inp; i += blockDim.x) {
            float v = 0.f;
            if (i < r4) {
                if (i < n_out && hb) v = (float)wl[(size_t)i * stride];
            } else {
                const int j = i - r4, o = j / inp, k = j % inp;
                if (k < q.l_in[l]) v = (float)wl[(size_t)o * stride + hb + k];
            }
            dt[q.t_off[l] + i] = v;
        }
    }
}

// route 2: acc[i] (+)= y[0][i] + ... + y[n - 1][i], i < per_set
__global__ __launch_bounds__(256) void pdp_add_kernel(const float* y, int n, long long per_set, float* acc, int accumulate) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= per_set) return;
    float a = accumulate ? acc[i] : 0.f;
    for (int j = 0; j < n; ++j) a += y[(size_t)j * per_set + i];
    acc[i] = a;
}

// ---- accumulated local effects (npbnn_predict_ale)

constexpr int kAleMaxBins = 1024;
constexpr size_t kAlePartBytes = 256ull << 20;   // device budget of route 1's per-workgroup partials [sets of a launch][workgroups][bins]
                                                 // [outputs] float64: a larger table runs in chunks of workgroups

struct AleParams {
    const int* bin;        // [n_rows]: each row's bin, 1 .. K (ale_bin_kernel)
    double* part;          // [sets of the launch][workgroups of the launch][K][C]
    long long row0;        // first row of the launch
    int K;
    int stride;            // floats between two rows' differences in LDS (odd: the rows' writes fall into different banks)
    int stage_floats;      // LDS floats before the tails: the first-layer image, later the differences and the rows' bins
};

// grid (ceil(n_rows / 256)), block 256: bin[row] = the smallest k in 1 .. K with X[row][col] <= edges[k], K when there is none
// (float32 against float32), and counts[k - 1] += the rows of bin k.  Integer atomics, one per workgroup and bin it holds rows of: the
// counts do not depend on the order.
__global__ __launch_bounds__(kPdpRows) void ale_bin_kernel(const float* X, long long n_rows, int Fp, int col, const float* edges, int K, int* bin,
                                                           unsigned long long* counts) {
    __shared__ int sbin[kPdpRows];
    const long long row = (long long)blockIdx.x * kPdpRows + threadIdx.x;
    int k = 0;
    if (row < n_rows) {
        const float x = X[row * Fp + col];
        int lo = 1, hi = K;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (x <= edges[mid]) hi = mid; else lo = mid + 1;
        }
        k = lo;
        bin[row] = k;
    }
    sbin[threadIdx.x] = k;
    __syncthreads();
    for (int kb = threadIdx.x + 1; kb <= K; kb += kPdpRows) {
        unsigned n = 0;
        for (int r = 0; r < kPdpRows; ++r) n += sbin[r] == kb;
        if (n) atomicAdd(&counts[kb - 1], (unsigned long long)n);
    }
}

// The local effect of set S (and, recursively, of the sets after it) on this thread's row - the prediction with the focal column at
// the upper edge of the row's bin k minus the one at the lower edge, both from the same layer-0 sums - staged in LDS, then added per
// (bin, output) over the workgroup's rows in row order: thread t owns the pairs t, t + 256, ...  No atomics: the same bits every call.
template <int S, int H0P, int NS>
__device__ __forceinline__ void ale_sets(const PdpParams& p, const AleParams& a, const float (&z0)[NS][H0P], int k, const float* stail, float* stage,
                                         const int* sbin) {
    if constexpr (S < NS) {
        if (S < p.n_set) {                                            // (block-uniform)
            float dlt[kPdpTail];
#pragma unroll
            for (int c = 0; c < kPdpTail; ++c) dlt[c] = 0.f;
            if (k > 0) {
                const float* b = p.bias + ((size_t)(p.set0 + S) * p.n_grid + k) * H0P;       // (edge k)
                const float* b_lo = b - H0P;                                                         // (edge k - 1)
                const float* w = stail + (size_t)S * p.tail_floats;
                const float* sl = p.slopes + (size_t)(p.set0 + S) * kMaxLayers;
                float h[H0P], y[kPdpTail];
#pragma unroll
                for (int i = 0; i < H0P; ++i) h[i] = z0[S][i] + b[i];
                pdp_forward<H0P>(p, h, w, sl, dlt);
#pragma unroll
                for (int i = 0; i < H0P; ++i) h[i] = z0[S][i] + b_lo[i];
                pdp_forward<H0P>(p, h, w, sl, y);
#pragma unroll
                for (int c = 0; c < kPdpTail; ++c) dlt[c] -= y[c];
            }
            __syncthreads();      // (the stage is free: layer 0, or the sums of the set before, are through with it)
#pragma unroll
            for (int c = 0; c < kPdpTail; ++c)
                if (c < p.C) stage[threadIdx.x * a.stride + c] = dlt[c];
            __syncthreads();
            double* dst = a.part + ((size_t)S * gridDim.x + blockIdx.x) * a.K * p.C;
            for (int pair = threadIdx.x; pair < a.K * p.C; pair += kPdpRows) {
                const int kb = pair / p.C + 1, c = pair % p.C;
                double s = 0.0;
#pragma unroll 8
                for (int r = 0; r < kPdpRows; ++r) {
                    const float v = stage[r * a.stride + c];
                    if (sbin[r] == kb) s += (double)v;
                }
                dst[pair] = s;
            }
            ale_sets<S + 1>(p, a, z0, k, stail, stage, sbin);
        }
    }
}

// grid (workgroups of the launch), block 256, dynamic LDS stage_floats + n_set tail_floats floats: pdp_kernel's layer 0 (one read of X
// for the sets of the launch), then both edges of each row's own bin.
template <int H0P, int NS>
__global__ __launch_bounds__(kPdpRows) void ale_kernel(const PdpParams p, const AleParams a) {
    extern __shared__ float4 pdp_lds[];
    float* stage = reinterpret_cast<float*>(pdp_lds);
    int* sbin = reinterpret_cast<int*>(stage + kPdpRows * a.stride);
    float* stail = stage + a.stage_floats;
    const int tid = threadIdx.x;
    const long long row = a.row0 + (long long)blockIdx.x * kPdpRows + tid;
    const bool live = row < p.n_rows;
    for (int i = tid; i < p.n_set * p.tail_floats; i += kPdpRows) stail[i] = p.tail[(size_t)p.set0 * p.tail_floats + i];

    float z0[NS][H0P];
    pdp_layer0<0>(p, z0, live, row);
    const int k = live ? a.bin[row] : 0;      // (0: a thread past the table's end, which belongs to no bin)
    __syncthreads();      // (the tails of every set are in LDS, and the first-layer image has been read)
    sbin[tid] = k;
    ale_sets<0>(p, a, z0, k, stail, stage, sbin);
}

// route 2, after the pass with the focal column at edge k: grid (ceil(n_rows / 256), sets of the pass), block 256.  Per workgroup and
// set, the float64 sums of the predictions y [set][n_rows][C] over its rows of bin k (slot 0) and of bin k + 1 (slot 1), in row order,
// into part [set][workgroup][2][C].
__global__ __launch_bounds__(kPdpRows) void ale_pick_kernel(const float* y, const int* bin, long long n_rows, int C, int k, double* part) {
    __shared__ int sbin[kPdpRows];
    const long long row0 = (long long)blockIdx.x * kPdpRows;
    const int n_r = (int)(n_rows - row0 < kPdpRows ? n_rows - row0 : kPdpRows);
    sbin[threadIdx.x] = (int)threadIdx.x < n_r ? bin[row0 + threadIdx.x] : 0;
    __syncthreads();
    const float* ys = y + ((size_t)blockIdx.y * n_rows + row0) * C;
    double* dst = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * C;
    for (int pair = threadIdx.x; pair < 2 * C; pair += kPdpRows) {
        const int want = k + pair / C, c = pair % C;
        double s = 0.0;
#pragma unroll 8
        for (int r = 0; r < n_r; ++r) {
            const float v = ys[(size_t)r * C + c];
            if (sbin[r] == want) s += (double)v;
        }
        dst[pair] = s;
    }
}

constexpr int kAleRuns = 16;                     // ale_reduce_kernel: runs of consecutive workgroups summed side by side
constexpr int kAleRunLanes = 256 / kAleRuns;     // ... and the sums a workgroup of it owns

// grid (ceil(n_set n_slot C / 16)), block 256: acc [all sets][K][C] (+)= the workgroups' partials part [n_set][n_wg][n_slot][C] in
// float64 and in a fixed order: the n_wg workgroups are cut into 16 runs of consecutive ones, 16 threads add a run each in workgroup
// order (16 adjacent sums per read: 128 bytes), and the first of them adds the runs in run order.  Slot q is bin bin0 + q (0-based; a
// slot outside 0 .. K - 1 holds nothing).  alt (route 2): slot 1 is subtracted - it holds the next bin's rows at their lower edge.
// finish: the sum is complete, so it is divided by the bin's row count (0 for an empty bin); under alt that holds for slot 0 only.
__global__ __launch_bounds__(256) void ale_reduce_kernel(const double* part, int n_set, int n_wg, int n_slot, int C, int K, int set0, int bin0,
                                                         int alt, int finish, const unsigned long long* counts, double* acc) {
    __shared__ double runs[kAleRuns][kAleRunLanes];
    const int lane = threadIdx.x % kAleRunLanes, run = threadIdx.x / kAleRunLanes;
    const long long i = (long long)blockIdx.x * kAleRunLanes + lane;
    const bool live = i < (long long)n_set * n_slot * C;
    const int s = (int)(i / ((long long)n_slot * C)), q = (int)(i / C % n_slot), c = (int)(i % C);
    double sum = 0.0;
    if (live) {
        const int b1 = (int)((long long)(run + 1) * n_wg / kAleRuns);
        for (int b = (int)((long long)run * n_wg / kAleRuns); b < b1; ++b) sum += part[(((size_t)s * n_wg + b) * n_slot + q) * C + c];
    }
    runs[run][lane] = sum;
    __syncthreads();
    const int kb = bin0 + q;
    if (run != 0 || !live || kb < 0 || kb >= K) return;
    for (int r = 1; r < kAleRuns; ++r) sum += runs[r][lane];
    double* dst = acc + ((size_t)(set0 + s) * K + kb) * C + c;
    double v = *dst + (alt && q == 1 ? -sum : sum);
    if (finish && !(alt && q == 1)) {
        const unsigned long long n = counts[kb];
        v = n ? v / (double)n : 0.0;
    }
    *dst = v;
}

// ---- what npbnn_predict_pdp and npbnn_predict_ale share on the host

// Route 2: one pass of the evaluation kernels per (point, group of sets), the point's constants d_co [n_points][F] folded into layer
// 0's bias; sets that share their activation slopes travel together, as many as one pass carries.  on_pass(p0, i, s0, ng): the float32
// predictions [ng][n_rows][C] of the sets s0 .. s0 + ng - 1 at point p0 + i are in ctx->d_y, to be read by what it enqueues.
// on_chunk(p0, n_p): the passes of the points p0 .. p0 + n_p - 1 are in and none of them raised a flag.  A layer-0 weight that leaves
// the fp16 range starts the call again, from its first point, on the exact float32 path.
using PassSink = std::function<int(int p0, int i, int s0, int ng)>;
using ChunkSink = std::function<int(int p0, int n_p)>;

int run_point_passes(npbnn_ctx* ctx, const char* who, int which, const Dataset& d, const double* d_w, const double* d_co, int n_points,
                     int p_chunk, const double* act_prm_sets, int n_sets, int apply_out_fn, const PassSink& on_pass, const ChunkSink& on_chunk) {
    const int F = ctx->arch.in_dim, n_act = ctx->net.n_layers - 1;
    const size_t wn = (size_t)ctx->n_weights;
    int rc;
    if ((rc = ctx->d_y.reserve(ctx, kMaxCand * (size_t)d.m->n_rows * ctx->net.n_out))) return rc;
    for (int attempt = 0; attempt < 2; ++attempt) {
        LaunchPlan lp;
        rc = plan_launch(ctx, which, &lp, attempt, kMaxCand, true);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_overflow, 0, (1 + kSetFlags) * sizeof(int), ctx->stream));
        bool redo = false;
        for (int p0 = 0; p0 < n_points && !redo; p0 += p_chunk) {
            const int n_p = std::min(p_chunk, n_points - p0);
            for (int i = 0; i < n_p; ++i) {
                const double* d_cop = d_co + (size_t)(p0 + i) * F;
                int s0 = 0;
                while (s0 < n_sets) {
                    const int ng = slope_group_len(act_prm_sets, n_act, s0, n_sets, lp.n_cand);
                    load_group_slopes(ctx, act_prm_sets, n_act, s0);
                    LaunchPlan lpg = lp;
                    if (lp.wide) lpg.n_cand = ng;      // (the weight-streamed pass has a build per number of sets)
                    launch_pack_group(ctx, lpg, d_w + (size_t)s0 * wn, d_cop, ng);
                    HIP_TRY(ctx, hipGetLastError());
                    rc = push_eval_params(ctx, predict_params(ctx, d, ctx->d_y, apply_out_fn));
                    if (rc) return rc;
                    rc = launch_plain_eval(ctx, lpg, which);
                    if (rc) return rc;
                    if ((rc = on_pass(p0, i, s0, ng))) return rc;
                    HIP_TRY(ctx, hipGetLastError());
                    // (push_eval_params stages through one pinned slot: the launch that reads it must be in before the next write)
                    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                    s0 += ng;
                }
            }
            int flags[1 + kSetFlags] = {0}, ovf = 0;      // (the weight-streamed path's packing reports per set: any of them restarts the call)
            HIP_TRY(ctx, hipMemcpyAsync(flags, ctx->d_overflow, sizeof(flags), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            for (int j = 0; j <= kSetFlags; ++j) ovf |= flags[j];
            if (ovf & kFlagStructure) return fail(ctx, NPBNN_E_ARG, "%s: a layer-0 weight is not zero where the mask given to npbnn_set_layer_mask is", who);
            if (ctx->net.l0_f16 && (ovf & kFlagF16Range)) {
                if (ctx->l0_option == NPBNN_L0_F16) return fail(ctx, NPBNN_E_RANGE, "%s: a layer-0 weight left the fp16 range", who);
                redo = true;         // (this call runs again on the exact float32 path)
                break;
            }
            if ((rc = on_chunk(p0, n_p))) return rc;
        }
        if (!redo) break;
    }
    return NPBNN_OK;
}

}  // namespace

// (npbnn_route1.hip.h)
int prepare_route1(npbnn_ctx* ctx, const npbnn_attrib_route& r, const FeatureTable& m, const double* d_w, const double* d_co, const double* act_prm_sets,
                   int n_sets, int apply_out_fn, Route1Blocks* b, PdpParams* out) {
    const PdpPrep& q = r.q;
    const int L = q.n_layers, n_act = L - 1;
    int rc;
    if ((rc = dev_alloc(ctx, b->w0t, (size_t)n_sets * q.Fp * q.H0P))) return rc;
    if ((rc = dev_alloc(ctx, b->bias, (size_t)n_sets * q.n_grid * q.H0P))) return rc;
    if ((rc = dev_alloc(ctx, b->tail, (size_t)n_sets * q.tail_floats))) return rc;
    if ((rc = dev_alloc(ctx, b->slopes, (size_t)n_sets * kMaxLayers))) return rc;
    std::vector<float> slopes((size_t)n_sets * kMaxLayers, 0.f);
    if (act_prm_sets)
        for (int s = 0; s < n_sets; ++s)
            for (int l = 0; l < n_act; ++l) slopes[(size_t)s * kMaxLayers + l] = (float)act_prm_sets[(size_t)s * n_act + l];
    // (pageable memory: the copy has left `slopes` when the call returns)
    HIP_TRY(ctx, hipMemcpyAsync(b->slopes.get(), slopes.data(), slopes.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(pdp_prep_kernel, dim3(n_sets), dim3(256), 0, ctx->stream, q, d_w, d_co, b->w0t.get(), b->bias.get(), b->tail.get());
    HIP_TRY(ctx, hipGetLastError());
    PdpParams p{};
    p.X = m.X; p.n_rows = m.n_rows; p.Fp = q.Fp;
    p.w0t = b->w0t.get(); p.bias = b->bias.get(); p.tail = b->tail.get(); p.slopes = b->slopes.get();
    p.n_grid = q.n_grid; p.tail_floats = q.tail_floats;
    p.n_layers = L; p.act_kind = ctx->arch.act_kind; p.final_act = ctx->arch.final_act; p.out_kind = ctx->arch.out_kind;
    p.apply_out = apply_out_fn ? 1 : 0; p.C = ctx->net.n_out;
    for (int l = 1; l < L; ++l) { p.t_out[l] = q.l_out[l]; p.t_inp[l] = q.t_inp[l]; p.t_off[l] = q.t_off[l]; }
    *out = p;
    return NPBNN_OK;
}

}  // namespace npbnn_api

extern "C" int npbnn_predict_pdp(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, const int32_t* focal,
                                 int32_t n_focal, const double* grid, int32_t n_grid, const double* col_override, int which, int apply_out_fn,
                                 double* out_mean) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (!W_sets || !out_mean || n_sets < 1 || n_grid < 1 || n_focal < 0 || (n_focal > 0 && (!focal || !grid)))
        return fail(ctx, NPBNN_E_ARG, "predict_pdp: bad arguments");
    SetsTable tb;
    int rc = open_sets_table(ctx, "predict_pdp", which, &tb);
    if (rc) return rc;
    Dataset& d = *tb.d;
    const int F = ctx->arch.in_dim;
    for (int k = 0; k < n_focal; ++k)
        if (focal[k] < 0 || focal[k] >= F) return fail(ctx, NPBNN_E_ARG, "predict_pdp: focal column %d outside 0..%d", focal[k], F - 1);
    const int C = ctx->net.n_out;
    const long long n_rows = tb.n_rows;
    const size_t per_set = (size_t)n_rows * C;

    const std::vector<double> co_all = point_constants(F, col_override, focal, n_focal, grid, n_grid);
    const npbnn_attrib_route r1 = plan_route(ctx, NPBNN_ATTRIB_PDP, d.m->Fp, n_grid, "NPBNN_PDP_PER_GRID");
    const int g_chunk = npbnn_attrib_pdp_g_chunk(n_grid, n_rows, C, (long long)env_bytes("NPBNN_PDP_ACC_BYTES", kPdpAccBytes));

    DevBuf<double> d_w, d_co;
    DevBuf<float> d_acc;
    if ((rc = upload_sets(ctx, W_sets, n_sets, co_all, d_w, d_co))) return rc;
    if ((rc = dev_alloc(ctx, d_acc, (size_t)g_chunk * per_set))) return rc;
    std::vector<float> host_acc((size_t)g_chunk * per_set);
    const double inv_sets = 1.0 / (double)n_sets;
    auto take_chunk = [&](int g0, int n_g) -> int {        // accumulator of grid points g0 .. g0 + n_g - 1 -> out_mean
        HIP_TRY(ctx, hipMemcpyAsync(host_acc.data(), d_acc.get(), (size_t)n_g * per_set * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        double* dst = out_mean + (size_t)g0 * per_set;
        for (size_t i = 0; i < (size_t)n_g * per_set; ++i) dst[i] = (double)host_acc[i] * inv_sets;
        return NPBNN_OK;
    };

    // ---- route 1: the grid-batched kernel
    if (r1.fits) {
        const int NS = r1.NS;
        Route1Blocks blocks1;
        PdpParams p{};
        if ((rc = prepare_route1(ctx, r1, *d.m, d_w.get(), d_co.get(), act_prm_sets, n_sets, apply_out_fn, &blocks1, &p))) return rc;
        p.acc = d_acc.get();
        Route1Kernel<PdpParams> kern;
        if ((rc = kern.pick(ctx, r1.H0P, pdp_kernel<32, 2>, pdp_kernel<64, 1>, r1.lds_bytes))) return rc;
        const unsigned blocks = (unsigned)((n_rows + kPdpRows - 1) / kPdpRows);
        for (int g0 = 0; g0 < n_grid; g0 += g_chunk) {
            p.g0 = g0;
            p.n_g = std::min(g_chunk, n_grid - g0);
            for (int s0 = 0; s0 < n_sets; s0 += NS) {
                p.set0 = s0;
                p.n_set = std::min(NS, n_sets - s0);
                p.accumulate = s0 > 0;
                kern.launch(dim3(blocks), ctx->stream, p);
                HIP_TRY(ctx, hipGetLastError());
            }
            if ((rc = take_chunk(g0, p.n_g))) return rc;
        }
        ctx->pdp_route = 1;
        return NPBNN_OK;
    }

    // ---- route 2: one pass of the evaluation kernels per (grid point, group of sets)
    const unsigned add_blocks = (unsigned)((per_set + 255) / 256);
    rc = run_point_passes(ctx, "predict_pdp", which, d, d_w.get(), d_co.get(), n_grid, g_chunk, act_prm_sets, n_sets, apply_out_fn,
                          [&](int, int gi, int s0, int ng) -> int {
                              hipLaunchKernelGGL(pdp_add_kernel, dim3(add_blocks), dim3(256), 0, ctx->stream, (const float*)ctx->d_y, ng,
                                                 (long long)per_set, d_acc.get() + (size_t)gi * per_set, s0 > 0 ? 1 : 0);
                              return NPBNN_OK;
                          },
                          take_chunk);
    if (rc) return rc;
    ctx->pdp_route = 2;
    return NPBNN_OK;
}

// Accumulated local effects (include/npbnn_hip.h).  Route 1: ale_bin_kernel, then per group of sets one ale_kernel launch - one read
// of X - and ale_reduce_kernel.  Route 2: run_point_passes with the edges as the points; after the pass at edge k, ale_pick_kernel and
// ale_reduce_kernel add its predictions to bin k and take them from bin k + 1.
extern "C" int npbnn_predict_ale(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int32_t focal,
                                 const double* edges, int32_t n_bins, const double* col_override, int which, int apply_out_fn,
                                 int64_t* out_counts, double* out_effect) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    ctx->ale_route = 0;
    if (!W_sets || !edges || !out_counts || !out_effect || n_sets < 1)
        return fail(ctx, NPBNN_E_ARG, "predict_ale: bad arguments");
    if (n_bins < 1 || n_bins > kAleMaxBins) return fail(ctx, NPBNN_E_ARG, "predict_ale: %d bins, outside 1..%d", n_bins, kAleMaxBins);
    const int K = n_bins;
    for (int k = 0; k <= K; ++k)
        if (!std::isfinite(edges[k]) || (k > 0 && !(edges[k] > edges[k - 1])))
            return fail(ctx, NPBNN_E_ARG, "predict_ale: the edges must be finite and strictly increasing (edge %d is %g)", k, edges[k]);
    SetsTable tb;
    int rc = open_sets_table(ctx, "predict_ale", which, &tb);
    if (rc) return rc;
    Dataset& d = *tb.d;
    const int F = ctx->arch.in_dim, C = ctx->net.n_out;
    if (focal < 0 || focal >= F) return fail(ctx, NPBNN_E_ARG, "predict_ale: focal column %d outside 0..%d", focal, F - 1);
    const long long n_rows = tb.n_rows;
    if (n_rows < 1) return fail(ctx, NPBNN_E_ARG, "predict_ale: the table has no rows");
    const size_t n_eff = (size_t)n_sets * K * C;
    const npbnn_attrib_route r1 = plan_route(ctx, NPBNN_ATTRIB_PDP, d.m->Fp, K + 1, "NPBNN_ALE_PER_EDGE");
    npbnn_attrib_ale ap;
    npbnn_attrib_ale_of(&r1, K, C, n_rows, (long long)env_bytes("NPBNN_ALE_PART_BYTES", kAlePartBytes), &ap);
    const unsigned n_wg = (unsigned)ap.n_wg;
    hipStream_t st = ctx->stream;

    const std::vector<double> co_all = point_constants(F, col_override, &focal, 1, edges, K + 1);
    std::vector<float> edges_f(K + 1);
    for (int k = 0; k <= K; ++k) edges_f[k] = (float)edges[k];
    DevBuf<double> d_w, d_co, d_acc, d_part;
    DevBuf<float> d_edges;
    DevBuf<int> d_bin;
    DevBuf<unsigned long long> d_counts;
    if ((rc = upload_sets(ctx, W_sets, n_sets, co_all, d_w, d_co))) return rc;
    if ((rc = dev_alloc(ctx, d_acc, n_eff))) return rc;
    if ((rc = dev_alloc(ctx, d_part, (size_t)ap.n_part))) return rc;
    if ((rc = dev_alloc(ctx, d_edges, edges_f.size()))) return rc;
    if ((rc = dev_alloc(ctx, d_bin, (size_t)n_rows))) return rc;
    if ((rc = dev_alloc(ctx, d_counts, (size_t)K))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_edges.get(), edges_f.data(), edges_f.size() * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(d_counts.get(), 0, (size_t)K * sizeof(unsigned long long), st));
    HIP_TRY(ctx, hipMemsetAsync(d_acc.get(), 0, n_eff * sizeof(double), st));
    hipLaunchKernelGGL(ale_bin_kernel, dim3(n_wg), dim3(kPdpRows), 0, st, (const float*)d.m->X, n_rows, d.m->Fp, (int)focal,
                       (const float*)d_edges.get(), K, d_bin.get(), d_counts.get());
    HIP_TRY(ctx, hipGetLastError());
    auto reduce = [&](int n_set, int wgs, int n_slot, int set0, int bin0, int alt, int finish) {
        const unsigned blocks = (unsigned)(((size_t)n_set * n_slot * C + kAleRunLanes - 1) / kAleRunLanes);
        hipLaunchKernelGGL(ale_reduce_kernel, dim3(blocks), dim3(256), 0, st, (const double*)d_part.get(), n_set, wgs, n_slot, C, K, set0, bin0, alt,
                           finish, (const unsigned long long*)d_counts.get(), d_acc.get());
    };
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts are copied out as they are");
    auto take = [&](int route) -> int {
        HIP_TRY(ctx, hipMemcpyAsync(out_counts, d_counts.get(), (size_t)K * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(out_effect, d_acc.get(), n_eff * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        ctx->ale_route = route;
        return NPBNN_OK;
    };

    // ---- route 1: both edges of a row's bin from one read of X
    if (r1.fits) {
        const int NS = r1.NS;
        const unsigned wg_chunk = (unsigned)ap.wg_chunk;
        Route1Blocks blocks1;
        PdpParams p{};
        if ((rc = prepare_route1(ctx, r1, *d.m, d_w.get(), d_co.get(), act_prm_sets, n_sets, apply_out_fn, &blocks1, &p))) return rc;
        AleParams a{};
        a.bin = d_bin.get(); a.K = K; a.stride = ap.stride; a.stage_floats = ap.stage_floats; a.part = d_part.get();
        Route1Kernel<PdpParams, AleParams> kern;
        if ((rc = kern.pick(ctx, r1.H0P, ale_kernel<32, 2>, ale_kernel<64, 1>, ap.lds_bytes))) return rc;
        for (int s0 = 0; s0 < n_sets; s0 += NS) {
            p.set0 = s0;
            p.n_set = std::min(NS, n_sets - s0);
            for (unsigned w0 = 0; w0 < n_wg; w0 += wg_chunk) {
                const unsigned wgs = std::min(wg_chunk, n_wg - w0);
                a.row0 = (long long)w0 * kPdpRows;
                kern.launch(dim3(wgs), st, p, a);
                HIP_TRY(ctx, hipGetLastError());
                reduce(p.n_set, (int)wgs, K, s0, 0, 0, w0 + wgs == n_wg ? 1 : 0);
                HIP_TRY(ctx, hipGetLastError());
            }
        }
        return take(1);
    }

    // ---- route 2: one pass of the evaluation kernels per (edge, group of sets)
    rc = run_point_passes(ctx, "predict_ale", which, d, d_w.get(), d_co.get(), K + 1, K + 1, act_prm_sets, n_sets, apply_out_fn,
                          [&](int, int k, int s0, int ng) -> int {
                              if (k == 0 && s0 == 0)      // (the first pass of the call, or of its repeat on the float32 path)
                                  HIP_TRY(ctx, hipMemsetAsync(d_acc.get(), 0, n_eff * sizeof(double), st));
                              hipLaunchKernelGGL(ale_pick_kernel, dim3(n_wg, ng), dim3(kPdpRows), 0, st, (const float*)ctx->d_y,
                                                 (const int*)d_bin.get(), n_rows, C, k, d_part.get());
                              HIP_TRY(ctx, hipGetLastError());
                              reduce(ng, (int)n_wg, 2, s0, k - 1, 1, 1);
                              return NPBNN_OK;
                          },
                          [](int, int) -> int { return NPBNN_OK; });
    if (rc) return rc;
    return take(2);
}
