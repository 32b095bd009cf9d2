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
#include "npbnn_sets.hip.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace npbnn_api {

namespace {

constexpr int kPdpRows = 256;                    // rows of a workgroup of pdp_kernel (one per thread)
constexpr int kPdpTail = 32;                     // widest later layer (and output) route 1 takes
constexpr int kPdpMaxH0 = 64;                    // widest first layer route 1 takes
constexpr size_t kPdpW0Lds = 64 * 1024;          // LDS bytes for one set's first-layer weights (Fp x H0P floats)
constexpr size_t kPdpTailLds = 32 * 1024;        // LDS bytes for the later layers of the sets of one launch
constexpr size_t kPdpAccBytes = 512ull << 20;    // device budget of the float32 accumulator [grid points][rows][outputs]: larger grids
                                                 // run in chunks of grid points, each chunk one more read of X per set group

struct PdpParams {
    const float* X;
    long long n_rows;
    int Fp;
    const float* w0t;      // [set][Fp][H0P]: layer 0 transposed, zero on the focal and overridden columns
    const float* bias;     // [set][n_grid][H0P]: layer-0 bias + the override and grid-point fold
    const float* tail;     // [set][tail_floats]: later layer l at t_off[l]: bias (outputs padded to 4), then W [out][t_inp[l]]
    const float* slopes;   // [set][kMaxLayers]
    int set0, n_set, g0, n_g, n_grid, tail_floats;
    int n_layers, act_kind, final_act, out_kind, apply_out, C, accumulate;
    int t_out[kMaxLayers], t_inp[kMaxLayers], t_off[kMaxLayers];
    float* acc;            // [n_g][n_rows][C]
};

struct PdpPrep {
    int F, Fp, H0, H0P, hb0, n_layers, n_grid, wn, tail_floats;
    int l_in[kMaxLayers], l_out[kMaxLayers], l_hb[kMaxLayers], l_woff[kMaxLayers], t_inp[kMaxLayers], t_off[kMaxLayers];
};

template <int KIND, int N>
__device__ __forceinline__ void pdp_act_k(float (&h)[N], float prm) {
#pragma unroll
    for (int i = 0; i < N; ++i) h[i] = act_apply(h[i], KIND, prm);
}

template <int N>
__device__ __forceinline__ void pdp_act(float (&h)[N], int kind, float prm) {
    switch (kind) {
        case NPBNN_ACT_RELU: pdp_act_k<NPBNN_ACT_RELU>(h, prm); break;
        case NPBNN_ACT_LEAKY: pdp_act_k<NPBNN_ACT_LEAKY>(h, prm); break;
        case NPBNN_ACT_SWISH: pdp_act_k<NPBNN_ACT_SWISH>(h, prm); break;
        default: pdp_act_k<NPBNN_ACT_TANH>(h, prm); break;
    }
}

// out[o] = w_bias[o] + sum_i W[o][i] in[i] for o < n_out (0 above); inp: the layer's inputs padded to 8 (zero weights on the padding).
// The weights are LDS reads at one address for the whole wave (broadcasts); the guards are wave-uniform.
template <int IN, int OUT>
__device__ __forceinline__ void pdp_dense(const float (&in)[IN], float (&out)[OUT], const float* w, int n_out, int inp) {
    const float* wm = w + ((n_out + 3) & ~3);
#pragma unroll
    for (int o = 0; o < OUT; ++o) {
        float a = 0.f;
        if (o < n_out) {
            a = w[o];
            const float* r = wm + o * inp;
#pragma unroll
            for (int i = 0; i < IN; i += 8)
                if (i < inp) {
                    const float4 u = *reinterpret_cast<const float4*>(r + i);
                    const float4 v = *reinterpret_cast<const float4*>(r + i + 4);
                    a = fmaf(in[i], u.x, a); a = fmaf(in[i + 1], u.y, a); a = fmaf(in[i + 2], u.z, a); a = fmaf(in[i + 3], u.w, a);
                    a = fmaf(in[i + 4], v.x, a); a = fmaf(in[i + 5], v.y, a); a = fmaf(in[i + 6], v.z, a); a = fmaf(in[i + 7], v.w, a);
                }
        }
        out[o] = a;
    }
}

// layer 0's pre-activation h (bias and grid shift included) -> the prediction y (first C entries; output function when asked)
template <int H0P>
__device__ __forceinline__ void pdp_forward(const PdpParams& p, float (&h)[H0P], const float* w, const float* sl, float (&y)[kPdpTail]) {
    static_assert(H0P >= kPdpTail, "layer 0 is at least as wide as the later layers' bound");
    const int L = p.n_layers;
    if (L == 1) {
        if (p.final_act) pdp_act(h, p.act_kind, sl[0]);
#pragma unroll
        for (int c = 0; c < kPdpTail; ++c) y[c] = h[c];
    } else {
        pdp_act(h, p.act_kind, sl[0]);
        pdp_dense<H0P, kPdpTail>(h, y, w + p.t_off[1], p.t_out[1], p.t_inp[1]);
        for (int l = 2; l < L; ++l) {
            pdp_act(y, p.act_kind, sl[l - 1]);
            float nx[kPdpTail];
            pdp_dense<kPdpTail, kPdpTail>(y, nx, w + p.t_off[l], p.t_out[l], p.t_inp[l]);
#pragma unroll
            for (int c = 0; c < kPdpTail; ++c) y[c] = nx[c];
        }
        if (p.final_act) pdp_act(y, p.act_kind, sl[L - 1]);
    }
    if (!p.apply_out) return;
    if (p.out_kind == NPBNN_OUT_SOFTMAX) {           // SoftMax (BNN_lib.py:166-168)
        float m = -3.402823466e38f;
#pragma unroll
        for (int c = 0; c < kPdpTail; ++c)
            if (c < p.C) m = fmaxf(m, y[c]);
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < kPdpTail; ++c)
            if (c < p.C) { y[c] = __expf(y[c] - m); s += y[c]; }
        const float r = 1.f / s;
#pragma unroll
        for (int c = 0; c < kPdpTail; ++c) y[c] *= r;
    } else if (p.out_kind == NPBNN_OUT_SOFTPLUS_HALF) {   // RegressTransformError (BNN_lib.py:177-182)
#pragma unroll
        for (int c = 0; c < kPdpTail; ++c)
            if (c < p.C && c >= p.C / 2) y[c] = softplus_f(y[c]);
    }
}

// layer 0 without bias of set S (and, recursively, of the sets after it) for this thread's row: the set's weights are staged in LDS
// by the whole workgroup, then every thread reads its row of X once.  (A recursion rather than a loop: z0[S] needs a constant index
// to stay in registers.)
template <int S, int H0P, int NS>
__device__ __forceinline__ void pdp_layer0(const PdpParams& p, float (&z0)[NS][H0P], bool live, long long row) {
    if constexpr (S < NS) {
        extern __shared__ float4 pdp_lds[];
        const float* sw0 = reinterpret_cast<const float*>(pdp_lds);
        float (&z)[H0P] = z0[S];
#pragma unroll
        for (int h = 0; h < H0P; ++h) z[h] = 0.f;
        if (S < p.n_set) {                                            // (block-uniform)
            __syncthreads();
            const float4* src = reinterpret_cast<const float4*>(p.w0t + (size_t)(p.set0 + S) * p.Fp * H0P);
            for (int i = threadIdx.x; i < p.Fp * H0P / 4; i += kPdpRows) pdp_lds[i] = src[i];
            __syncthreads();
            if (live) {
                const float4* xr = reinterpret_cast<const float4*>(p.X + row * p.Fp);
                for (int f4 = 0; f4 < p.Fp / 4; ++f4) {
                    const float4 x = xr[f4];
                    const float* w = sw0 + (size_t)f4 * 4 * H0P;
#pragma unroll
                    for (int h = 0; h < H0P; h += 4) {
                        const float4 a = *reinterpret_cast<const float4*>(w + h);
                        const float4 b = *reinterpret_cast<const float4*>(w + H0P + h);
                        const float4 c = *reinterpret_cast<const float4*>(w + 2 * H0P + h);
                        const float4 d = *reinterpret_cast<const float4*>(w + 3 * H0P + h);
                        z[h] = fmaf(x.w, d.x, fmaf(x.z, c.x, fmaf(x.y, b.x, fmaf(x.x, a.x, z[h]))));
                        z[h + 1] = fmaf(x.w, d.y, fmaf(x.z, c.y, fmaf(x.y, b.y, fmaf(x.x, a.y, z[h + 1]))));
                        z[h + 2] = fmaf(x.w, d.z, fmaf(x.z, c.z, fmaf(x.y, b.z, fmaf(x.x, a.z, z[h + 2]))));
                        z[h + 3] = fmaf(x.w, d.w, fmaf(x.z, c.w, fmaf(x.y, b.w, fmaf(x.x, a.w, z[h + 3]))));
                    }
                }
            }
        }
        pdp_layer0<S + 1>(p, z0, live, row);
    }
}

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

bool env_on(const char* name) {
    const char* e = getenv(name);
    return e && *e && strcmp(e, "0") != 0;
}

}  // namespace

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
    const int L = ctx->net.n_layers, C = ctx->net.n_out, n_act = L - 1;
    const long long n_rows = tb.n_rows;
    const size_t wn = (size_t)ctx->n_weights;
    const size_t per_set = (size_t)n_rows * C;

    // per grid point, every column's constant: col_override's where it has one (it applies after the grid values), else the grid
    // value on a focal column, else NaN
    std::vector<double> co_all((size_t)n_grid * F);
    for (int g = 0; g < n_grid; ++g) {
        double* co = co_all.data() + (size_t)g * F;
        for (int f = 0; f < F; ++f) co[f] = col_override ? col_override[f] : NAN;
        for (int k = 0; k < n_focal; ++k)
            if (std::isnan(col_override ? col_override[focal[k]] : NAN)) co[focal[k]] = grid[(size_t)g * n_focal + k];
    }
    size_t budget = kPdpAccBytes;
    if (const char* e = getenv("NPBNN_PDP_ACC_BYTES")) { const long long v = atoll(e); if (v > 0) budget = (size_t)v; }
    const size_t chunk_bytes = per_set * sizeof(float);
    const int g_chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_grid, budget / std::max<size_t>(chunk_bytes, 1)));

    DevBuf<double> d_w, d_co;
    DevBuf<float> d_acc;
    if ((rc = dev_alloc(ctx, d_w, (size_t)n_sets * wn))) return rc;
    if ((rc = dev_alloc(ctx, d_co, co_all.size()))) return rc;
    if ((rc = dev_alloc(ctx, d_acc, (size_t)g_chunk * per_set))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_w.get(), W_sets, (size_t)n_sets * wn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_co.get(), co_all.data(), co_all.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
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
    const int H0 = ctx->arch.out_dim[0];
    const int H0P = H0 <= 32 ? 32 : 64;
    const int Fp = d.m->Fp;
    bool batched = !ctx->wide && !env_on("NPBNN_PDP_PER_GRID") && H0 <= kPdpMaxH0 && (size_t)Fp * H0P * 4 <= kPdpW0Lds;
    PdpPrep q{};
    q.F = F; q.Fp = Fp; q.H0 = H0; q.H0P = H0P; q.hb0 = ctx->arch.has_bias[0]; q.n_layers = L; q.n_grid = n_grid; q.wn = (int)wn;
    {
        int woff = H0 * (F + q.hb0), toff = 0;
        for (int l = 1; l < L; ++l) {
            q.l_in[l] = ctx->arch.out_dim[l - 1];
            q.l_out[l] = ctx->arch.out_dim[l];
            q.l_hb[l] = ctx->arch.has_bias[l];
            q.l_woff[l] = woff;
            woff += q.l_out[l] * (q.l_in[l] + q.l_hb[l]);
            q.t_inp[l] = round_up(q.l_in[l], 8);
            q.t_off[l] = toff;
            toff += round_up(q.l_out[l], 4) + q.l_out[l] * q.t_inp[l];
            if (q.l_out[l] > kPdpTail) batched = false;
        }
        q.tail_floats = toff;
        if (L == 1 && C > kPdpTail) batched = false;
    }
    const int NS = 64 / H0P;
    if ((size_t)NS * q.tail_floats * 4 > kPdpTailLds) batched = false;

    if (batched) {
        DevBuf<float> d_w0t, d_bias, d_tail, d_slopes;
        if ((rc = dev_alloc(ctx, d_w0t, (size_t)n_sets * Fp * H0P))) return rc;
        if ((rc = dev_alloc(ctx, d_bias, (size_t)n_sets * n_grid * H0P))) return rc;
        if ((rc = dev_alloc(ctx, d_tail, (size_t)n_sets * q.tail_floats))) return rc;
        if ((rc = dev_alloc(ctx, d_slopes, (size_t)n_sets * kMaxLayers))) return rc;
        std::vector<float> slopes((size_t)n_sets * kMaxLayers, 0.f);
        if (act_prm_sets)
            for (int s = 0; s < n_sets; ++s)
                for (int l = 0; l < n_act; ++l) slopes[(size_t)s * kMaxLayers + l] = (float)act_prm_sets[(size_t)s * n_act + l];
        HIP_TRY(ctx, hipMemcpyAsync(d_slopes.get(), slopes.data(), slopes.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(pdp_prep_kernel, dim3(n_sets), dim3(256), 0, ctx->stream, q, d_w.get(), d_co.get(),
                           d_w0t.get(), d_bias.get(), d_tail.get());
        HIP_TRY(ctx, hipGetLastError());
        PdpParams p{};
        p.X = d.m->X; p.n_rows = n_rows; p.Fp = Fp;
        p.w0t = d_w0t.get(); p.bias = d_bias.get(); p.tail = d_tail.get(); p.slopes = d_slopes.get();
        p.n_grid = n_grid; p.tail_floats = q.tail_floats;
        p.n_layers = L; p.act_kind = ctx->arch.act_kind; p.final_act = ctx->arch.final_act; p.out_kind = ctx->arch.out_kind;
        p.apply_out = apply_out_fn ? 1 : 0; p.C = C;
        for (int l = 1; l < L; ++l) { p.t_out[l] = q.l_out[l]; p.t_inp[l] = q.t_inp[l]; p.t_off[l] = q.t_off[l]; }
        p.acc = d_acc.get();
        const void* fn = H0P == 32 ? reinterpret_cast<const void*>(pdp_kernel<32, 2>) : reinterpret_cast<const void*>(pdp_kernel<64, 1>);
        const size_t lds = ((size_t)Fp * H0P + (size_t)NS * q.tail_floats) * sizeof(float);
        HIP_TRY(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const unsigned blocks = (unsigned)((n_rows + kPdpRows - 1) / kPdpRows);
        for (int g0 = 0; g0 < n_grid; g0 += g_chunk) {
            p.g0 = g0;
            p.n_g = std::min(g_chunk, n_grid - g0);
            for (int s0 = 0; s0 < n_sets; s0 += NS) {
                p.set0 = s0;
                p.n_set = std::min(NS, n_sets - s0);
                p.accumulate = s0 > 0;
                if (H0P == 32) hipLaunchKernelGGL((pdp_kernel<32, 2>), dim3(blocks), dim3(kPdpRows), lds, ctx->stream, p);
                else hipLaunchKernelGGL((pdp_kernel<64, 1>), dim3(blocks), dim3(kPdpRows), lds, ctx->stream, p);
                HIP_TRY(ctx, hipGetLastError());
            }
            if ((rc = take_chunk(g0, p.n_g))) return rc;
        }
        ctx->pdp_route = 1;
        return NPBNN_OK;
    }

    // ---- route 2: one pass of the evaluation kernels per (grid point, group of sets)
    if ((rc = ctx->d_y.reserve(ctx, kMaxCand * per_set))) return rc;
    const unsigned add_blocks = (unsigned)((per_set + 255) / 256);
    for (int attempt = 0; attempt < 2; ++attempt) {
        LaunchPlan lp;
        rc = plan_launch(ctx, which, &lp, attempt, kMaxCand, true);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_overflow, 0, (1 + kSetFlags) * sizeof(int), ctx->stream));
        bool redo = false;
        for (int g0 = 0; g0 < n_grid && !redo; g0 += g_chunk) {
            const int n_g = std::min(g_chunk, n_grid - g0);
            for (int gi = 0; gi < n_g; ++gi) {
                const double* d_cog = d_co.get() + (size_t)(g0 + gi) * F;
                int s0 = 0;
                while (s0 < n_sets) {
                    // sets that share their activation slopes travel together, as many as one pass carries
                    const int ng = slope_group_len(act_prm_sets, n_act, s0, n_sets, lp.n_cand);
                    load_group_slopes(ctx, act_prm_sets, n_act, s0);
                    LaunchPlan lpg = lp;
                    if (lp.wide) lpg.n_cand = ng;      // (the weight-streamed pass has a build per number of sets)
                    launch_pack_group(ctx, lpg, d_w.get() + (size_t)s0 * wn, d_cog, ng);
                    HIP_TRY(ctx, hipGetLastError());
                    rc = push_eval_params(ctx, predict_params(ctx, d, ctx->d_y, apply_out_fn));
                    if (rc) return rc;
                    rc = launch_plain_eval(ctx, lpg, which);
                    if (rc) return rc;
                    hipLaunchKernelGGL(pdp_add_kernel, dim3(add_blocks), dim3(256), 0, ctx->stream, (const float*)ctx->d_y, ng,
                                       (long long)per_set, d_acc.get() + (size_t)gi * per_set, s0 > 0 ? 1 : 0);
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
            if (ovf & kFlagStructure) return fail(ctx, NPBNN_E_ARG, "predict_pdp: a layer-0 weight is not zero where the mask given to npbnn_set_layer_mask is");
            if (ctx->net.l0_f16 && (ovf & kFlagF16Range)) {
                if (ctx->l0_option == NPBNN_L0_F16) return fail(ctx, NPBNN_E_RANGE, "predict_pdp: a layer-0 weight left the fp16 range");
                redo = true;         // (this call runs again on the exact float32 path)
                break;
            }
            if ((rc = take_chunk(g0, n_g))) return rc;
        }
        if (!redo) break;
    }
    ctx->pdp_route = 2;
    return NPBNN_OK;
}
