// Route 1 of npbnn_predict_pdp, npbnn_predict_ale (npbnn_pdp.hip), npbnn_predict_saliency (npbnn_saliency.hip) and
// npbnn_predict_shapley (npbnn_shapley.hip): what they share.  A set's float64 weights as float32 blocks (pdp_prep_kernel: layer 0
// transposed with zero rows on the overridden columns, its bias with the overrides folded in, the later layers), the layer-0 product
// of one thread per row from a weight image staged in LDS (pdp_layer0), the later layers from LDS broadcasts (pdp_dense), the
// prediction from layer 0's pre-activation (pdp_forward), the envelope (plan_route1) and the host set-up (prepare_route1).
// Every unit that includes this header gets its own copy of the kernels.  Not part of the ABI.
#pragma once
#include "npbnn_sets.hip.h"

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

bool env_on(const char* name) {
    const char* e = getenv(name);
    return e && *e && strcmp(e, "0") != 0;
}

size_t env_bytes(const char* name, size_t otherwise) {
    if (const char* e = getenv(name)) { const long long v = atoll(e); if (v > 0) return (size_t)v; }
    return otherwise;
}

// Route 1's shapes for a network and n_points shifted biases (grid points, or bin edges), and whether the network is inside its
// envelope (include/npbnn_hip.h); `off`: the environment variable that forces route 2.
struct Route1Plan {
    PdpPrep q{};
    int H0P = 32, NS = 2;
    bool fits = false;
};

Route1Plan plan_route1(const npbnn_ctx* ctx, int Fp, int n_points, const char* off) {
    Route1Plan r;
    const int F = ctx->arch.in_dim, L = ctx->net.n_layers, H0 = ctx->arch.out_dim[0];
    r.H0P = H0 <= 32 ? 32 : 64;
    r.NS = 64 / r.H0P;
    r.fits = !ctx->wide && !env_on(off) && H0 <= kPdpMaxH0 && (size_t)Fp * r.H0P * 4 <= kPdpW0Lds;
    PdpPrep& q = r.q;
    q.F = F; q.Fp = Fp; q.H0 = H0; q.H0P = r.H0P; q.hb0 = ctx->arch.has_bias[0]; q.n_layers = L; q.n_grid = n_points; q.wn = ctx->n_weights;
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
        if (q.l_out[l] > kPdpTail) r.fits = false;
    }
    q.tail_floats = toff;
    if (L == 1 && ctx->net.n_out > kPdpTail) r.fits = false;
    if ((size_t)r.NS * q.tail_floats * 4 > kPdpTailLds) r.fits = false;
    return r;
}

struct Route1Blocks {
    DevBuf<float> w0t, bias, tail, slopes;
};

// Route 1's float32 blocks of every set (pdp_prep_kernel, enqueued on ctx->stream) and the kernel parameters that do not change from
// launch to launch; d_w [n_sets][n_weights], d_co [n_points][F] on the device.
int prepare_route1(npbnn_ctx* ctx, const Route1Plan& r, const FeatureTable& m, const double* d_w, const double* d_co, const double* act_prm_sets,
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

}  // namespace

}  // namespace npbnn_api
