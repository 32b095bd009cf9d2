// What npbnn_predict_pdp, npbnn_predict_ale (npbnn_pdp.hip), npbnn_predict_saliency (npbnn_saliency.hip) and npbnn_predict_shapley
// (npbnn_shapley.hip) share.  Route 1: a set's float64 weights as float32 blocks (prepare_route1: layer 0 transposed with zero rows on
// the overridden columns, its bias with the overrides folded in, the later layers), the layer-0 product of one thread per row from a
// weight image staged in LDS (pdp_layer0), the later layers from LDS broadcasts (pdp_dense), the prediction from layer 0's
// pre-activation (pdp_forward).  Route 2 of saliency and Shapley: the same blocks behind one runtime-width network (PlainNet,
// plain_later_layers).  Both: the output function (out_function), the plan (plan_route over npbnn_attrib_plan.h) and the entries' host
// steps (upload_sets, Route1Kernel).  The device routines here are inlined into the kernels of the unit that includes this header;
// the preparation kernel and prepare_route1 live in npbnn_pdp.hip alone.  Not part of the ABI.
#pragma once
#include "npbnn_attrib_plan.h"
#include "npbnn_sets.hip.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace npbnn_api {

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

struct Route1Blocks {
    DevBuf<float> w0t, bias, tail, slopes;
};

// Route 1's float32 blocks of every set (a preparation kernel, enqueued on ctx->stream) and the kernel parameters that do not change
// from launch to launch; d_w [n_sets][n_weights], d_co [n_points][F] on the device.  (npbnn_pdp.hip)
int prepare_route1(npbnn_ctx* ctx, const npbnn_attrib_route& r, const FeatureTable& m, const double* d_w, const double* d_co,
                   const double* act_prm_sets, int n_sets, int apply_out_fn, Route1Blocks* b, PdpParams* out);

namespace {

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

// f(c) for the outputs c < C.  N > 0: the values are registers, so the loop runs to N unrolled and c is a constant in every copy.
template <int N, class F>
__device__ __forceinline__ void each_output(int C, F f) {
    if constexpr (N > 0) {
#pragma unroll
        for (int c = 0; c < N; ++c)
            if (c < C) f(c);
    } else {
        for (int c = 0; c < C; ++c) f(c);
    }
}

// v(c), c < C, in place: the softmax probabilities (SoftMax, BNN_lib.py:166-168)
template <int N, class V>
__device__ __forceinline__ void out_softmax(int C, V v) {
    float m = -3.402823466e38f;
    each_output<N>(C, [&](int c) { m = fmaxf(m, v(c)); });
    float s = 0.f;
    each_output<N>(C, [&](int c) { v(c) = __expf(v(c) - m); s += v(c); });
    const float r = 1.f / s;
    each_output<N>(C, [&](int c) { v(c) *= r; });
}

// the output function on v(c), c < C, in place: softmax, or softplus on the second half (RegressTransformError, BNN_lib.py:177-182)
template <int N, class V>
__device__ __forceinline__ void out_function(int out_kind, int C, V v) {
    if (out_kind == NPBNN_OUT_SOFTMAX) out_softmax<N>(C, v);
    else if (out_kind == NPBNN_OUT_SOFTPLUS_HALF)
        each_output<N>(C, [&](int c) { if (c >= C / 2) v(c) = softplus_f(v(c)); });
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
    // out_function's arithmetic on the registers, spelled out: through out_function the compiler allots the walk kernels' registers
    // differently (shap_walk_kernel<32> 215 -> 201 VGPRs) and npbnn_predict_shapley's route 1 takes 7.6 % longer (NOTES 8.15)
    if (p.out_kind == NPBNN_OUT_SOFTMAX) {
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
    } else if (p.out_kind == NPBNN_OUT_SOFTPLUS_HALF) {
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

bool env_on(const char* name) {
    const char* e = getenv(name);
    return e && *e && strcmp(e, "0") != 0;
}

size_t env_bytes(const char* name, size_t otherwise) {
    if (const char* e = getenv(name)) { const long long v = atoll(e); if (v > 0) return (size_t)v; }
    return otherwise;
}

// The route and route 1's shapes for the context's network and n_points shifted biases (grid points, bin edges, or 1);
// `off`: the entry's environment variable that forces route 2.
npbnn_attrib_route plan_route(const npbnn_ctx* ctx, int entry, int Fp, int n_points, const char* off) {
    const npbnn_attrib_route_req req = {&ctx->arch, ctx->n_weights, Fp, n_points, ctx->wide ? 1 : 0, env_on(off) ? 1 : 0, entry};
    npbnn_attrib_route r{};
    npbnn_attrib_route_of(&req, &r);
    return r;
}

// per point, every column's constant: col_override's where it has one (it applies after the point's values), else the point's value
// on a focal column, else NaN
std::vector<double> point_constants(int F, const double* col_override, const int32_t* focal, int n_focal, const double* values, int n_points) {
    std::vector<double> co_all((size_t)n_points * F);
    for (int g = 0; g < n_points; ++g) {
        double* co = co_all.data() + (size_t)g * F;
        for (int f = 0; f < F; ++f) co[f] = col_override ? col_override[f] : NAN;
        for (int k = 0; k < n_focal; ++k)
            if (std::isnan(col_override ? col_override[focal[k]] : NAN)) co[focal[k]] = values[(size_t)g * n_focal + k];
    }
    return co_all;
}

// The sets' float64 weights and the points' constants on the device, enqueued on ctx->stream (co_all outlives the copy: the entries
// end with a wait for the stream).
int upload_sets(npbnn_ctx* ctx, const double* W_sets, int n_sets, const std::vector<double>& co_all, DevBuf<double>& d_w, DevBuf<double>& d_co) {
    const size_t n_w = (size_t)n_sets * ctx->n_weights;
    int rc;
    if ((rc = dev_alloc(ctx, d_w, n_w))) return rc;
    if ((rc = dev_alloc(ctx, d_co, co_all.size()))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_w.get(), W_sets, n_w * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_co.get(), co_all.data(), co_all.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return NPBNN_OK;
}

// A route-1 kernel at the plan's H0P: the <32, ...> or the <64, ...> instantiation with its dynamic LDS, allowed once, then launched
// by blocks of 256 threads.
template <class... A>
struct Route1Kernel {
    void (*fn)(A...) = nullptr;
    size_t lds = 0;
    int pick(npbnn_ctx* ctx, int H0P, void (*k32)(A...), void (*k64)(A...), long long lds_bytes) {
        fn = H0P == 32 ? k32 : k64;
        lds = (size_t)lds_bytes;
        if (lds) HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        return NPBNN_OK;
    }
    void launch(dim3 grid, hipStream_t st, A... args) const { hipLaunchKernelGGL(fn, grid, dim3(256), lds, st, args...); }
};

// ---- route 2 of saliency and Shapley: one network at run-time widths behind route 1's float32 blocks

struct PlainNet {
    const float* w0t;      // [prepared set][Fp][H0P], bias [.][H0P], later layers [.][tail_floats], slopes [.][kMaxLayers]
    const float* bias;
    const float* tail;
    const float* slopes;
    int Fp, H0P, tail_floats;
    int n_layers, act_kind, final_act, out_kind, apply_out, C, max_w;
    int width[kMaxLayers], t_inp[kMaxLayers], t_off[kMaxLayers];
};

PlainNet plain_net(const PdpParams& p, const npbnn_attrib_route& r) {
    PlainNet n{};
    n.w0t = p.w0t; n.bias = p.bias; n.tail = p.tail; n.slopes = p.slopes; n.Fp = p.Fp; n.H0P = r.H0P; n.tail_floats = p.tail_floats;
    n.n_layers = p.n_layers; n.act_kind = p.act_kind; n.final_act = p.final_act; n.out_kind = p.out_kind; n.apply_out = p.apply_out;
    n.C = p.C; n.max_w = r.max_w;
    for (int l = 0; l < p.n_layers; ++l) { n.width[l] = l ? r.q.l_out[l] : r.q.H0; n.t_inp[l] = p.t_inp[l]; n.t_off[l] = p.t_off[l]; }
    return n;
}

// a'(z) on the branch act_apply takes
template <int KIND>
__device__ __forceinline__ float dact_k(float z, float prm) {
    if (KIND == NPBNN_ACT_RELU) return z > 0.f ? 1.f : 0.f;
    if (KIND == NPBNN_ACT_LEAKY) return z < 0.f ? prm : 1.f;
    if (KIND == NPBNN_ACT_SWISH) {
        const float s = __builtin_amdgcn_rcpf(1.f + __expf(-z));
        return s * (1.f + z * (1.f - s));
    }
    const float t = act_apply(z, NPBNN_ACT_TANH, prm);
    return 1.f - t * t;
}

__device__ __forceinline__ float dact(float z, int kind, float prm) {
    switch (kind) {
        case NPBNN_ACT_RELU: return dact_k<NPBNN_ACT_RELU>(z, prm);
        case NPBNN_ACT_LEAKY: return dact_k<NPBNN_ACT_LEAKY>(z, prm);
        case NPBNN_ACT_SWISH: return dact_k<NPBNN_ACT_SWISH>(z, prm);
        default: return dact_k<NPBNN_ACT_TANH>(z, prm);
    }
}

// The later layers of one thread's row.  A value sits `stride` floats from the next unit's; layer l's units start at unit at(l) of
// val, layer 0's hold its values after the activation.  der (or nullptr), laid out like val: a'(z), 1 where the layer has no
// activation.  Bias first, inputs ascending; the weights are read at wave-uniform addresses.
template <class At>
__device__ __forceinline__ void plain_later_layers(const PlainNet& n, const float* tail, const float* sl, float* val, float* der, size_t stride, At at) {
    const int L = n.n_layers, kind = n.act_kind;
    for (int l = 1; l < L; ++l) {
        const int n_in = n.width[l - 1], n_out = n.width[l], inp = n.t_inp[l];
        const float* wb = tail + n.t_off[l];
        const float* wm = wb + ((n_out + 3) & ~3);
        const float* in = val + (size_t)at(l - 1) * stride;
        const size_t out = (size_t)at(l) * stride;
        const bool has_act = l < L - 1 || n.final_act;
        const float prm = sl[l];
        for (int o = 0; o < n_out; ++o) {
            float z = wb[o];
            const float* wr = wm + (size_t)o * inp;
            for (int i = 0; i < n_in; ++i) z = fmaf(in[(size_t)i * stride], wr[i], z);
            val[out + (size_t)o * stride] = has_act ? act_apply(z, kind, prm) : z;
            if (der) der[out + (size_t)o * stride] = has_act ? dact(z, kind, prm) : 1.f;
        }
    }
}

}  // namespace

}  // namespace npbnn_api
