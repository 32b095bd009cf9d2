// Input-gradient saliency (npbnn_predict_saliency, include/npbnn_hip.h): per stored weight set, output c and feature j the mean over the
// table's rows of G = d f_c / d x_j, of |G| and of G^2.  G is never stored: a launch runs in two phases over a chunk of rows.
//
// Phase 1, one thread per row: the forward pass, then per output the backward sweep down to layer 0's pre-activation,
// D[c][row][h] = d f_c / d z0_h, H0P floats per row and output into a device scratch.  Route 1 (networks inside npbnn_predict_pdp's
// route-1 envelope): layer 0 from pdp_layer0 - the set's first layer staged in LDS, one read of the float32 X per group of sets - the
// later layers through pdp_dense in registers and back through its transpose; the activation derivatives of the later layers wait in
// a scratch [workgroup][layer][unit][row] (coalesced), layer 0's in registers.  Route 2 (every other network): a plain kernel with
// runtime widths whose activations, derivative factors and gradients live in scratches [unit][row of the chunk]; its weights are
// the same float32 blocks (pdp_prep_kernel), read at wave-uniform addresses.
//
// Phase 2, both routes: per (set, output) G_tile = D_c [rows x H0] W0^T [H0 x F] on v_mfma_f32_32x32x2_f32, a tile of 32 rows x 32
// features at a time, folded at once.  A lane's 16 accumulators - 16 rows of one feature - are added in float32; from there on the
// sums are float64: over a wave's 256 rows in row order, the two half-waves added last, one partial per (wave, feature); then
// sal_reduce_kernel adds the partials in a fixed order.  No atomics: the same input gives the same bits.  W0^T has zero rows on the
// overridden columns (pdp_prep_kernel), so those columns are exactly 0.
#include "npbnn_route1.hip.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace npbnn_api {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kSalNB = 4;                        // feature tiles of 32 a wave of sal_fold_kernel carries
constexpr size_t kSalScratchBytes = 128ull << 20;   // device budget of D, the partials and phase 1's scratches: a larger table runs in
                                                    // chunks of rows (and, on route 2, a wide output layer in chunks of outputs)
constexpr size_t kSalPrepBytes = 256ull << 20;   // device budget of the float32 blocks: more sets are prepared group after group
// (NPBNN_SALIENCY_SCRATCH_BYTES and NPBNN_SALIENCY_PREP_BYTES override them; the cut itself is npbnn_attrib_sal_of's)

template <int KIND, int N>
__device__ __forceinline__ void sal_act_d_k(float (&h)[N], float (&d)[N], float prm) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        d[i] = dact_k<KIND>(h[i], prm);
        h[i] = act_apply(h[i], KIND, prm);
    }
}

// d = a'(h), then h = a(h)
template <int N>
__device__ __forceinline__ void sal_act_d(float (&h)[N], float (&d)[N], int kind, float prm) {
    switch (kind) {
        case NPBNN_ACT_RELU: sal_act_d_k<NPBNN_ACT_RELU>(h, d, prm); break;
        case NPBNN_ACT_LEAKY: sal_act_d_k<NPBNN_ACT_LEAKY>(h, d, prm); break;
        case NPBNN_ACT_SWISH: sal_act_d_k<NPBNN_ACT_SWISH>(h, d, prm); break;
        default: sal_act_d_k<NPBNN_ACT_TANH>(h, d, prm); break;
    }
}

__device__ __forceinline__ float sal_sigmoid(float z) { return 1.f / (1.f + __expf(-z)); }

// pdp_dense's transpose: gp[i] = sum_o W[o][i] g[o] for i < inp (0 above), the layer's block w as pdp_dense reads it
template <int IN>
__device__ __forceinline__ void sal_dense_t(const float (&g)[kPdpTail], float (&gp)[IN], const float* w, int n_out, int inp) {
    const float* wm = w + ((n_out + 3) & ~3);
#pragma unroll
    for (int i = 0; i < IN; ++i) gp[i] = 0.f;
#pragma unroll
    for (int o = 0; o < kPdpTail; ++o)
        if (o < n_out) {
            const float* r = wm + o * inp;
#pragma unroll
            for (int i = 0; i < IN; i += 8)
                if (i < inp) {
                    const float4 u = *reinterpret_cast<const float4*>(r + i);
                    const float4 v = *reinterpret_cast<const float4*>(r + i + 4);
                    gp[i] = fmaf(u.x, g[o], gp[i]); gp[i + 1] = fmaf(u.y, g[o], gp[i + 1]);
                    gp[i + 2] = fmaf(u.z, g[o], gp[i + 2]); gp[i + 3] = fmaf(u.w, g[o], gp[i + 3]);
                    gp[i + 4] = fmaf(v.x, g[o], gp[i + 4]); gp[i + 5] = fmaf(v.y, g[o], gp[i + 5]);
                    gp[i + 6] = fmaf(v.z, g[o], gp[i + 6]); gp[i + 7] = fmaf(v.w, g[o], gp[i + 7]);
                }
        }
}

// ---- phase 1, route 1

struct SalParams {
    float* D;              // [sets of the launch][C][rows_cap][H0P]
    float* fac;            // [workgroup][n_layers][kPdpTail][256]: a'(z) of the later layers' units for the backward sweep
    long long row0;        // first row of the chunk
    int rows_cap;          // rows D has room for per (set, output)
};

// Set S (and, recursively, the sets after it) on this thread's row r of the chunk: forward from layer 0's sums, the output function,
// then per output the sweep back to layer 0's pre-activation.
template <int S, int H0P, int NS>
__device__ __forceinline__ void sal_sets(const PdpParams& p, const SalParams& a, const float (&z0)[NS][H0P], const float* stail, long long r) {
    if constexpr (S < NS) {
        if (S < p.n_set) {                                            // (block-uniform)
            const float* b = p.bias + (size_t)(p.set0 + S) * H0P;         // (one bias point: the bias and the override fold)
            const float* w = stail + (size_t)S * p.tail_floats;
            const float* sl = p.slopes + (size_t)(p.set0 + S) * kMaxLayers;
            const int L = p.n_layers, kind = p.act_kind, C = p.C;
            float* fac = a.fac + (size_t)blockIdx.x * L * kPdpTail * kPdpRows + threadIdx.x;
            float h[H0P], d0[H0P], y[kPdpTail];
#pragma unroll
            for (int k = 0; k < H0P; ++k) h[k] = z0[S][k] + b[k];
            if (L == 1) {
                if (p.final_act) sal_act_d(h, d0, kind, sl[0]);
                else {
#pragma unroll
                    for (int k = 0; k < H0P; ++k) d0[k] = 1.f;
                }
#pragma unroll
                for (int c = 0; c < kPdpTail; ++c) y[c] = h[c];
            } else {
                sal_act_d(h, d0, kind, sl[0]);
                pdp_dense<H0P, kPdpTail>(h, y, w + p.t_off[1], p.t_out[1], p.t_inp[1]);
                for (int l = 2; l <= L; ++l) {
                    if (l == L && !p.final_act) break;
                    float dl[kPdpTail];
                    sal_act_d(y, dl, kind, sl[l - 1]);
#pragma unroll
                    for (int u = 0; u < kPdpTail; ++u) fac[((l - 1) * kPdpTail + u) * kPdpRows] = dl[u];
                    if (l == L) break;
                    float nx[kPdpTail];
                    pdp_dense<kPdpTail, kPdpTail>(y, nx, w + p.t_off[l], p.t_out[l], p.t_inp[l]);
#pragma unroll
                    for (int c = 0; c < kPdpTail; ++c) y[c] = nx[c];
                }
            }
            // the output side, in place: softmax - the probabilities; softplus-half - the factor sigma(z) (1 on the first half); else 1
            const int out_kind = p.apply_out ? p.out_kind : NPBNN_OUT_IDENTITY;
            if (out_kind == NPBNN_OUT_SOFTMAX) {
                out_softmax<kPdpTail>(C, [&](int c) -> float& { return y[c]; });
            } else {
#pragma unroll
                for (int c = 0; c < kPdpTail; ++c) y[c] = (out_kind == NPBNN_OUT_SOFTPLUS_HALF && c >= C / 2) ? sal_sigmoid(y[c]) : 1.f;
            }
            for (int c = 0; c < C; ++c) {
                float yc = 0.f;
#pragma unroll
                for (int k = 0; k < kPdpTail; ++k) yc = k == c ? y[k] : yc;
                float g[kPdpTail];
#pragma unroll
                for (int k = 0; k < kPdpTail; ++k) {
                    if (out_kind == NPBNN_OUT_SOFTMAX) g[k] = k < C ? yc * ((k == c ? 1.f : 0.f) - y[k]) : 0.f;
                    else g[k] = k == c ? yc : 0.f;
                }
                float g0[H0P];
                if (L == 1) {
#pragma unroll
                    for (int k = 0; k < H0P; ++k) g0[k] = k < kPdpTail ? g[k < kPdpTail ? k : 0] : 0.f;
                } else {
                    if (p.final_act) {
#pragma unroll
                        for (int k = 0; k < kPdpTail; ++k) g[k] *= fac[((L - 1) * kPdpTail + k) * kPdpRows];
                    }
                    for (int l = L - 1; l >= 2; --l) {
                        float gp[kPdpTail];
                        sal_dense_t<kPdpTail>(g, gp, w + p.t_off[l], p.t_out[l], p.t_inp[l]);
#pragma unroll
                        for (int k = 0; k < kPdpTail; ++k) g[k] = gp[k] * fac[((l - 1) * kPdpTail + k) * kPdpRows];
                    }
                    sal_dense_t<H0P>(g, g0, w + p.t_off[1], p.t_out[1], p.t_inp[1]);
                }
                float4* dst = reinterpret_cast<float4*>(a.D + (((size_t)S * C + c) * a.rows_cap + r) * H0P);
#pragma unroll
                for (int k = 0; k < H0P; k += 4)
                    dst[k / 4] = make_float4(g0[k] * d0[k], g0[k + 1] * d0[k + 1], g0[k + 2] * d0[k + 2], g0[k + 3] * d0[k + 3]);
            }
            sal_sets<S + 1>(p, a, z0, stail, r);
        }
    }
}

// grid (ceil(rows of the chunk / 256)), block 256, dynamic LDS Fp H0P + n_set tail_floats floats
template <int H0P, int NS>
__global__ __launch_bounds__(kPdpRows) void sal_route1_kernel(const PdpParams p, const SalParams a) {
    extern __shared__ float4 pdp_lds[];
    float* stail = reinterpret_cast<float*>(pdp_lds) + (size_t)p.Fp * H0P;
    const int tid = threadIdx.x;
    const long long r = (long long)blockIdx.x * kPdpRows + tid;
    const long long row = a.row0 + r;
    const bool live = row < p.n_rows && r < a.rows_cap;
    for (int i = tid; i < p.n_set * p.tail_floats; i += kPdpRows) stail[i] = p.tail[(size_t)p.set0 * p.tail_floats + i];

    float z0[NS][H0P];
    pdp_layer0<0>(p, z0, live, row);
    __syncthreads();      // (the tails of every set are in LDS)
    if (!live) return;
    sal_sets<0>(p, a, z0, stail, r);
}

// ---- phase 1, route 2

struct SalPlain {
    const float* X;
    long long n_rows, row0;
    int rows_cap;
    int set0;              // the launch's set among the prepared ones
    int c0, n_c;           // the outputs of this launch; the forward pass runs with c0 == 0 and stays in the scratches
    int a_off[kMaxLayers];
    float* act;            // [a_off[l] + unit][rows_cap]: a layer's values after its activation (the last layer's: the output side)
    float* fac;            // likewise: a'(z), 1 where the layer has no activation
    float* g;              // [2][max_w][rows_cap]: the gradient at two neighbouring layers
    float* D;              // [n_c][rows_cap][H0P]
};

// grid (ceil(rows of the chunk / 256)), block 256: one thread per row, every width at run time; the weights are read at wave-uniform
// addresses, the scratches at consecutive ones.
__global__ __launch_bounds__(256) void sal_plain_kernel(const PlainNet p, const SalPlain a) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = a.row0 + r;
    if (r >= a.rows_cap || row >= a.n_rows) return;
    const size_t R = (size_t)a.rows_cap;
    const int L = p.n_layers, C = p.C, kind = p.act_kind;
    const float* tail = p.tail + (size_t)a.set0 * p.tail_floats;
    float* act = a.act + r;
    float* fac = a.fac + r;
    float* y = act + (size_t)a.a_off[L - 1] * R;
    const int out_kind = p.apply_out ? p.out_kind : NPBNN_OUT_IDENTITY;
    if (a.c0 == 0) {
        const float4* xr = reinterpret_cast<const float4*>(a.X + row * p.Fp);
        const float* w0t = p.w0t + (size_t)a.set0 * p.Fp * p.H0P;
        const float* bias = p.bias + (size_t)a.set0 * p.H0P;
        const float* sl = p.slopes + (size_t)a.set0 * kMaxLayers;
        const bool act0 = L > 1 || p.final_act;
        const int H0 = p.width[0];
        for (int h0 = 0; h0 < H0; h0 += 8) {
            float z[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) z[e] = bias[h0 + e];
            for (int f4 = 0; f4 < p.Fp / 4; ++f4) {
                const float4 x = xr[f4];
                const float* w = w0t + (size_t)f4 * 4 * p.H0P + h0;
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    z[e] = fmaf(x.w, w[3 * p.H0P + e], fmaf(x.z, w[2 * p.H0P + e], fmaf(x.y, w[p.H0P + e], fmaf(x.x, w[e], z[e]))));
            }
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (h0 + e < H0) {
                    act[(size_t)(h0 + e) * R] = act0 ? act_apply(z[e], kind, sl[0]) : z[e];
                    fac[(size_t)(h0 + e) * R] = act0 ? dact(z[e], kind, sl[0]) : 1.f;
                }
        }
        plain_later_layers(p, tail, sl, act, fac, R, [&](int l) { return a.a_off[l]; });
        // the output side, in place: softmax - the probabilities; softplus-half - the factor sigma(z) (1 on the first half); else 1
        if (out_kind == NPBNN_OUT_SOFTMAX) {
            out_softmax<0>(C, [&](int c) -> float& { return y[(size_t)c * R]; });
        } else {
            for (int c = 0; c < C; ++c) y[(size_t)c * R] = (out_kind == NPBNN_OUT_SOFTPLUS_HALF && c >= C / 2) ? sal_sigmoid(y[(size_t)c * R]) : 1.f;
        }
    }
    const float* f_last = fac + (size_t)a.a_off[L - 1] * R;
    for (int c = a.c0; c < a.c0 + a.n_c; ++c) {
        float* g = a.g + r;
        float* gn = g + (size_t)p.max_w * R;
        const float yc = y[(size_t)c * R];
        for (int k = 0; k < C; ++k) {
            const float v = out_kind == NPBNN_OUT_SOFTMAX ? yc * ((k == c ? 1.f : 0.f) - y[(size_t)k * R]) : (k == c ? yc : 0.f);
            g[(size_t)k * R] = v * f_last[(size_t)k * R];
        }
        for (int l = L - 1; l >= 1; --l) {
            const int n_in = p.width[l - 1], n_out = p.width[l], inp = p.t_inp[l];
            const float* wm = tail + p.t_off[l] + ((n_out + 3) & ~3);
            const float* fp = fac + (size_t)a.a_off[l - 1] * R;
            for (int i = 0; i < n_in; ++i) {
                float s = 0.f;
                for (int o = 0; o < n_out; ++o) s = fmaf(wm[(size_t)o * inp + i], g[(size_t)o * R], s);
                gn[(size_t)i * R] = s * fp[(size_t)i * R];
            }
            float* t = g; g = gn; gn = t;
        }
        float* d = a.D + ((size_t)(c - a.c0) * R + r) * p.H0P;
        for (int h = 0; h < p.H0P; ++h) d[h] = h < p.width[0] ? g[(size_t)h * R] : 0.f;
    }
}

// ---- phase 2

struct SalFold {
    const float* D;        // [n_sc][rows_cap][H0P]: phase 1's derivatives of the launch's (set, output) pairs
    const float* w0t;      // [set][Fp][H0P]
    double* part;          // [n_sc][n_slot][3][Fq]
    int rows;              // rows of the chunk that are rows of the table
    int rows_cap, H0P, Fp, Fq, n_c, set0, n_slot;
};

// grid (ceil(n_slot / 4), ceil(Fq / 128), n_sc), block 256: wave `slot` folds the chunk's rows 256 slot .. 256 slot + 255 into the sums
// of G, |G| and G^2 of up to four tiles of 32 features.  Per tile of 32 rows, G = D W0^T on v_mfma_f32_32x32x2_f32: lane (j, g) =
// (lane & 31, lane >> 5) supplies row j of D as A and feature j of W0^T as B, hidden unit 32 kc + 8 q + 4 g + e at step (kc, q, e) -
// a float4 of either operand is four steps - and receives the rows (reg & 3) + 8 (reg >> 2) + 4 g of feature j.  KCH: the 32-wide
// K chunks of H0P when W0^T's fragments stay in registers over the rows (1, 2); 0: any H0P, the fragments read again per tile.
template <int KCH>
__global__ __launch_bounds__(256) void sal_fold_kernel(const SalFold q) {
    constexpr int NB = kSalNB, NK = KCH > 0 ? KCH : 1;
    const int lane = threadIdx.x & 63, slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= q.n_slot) return;                                     // (wave-uniform; the kernel has no barrier)
    const int j = lane & 31, g = lane >> 5;
    const int sc = blockIdx.z, s = sc / q.n_c;
    const int f0 = blockIdx.y * 32 * NB;
    const int n_t = min(NB, (q.Fq - f0) / 32);
    const int H0P = q.H0P, n_kc = H0P / 32;
    const float* w0 = q.w0t + (size_t)(q.set0 + s) * q.Fp * H0P + 4 * g;
    const float* Dsc = q.D + (size_t)sc * q.rows_cap * H0P + 4 * g;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    float4 b[NB][NK][4];
    auto load_b = [&](int kc, int slot_k) {
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const int f = f0 + 32 * t + j;
            const bool on = t < n_t && f < q.Fp;
#pragma unroll
            for (int u = 0; u < 4; ++u) b[t][slot_k][u] = on ? *reinterpret_cast<const float4*>(w0 + (size_t)f * H0P + 32 * kc + 8 * u) : zero4;
        }
    };
    if (KCH > 0) {
#pragma unroll
        for (int kc = 0; kc < NK; ++kc) load_b(kc, kc);
    }
    double sum[NB][3];
#pragma unroll
    for (int t = 0; t < NB; ++t) sum[t][0] = sum[t][1] = sum[t][2] = 0.0;

    const int r_end = min(q.rows, (slot + 1) * kSalWaveRows);
    for (int r0 = slot * kSalWaveRows; r0 < r_end; r0 += 32) {
        f32x16 acc[NB];
#pragma unroll
        for (int t = 0; t < NB; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
        const int r = r0 + j;
        const float* dr = Dsc + (size_t)r * H0P;
        auto step = [&](int kc, int slot_k) {
            float4 a4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a4[u] = r < q.rows ? *reinterpret_cast<const float4*>(dr + 32 * kc + 8 * u) : zero4;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float av[4] = {a4[u].x, a4[u].y, a4[u].z, a4[u].w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < NB; ++t)
                        if (t < n_t) {
                            const float4 bq = b[t][slot_k][u];
                            const float bv = e == 0 ? bq.x : e == 1 ? bq.y : e == 2 ? bq.z : bq.w;
                            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv, acc[t], 0, 0, 0);
                        }
            }
        };
        if (KCH > 0) {
#pragma unroll
            for (int kc = 0; kc < NK; ++kc) step(kc, kc);
        } else {
            for (int kc = 0; kc < n_kc; ++kc) {
                load_b(kc, 0);
                step(kc, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < NB; ++t)
            if (t < n_t) {
                float s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float v = acc[t][i];
                    s1 += v;
                    s2 += fabsf(v);
                    s3 = fmaf(v, v, s3);
                }
                sum[t][0] += (double)s1;
                sum[t][1] += (double)s2;
                sum[t][2] += (double)s3;
            }
    }
    double* dst = q.part + ((size_t)sc * q.n_slot + slot) * 3 * q.Fq + f0 + j;
#pragma unroll
    for (int t = 0; t < NB; ++t)
        if (t < n_t) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const double v = sum[t][m] + __shfl_down(sum[t][m], 32);
                if (g == 0) dst[(size_t)m * q.Fq + 32 * t] = v;
            }
        }
}

constexpr int kSalRuns = 16;                     // sal_reduce_kernel: runs of consecutive slots summed side by side
constexpr int kSalRunLanes = 256 / kSalRuns;     // ... and the sums a workgroup of it owns

// grid (ceil(n_sc 3 Fq / 16)), block 256: acc [3][n_sets][C][F] += the waves' partials part [n_sc][n_slot][3][Fq], in float64 and in a
// fixed order as ale_reduce_kernel adds its workgroups: the slots cut into 16 runs of consecutive ones, 16 threads add a run each in slot
// order (16 adjacent features per read), and the first of them adds the runs in run order.  Pair sc is set set0 + sc / n_c, output
// c0 + sc % n_c.  Features from F on are not written.
__global__ __launch_bounds__(256) void sal_reduce_kernel(const double* part, int n_sc, int n_slot, int Fq, int F, int C, int n_sets, int set0, int c0,
                                                         int n_c, double* acc) {
    __shared__ double runs[kSalRuns][kSalRunLanes];
    const int lane = threadIdx.x % kSalRunLanes, run = threadIdx.x / kSalRunLanes;
    const long long i = (long long)blockIdx.x * kSalRunLanes + lane;
    const bool live = i < (long long)n_sc * 3 * Fq;
    const int sc = (int)(i / (3ll * Fq)), m = (int)(i / Fq % 3), f = (int)(i % Fq);
    double sum = 0.0;
    if (live) {
        const int b1 = (int)((long long)(run + 1) * n_slot / kSalRuns);
        for (int b = (int)((long long)run * n_slot / kSalRuns); b < b1; ++b) sum += part[(((size_t)sc * n_slot + b) * 3 + m) * Fq + f];
    }
    runs[run][lane] = sum;
    __syncthreads();
    if (run != 0 || !live || f >= F) return;
    for (int r = 1; r < kSalRuns; ++r) sum += runs[r][lane];
    double* dst = acc + (((size_t)m * n_sets + set0 + sc / n_c) * C + c0 + sc % n_c) * F + f;
    *dst += sum;
}

}  // namespace

}  // namespace npbnn_api

// Saliency (include/npbnn_hip.h).  The sets are prepared group after group (pdp_prep_kernel with one bias point); per launch group of
// sets and chunk of rows: phase 1 (sal_route1_kernel or sal_plain_kernel), sal_fold_kernel, sal_reduce_kernel.
extern "C" int npbnn_predict_saliency(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, const double* col_override,
                                      int which, int apply_out_fn, double* out_mean, double* out_abs, double* out_sq) {
    using namespace npbnn_api;
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    ctx->saliency_route = 0;
    ctx->saliency_ns = 0;
    if (!W_sets || !out_mean || !out_abs || !out_sq || n_sets < 1) return fail(ctx, NPBNN_E_ARG, "predict_saliency: bad arguments");
    SetsTable tb;
    int rc = open_sets_table(ctx, "predict_saliency", which, &tb);
    if (rc) return rc;
    Dataset& d = *tb.d;
    const long long n_rows = tb.n_rows;
    if (n_rows < 1) return fail(ctx, NPBNN_E_ARG, "predict_saliency: the table has no rows");
    const int F = ctx->arch.in_dim, C = ctx->net.n_out, n_act = ctx->net.n_layers - 1, Fp = d.m->Fp;
    const size_t wn = (size_t)ctx->n_weights, n_res = (size_t)n_sets * C * F;
    hipStream_t st = ctx->stream;

    // ---- the route, the cut of the job and the buffers it needs (npbnn_attrib_plan.h)
    const npbnn_attrib_route r1 = plan_route(ctx, NPBNN_ATTRIB_SALIENCY, Fp, 1, "NPBNN_SALIENCY_PLAIN");
    const npbnn_attrib_sal_req req = {&r1, C, F, n_rows, n_sets, (long long)env_bytes("NPBNN_SALIENCY_SCRATCH_BYTES", kSalScratchBytes),
                                      (long long)env_bytes("NPBNN_SALIENCY_PREP_BYTES", kSalPrepBytes)};
    npbnn_attrib_sal cut;
    npbnn_attrib_sal_of(&req, &cut);
    const int route = r1.route, H0P = r1.H0P, NS = r1.NS, Fq = cut.Fq, n_c = cut.n_c, rows_cap = cut.rows_cap, prep_sets = cut.prep_sets;

    DevBuf<double> d_w, d_co, d_acc, d_part;
    DevBuf<float> d_D, d_fac, d_act, d_g;
    const std::vector<double> co = point_constants(F, col_override, nullptr, 0, nullptr, 1);
    if ((rc = upload_sets(ctx, W_sets, n_sets, co, d_w, d_co))) return rc;
    if ((rc = dev_alloc(ctx, d_acc, 3 * n_res))) return rc;
    if ((rc = dev_alloc(ctx, d_D, (size_t)cut.n_D))) return rc;
    if ((rc = dev_alloc(ctx, d_part, (size_t)cut.n_part))) return rc;
    if ((rc = dev_alloc(ctx, d_fac, (size_t)cut.n_fac))) return rc;
    if (route == 2) {
        if ((rc = dev_alloc(ctx, d_act, (size_t)cut.n_act))) return rc;
        if ((rc = dev_alloc(ctx, d_g, (size_t)cut.n_g))) return rc;
    }
    HIP_TRY(ctx, hipMemsetAsync(d_acc.get(), 0, 3 * n_res * sizeof(double), st));

    Route1Kernel<PdpParams, SalParams> kern;
    if (route == 1 && (rc = kern.pick(ctx, H0P, sal_route1_kernel<32, 2>, sal_route1_kernel<64, 1>, cut.lds_bytes))) return rc;
    SalParams a{};
    a.D = d_D.get(); a.fac = d_fac.get(); a.rows_cap = rows_cap;
    SalPlain k{};
    k.rows_cap = rows_cap; k.act = d_act.get(); k.fac = d_fac.get(); k.g = d_g.get(); k.D = d_D.get();
    for (int l = 0; l < r1.q.n_layers; ++l) k.a_off[l] = cut.a_off[l];
    FiTimer tm;
    double fold_ns = 0.0;
    Route1Blocks blocks1;
    for (int g0 = 0; g0 < n_sets; g0 += prep_sets) {
        const int ng = std::min(prep_sets, n_sets - g0);
        PdpParams p{};
        if ((rc = prepare_route1(ctx, r1, *d.m, d_w.get() + (size_t)g0 * wn, d_co.get(), act_prm_sets ? act_prm_sets + (size_t)g0 * n_act : nullptr, ng,
                                 apply_out_fn, &blocks1, &p)))
            return rc;
        const PlainNet net = plain_net(p, r1);
        k.X = p.X; k.n_rows = n_rows;
        for (int s0 = 0; s0 < ng; s0 += NS) {
            p.set0 = k.set0 = s0;
            p.n_set = std::min(NS, ng - s0);
            for (long long row0 = 0; row0 < n_rows; row0 += rows_cap) {
                const int rows = (int)std::min<long long>(rows_cap, n_rows - row0);
                const unsigned wgs = (unsigned)((rows + kPdpRows - 1) / kPdpRows);
                const int n_slot = (rows + kSalWaveRows - 1) / kSalWaveRows;
                a.row0 = k.row0 = row0;
                for (int c0 = 0; c0 < C; c0 += n_c) {
                    const int nc = std::min(n_c, C - c0);
                    if (route == 1) {
                        kern.launch(dim3(wgs), st, p, a);
                    } else {
                        k.c0 = c0; k.n_c = nc;
                        hipLaunchKernelGGL(sal_plain_kernel, dim3(wgs), dim3(256), 0, st, net, k);
                    }
                    HIP_TRY(ctx, hipGetLastError());
                    SalFold q{};
                    q.D = d_D.get(); q.w0t = p.w0t; q.part = d_part.get(); q.rows = rows; q.rows_cap = rows_cap; q.H0P = H0P; q.Fp = Fp;
                    q.Fq = Fq; q.n_c = nc; q.set0 = s0; q.n_slot = n_slot;
                    const int n_sc = p.n_set * nc;
                    const dim3 grid((unsigned)((n_slot + 3) / 4), (unsigned)((Fq + 32 * kSalNB - 1) / (32 * kSalNB)), (unsigned)n_sc);
                    tm.mark(0, st);
                    if (H0P == 32) hipLaunchKernelGGL((sal_fold_kernel<1>), grid, dim3(256), 0, st, q);
                    else if (H0P == 64) hipLaunchKernelGGL((sal_fold_kernel<2>), grid, dim3(256), 0, st, q);
                    else hipLaunchKernelGGL((sal_fold_kernel<0>), grid, dim3(256), 0, st, q);
                    HIP_TRY(ctx, hipGetLastError());
                    const unsigned rblocks = (unsigned)(((size_t)n_sc * 3 * Fq + kSalRunLanes - 1) / kSalRunLanes);
                    hipLaunchKernelGGL(sal_reduce_kernel, dim3(rblocks), dim3(256), 0, st, (const double*)d_part.get(), n_sc, n_slot, Fq, F, C, (int)n_sets,
                                       g0 + s0, c0, nc, d_acc.get());
                    HIP_TRY(ctx, hipGetLastError());
                    if (tm.on) {                       // (timing runs wait for every launch pair)
                        tm.mark(1, st);
                        HIP_TRY(ctx, hipStreamSynchronize(st));
                        fold_ns += tm.ns(0, 1);
                    }
                }
            }
        }
        // (the next group's blocks go into the same buffers: its preparation is behind these launches on the stream)
    }
    std::vector<double> host(3 * n_res);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), d_acc.get(), host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const double inv_n = 1.0 / (double)n_rows;
    for (size_t i = 0; i < n_res; ++i) {
        out_mean[i] = host[i] * inv_n;
        out_abs[i] = host[n_res + i] * inv_n;
        out_sq[i] = host[2 * n_res + i] * inv_n;
    }
    ctx->saliency_ns = fold_ns > (double)INT_MAX ? INT_MAX : (int)fold_ns;
    ctx->saliency_route = route;
    return NPBNN_OK;
}
