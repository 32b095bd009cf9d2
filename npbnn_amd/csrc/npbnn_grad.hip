// The log-likelihood and its gradient with respect to the weights (npbnn_loglik_grad, include/npbnn_hip.h): out_grad = sum over the
// table's rows of d l_i / d W, in packed-weight order.  One route, every network the library takes at runtime widths; a launch runs
// in two phases over a chunk of rows.
//
// Phase 1, grad_rows_kernel, one thread per row, the shape of sal_plain_kernel: the forward pass from the float32 blocks of saliency's
// route 2 (pdp_prep_kernel with one bias point: the overridden columns are folded into layer 0's bias), the row's log-likelihood term,
// and the backward pass of that scalar down to layer 0.  It leaves in scratches [unit][row of the chunk] every layer's values after
// the activation (act: the next layer's inputs), the derivative factors a'(z) (fac) and every layer's delta = d l_i / d z (dl), and
// layer 0's delta once more row-major, D0 [row][H0P], so that phase 2 reads it coalesced.  The workgroup's 256 log-likelihood terms
// and residual moments are added in float64 in a fixed order (block_sum) into the slot's partials.
//
// Phase 2, the products dW_l = delta_l^T h_(l-1), whose reduction dimension is the rows.  Layer 0, grad_fold_kernel: [H0P x rows] .
// [rows x Fp] against X itself on v_mfma_f32_32x32x2_f32; lane (j, g) = (lane & 31, lane >> 5) supplies D0[row 2k + g][h0 + j] as A
// and X[row 2k + g][f0 + j] as B, both 128-byte coalesced reads; a wave owns a slot of kGradSlotRows = 256 consecutive rows, 32
// hidden units and up to kGradNB = 4 tiles of 32 features, so X is read once in phase 1 and once per 32 hidden units here.  The same
// lanes add their A values: layer 0's bias sums.  The later layers, grad_later_kernel: one thread per weight and slot.
//
// Sums over rows run in float32 inside one slot only; a slot's sums are float64 partials part [slot][n_tot] in HBM, and
// grad_reduce_kernel adds the slots in a fixed order (sal_reduce_kernel's: 16 runs of consecutive slots) into acc [n_tot], chunk
// after chunk.  No atomics: the same input gives the same bits.  The host multiplies by lik_temp, puts c_j times layer 0's bias sum
// on the overridden columns and forms the Gaussian log-likelihood from the moments, as finalize_kernel does.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950) are in NOTES 8.22.
#include "npbnn_route1.hip.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

namespace npbnn_api {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kGradNB = 4;                            // feature tiles of 32 a wave of grad_fold_kernel carries
constexpr size_t kGradScratchBytes = 128ull << 20;    // device budget of the scratches and the partials: a larger table runs in chunks
                                                      // of rows (NPBNN_GRAD_SCRATCH_BYTES overrides it; the cut is npbnn_attrib_grad_of's)
static_assert(kGradSlotRows == kFiThreads, "a workgroup of phase 1 is one slot: block_sum adds its rows");

// The buffers of a call.  The context keeps them from call to call (npbnn_ctx::grad_work): an optimiser calls the entry hundreds of
// times on one table, and allocating them costs more than the kernels take.  They grow when a call needs more, and go when a table
// of the context is replaced (forget_rows, npbnn_capi.hip) and with the context: up to the scratch budget and the blocks until then.
struct GradWork {
    DevBuf<double> w, co, acc, part;
    DevBuf<float> act, fac, dl, D0;
    DevBuf<int> flag;
    Route1Blocks blocks;
};

// ---- phase 1

struct GradRows {
    const float* X;
    long long n_rows, row0;
    int rows_cap;
    int a_off[kMaxLayers];
    float* act;            // [a_off[l] + unit][rows_cap]: a layer's values after its activation
    float* fac;            // likewise: a'(z), 1 where the layer has no activation
    float* dl;             // likewise: d l_i / d z of the unit (without lik_temp)
    float* D0;             // [rows_cap][H0P]: layer 0's delta, zero on the padding
    double* part;          // [slot][n_tot]
    int n_tot, lik_off;
    const int* labels;
    const float* targets;
    const float* inst_w;   // or nullptr
    const double* classw;  // or nullptr
    int n_classw;
    int lik, k;
    float inv_s2[NPBNN_MAX_TARGETS];   // NPBNN_LIK_GAUSS: 1 / sigma_t^2
    int* flag;
};

// grid (slots of the chunk), block 256
__global__ __launch_bounds__(256) void grad_rows_kernel(const PlainNet p, const GradRows a) {
    __shared__ double lds[kFiWaves];
    const int r = blockIdx.x * kGradSlotRows + threadIdx.x;
    const long long row = a.row0 + r;
    const bool live = r < a.rows_cap && row < a.n_rows;
    const size_t R = (size_t)a.rows_cap;
    const int L = p.n_layers, C = p.C, kind = p.act_kind, k = a.k;
    float* act = a.act + r;
    float* fac = a.fac + r;
    float* dl = a.dl + r;
    float* y = act + (size_t)a.a_off[L - 1] * R;
    double term = 0.0;
    if (live) {
        const float4* xr = reinterpret_cast<const float4*>(a.X + row * p.Fp);
        const float* sl = p.slopes;
        const bool act0 = L > 1 || p.final_act;
        const int H0 = p.width[0];
        for (int h0 = 0; h0 < H0; h0 += 8) {
            float z[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) z[e] = p.bias[h0 + e];
            for (int f4 = 0; f4 < p.Fp / 4; ++f4) {
                const float4 x = xr[f4];
                const float* w = p.w0t + (size_t)f4 * 4 * p.H0P + h0;
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
        plain_later_layers(p, p.tail, sl, act, fac, R, [&](int l) { return a.a_off[l]; });

        // the row's term and d l_i / d y, times the last layer's factor: the last layer's delta
        const float* f_last = fac + (size_t)a.a_off[L - 1] * R;
        float* d_last = dl + (size_t)a.a_off[L - 1] * R;
        if (a.lik == NPBNN_LIK_CATEGORICAL) {
            const int lab = a.labels[row];
            if (lab < 0 || lab >= C) {
                *a.flag = kFlagBadLabel;                               // (every writer writes the same word)
                for (int c = 0; c < C; ++c) d_last[(size_t)c * R] = 0.f;
            } else {
                float m = -3.402823466e38f;
                for (int c = 0; c < C; ++c) m = fmaxf(m, y[(size_t)c * R]);
                float s = 0.f;
                for (int c = 0; c < C; ++c) s += __expf(y[(size_t)c * R] - m);
                float w = 1.f;
                if (a.inst_w) w *= a.inst_w[row];
                if (a.classw && lab < a.n_classw) w *= (float)a.classw[lab];
                const float inv = 1.f / s;
                for (int c = 0; c < C; ++c) {
                    const float pc = __expf(y[(size_t)c * R] - m) * inv;
                    d_last[(size_t)c * R] = w * ((c == lab ? 1.f : 0.f) - pc) * f_last[(size_t)c * R];
                }
                term = (double)w * ((double)(y[(size_t)lab * R] - m) - (double)logf(s));
            }
        } else if (a.lik == NPBNN_LIK_GAUSS) {
            for (int t = 0; t < k; ++t) d_last[(size_t)t * R] = (a.targets[row * k + t] - y[(size_t)t * R]) * a.inv_s2[t] * f_last[(size_t)t * R];
        } else {
            for (int t = 0; t < k; ++t) {
                const double res = (double)a.targets[row * k + t] - (double)y[(size_t)t * R];
                const double zs = (double)y[(size_t)(k + t) * R];
                const double sg = fmax(zs, 0.0) + log1p(exp(-fabs(zs)));      // softplus, as the evaluation kernels have it
                const double q = res / sg;
                term += -0.9189385332046727418 - log(sg) - 0.5 * q * q;
                d_last[(size_t)t * R] = (float)(res / (sg * sg)) * f_last[(size_t)t * R];
                d_last[(size_t)(k + t) * R] = (float)((q * q - 1.0) / sg / (1.0 + exp(-zs))) * f_last[(size_t)(k + t) * R];
            }
        }
        // back through the later layers: delta_(l-1) = (W_l^T delta_l) a'(z_(l-1))
        for (int l = L - 1; l >= 1; --l) {
            const int n_in = p.width[l - 1], n_out = p.width[l], inp = p.t_inp[l];
            const float* wm = p.tail + p.t_off[l] + ((n_out + 3) & ~3);
            const float* g = dl + (size_t)a.a_off[l] * R;
            float* gn = dl + (size_t)a.a_off[l - 1] * R;
            const float* fp = fac + (size_t)a.a_off[l - 1] * R;
            for (int i = 0; i < n_in; ++i) {
                float s = 0.f;
                for (int o = 0; o < n_out; ++o) s = fmaf(wm[(size_t)o * inp + i], g[(size_t)o * R], s);
                gn[(size_t)i * R] = s * fp[(size_t)i * R];
            }
        }
        float* d = a.D0 + (size_t)r * p.H0P;
        for (int h = 0; h < p.H0P; ++h) d[h] = h < H0 ? dl[(size_t)h * R] : 0.f;
    }
    // the slot's log-likelihood terms and residual moments (every thread of the workgroup takes part in the sums)
    double* lik = a.part + (size_t)blockIdx.x * a.n_tot + a.lik_off;
    const double s0 = block_sum(term, lds);
    if (threadIdx.x == 0) lik[0] = s0;
    for (int t = 0; t < NPBNN_MAX_TARGETS; ++t) {
        double res = 0.0;
        if (a.lik == NPBNN_LIK_GAUSS && t < k && live) res = (double)a.targets[row * k + t] - (double)y[(size_t)t * R];
        const bool on = a.lik == NPBNN_LIK_GAUSS && t < k;               // (workgroup-uniform)
        const double s1 = on ? block_sum(res, lds) : 0.0;
        const double s2 = on ? block_sum(res * res, lds) : 0.0;
        if (threadIdx.x == 0) {
            lik[1 + t] = s1;
            lik[1 + NPBNN_MAX_TARGETS + t] = s2;
        }
    }
}

// ---- phase 2, layer 0

struct GradFold {
    const float* D0;       // [rows_cap][H0P]
    const float* X;        // the table, Fp floats a row
    double* part;          // [slot][n_tot]
    long long row0;        // the chunk's first row in the table
    int rows;              // rows of the chunk that are rows of the table
    int H0P, H0, Fp, F, hb0, n_slot, n_tot, bsum_off;
};

// grid (ceil(n_slot / 4), ceil(Fp / 128), H0P / 32), block 256: wave `slot` adds, over the chunk's rows 256 slot .. 256 slot + 255,
// D0^T X for the hidden units h0 .. h0 + 31 and up to four tiles of 32 features.  Per pair of rows one v_mfma_f32_32x32x2_f32 a tile:
// lane (j, g) supplies D0[row + g][h0 + j] as A and X[row + g][f + j] as B and receives the hidden units (reg & 3) + 8 (reg >> 2) + 4 g
// of feature j.  The waves of the first feature group also add their A values: the bias sums of layer 0.
__global__ __launch_bounds__(256) void grad_fold_kernel(const GradFold q) {
    constexpr int NB = kGradNB;
    const int lane = threadIdx.x & 63, slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= q.n_slot) return;                                     // (wave-uniform; the kernel has no barrier)
    const int j = lane & 31, g = lane >> 5;
    const int f0 = blockIdx.y * 32 * NB, h0 = blockIdx.z * 32;
    const int n_t = min(NB, (q.Fp - f0 + 31) / 32);
    const float* dcol = q.D0 + h0 + j;
    const float* xcol = q.X + (size_t)q.row0 * q.Fp + f0 + j;
    bool fon[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) fon[t] = f0 + 32 * t + j < q.Fp;

    f32x16 acc[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    float bs = 0.f;
    const int r_end = min(q.rows, (slot + 1) * kGradSlotRows);
    for (int r0 = slot * kGradSlotRows; r0 < r_end; r0 += 8) {
        float av[4], bv[4][NB];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + 2 * u + g;
            const bool ok = r < r_end;
            av[u] = ok ? dcol[(size_t)r * q.H0P] : 0.f;
#pragma unroll
            for (int t = 0; t < NB; ++t) bv[u][t] = ok && fon[t] ? xcol[(size_t)r * q.Fp + 32 * t] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            bs += av[u];
#pragma unroll
            for (int t = 0; t < NB; ++t)
                if (t < n_t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u][t], acc[t], 0, 0, 0);
        }
    }
    double* dst = q.part + (size_t)slot * q.n_tot;
    const int stride = q.F + q.hb0;
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const int f = f0 + 32 * t + j;
        if (t < n_t && f < q.F) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int h = h0 + (i & 3) + 8 * (i >> 2) + 4 * g;
                if (h < q.H0) dst[(size_t)h * stride + q.hb0 + f] = (double)acc[t][i];
            }
        }
    }
    const double b = (double)bs + __shfl_down((double)bs, 32);
    if (blockIdx.y == 0 && g == 0) {
        const int h = h0 + j;
        dst[q.bsum_off + h] = b;                                      // (h < H0P; 0 on the padding, where D0 is 0)
        if (q.hb0 && h < q.H0) dst[(size_t)h * stride] = b;
    }
}

// ---- phase 2, the later layers

struct GradLater {
    const float* act;
    const float* dl;
    double* part;
    int rows, rows_cap, n_tot, n_layers, n_later;
    int a_off[kMaxLayers], width[kMaxLayers], hb[kMaxLayers], woff[kMaxLayers];
};

// grid (n_slot, ceil(n_later / 256)), block 256: thread e of a slot owns weight e of the later layers' n_later and adds delta_l[o] h_(l-1)[i]
// (delta_l[o] alone on a bias column) over the slot's rows in four interleaved float32 sums, added in float64.
__global__ __launch_bounds__(256) void grad_later_kernel(const GradLater q) {
    int e = blockIdx.y * 256 + threadIdx.x;
    if (e >= q.n_later) return;
    int l = 1;
    for (; l < q.n_layers - 1; ++l) {
        const int cnt = q.width[l] * (q.width[l - 1] + q.hb[l]);
        if (e < cnt) break;
        e -= cnt;
    }
    const int stride = q.width[l - 1] + q.hb[l];
    const int o = e / stride, c = e % stride;
    const size_t R = (size_t)q.rows_cap;
    const float* dp = q.dl + (size_t)(q.a_off[l] + o) * R;
    const bool bias = q.hb[l] && c == 0;
    const float* ip = q.act + (size_t)(q.a_off[l - 1] + (bias ? 0 : c - q.hb[l])) * R;
    const int r0 = blockIdx.x * kGradSlotRows, r1 = min(q.rows, r0 + kGradSlotRows);
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = r0; r < r1; r += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (r + u < r1) s[u] = bias ? s[u] + dp[r + u] : fmaf(dp[r + u], ip[r + u], s[u]);
    }
    q.part[(size_t)blockIdx.x * q.n_tot + q.woff[l] + e] = ((double)s[0] + (double)s[1]) + ((double)s[2] + (double)s[3]);
}

// ---- the slots' partials into the totals

constexpr int kGradRuns = 16;                    // grad_reduce_kernel: runs of consecutive slots summed side by side
constexpr int kGradRunLanes = 256 / kGradRuns;   // ... and the sums a workgroup of it owns

// grid (ceil(n_tot / 16)), block 256: acc [n_tot] += part [n_slot][n_tot], in float64 and in a fixed order as sal_reduce_kernel adds its
// waves: the slots cut into 16 runs of consecutive ones, 16 threads add a run each in slot order, and the first of them adds the
// runs in run order.
__global__ __launch_bounds__(256) void grad_reduce_kernel(const double* part, int n_slot, int n_tot, double* acc) {
    __shared__ double runs[kGradRuns][kGradRunLanes];
    const int lane = threadIdx.x % kGradRunLanes, run = threadIdx.x / kGradRunLanes;
    const int i = blockIdx.x * kGradRunLanes + lane;
    const bool live = i < n_tot;
    double sum = 0.0;
    if (live) {
        const int b1 = (int)((long long)(run + 1) * n_slot / kGradRuns);
        for (int b = (int)((long long)run * n_slot / kGradRuns); b < b1; ++b) sum += part[(size_t)b * n_tot + i];
    }
    runs[run][lane] = sum;
    __syncthreads();
    if (run != 0 || !live) return;
    for (int r = 1; r < kGradRuns; ++r) sum += runs[r][lane];
    acc[i] += sum;
}

}  // namespace

}  // namespace npbnn_api

extern "C" int npbnn_loglik_grad(npbnn_ctx* ctx, const double* W_packed, const double* act_prm, const double* col_override, double lik_temp,
                                 const double* sigma, int which, npbnn_eval_out* out, double* out_grad) {
    using namespace npbnn_api;
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    ctx->grad_ns[0] = ctx->grad_ns[1] = 0;
    if (!W_packed || !out || !out_grad) return fail(ctx, NPBNN_E_ARG, "loglik_grad: null weights, out or out_grad");
    SetsTable tb;
    int rc = open_sets_table(ctx, "loglik_grad", which, &tb);
    if (rc) return rc;
    if (ctx->shard_n > 0) return fail(ctx, NPBNN_E_STATE, "loglik_grad: the context holds a share of the rows (npbnn_set_row_shard)");
    const int lik = ctx->net.lik_kind;
    static const char* const kCountNames[] = {"NPBNN_LIK_POISSON", "NPBNN_LIK_NEGBIN", "NPBNN_LIK_NEGBIN2D", "NPBNN_LIK_NEGBIN_BASE10", "NPBNN_LIK_NONE"};
    if (lik != NPBNN_LIK_CATEGORICAL && lik != NPBNN_LIK_GAUSS && lik != NPBNN_LIK_GAUSS_PRED_SIGMA)
        return fail(ctx, NPBNN_E_ARG, "loglik_grad: no gradient for %s",
                    lik >= NPBNN_LIK_POISSON && lik <= NPBNN_LIK_NONE ? kCountNames[lik - NPBNN_LIK_POISSON] : "this likelihood");
    Dataset& d = *tb.d;
    if ((rc = check_dataset_for_lik(ctx, d, lik))) return rc;
    const long long n_rows = tb.n_rows;
    if (n_rows < 1) return fail(ctx, NPBNN_E_ARG, "loglik_grad: the table has no rows");
    const int F = ctx->arch.in_dim, C = ctx->net.n_out, L = ctx->arch.n_layers, Fp = d.m->Fp, k = lik == NPBNN_LIK_CATEGORICAL ? 0 : ctx->net.k_targets;
    if (lik == NPBNN_LIK_GAUSS && !sigma) return fail(ctx, NPBNN_E_ARG, "loglik_grad: NPBNN_LIK_GAUSS needs sigma (the empirical sigma has no gradient here)");
    if (lik == NPBNN_LIK_GAUSS && C != k) return fail(ctx, NPBNN_E_ARG, "loglik_grad: %d outputs for %d targets", C, k);
    if (lik == NPBNN_LIK_GAUSS_PRED_SIGMA && C != 2 * k) return fail(ctx, NPBNN_E_ARG, "loglik_grad: NPBNN_LIK_GAUSS_PRED_SIGMA needs out_dim = 2 k, got %d for k = %d", C, k);
    const int wn = ctx->n_weights;
    hipStream_t st = ctx->stream;

    // ---- the blocks' shapes (saliency's route 2), the cut of the job and the buffers it needs (npbnn_attrib_plan.h)
    const npbnn_attrib_route_req rreq = {&ctx->arch, wn, Fp, 1, ctx->wide ? 1 : 0, 1, NPBNN_ATTRIB_SALIENCY};
    npbnn_attrib_route r2{};
    npbnn_attrib_route_of(&rreq, &r2);
    const npbnn_attrib_grad_req req = {&r2, wn, n_rows, (long long)env_bytes("NPBNN_GRAD_SCRATCH_BYTES", kGradScratchBytes)};
    npbnn_attrib_grad cut;
    npbnn_attrib_grad_of(&req, &cut);
    const int H0P = r2.H0P, H0 = r2.q.H0, hb0 = r2.q.hb0, rows_cap = cut.rows_cap, n_tot = cut.n_tot;

    if (!ctx->grad_work) ctx->grad_work = std::make_shared<GradWork>();
    GradWork& wk = *static_cast<GradWork*>(ctx->grad_work.get());
    DevBuf<double>&d_w = wk.w, &d_co = wk.co, &d_acc = wk.acc, &d_part = wk.part;
    DevBuf<float>&d_act = wk.act, &d_fac = wk.fac, &d_dl = wk.dl, &d_D0 = wk.D0;
    DevBuf<int>& d_flag = wk.flag;
    const std::vector<double> co = point_constants(F, col_override, nullptr, 0, nullptr, 1);
    if ((rc = upload_sets(ctx, W_packed, 1, co, d_w, d_co))) return rc;
    if ((rc = dev_alloc(ctx, d_acc, (size_t)cut.n_acc))) return rc;
    if ((rc = dev_alloc(ctx, d_part, (size_t)cut.n_part))) return rc;
    if ((rc = dev_alloc(ctx, d_act, (size_t)cut.n_act))) return rc;
    if ((rc = dev_alloc(ctx, d_fac, (size_t)cut.n_fac))) return rc;
    if ((rc = dev_alloc(ctx, d_dl, (size_t)cut.n_dl))) return rc;
    if ((rc = dev_alloc(ctx, d_D0, (size_t)cut.n_D0))) return rc;
    if ((rc = dev_alloc(ctx, d_flag, 1))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_acc.get(), 0, (size_t)cut.n_acc * sizeof(double), st));
    HIP_TRY(ctx, hipMemsetAsync(d_flag.get(), 0, sizeof(int), st));

    Route1Blocks& blocks = wk.blocks;
    PdpParams p{};
    if ((rc = prepare_route1(ctx, r2, *d.m, d_w.get(), d_co.get(), act_prm, 1, 0, &blocks, &p))) return rc;
    const PlainNet net = plain_net(p, r2);

    GradRows a{};
    a.X = p.X; a.n_rows = n_rows; a.rows_cap = rows_cap;
    a.act = d_act.get(); a.fac = d_fac.get(); a.dl = d_dl.get(); a.D0 = d_D0.get(); a.part = d_part.get();
    a.n_tot = n_tot; a.lik_off = cut.lik_off;
    a.labels = d.labels; a.targets = d.targets;
    a.inst_w = which == 0 ? d.inst_w.get() : nullptr;
    a.classw = which == 0 && ctx->n_classw > 0 ? ctx->d_classw.get() : nullptr;
    a.n_classw = ctx->n_classw;
    a.lik = lik; a.k = k; a.flag = d_flag.get();
    if (lik == NPBNN_LIK_GAUSS)
        for (int t = 0; t < k; ++t) a.inv_s2[t] = (float)(1.0 / (sigma[t] * sigma[t]));
    GradFold q{};
    q.D0 = d_D0.get(); q.X = p.X; q.part = d_part.get(); q.H0P = H0P; q.H0 = H0; q.Fp = Fp; q.F = F; q.hb0 = hb0; q.n_tot = n_tot;
    q.bsum_off = cut.bsum_off;
    GradLater lt{};
    lt.act = d_act.get(); lt.dl = d_dl.get(); lt.part = d_part.get(); lt.rows_cap = rows_cap; lt.n_tot = n_tot; lt.n_layers = L;
    const int n0 = H0 * (F + hb0);
    lt.n_later = wn - n0;
    for (int l = 0; l < L; ++l) {
        a.a_off[l] = lt.a_off[l] = cut.a_off[l];
        lt.width[l] = l ? r2.q.l_out[l] : H0;
        lt.hb[l] = l ? r2.q.l_hb[l] : hb0;
        lt.woff[l] = l ? r2.q.l_woff[l] : 0;
    }
    // (thread e of grad_later_kernel writes part[woff[l] + its index in layer l]: the layers follow one another from n0 on)

    FiTimer tm;
    double ns[2] = {0.0, 0.0};
    for (long long row0 = 0; row0 < n_rows; row0 += rows_cap) {
        const int rows = (int)std::min<long long>(rows_cap, n_rows - row0);
        const int n_slot = (rows + kGradSlotRows - 1) / kGradSlotRows;
        a.row0 = q.row0 = row0;
        q.rows = lt.rows = rows;
        q.n_slot = n_slot;
        tm.mark(0, st);
        hipLaunchKernelGGL(grad_rows_kernel, dim3((unsigned)n_slot), dim3(256), 0, st, net, a);
        HIP_TRY(ctx, hipGetLastError());
        tm.mark(1, st);
        hipLaunchKernelGGL(grad_fold_kernel, dim3((unsigned)((n_slot + 3) / 4), (unsigned)((Fp + 32 * kGradNB - 1) / (32 * kGradNB)), (unsigned)(H0P / 32)),
                           dim3(256), 0, st, q);
        HIP_TRY(ctx, hipGetLastError());
        if (lt.n_later > 0) {
            hipLaunchKernelGGL(grad_later_kernel, dim3((unsigned)n_slot, (unsigned)((lt.n_later + 255) / 256)), dim3(256), 0, st, lt);
            HIP_TRY(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL(grad_reduce_kernel, dim3((unsigned)((n_tot + kGradRunLanes - 1) / kGradRunLanes)), dim3(256), 0, st,
                           (const double*)d_part.get(), n_slot, n_tot, d_acc.get());
        HIP_TRY(ctx, hipGetLastError());
        if (tm.on) {                           // (timing runs wait for every chunk)
            tm.mark(2, st);
            HIP_TRY(ctx, hipStreamSynchronize(st));
            ns[0] += tm.ns(0, 1);
            ns[1] += tm.ns(1, 2);
        }
    }
    std::vector<double> host((size_t)n_tot);
    int flags = 0;
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), d_acc.get(), host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(&flags, d_flag.get(), sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (flags & kFlagBadLabel) return fail(ctx, NPBNN_E_ARG, "loglik_grad: a label outside [0, %d)", C);

    // ---- the totals into the outputs
    const double* bsum = host.data() + cut.bsum_off;
    const double* lk = host.data() + cut.lik_off;
    for (int i = 0; i < wn; ++i) out_grad[i] = lik_temp * host[i];
    for (int f = 0; f < F; ++f)
        if (!std::isnan(co[f]))
            for (int h = 0; h < H0; ++h) out_grad[(size_t)h * (F + hb0) + hb0 + f] = lik_temp * (co[f] * bsum[h]);
    npbnn_eval_out o{};
    o.n_rows = n_rows;
    if (lik == NPBNN_LIK_GAUSS) {
        // sum_t [ -N (0.5 log 2 pi + log s_t) - S2_t / (2 s_t^2) ], as loglik_from_totals has it
        const double N = (double)n_rows;
        double ll = 0.0;
        for (int t = 0; t < k; ++t) {
            o.sigma[t] = sigma[t]; o.sum_r[t] = lk[1 + t]; o.sum_r2[t] = lk[1 + NPBNN_MAX_TARGETS + t];
            ll += -N * (0.9189385332046727418 + std::log(sigma[t])) - o.sum_r2[t] / (2.0 * sigma[t] * sigma[t]);
        }
        o.loglik = lik_temp * ll;
    } else {
        o.loglik = lik_temp * lk[0];
    }
    *out = o;
    ctx->grad_ns[0] = ns[0] > (double)INT_MAX ? INT_MAX : (int)ns[0];
    ctx->grad_ns[1] = ns[1] > (double)INT_MAX ? INT_MAX : (int)ns[1];
    return NPBNN_OK;
}
