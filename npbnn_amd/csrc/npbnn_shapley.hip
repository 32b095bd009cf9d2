// Permutation-sampling Shapley attributions (npbnn_predict_shapley, include/npbnn_hip.h): per stored weight set s, explained row e,
// player p and output c the mean over the n_bg n_perm walks (b, pi) of f_s(after step k) - f_s(before step k), pi[k] = p.  A walk
// starts at background row b and sets the columns of one player after the other to the explained row's values, so layer 0's
// pre-activation moves by W0[:, j] (x_ej - b_j) per column: H0 multiply-adds where a forward pass from the row takes F H0.
//
// The explained rows of a chunk and the background rows are gathered once into transposed buffers [feature][row]: 64 lanes read one
// feature of their 64 rows at consecutive addresses.  A direct pass (shap_direct_kernel / shap_direct_plain_kernel), one thread per
// row, gives f_s(x_e), f_s(b) and the walks' starting z0(b) [set][b][H0P].  Then the walk kernel: a lane owns one explained row, the
// 64 lanes of a wave share (set, b, pi); wave `unit` = (block of 64 rows, split q) runs the walks q W / n_split .. (q + 1) W / n_split
// - 1 of W = n_bg n_perm, b-major, one after the other, and adds each step's differences in float64 to its own block of partials
// [player][output][lane]: no other wave writes there.  Route 1 (networks inside npbnn_predict_pdp's route-1 envelope): the set's
// transposed first layer and later layers staged in LDS, z0 in registers, the later layers through pdp_forward.  Route 2 (every other
// network): runtime widths, z0 and the activations in a device scratch [unit][lane], the weights read at wave-uniform addresses.
// shap_fold_kernel adds the splits in split order, divides by W, and adds phi, phi^2 and the rows' |phi| to the float64 accumulators
// in set, row and chunk order.  No floating-point atomics: the same input gives the same bits.
#include "npbnn_route1.hip.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace npbnn_api {

namespace {

constexpr size_t kShapScratchBytes = 128ull << 20;   // device budget of the walks' partials (and route 2's scratches): a larger job runs
                                                     // in chunks of explained rows and launches of fewer sets
constexpr size_t kShapPhiBytes = 256ull << 20;       // budget of out_phi on the device
constexpr size_t kShapPrepBytes = 256ull << 20;      // device budget of the float32 blocks: more sets are prepared group after group
// (NPBNN_SHAPLEY_SCRATCH_BYTES, NPBNN_SHAPLEY_PHI_BYTES and NPBNN_SHAPLEY_PREP_BYTES override them; the cut itself is npbnn_attrib_shap_of's)

// dst [Fp][cap] <- the rows `rows` [n] of X [.][Fp_src], transposed; 0 on the padding (features from F on, rows from n on)
__global__ __launch_bounds__(256) void shap_gather_kernel(const float* X, int Fp_src, int F, const long long* rows, int n, int cap, int Fp, float* dst) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)Fp * cap) return;
    const int f = (int)(i / cap), r = (int)(i % cap);
    dst[i] = (f < F && r < n) ? X[rows[r] * Fp_src + f] : 0.f;
}

struct ShapWalk {
    const float* xeT;      // [Fp][e_cap]: the chunk's explained rows
    const float* xbT;      // [Fp][b_cap]: the background rows
    const float* z0b;      // [prepared set][n_bg][H0P]: layer 0's pre-activation of the background rows
    const int* perms;      // [n_perm][P]
    const int* pstart;     // [P + 1]: player p's columns are pcols[pstart[p] .. pstart[p + 1] - 1]
    const int* pcols;      // [F]
    const int* pskip;      // [P]: 1 - every column of the player is overridden
    double* part;          // [set of the launch][n_rb][n_split][P][C][64]
    int e_cap, b_cap, rows, n_bg, n_perm, P, n_rb, n_split, W;
};

// grid (ceil(n_rb n_split / 4), sets of the launch), block 256, dynamic LDS (Fp H0P + tail_floats) floats
template <int H0P>
__global__ __launch_bounds__(256) void shap_walk_kernel(const PdpParams p, const ShapWalk a) {
    extern __shared__ float4 pdp_lds[];
    float* sw0 = reinterpret_cast<float*>(pdp_lds);
    float* stail = sw0 + (size_t)p.Fp * H0P;
    const int set = p.set0 + blockIdx.y;
    {
        const float4* src = reinterpret_cast<const float4*>(p.w0t + (size_t)set * p.Fp * H0P);
        for (int i = threadIdx.x; i < p.Fp * H0P / 4; i += 256) pdp_lds[i] = src[i];
        for (int i = threadIdx.x; i < p.tail_floats; i += 256) stail[i] = p.tail[(size_t)set * p.tail_floats + i];
    }
    __syncthreads();
    const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (unit >= a.n_rb * a.n_split) return;                           // (wave-uniform; no barrier below)
    const int lane = threadIdx.x & 63, rb = unit / a.n_split, q = unit % a.n_split;
    const int e = rb * 64 + lane;
    const bool live = e < a.rows;
    const int C = p.C, P = a.P;
    const float* sl = p.slopes + (size_t)set * kMaxLayers;
    const float* xe = a.xeT + e;                                      // (e < e_cap: a multiple of 64; zeros behind the chunk's rows)
    double* dst = a.part + (((size_t)blockIdx.y * a.n_rb + rb) * a.n_split + q) * ((size_t)P * C * 64) + lane;
    const int w0 = (int)((long long)q * a.W / a.n_split), w1 = (int)((long long)(q + 1) * a.W / a.n_split);
    for (int w = w0; w < w1; ++w) {
        const int b = w / a.n_perm;
        const int* pi = a.perms + (size_t)(w % a.n_perm) * P;
        const float* zb = a.z0b + ((size_t)set * a.n_bg + b) * H0P;
        float z0[H0P], h[H0P], prev[kPdpTail], y[kPdpTail];
#pragma unroll
        for (int k = 0; k < H0P; ++k) h[k] = z0[k] = zb[k];
        pdp_forward<H0P>(p, h, stail, sl, prev);
        for (int k = 0; k < P; ++k) {
            const int pl = pi[k];
            double* d = dst + (size_t)pl * C * 64;
            if (a.pskip[pl]) {                                        // (wave-uniform)
                if (w == w0 && live)
                    for (int c = 0; c < C; ++c) d[c * 64] = 0.0;
                continue;
            }
            for (int t = a.pstart[pl]; t < a.pstart[pl + 1]; ++t) {
                const int j = a.pcols[t];
                const float dx = xe[(size_t)j * a.e_cap] - a.xbT[(size_t)j * a.b_cap + b];
                const float* wj = sw0 + (size_t)j * H0P;
#pragma unroll
                for (int u = 0; u < H0P; u += 4) {
                    const float4 v = *reinterpret_cast<const float4*>(wj + u);
                    z0[u] = fmaf(v.x, dx, z0[u]); z0[u + 1] = fmaf(v.y, dx, z0[u + 1]);
                    z0[u + 2] = fmaf(v.z, dx, z0[u + 2]); z0[u + 3] = fmaf(v.w, dx, z0[u + 3]);
                }
            }
#pragma unroll
            for (int u = 0; u < H0P; ++u) h[u] = z0[u];
            pdp_forward<H0P>(p, h, stail, sl, y);
#pragma unroll
            for (int c = 0; c < kPdpTail; ++c)
                if (c < C) {
                    const double diff = (double)(y[c] - prev[c]);
                    prev[c] = y[c];
                    if (live) d[c * 64] = w == w0 ? diff : d[c * 64] + diff;
                }
        }
    }
}

struct ShapDirect {
    const float* xT;       // [Fp][cap]
    int cap, n;
    float* z0out;          // [prepared set][n][H0P], or nullptr
    float* fout;           // [set of the call][f_stride][C] from row f_row0 on
    long long f_stride, f_row0;
    int f_set0;            // the launch's first set among the call's
};

// grid (ceil(n / 256), sets of the launch), block 256: one thread per row, layer 0 from the transposed rows and the set's W0^T in
// global memory (wave-uniform addresses), then pdp_forward
template <int H0P>
__global__ __launch_bounds__(256) void shap_direct_kernel(const PdpParams p, const ShapDirect a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int set = p.set0 + blockIdx.y;
    const float* w0 = p.w0t + (size_t)set * p.Fp * H0P;
    const float* bias = p.bias + (size_t)set * H0P;
    float z[H0P], y[kPdpTail];
#pragma unroll
    for (int k = 0; k < H0P; ++k) z[k] = bias[k];
    for (int f = 0; f < p.Fp; ++f) {
        const float x = a.xT[(size_t)f * a.cap + i];
        const float* wf = w0 + (size_t)f * H0P;
#pragma unroll
        for (int k = 0; k < H0P; ++k) z[k] = fmaf(wf[k], x, z[k]);
    }
    if (a.z0out) {
        float* zo = a.z0out + ((size_t)set * a.n + i) * H0P;
#pragma unroll
        for (int k = 0; k < H0P; ++k) zo[k] = z[k];
    }
    pdp_forward<H0P>(p, z, p.tail + (size_t)set * p.tail_floats, p.slopes + (size_t)set * kMaxLayers, y);
    float* fo = a.fout + (((size_t)a.f_set0 + blockIdx.y) * a.f_stride + a.f_row0 + i) * p.C;
#pragma unroll
    for (int c = 0; c < kPdpTail; ++c)
        if (c < p.C) fo[c] = y[c];
}

// ---- route 2: runtime widths, the values of a wave's 64 rows in a scratch [unit][value][lane]

struct ShapPlain {
    int set0;              // the launch's first set among the prepared ones
    float* scr;            // [unit][H0 + 2 max_w + C][64]: z0, two layers' values, the previous step's outputs
};

// z0 [H0][64] -> the prediction, in va [2][max_w][64]; returns where.  Every address but the lane's offset is wave-uniform.
__device__ __forceinline__ float* shap_plain_forward(const PlainNet& k, int set, const float* z0, float* va) {
    const int L = k.n_layers, max_w = k.max_w;
    const float* sl = k.slopes + (size_t)set * kMaxLayers;
    const bool act0 = L > 1 || k.final_act;
    for (int i = 0; i < k.width[0]; ++i) va[i * 64] = act0 ? act_apply(z0[i * 64], k.act_kind, sl[0]) : z0[i * 64];
    // (layer l's values go to the half of va the layer before it did not write)
    plain_later_layers(k, k.tail + (size_t)set * k.tail_floats, sl, va, nullptr, 64, [&](int l) { return (l & 1) * max_w; });
    float* cur = va + (size_t)((L - 1) & 1) * max_w * 64;
    if (k.apply_out) out_function<0>(k.out_kind, k.C, [&](int c) -> float& { return cur[c * 64]; });
    return cur;
}

// grid (ceil(n / 256), sets of the launch), block 256: shap_direct_kernel with runtime widths; wave (set, 64 rows) owns scratch unit
// (blockIdx.y gridDim.x + blockIdx.x) 4 + wave
__global__ __launch_bounds__(256) void shap_direct_plain_kernel(const PlainNet k, const ShapPlain u, const ShapDirect a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int set = u.set0 + blockIdx.y, H0 = k.width[0], H0P = k.H0P;
    const size_t unit = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + (threadIdx.x >> 6);
    float* z0 = u.scr + unit * (size_t)(H0 + 2 * k.max_w + k.C) * 64 + (threadIdx.x & 63);
    float* va = z0 + (size_t)H0 * 64;
    const float* w0 = k.w0t + (size_t)set * k.Fp * H0P;
    const float* bias = k.bias + (size_t)set * H0P;
    for (int h0 = 0; h0 < H0; h0 += 8) {                              // (H0P is a multiple of 32: h0 + 7 < H0P)
        float z[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) z[u] = bias[h0 + u];
        for (int f = 0; f < k.Fp; ++f) {
            const float x = a.xT[(size_t)f * a.cap + i];
            const float* wf = w0 + (size_t)f * H0P + h0;
#pragma unroll
            for (int u = 0; u < 8; ++u) z[u] = fmaf(wf[u], x, z[u]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (h0 + u < H0) {
                z0[(h0 + u) * 64] = z[u];
                if (a.z0out) a.z0out[((size_t)set * a.n + i) * H0P + h0 + u] = z[u];
            }
    }
    const float* y = shap_plain_forward(k, set, z0, va);
    float* fo = a.fout + (((size_t)a.f_set0 + blockIdx.y) * a.f_stride + a.f_row0 + i) * k.C;
    for (int c = 0; c < k.C; ++c) fo[c] = y[c * 64];
}

// grid (ceil(n_rb n_split / 4), sets of the launch), block 256: shap_walk_kernel with runtime widths; wave (set, unit) owns scratch
// unit blockIdx.y n_rb n_split + unit
__global__ __launch_bounds__(256) void shap_walk_plain_kernel(const PlainNet k, const ShapPlain u, const ShapWalk a) {
    const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (unit >= a.n_rb * a.n_split) return;                           // (wave-uniform; the kernel has no barrier)
    const int lane = threadIdx.x & 63, rb = unit / a.n_split, q = unit % a.n_split;
    const int e = rb * 64 + lane;
    const bool live = e < a.rows;
    const int set = u.set0 + blockIdx.y, C = k.C, P = a.P, H0 = k.width[0], H0P = k.H0P;
    const size_t su = (size_t)blockIdx.y * a.n_rb * a.n_split + unit;
    float* z0 = u.scr + su * (size_t)(H0 + 2 * k.max_w + C) * 64 + lane;
    float* va = z0 + (size_t)H0 * 64;
    float* prev = va + 2 * (size_t)k.max_w * 64;
    const float* w0 = k.w0t + (size_t)set * k.Fp * H0P;
    const float* xe = a.xeT + e;
    double* dst = a.part + (((size_t)blockIdx.y * a.n_rb + rb) * a.n_split + q) * ((size_t)P * C * 64) + lane;
    const int w0i = (int)((long long)q * a.W / a.n_split), w1i = (int)((long long)(q + 1) * a.W / a.n_split);
    for (int w = w0i; w < w1i; ++w) {
        const int b = w / a.n_perm;
        const int* pi = a.perms + (size_t)(w % a.n_perm) * P;
        const float* zb = a.z0b + ((size_t)set * a.n_bg + b) * H0P;
        for (int u = 0; u < H0; ++u) z0[u * 64] = zb[u];
        {
            const float* y = shap_plain_forward(k, set, z0, va);
            for (int c = 0; c < C; ++c) prev[c * 64] = y[c * 64];
        }
        for (int s = 0; s < P; ++s) {
            const int pl = pi[s];
            double* d = dst + (size_t)pl * C * 64;
            if (a.pskip[pl]) {                                        // (wave-uniform)
                if (w == w0i && live)
                    for (int c = 0; c < C; ++c) d[c * 64] = 0.0;
                continue;
            }
            for (int t = a.pstart[pl]; t < a.pstart[pl + 1]; ++t) {
                const int j = a.pcols[t];
                const float dx = xe[(size_t)j * a.e_cap] - a.xbT[(size_t)j * a.b_cap + b];
                const float* wj = w0 + (size_t)j * H0P;
                for (int u = 0; u < H0; ++u) z0[u * 64] = fmaf(wj[u], dx, z0[u * 64]);
            }
            const float* y = shap_plain_forward(k, set, z0, va);
            for (int c = 0; c < C; ++c) {
                const float yc = y[c * 64];
                const double diff = (double)(yc - prev[c * 64]);
                prev[c * 64] = yc;
                if (live) d[c * 64] = w == w0i ? diff : d[c * 64] + diff;
            }
        }
    }
}

// ---- the fold, both routes

struct ShapFold {
    const double* part;    // [set of the launch][n_rb][n_split][PC][64]
    double* mean;          // [PC][E]: sum over the sets of phi, and of phi^2
    double* sq;
    double* abs;           // [n_sets][PC]: sum over the rows of |phi|
    double* phi;           // [n_sets][PC][E], or nullptr
    long long E, e0;       // explained rows of the call, first of the chunk
    int rows, n_rb, n_split, PC, n_set, set0;   // the chunk's rows; the launch's sets and the first one among the call's
    double inv_w;
};

// grid (PC), block 256: pair pc of every set of the launch, in set order.  A thread takes the chunk's rows tid, tid + 256, ...: phi is
// the sum of the splits in split order over W; a row's sums over the sets belong to one thread in every launch, and the launches of a
// call follow each other in set order on one stream.  |phi| is added over a thread's rows in row order, then over the workgroup by
// block_sum, then by thread 0 to the set's sum - in chunk order over the launches.
__global__ __launch_bounds__(kFiThreads) void shap_fold_kernel(const ShapFold q) {
    __shared__ double lds[kFiWaves];
    const int pc = blockIdx.x;
    for (int s = 0; s < q.n_set; ++s) {
        double sum_abs = 0.0;
        for (int e = threadIdx.x; e < q.rows; e += kFiThreads) {
            const double* src = q.part + (((size_t)s * q.n_rb + e / 64) * q.n_split * q.PC + pc) * 64 + e % 64;
            double v = 0.0;
            for (int k = 0; k < q.n_split; ++k) v += src[(size_t)k * q.PC * 64];
            v *= q.inv_w;
            const size_t at = (size_t)pc * q.E + q.e0 + e;
            q.mean[at] += v;
            q.sq[at] += v * v;
            if (q.phi) q.phi[((size_t)(q.set0 + s) * q.PC) * q.E + at] = v;
            sum_abs += fabs(v);
        }
        const double tot = block_sum(sum_abs, lds);
        if (threadIdx.x == 0) q.abs[(size_t)(q.set0 + s) * q.PC + pc] += tot;
    }
}

}  // namespace

}  // namespace npbnn_api

extern "C" int npbnn_predict_shapley(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, const double* col_override,
                                     int which, const int64_t* rows, int32_t n_explain, int which_bg, const int64_t* bg_rows, int32_t n_bg,
                                     const int32_t* player_of, int32_t n_players, const int32_t* perms, int32_t n_perm, int apply_out_fn,
                                     double* out_mean, double* out_sq, double* out_abs, double* out_fx, double* out_base, double* out_phi) {
    using namespace npbnn_api;
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    ctx->shapley_route = 0;
    ctx->shapley_ns = 0;
    if (!W_sets || !rows || !bg_rows || !perms || !out_mean || !out_sq || !out_abs || !out_fx || !out_base)
        return fail(ctx, NPBNN_E_ARG, "predict_shapley: a required pointer is null");
    if (n_sets < 1 || n_explain < 1 || n_bg < 1 || n_perm < 1 || n_players < 1)
        return fail(ctx, NPBNN_E_ARG, "predict_shapley: n_sets, n_explain, n_bg, n_perm and n_players must be at least 1");
    SetsTable tb, tg;
    int rc = open_sets_table(ctx, "predict_shapley", which, &tb);
    if (rc) return rc;
    if ((rc = open_sets_table(ctx, "predict_shapley", which_bg, &tg))) return rc;
    const FeatureTable& mx = *tb.d->m;
    const FeatureTable& mb = *tg.d->m;
    const int F = ctx->arch.in_dim, C = ctx->net.n_out, n_act = ctx->net.n_layers - 1, Fp = mx.Fp, P = n_players;
    for (int i = 0; i < n_explain; ++i)
        if (rows[i] < 0 || rows[i] >= tb.n_rows) return fail(ctx, NPBNN_E_ARG, "predict_shapley: rows[%d] = %lld is outside the table's %lld rows", i, (long long)rows[i], tb.n_rows);
    for (int i = 0; i < n_bg; ++i)
        if (bg_rows[i] < 0 || bg_rows[i] >= tg.n_rows)
            return fail(ctx, NPBNN_E_ARG, "predict_shapley: bg_rows[%d] = %lld is outside the table's %lld rows", i, (long long)bg_rows[i], tg.n_rows);
    if (!player_of && P != F) return fail(ctx, NPBNN_E_ARG, "predict_shapley: without player_of n_players must be in_dim = %d", F);
    // the players' columns, and which players have none but overridden ones
    std::vector<int> pstart((size_t)P + 1, 0), pcols((size_t)F), pskip((size_t)P, 1);
    for (int f = 0; f < F; ++f) {
        const int pl = player_of ? player_of[f] : f;
        if (pl < 0 || pl >= P) return fail(ctx, NPBNN_E_ARG, "predict_shapley: player_of[%d] = %d is outside 0 .. %d", f, pl, P - 1);
        ++pstart[(size_t)pl + 1];
    }
    for (int p = 0; p < P; ++p) {
        if (pstart[(size_t)p + 1] == 0) return fail(ctx, NPBNN_E_ARG, "predict_shapley: player %d has no column", p);
        pstart[(size_t)p + 1] += pstart[p];
    }
    {
        std::vector<int> fill(pstart.begin(), pstart.end() - 1);
        for (int f = 0; f < F; ++f) {
            const int pl = player_of ? player_of[f] : f;
            pcols[(size_t)fill[pl]++] = f;
            if (!col_override || std::isnan(col_override[f])) pskip[pl] = 0;
        }
        std::vector<char> seen((size_t)P);
        for (int r = 0; r < n_perm; ++r) {
            std::fill(seen.begin(), seen.end(), 0);
            for (int k = 0; k < P; ++k) {
                const int v = perms[(size_t)r * P + k];
                if (v < 0 || v >= P || seen[v]) return fail(ctx, NPBNN_E_ARG, "predict_shapley: row %d of perms is not a permutation of 0 .. %d", r, P - 1);
                seen[v] = 1;
            }
        }
    }
    const size_t PC = (size_t)P * C, E = (size_t)n_explain, wn = (size_t)ctx->n_weights;
    hipStream_t st = ctx->stream;

    // ---- the route, the cut of the job and the buffers it needs (npbnn_attrib_plan.h)
    const npbnn_attrib_route r1 = plan_route(ctx, NPBNN_ATTRIB_SHAPLEY, Fp, 1, "NPBNN_SHAPLEY_PLAIN");
    const npbnn_attrib_shap_req req = {&r1, C, P, n_explain, n_bg, n_perm, n_sets, ctx->n_cu, out_phi ? 1 : 0,
                                       (long long)env_bytes("NPBNN_SHAPLEY_SCRATCH_BYTES", kShapScratchBytes),
                                       (long long)env_bytes("NPBNN_SHAPLEY_PREP_BYTES", kShapPrepBytes),
                                       (long long)env_bytes("NPBNN_SHAPLEY_PHI_BYTES", kShapPhiBytes)};
    npbnn_attrib_shap cut;
    switch (npbnn_attrib_shap_of(&req, &cut)) {
        case NPBNN_ATTRIB_E_PHI:
            return fail(ctx, NPBNN_E_NOMEM, "predict_shapley: out_phi of %d sets x %d rows x %d players x %d outputs is over its budget of %zu bytes; at most %zu explained rows fit",
                        n_sets, n_explain, P, C, (size_t)req.phi_bytes, (size_t)cut.phi_rows_fit);
        case NPBNN_ATTRIB_E_WALKS:
            return fail(ctx, NPBNN_E_ARG, "predict_shapley: n_bg x n_perm = %lld walks are more than %d", cut.walks, INT_MAX);
        default: break;
    }
    const int route = r1.route, H0P = r1.H0P, n_split = cut.n_split, nsl = cut.nsl, e_cap = cut.e_cap, b_cap = cut.b_cap, prep_sets = cut.prep_sets;

    std::vector<int> ints;                                            // perms | pstart | pcols | pskip
    ints.insert(ints.end(), perms, perms + (size_t)n_perm * P);
    ints.insert(ints.end(), pstart.begin(), pstart.end());
    ints.insert(ints.end(), pcols.begin(), pcols.end());
    ints.insert(ints.end(), pskip.begin(), pskip.end());
    std::vector<long long> idx((size_t)n_explain + n_bg);
    for (int i = 0; i < n_explain; ++i) idx[i] = rows[i];
    for (int i = 0; i < n_bg; ++i) idx[(size_t)n_explain + i] = bg_rows[i];

    DevBuf<double> d_w, d_co, d_part, d_mean, d_abs, d_phi;
    DevBuf<float> d_xeT, d_xbT, d_z0b, d_fx, d_fb, d_scr;
    DevBuf<int> d_ints;
    DevBuf<long long> d_idx;
    const std::vector<double> co = point_constants(F, col_override, nullptr, 0, nullptr, 1);
    if ((rc = upload_sets(ctx, W_sets, n_sets, co, d_w, d_co))) return rc;
    if ((rc = dev_alloc(ctx, d_ints, ints.size()))) return rc;
    if ((rc = dev_alloc(ctx, d_idx, idx.size()))) return rc;
    if ((rc = dev_alloc(ctx, d_xeT, (size_t)cut.n_xeT))) return rc;
    if ((rc = dev_alloc(ctx, d_xbT, (size_t)cut.n_xbT))) return rc;
    if ((rc = dev_alloc(ctx, d_z0b, (size_t)cut.n_z0b))) return rc;
    if ((rc = dev_alloc(ctx, d_fx, (size_t)cut.n_fx))) return rc;
    if ((rc = dev_alloc(ctx, d_fb, (size_t)cut.n_fb))) return rc;
    if ((rc = dev_alloc(ctx, d_part, (size_t)cut.n_part))) return rc;
    if ((rc = dev_alloc(ctx, d_mean, (size_t)cut.n_mean))) return rc;
    if ((rc = dev_alloc(ctx, d_abs, (size_t)cut.n_abs))) return rc;
    if (out_phi && (rc = dev_alloc(ctx, d_phi, (size_t)cut.n_phi))) return rc;
    if (route == 2 && (rc = dev_alloc(ctx, d_scr, (size_t)cut.n_scr))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_ints.get(), ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_idx.get(), idx.data(), idx.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(d_mean.get(), 0, (size_t)cut.n_mean * sizeof(double), st));
    HIP_TRY(ctx, hipMemsetAsync(d_abs.get(), 0, (size_t)cut.n_abs * sizeof(double), st));
    hipLaunchKernelGGL(shap_gather_kernel, dim3((unsigned)(((size_t)cut.n_xbT + 255) / 256)), dim3(256), 0, st, (const float*)mb.X.get(), mb.Fp, F,
                       (const long long*)d_idx.get() + n_explain, (int)n_bg, b_cap, Fp, d_xbT.get());
    HIP_TRY(ctx, hipGetLastError());

    Route1Kernel<PdpParams, ShapWalk> walk;
    Route1Kernel<PdpParams, ShapDirect> direct1;
    if (route == 1) {
        if ((rc = walk.pick(ctx, H0P, shap_walk_kernel<32>, shap_walk_kernel<64>, cut.lds_bytes))) return rc;
        if ((rc = direct1.pick(ctx, H0P, shap_direct_kernel<32>, shap_direct_kernel<64>, 0))) return rc;
    }
    ShapWalk a{};
    a.xeT = d_xeT.get(); a.xbT = d_xbT.get(); a.z0b = d_z0b.get();
    a.perms = d_ints.get(); a.pstart = a.perms + (size_t)n_perm * P; a.pcols = a.pstart + P + 1; a.pskip = a.pcols + F;
    a.part = d_part.get(); a.e_cap = e_cap; a.b_cap = b_cap; a.n_bg = n_bg; a.n_perm = n_perm; a.P = P; a.n_split = n_split; a.W = cut.W;
    ShapFold q{};
    q.part = d_part.get(); q.mean = d_mean.get(); q.sq = d_mean.get() + PC * E; q.abs = d_abs.get(); q.phi = out_phi ? d_phi.get() : nullptr;
    q.E = (long long)E; q.n_split = n_split; q.PC = (int)PC; q.inv_w = 1.0 / (double)cut.W;

    FiTimer tm;
    double walk_ns = 0.0;
    Route1Blocks blocks1;
    PdpParams p{};
    PlainNet k{};
    ShapPlain u{};
    u.scr = d_scr.get();
    // one launch of a direct kernel: the sets s0 .. s0 + ns - 1 of the prepared group on the n rows of xT
    auto direct = [&](int s0, int ns, const ShapDirect& dk) {
        const dim3 grid((unsigned)((dk.n + 255) / 256), (unsigned)ns);
        p.set0 = u.set0 = s0;
        if (route == 1) direct1.launch(grid, st, p, dk);
        else hipLaunchKernelGGL(shap_direct_plain_kernel, grid, dim3(256), 0, st, k, u, dk);
    };
    // Groups of prepared sets outside, chunks of explained rows inside: a group is prepared once.  A row's sums over the sets still grow
    // in set order, a set's sum of |phi| in chunk order.  (A group's blocks go into the same buffers as the one before: its preparation
    // is behind those launches on the stream.  With more than one group a chunk's rows are gathered once per group.)
    for (int g0 = 0; g0 < n_sets; g0 += prep_sets) {
        const int ng = std::min(prep_sets, n_sets - g0);
        if ((rc = prepare_route1(ctx, r1, mx, d_w.get() + (size_t)g0 * wn, d_co.get(), act_prm_sets ? act_prm_sets + (size_t)g0 * n_act : nullptr, ng,
                                 apply_out_fn, &blocks1, &p)))
            return rc;
        k = plain_net(p, r1);
        // the background rows: z0(b) and f(b) of the group's sets
        for (int s0 = 0; s0 < ng; s0 += nsl) {
            ShapDirect dk{};
            dk.xT = d_xbT.get(); dk.cap = b_cap; dk.n = n_bg; dk.z0out = d_z0b.get(); dk.fout = d_fb.get(); dk.f_stride = n_bg; dk.f_row0 = 0;
            dk.f_set0 = g0 + s0;
            direct(s0, std::min(nsl, ng - s0), dk);
            HIP_TRY(ctx, hipGetLastError());
        }
        for (long long e0 = 0; e0 < n_explain; e0 += e_cap) {
            const int rows_c = (int)std::min<long long>(e_cap, n_explain - e0);
            if (g0 == 0 || e_cap < n_explain) {            // (one chunk: its rows stay gathered from the first group on)
                hipLaunchKernelGGL(shap_gather_kernel, dim3((unsigned)(((size_t)cut.n_xeT + 255) / 256)), dim3(256), 0, st, (const float*)mx.X.get(), mx.Fp,
                                   F, (const long long*)d_idx.get() + e0, rows_c, e_cap, Fp, d_xeT.get());
                HIP_TRY(ctx, hipGetLastError());
            }
            a.rows = rows_c; a.n_rb = (rows_c + 63) / 64;
            q.rows = rows_c; q.n_rb = a.n_rb; q.e0 = e0;
            for (int s0 = 0; s0 < ng; s0 += nsl) {
                const int ns = std::min(nsl, ng - s0);
                ShapDirect dk{};
                dk.xT = d_xeT.get(); dk.cap = e_cap; dk.n = rows_c; dk.z0out = nullptr; dk.fout = d_fx.get(); dk.f_stride = (long long)E; dk.f_row0 = e0;
                dk.f_set0 = g0 + s0;
                direct(s0, ns, dk);
                HIP_TRY(ctx, hipGetLastError());
                const dim3 grid((unsigned)((a.n_rb * n_split + 3) / 4), (unsigned)ns);
                tm.mark(0, st);
                if (route == 1) walk.launch(grid, st, p, a);
                else hipLaunchKernelGGL(shap_walk_plain_kernel, grid, dim3(256), 0, st, k, u, a);
                HIP_TRY(ctx, hipGetLastError());
                tm.mark(1, st);
                q.n_set = ns; q.set0 = g0 + s0;
                hipLaunchKernelGGL(shap_fold_kernel, dim3((unsigned)PC), dim3(kFiThreads), 0, st, q);
                HIP_TRY(ctx, hipGetLastError());
                if (tm.on) {                           // (timing runs wait for every launch)
                    HIP_TRY(ctx, hipStreamSynchronize(st));
                    walk_ns += tm.ns(0, 1);
                }
            }
        }
    }
    std::vector<double> h_mean((size_t)cut.n_mean), h_abs((size_t)cut.n_abs), h_phi((size_t)cut.n_phi);
    std::vector<float> h_fx((size_t)cut.n_fx), h_fb((size_t)cut.n_fb);
    HIP_TRY(ctx, hipMemcpyAsync(h_mean.data(), d_mean.get(), h_mean.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(h_abs.data(), d_abs.get(), h_abs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(h_fx.data(), d_fx.get(), h_fx.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(h_fb.data(), d_fb.get(), h_fb.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    if (out_phi) HIP_TRY(ctx, hipMemcpyAsync(h_phi.data(), d_phi.get(), h_phi.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    // the device keeps the explained rows innermost: [pair][row] -> [row][pair]
    const double inv_s = 1.0 / (double)n_sets, inv_e = 1.0 / (double)n_explain;
    for (size_t e = 0; e < E; ++e)
        for (size_t pc = 0; pc < PC; ++pc) {
            out_mean[e * PC + pc] = h_mean[pc * E + e] * inv_s;
            out_sq[e * PC + pc] = h_mean[PC * E + pc * E + e] * inv_s;
        }
    for (size_t i = 0; i < h_abs.size(); ++i) out_abs[i] = h_abs[i] * inv_e;
    for (size_t i = 0; i < h_fx.size(); ++i) out_fx[i] = (double)h_fx[i];
    for (int s = 0; s < n_sets; ++s)
        for (int c = 0; c < C; ++c) {
            double sum = 0.0;
            for (int b = 0; b < n_bg; ++b) sum += (double)h_fb[((size_t)s * n_bg + b) * C + c];
            out_base[(size_t)s * C + c] = sum / (double)n_bg;
        }
    if (out_phi)
        for (size_t s = 0; s < (size_t)n_sets; ++s)
            for (size_t e = 0; e < E; ++e)
                for (size_t pc = 0; pc < PC; ++pc) out_phi[(s * E + e) * PC + pc] = h_phi[(s * PC + pc) * E + e];
    ctx->shapley_ns = walk_ns > (double)INT_MAX ? INT_MAX : (int)walk_ns;
    ctx->shapley_route = route;
    return NPBNN_OK;
}
