// C ABI of the gfx950 backend (see include/npbnn_hip.h for the contract and the reference
// functions each entry point replaces).  Host-side orchestration only: device buffers, launches,
// the HIP stream of the chain.  No torch, no BLAS library, no CPU fallback for the numerics.
#include <algorithm>
#include <memory>
#define NPBNN_KERNELS_MAIN
#include "npbnn_sets.hip.h"

namespace npbnn_api {

thread_local std::string g_last_error;

int fail(npbnn_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (ctx) ctx->err = buf;
    return code;
}

// What a context keeps for a table (labels, targets, weights, permuted columns) belongs to the matrix it came with, and goes with it.
void forget_rows(npbnn_ctx* ctx, int which) {
    ctx->grad_work.reset();      // (npbnn_loglik_grad's buffers were sized for the table that goes: the next call allocates for the new one)
    ctx->ds[which] = Dataset();
    ctx->ds[which].m = &ctx->store->table[which];
}

// The context lets go of the store it holds (freed here if nobody else holds it: the device is current) and holds `store` instead.
// taken: from another context (npbnn_share_data), not for its own uploads.
void hold_store(npbnn_ctx* ctx, std::shared_ptr<FeatureStore> store, bool taken) {
    ctx->store = std::move(store);
    ctx->store_taken = taken;
    forget_rows(ctx, 0);
    forget_rows(ctx, 1);
}

template <typename T>
int upload_matrix(npbnn_ctx* ctx, const T* X, int64_t n_rows, int32_t F, int which) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (!X || n_rows <= 0 || F <= 0 || (which != 0 && which != 1))
        return fail(ctx, NPBNN_E_ARG, "set_data: bad arguments (rows=%lld, features=%d, which=%d)",
                    (long long)n_rows, F, which);
    if (n_rows > (int64_t)1 << 30) return fail(ctx, NPBNN_E_ARG, "set_data: too many rows");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->store_taken && ctx->store.use_count() > 1)
        return fail(ctx, NPBNN_E_STATE, "set_data: %d other context(s) use this one's matrices (npbnn_share_data)", (int)ctx->store.use_count() - 1);
    if (ctx->store_taken)        // data of its own for a context that took another's: it lets go of both tables first
        hold_store(ctx, std::make_shared<FeatureStore>(ctx->device), false);
    ctx->store->table[which] = FeatureTable();
    forget_rows(ctx, which);
    Dataset& d = ctx->ds[which];
    if (which == 0) {            // the fp16-split scales come from the training matrix
        FeatureStore& fs = *ctx->store;
        fs.xscale.reset();
        fs.wscale.reset();
        fs.scale_F = 0;
        fs.table[1].X16.reset();
        fs.table[1].X16w.reset();
        fs.table[1].f16_state = 0;
    }
    d.m->n_rows = n_rows;
    d.m->F = F;
    d.m->Fp = round_up(F, 16);
    d.m->n_tiles = (int)((n_rows + 15) / 16);
    const size_t n_pad = (size_t)d.m->n_tiles * 16;
    if (int rc = d.m->X.reserve(ctx, n_pad * d.m->Fp)) return rc;
    // convert + pad on the host in slabs, so the staging buffer stays small
    const size_t slab_rows = 16384;
    std::vector<float> stage(slab_rows * d.m->Fp);
    for (size_t r0 = 0; r0 < n_pad; r0 += slab_rows) {
        const size_t nr = std::min(slab_rows, n_pad - r0);
        std::fill(stage.begin(), stage.begin() + nr * d.m->Fp, 0.0f);
        for (size_t r = 0; r < nr; ++r) {
            const size_t gr = r0 + r;
            if (gr >= (size_t)n_rows) break;
            const T* src = X + gr * F;
            float* dst = stage.data() + r * d.m->Fp;
            for (int c = 0; c < F; ++c) dst[c] = (float)src[c];
        }
        HIP_TRY(ctx, hipMemcpy(d.m->X + r0 * d.m->Fp, stage.data(), nr * d.m->Fp * sizeof(float), hipMemcpyHostToDevice));
    }
    // A net built on another training matrix is built again, as npbnn_set_arch would build it on this one: the choice of path reads
    // the row count (wide_needed) and the fp16-split positions of the chain's proposals carry the old matrix's column scales
    // (d_w2scale).  Float32 layout first, as npbnn_set_arch; plan_launch moves to fp16-split when it applies.
    if (which == 0 && ctx->arch_set) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return rebuild_net(ctx, false);
    }
    return NPBNN_OK;
}

int check_rows(npbnn_ctx* ctx, int which, int64_t n_rows, const char* what) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (which != 0 && which != 1) return fail(ctx, NPBNN_E_ARG, "%s: which must be 0 or 1", what);
    if (!ctx->ds[which].m->X) return fail(ctx, NPBNN_E_STATE, "%s: call npbnn_set_data first", what);
    if (ctx->ds[which].m->n_rows != n_rows)
        return fail(ctx, NPBNN_E_ARG, "%s: %lld rows but the data matrix has %lld", what, (long long)n_rows,
                    (long long)ctx->ds[which].m->n_rows);
    return NPBNN_OK;
}

int build_net(npbnn_ctx* ctx, const npbnn_arch* a, bool f16) {
    if (a->n_layers < 1 || a->n_layers > NPBNN_MAX_LAYERS)
        return fail(ctx, NPBNN_E_ARG, "set_arch: n_layers=%d outside 1..%d", a->n_layers, NPBNN_MAX_LAYERS);
    if (a->in_dim < 1) return fail(ctx, NPBNN_E_ARG, "set_arch: in_dim=%d", a->in_dim);
    if (a->act_kind < 0 || a->act_kind > NPBNN_ACT_TANH) return fail(ctx, NPBNN_E_ARG, "set_arch: act_kind=%d", a->act_kind);
    if (a->out_kind < 0 || a->out_kind > NPBNN_OUT_SOFTPLUS_HALF) return fail(ctx, NPBNN_E_ARG, "set_arch: out_kind=%d", a->out_kind);
    if (a->lik_kind < 0 || a->lik_kind > NPBNN_LIK_NONE) return fail(ctx, NPBNN_E_ARG, "set_arch: lik_kind=%d", a->lik_kind);
    for (int l = 0; l < a->n_layers; ++l)
        if (a->out_dim[l] < 1 || a->out_dim[l] > NPBNN_MAX_WIDTH)
            return fail(ctx, NPBNN_E_ARG, "set_arch: layer %d has %d nodes; this backend supports 1..%d per layer", l, a->out_dim[l],
                        NPBNN_MAX_WIDTH);
    {
        long long nw = 0;
        int in_l = a->in_dim;
        for (int l = 0; l < a->n_layers; ++l) { nw += (long long)a->out_dim[l] * (in_l + (a->has_bias[l] ? 1 : 0)); in_l = a->out_dim[l]; }
        if (nw >= (1ll << 31)) return fail(ctx, NPBNN_E_ARG, "set_arch: %lld weights; this backend indexes up to 2^31", nw);
    }
    // the resident image's layout (npbnn_resident_plan.h); the A/B timing switches are read here
    npbnn_resident_req req{};
    req.arch = a;
    req.f16 = f16;
    req.l0_blocks = ctx->l0_blocks.empty() ? nullptr : ctx->l0_blocks.data();
    req.has_classw = ctx->n_classw > 0;
    req.slopes_option = ctx->slopes_option;
    req.no_pad_mask = getenv("NPBNN_NO_PAD_MASK") != nullptr;
    req.no_l1_f16 = getenv("NPBNN_NO_L1_F16") != nullptr;
    req.no_tile_perm = getenv("NPBNN_NO_TILE_PERM") != nullptr;
    req.no_compact_rows = getenv("NPBNN_NO_COMPACT_ROWS") != nullptr;
    npbnn_resident_layout lay{};
    const int rc_lay = npbnn_resident_layout_of(&req, &lay);
    if (rc_lay == NPBNN_RESIDENT_E_ARG) return fail(ctx, NPBNN_E_INTERNAL, "set_arch: the layout rule refused a checked network (internal error)");
    NetMeta net{};
    net.n_layers = a->n_layers;
    net.act_kind = a->act_kind;
    net.out_kind = a->out_kind;
    net.lik_kind = a->lik_kind;
    net.k_targets = a->n_targets;
    net.final_act = a->final_act ? 1 : 0;
    net.l0_f16 = f16 ? 1 : 0;
    // Networks the LDS of a compute unit cannot hold (or a layer wider than the resident builds' tiles) run on the weight-streamed
    // path (npbnn_wide.hip): the description below then carries what the chain step and the likelihood need - shapes, offsets into
    // the packed weights, kinds - and none of the resident image's layout.
    ctx->wide = wide_needed(ctx, a, rc_lay, lay);
    int woff = 0;
    if (ctx->wide) {
        int in = a->in_dim;
        net.l0_rows = 16;
        for (int l = 0; l < a->n_layers; ++l) {
            LayerMeta& L = net.L[l];
            L.in_dim = in;
            L.out_dim = a->out_dim[l];
            L.has_bias = a->has_bias[l] ? 1 : 0;
            L.kt = (in + 15) / 16;
            L.mt = (L.out_dim + 15) / 16;
            L.in_live = 4;
            L.w_off = woff;
            woff += L.out_dim * (in + L.has_bias);
            in = L.out_dim;
        }
        net.classw_off = -1;
        net.slope_off = ctx->slopes_option ? 0 : -1;     // (>= 0 says "candidates carry their own slopes": the streamed kernels read them from the chain)
    } else {
        for (int l = 0; l < a->n_layers; ++l) net.L[l] = lay.L[l];
        for (int mt = 0; mt < kMaxMT; ++mt) { net.l0_begin[mt] = lay.l0_begin[mt]; net.l0_end[mt] = lay.l0_end[mt]; net.l0_base[mt] = lay.l0_base[mt]; }
        net.l0_rows = lay.l0_rows;
        net.l1_f16 = lay.l1_f16;
        net.pad_masked = lay.pad_masked;
        net.classw_off = lay.classw_off;
        net.slope_off = lay.slope_off;
        net.image_floats = lay.image_floats;
        woff = lay.n_weights;
    }
    net.n_out = a->out_dim[a->n_layers - 1];
    if (a->lik_kind == NPBNN_LIK_GAUSS) {
        if (a->n_targets < 1 || a->n_targets > NPBNN_MAX_TARGETS || a->n_targets > net.n_out)
            return fail(ctx, NPBNN_E_ARG, "set_arch: Gaussian likelihood needs 1..%d target columns (<= outputs), got %d",
                        NPBNN_MAX_TARGETS, a->n_targets);
    } else if (lik_needs_row_scratch(a->lik_kind)) {
        const int k = a->n_targets;
        int need_out = 1;
        if (a->lik_kind == NPBNN_LIK_GAUSS_PRED_SIGMA || a->lik_kind == NPBNN_LIK_NEGBIN2D) need_out = 2 * k;
        else if (a->lik_kind != NPBNN_LIK_POISSON) need_out = 2;
        if (k < 1 || k > 8 || net.n_out > 16 || net.n_out < need_out)
            return fail(ctx, NPBNN_E_ARG, "set_arch: likelihood kind %d needs 1..8 target columns and %d..16 outputs (got %d targets, %d outputs)",
                        a->lik_kind, need_out, k, net.n_out);
    }
    ctx->net = net;
    ctx->rlay = lay;
    ctx->n_weights = woff;
    ctx->mt0_template = net.L[0].mt;
    return NPBNN_OK;
}

WaveLayout layout_for(const npbnn_ctx* ctx, const Dataset& d, bool predict_only) {
    return make_wave_layout(d.labels != nullptr, d.inst_w != nullptr, d.targets ? ctx->net.k_targets : 0, ctx->net.L[0].kt,
                            predict_only ? NPBNN_LIK_NONE : ctx->net.lik_kind);
}

// the launch rule (npbnn_resident_plan.h) on the context's network, table and options; NPBNN_WAVES is the caller's to read
static int resident_launch(const npbnn_ctx* ctx, const Dataset& d, int want_cand, bool predict_only, bool lik_only, bool plain, int waves_override,
                           npbnn_resident_launch* out) {
    npbnn_resident_launch_req q{};
    q.has_labels = d.labels != nullptr;
    q.has_row_w = d.inst_w != nullptr;
    q.has_targets = d.targets != nullptr;
    q.n_tiles = d.m->n_tiles;
    q.n_cu = ctx->n_cu > 0 ? ctx->n_cu : 1;
    q.lds_limit = (int)ctx->lds_limit;
    q.want_cand = want_cand;
    q.predict_only = predict_only;
    q.lik_only = lik_only;
    q.plain = plain;
    q.fast_option = ctx->fast_option;
    q.waves_override = waves_override;
    return npbnn_resident_launch_of(&ctx->rlay, &q, out);
}

// Per column of a resident matrix under the context's scales (split_quality_kernel): how far the fp16 pair's largest counted entry
// error is from its bounds - max(error / (2^-17 x mean |entry|), error / (2^-12 x typical |entry|)); <= 1 passes, 0 for an exact column.
static int column_quality(npbnn_ctx* ctx, const Dataset& d, std::vector<double>* badness) {
    const int Fq = d.m->Fp;
    DevBuf<unsigned> d_err;
    DevBuf<unsigned long long> d_sum;
    if (int rc = d_err.reserve(ctx, (size_t)Fq)) return rc;
    if (int rc = d_sum.reserve(ctx, (size_t)Fq * 3)) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_err, 0, (size_t)Fq * sizeof(unsigned), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_sum, 0, (size_t)Fq * 3 * sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(split_quality_kernel, dim3((Fq + 255) / 256, (unsigned)((d.m->n_rows + 1023) / 1024)), dim3(256), 0, ctx->stream,
                       (const float*)d.m->X, (long long)d.m->n_rows, d.m->Fp, (const float*)ctx->store->xscale, d_err.get(), d_sum.get(), d_sum + Fq, d_sum + 2 * (size_t)Fq);
    std::vector<unsigned> h_err((size_t)Fq);
    std::vector<unsigned long long> h_sum((size_t)Fq * 3);
    HIP_TRY(ctx, hipMemcpyAsync(h_err.data(), d_err, h_err.size() * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h_sum.data(), d_sum, h_sum.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    badness->assign((size_t)d.m->F, 0.0);
    for (int c = 0; c < d.m->F; ++c) {
        float e;
        memcpy(&e, &h_err[(size_t)c], 4);
        const unsigned long long cnt = h_sum[2 * (size_t)Fq + c];
        if (cnt == 0 || !(e > 0.f)) continue;                 // an all-zero column, or one the pair holds exactly
        const double mean_abs = (double)h_sum[(size_t)c] / 268435456.0 / (double)d.m->n_rows;
        const double typical = std::exp2((double)(long long)h_sum[(size_t)Fq + c] / 65536.0 / (double)cnt);
        const double by_mean = mean_abs > 0.0 ? (double)e / mean_abs / (double)kF16QualityTol : 1e300;
        const double by_typical = (double)e / typical / (double)kF16TypicalTol;
        (*badness)[(size_t)c] = by_mean > by_typical ? by_mean : by_typical;
    }
    return NPBNN_OK;
}

// ---- fp16-split data: scales from the training matrix, split copies built on the device ----
int ensure_scales(npbnn_ctx* ctx) {
    Dataset& tr = ctx->ds[0];
    if (!tr.m->X) return fail(ctx, NPBNN_E_STATE, "the fp16-split path needs the training matrix first");
    if (ctx->store->xscale && ctx->store->scale_F == tr.m->F) return NPBNN_OK;
    const int Fp16 = round_up(tr.m->F, 32);
    DevBuf<unsigned> d_max;
    if (int rc = d_max.reserve(ctx, (size_t)Fp16)) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_max, 0, (size_t)Fp16 * sizeof(unsigned), ctx->stream));
    const int row_blocks = (int)((tr.m->n_rows + 1023) / 1024);
    hipLaunchKernelGGL(col_absmax_kernel, dim3((tr.m->Fp + 255) / 256, row_blocks), dim3(256), 0, ctx->stream, tr.m->X,
                       (long long)tr.m->n_rows, tr.m->Fp, d_max);
    if (int rc = ctx->store->xscale.reserve(ctx, (size_t)Fp16)) return rc;
    if (int rc = ctx->store->wscale.reserve(ctx, (size_t)Fp16)) return rc;
    hipLaunchKernelGGL(col_scale_kernel, dim3((Fp16 + 255) / 256), dim3(256), 0, ctx->stream, d_max, Fp16, ctx->store->xscale,
                       ctx->store->wscale, (const int*)nullptr);
    std::vector<unsigned> h((size_t)Fp16);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), d_max, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->store->scale_F = tr.m->F;
    ctx->store->f16_shifted_cols = 0;
    ctx->store->f16_max_shift = 0;
    tr.m->f16_state = 0;
    for (unsigned bits : h) {
        float m;
        memcpy(&m, &bits, 4);
        if (!std::isfinite(m)) tr.m->f16_state = -1;     // inf / NaN in the data: stay on the exact float32 path
    }
    // Heavy-tailed columns: with the largest entry just under 1 the typical entries sit where the pair's absolute error floor
    // (2^-25) is a visible fraction of them.  Such a column's scale moves up by the power of two that brings its error / typical |value|
    // under the bound with a factor 2 to spare (the fp16 range above 1 is otherwise unused); the weights' scale moves down with it.
    // Columns inside the bound keep the scale they always had.
    if (tr.m->f16_state == 0 && !getenv("NPBNN_F16_NO_SHIFT")) {
        std::vector<double> ratio;
        int rcq = column_quality(ctx, tr, &ratio);
        if (rcq) return rcq;
        std::vector<int> shift((size_t)Fp16, 0);
        for (int c = 0; c < tr.m->F; ++c) {
            if (!(ratio[(size_t)c] > 1.0)) continue;
            int k = (int)std::ceil(std::log2(ratio[(size_t)c])) + 1;
            if (k > kF16MaxShift) k = kF16MaxShift;
            shift[(size_t)c] = k;
            ++ctx->store->f16_shifted_cols;
            if (k > ctx->store->f16_max_shift) ctx->store->f16_max_shift = k;
        }
        if (ctx->store->f16_shifted_cols > 0) {
            DevBuf<int> d_shift;
            if (int rc = d_shift.reserve(ctx, (size_t)Fp16)) return rc;
            HIP_TRY(ctx, hipMemcpy(d_shift, shift.data(), (size_t)Fp16 * sizeof(int), hipMemcpyHostToDevice));
            hipLaunchKernelGGL(col_scale_kernel, dim3((Fp16 + 255) / 256), dim3(256), 0, ctx->stream, d_max, Fp16, ctx->store->xscale,
                               ctx->store->wscale, (const int*)d_shift);
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    return NPBNN_OK;
}

// 1 = the set has a usable fp16-split copy, 0 = it cannot be represented (the caller stays on float32)
int ensure_x16(npbnn_ctx* ctx, int which, int* usable) {
    *usable = 0;
    if (ctx->store_taken) {      // a store taken from another context comes with its split copy, or without one
        *usable = ctx->ds[which].m->f16_state > 0 ? 1 : 0;
        return NPBNN_OK;
    }
    int rc = ensure_scales(ctx);
    if (rc) return rc;
    if (ctx->ds[0].m->f16_state < 0) return NPBNN_OK;
    Dataset& d = ctx->ds[which];
    if (d.m->f16_state == 0) {
        d.m->Fp16 = round_up(d.m->F, 32);
        const size_t n_pad = (size_t)d.m->n_tiles * 16;
        if (int rc1 = d.m->X16.reserve(ctx, n_pad * d.m->Fp16)) return rc1;
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_overflow, 0, sizeof(int), ctx->stream));
        const long long items = (long long)n_pad * (d.m->Fp16 / 8);
        hipLaunchKernelGGL(split_x_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, ctx->stream, d.m->X, (long long)n_pad, d.m->Fp,
                           d.m->Fp16, ctx->store->xscale, d.m->X16, reinterpret_cast<unsigned*>(ctx->d_overflow.get()));
        unsigned bits = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&bits, ctx->d_overflow, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        float m;
        memcpy(&m, &bits, 4);
        d.m->f16_state = (std::isfinite(m) && m <= kF16Safe) ? 1 : -1;    // a test set far outside the training range
        if (d.m->f16_state > 0) {      // and is the pair of fp16 numbers a fair picture of every column? (split_quality_kernel)
            std::vector<double> ratio;
            int rcq = column_quality(ctx, d, &ratio);
            if (rcq) return rcq;
            d.m->f16_worst_col = -1;
            d.m->f16_worst_ratio = 0.0;
            for (int c = 0; c < d.m->F; ++c)
                if (ratio[(size_t)c] > d.m->f16_worst_ratio) { d.m->f16_worst_ratio = ratio[(size_t)c]; d.m->f16_worst_col = c; }
            if (d.m->f16_worst_ratio > 1.0 && !getenv("NPBNN_F16_NO_QUALITY_CHECK")) d.m->f16_state = -2;   // heavy-tailed column(s) past what a moved scale holds
        }
        d.m->f16_floor_sum = 0.0;
        if (d.m->f16_state > 0 && which != 0) {     // not the table the scales came from: can a weight's floor show? (kF16FloorSum)
            const int Fs = std::min(d.m->F, ctx->store->scale_F);
            DevBuf<unsigned> d_max;
            if (int rc1 = d_max.reserve(ctx, (size_t)d.m->Fp)) return rc1;
            HIP_TRY(ctx, hipMemsetAsync(d_max, 0, (size_t)d.m->Fp * sizeof(unsigned), ctx->stream));
            hipLaunchKernelGGL(col_absmax_kernel, dim3((d.m->Fp + 255) / 256, (unsigned)((d.m->n_rows + 1023) / 1024)), dim3(256), 0, ctx->stream,
                               (const float*)d.m->X, (long long)d.m->n_rows, d.m->Fp, d_max.get());
            std::vector<float> h_max((size_t)d.m->Fp), h_scale((size_t)Fs);
            HIP_TRY(ctx, hipMemcpyAsync(h_max.data(), d_max, h_max.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(h_scale.data(), ctx->store->xscale, h_scale.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            for (int c = 0; c < Fs; ++c) {
                const double scaled = (double)h_max[(size_t)c] * (double)h_scale[(size_t)c];
                if (scaled > 1.0) d.m->f16_floor_sum += scaled - 1.0;
            }
            if (d.m->f16_floor_sum > kF16FloorSum && !getenv("NPBNN_F16_NO_FLOOR_CHECK")) d.m->f16_state = -3;
        }
        if (d.m->f16_state < 0) d.m->X16.reset();      // (nobody will read it)
    }
    *usable = d.m->f16_state > 0 ? 1 : 0;
    return NPBNN_OK;
}

// lik_only: the caller wants the likelihood terms and nothing else from the launch (no statistics, no predictions)
int plan_launch(npbnn_ctx* ctx, int which, LaunchPlan* lp, int force_f32, int want_cand, bool predict_only, bool lik_only, bool plain) {
    Dataset& d = ctx->ds[which];
    bool want_f16 = false;
    if (!force_f32 && ctx->l0_option != NPBNN_L0_F32) {
        int usable = 0;
        int rc0 = ensure_x16(ctx, which, &usable);
        if (rc0) return rc0;
        if (!usable && ctx->l0_option == NPBNN_L0_F16) {
            if (d.m->f16_state == -2)
                return fail(ctx, NPBNN_E_RANGE, "fp16-split layer 0 was requested but column %d spans too many powers of two for a pair of fp16 "
                                                "numbers, even with its scale moved as far as fp16 allows (largest entry error %.1f x the bound: 2^-17 of the column's mean, "
                                                "2^-12 of its typical |value|)", d.m->f16_worst_col, d.m->f16_worst_ratio);
            if (d.m->f16_state == -3)
                return fail(ctx, NPBNN_E_RANGE, "fp16-split layer 0 was requested but this table's entries are too large under the training table's "
                                                "column scales: its scaled column maxima exceed 1 by %.1f in all, and past %.1f a weight's absolute "
                                                "error of 2^-25 as a pair of fp16 numbers can leave the prediction tolerance", d.m->f16_floor_sum,
                            kF16FloorSum);
            return fail(ctx, NPBNN_E_RANGE, "fp16-split layer 0 was requested but the data cannot be represented in it");
        }
        want_f16 = usable != 0;
    }
    if ((ctx->net.l0_f16 != 0) != want_f16) {
        int rc0 = rebuild_net(ctx, want_f16);
        if (rc0) return rc0;
    }
    if (ctx->wide) return wide_plan(ctx, which, lp, (predict_only || lik_only) ? want_cand : 1, predict_only);
    lp->wide = false;
    int waves_override = 0;
    if (const char* e = getenv("NPBNN_WAVES")) { const int v = atoi(e); if (v >= 1) waves_override = v; }      // (A/B switch)
    npbnn_resident_launch r;
    const int refusal = resident_launch(ctx, d, want_cand, predict_only, lik_only, plain, waves_override, &r);
    if (refusal == NPBNN_RESIDENT_NO_FIT)
        return fail(ctx, NPBNN_E_ARG, "network too large: weight image of %d KiB does not fit the %zu KiB LDS of a CU",
                    ctx->net.image_floats * 4 / 1024, ctx->lds_limit / 1024);
    if (refusal == NPBNN_RESIDENT_FEW_WAVES)
        return fail(ctx, NPBNN_E_ARG, "network too large for the LDS-resident path on this data set (%d waves beside a weight image of %d KiB); "
                                      "NPBNN_OPT_WIDE = 1 runs it on the weight-streamed path", r.waves, ctx->net.image_floats * 4 / 1024);
    if (refusal) return fail(ctx, NPBNN_E_INTERNAL, "the launch rule refused its request (internal error)");
    const int mt0 = ctx->net.L[0].mt, l0f16 = ctx->net.l0_f16;
    lp->n_cand = r.n_cand;
    lp->fast = r.fast != 0;
    lp->fn = npbnn_pick_eval_kernel(mt0, r.mti, l0f16, r.n_cand, r.lk, r.fast, r.fast && r.blocked, plain && r.fast);
    if (!lp->fn) return fail(ctx, NPBNN_E_STATE, "no evaluation kernel for this shape (internal error)");
    lp->fn_spec = nullptr;
    if (r.want_spec) {
        const bool g = r.lk == kLikGauss;
        lp->fn_spec = r.n_cand == 1 ? (g ? pick_eval_d1_gauss_spec(mt0, l0f16) : pick_eval_d1_cat_spec(mt0, l0f16))
                                    : (g ? pick_eval_d3_gauss_spec(mt0, l0f16) : pick_eval_d3_cat_spec(mt0, l0f16));
    }
    lp->wpb = r.waves;
    lp->grid = r.grid;
    lp->n_waves = r.grid;          // one partial record per workgroup
    lp->lds = (size_t)r.lds_bytes;
    if (ctx->attr_fn != reinterpret_cast<const void*>(lp->fn) || ctx->attr_lds < lp->lds) {      // (not free: once per kernel and size)
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(lp->fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lp->lds));
        if (lp->fn_spec)
            HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(lp->fn_spec), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lp->lds));
        ctx->attr_fn = reinterpret_cast<const void*>(lp->fn);
        ctx->attr_lds = lp->lds;
    }
    return NPBNN_OK;
}

int ensure_work_buffers(npbnn_ctx* ctx, int n_waves) {
    return ctx->d_partials.reserve(ctx, (size_t)2 * kMaxCand * n_waves * kPartialStride);   // two pass parities
}

int stage_weights(npbnn_ctx* ctx, const double* W, const double* act_prm, const double* col_override) {
    if (!ctx->arch_set) return fail(ctx, NPBNN_E_STATE, "call npbnn_set_arch first");
    if (!W) return fail(ctx, NPBNN_E_ARG, "null weights");
    memcpy(ctx->h_w, W, (size_t)ctx->n_weights * sizeof(double));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_wraw, ctx->h_w, (size_t)ctx->n_weights * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const double* d_co = nullptr;
    if (col_override) {
        double* h_co = ctx->h_w + ctx->n_weights;
        memcpy(h_co, col_override, (size_t)ctx->arch.in_dim * sizeof(double));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_colov, h_co, (size_t)ctx->arch.in_dim * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        d_co = ctx->d_colov;
    }
    for (int l = 0; l < kMaxLayers; ++l) ctx->net.act_prm[l] = 0.f;
    if (act_prm)
        for (int l = 0; l + 1 < ctx->net.n_layers; ++l) ctx->net.act_prm[l] = (float)act_prm[l];
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_overflow, 0, sizeof(int), ctx->stream));
    launch_pack_weights(ctx, ctx->d_wraw, d_co, ctx->d_image, ctx->d_overflow);
    HIP_TRY(ctx, hipGetLastError());
    return NPBNN_OK;
}

// copy a parameter block to its device slot through the pinned staging area (stream ordered; the staging slot is
// reused only after the stream has been synchronised by the caller's epilogue)
int push_eval_params(npbnn_ctx* ctx, const EvalParams& p) {
    memcpy(ctx->h_params, &p, sizeof(EvalParams));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_eparams, ctx->h_params, sizeof(EvalParams), hipMemcpyHostToDevice, ctx->stream));
    return NPBNN_OK;
}
int push_finalize_params(npbnn_ctx* ctx, const FinalizeParams& f) {
    char* slot = ctx->h_params + sizeof(EvalParams);
    memcpy(slot, &f, sizeof(FinalizeParams));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_fparams, slot, sizeof(FinalizeParams), hipMemcpyHostToDevice, ctx->stream));
    return NPBNN_OK;
}
int push_chain_params(npbnn_ctx* ctx, const ChainParams& c) {
    char* slot = ctx->h_params + sizeof(EvalParams) + sizeof(FinalizeParams);
    memcpy(slot, &c, sizeof(ChainParams));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cparams, slot, sizeof(ChainParams), hipMemcpyHostToDevice, ctx->stream));
    return NPBNN_OK;
}

// diagnostics (NPBNN_EVAL_STAMPS): what the evaluating workgroups of the last launch (or, in a persistent launch, of its last pass)
// stamped - [grid][8] phases of wave 0, [grid][16] tile-loop ends per wave, [grid][8] prologue points (NPBNN_EXP_PROLOGUE_STAMPS builds).
// first_wg: workgroups before it do not evaluate (the step workgroup of the flag-ordered schedules).
void report_eval_stamps(const DevBuf<unsigned long long>& stamps, int grid, int wpb, int first_wg) {
    std::vector<unsigned long long> hs((size_t)grid * 32);
    (void)hipMemcpy(hs.data(), stamps, hs.size() * 8, hipMemcpyDeviceToHost);
    const int nwg = grid - first_wg;
    if (nwg < 1) return;
    if (getenv("NPBNN_EVAL_STAMPS") && atoi(getenv("NPBNN_EVAL_STAMPS")) >= 2) {
        // per workgroup: pass start -> end of the pass (prologue stamp 4), the tile phase of wave 0, by (b - first_wg) % 8 (its place in the
        // round-robin over the 8 XCDs)
        auto start_of_wg = [&](int b) { const unsigned long long* q = &hs[(size_t)b * 8]; return q[0] <= q[1] ? q[0] : q[1]; };
        double by_xcd[8] = {0}, tiles_xcd[8] = {0};
        int n_xcd[8] = {0};
        std::vector<std::pair<double, int>> dur;
        for (int b = first_wg; b < grid; ++b) {
            const double d = (double)(hs[(size_t)b * 8 + 6] - start_of_wg(b)) * 0.01;      // (start: see below)
            const double t = (double)(hs[(size_t)b * 8 + 4] - hs[(size_t)b * 8 + 3]) * 0.01;
            dur.push_back({d, b});
            by_xcd[b % 8] += d; tiles_xcd[b % 8] += t; ++n_xcd[b % 8];
        }
        std::sort(dur.begin(), dur.end());
        fprintf(stderr, "[npbnn eval stamps] pass start -> end per workgroup, us: fastest %.2f (wg %d), median %.2f, slowest", dur.front().first, dur.front().second,
                dur[dur.size() / 2].first);
        for (size_t i = dur.size() >= 6 ? dur.size() - 6 : 0; i < dur.size(); ++i) fprintf(stderr, " %.2f (wg %d)", dur[i].first, dur[i].second);
        fprintf(stderr, "\n[npbnn eval stamps] mean by blockIdx %% 8:");
        for (int x = 0; x < 8; ++x) fprintf(stderr, " %.2f/%.2f", n_xcd[x] ? by_xcd[x] / n_xcd[x] : 0.0, n_xcd[x] ? tiles_xcd[x] / n_xcd[x] : 0.0);
        fprintf(stderr, " (pass/tile phase)\n");
        const int b = first_wg;
        fprintf(stderr, "[npbnn eval stamps] raw, workgroup %d:", b);
        for (int k = 0; k < 8; ++k) fprintf(stderr, " %llu", hs[(size_t)b * 8 + k]);
        fprintf(stderr, " | prologue:");
        for (int k = 0; k < 8; ++k) fprintf(stderr, " %llu", hs[(size_t)grid * 24 + (size_t)b * 8 + k]);
        fprintf(stderr, "\n");
    }
    {   // when each wave of a workgroup finished its tiles, relative to the workgroup's tile-loop start (mean over workgroups)
        double done[16] = {0};
        for (int b = first_wg; b < grid; ++b)
            for (int w = 0; w < wpb && w < 16; ++w)
                done[w] += (double)(hs[(size_t)grid * 8 + (size_t)b * 16 + w] - hs[(size_t)b * 8 + 3]) * 0.01;
        fprintf(stderr, "[npbnn eval stamps] tiles done per wave, us after the tile loop starts:");
        for (int w = 0; w < wpb && w < 16; ++w) fprintf(stderr, " %.1f", done[w] / nwg);
        fprintf(stderr, "\n");
    }
    // (a pass in the middle of a persistent launch: stamp 0 is then the start of the turn AFTER it - the launch's last, empty one - and
    // the pass is taken to start where its first barrier is reached, stamp 1; "issue" is not known for it)
    auto start_of = [&](const unsigned long long* q) { return q[0] <= q[1] ? q[0] : q[1]; };
    unsigned long long first = ~0ull, last = 0, first_end = ~0ull;
    double acc[8] = {0};
    for (int b = first_wg; b < grid; ++b) {
        const unsigned long long* q = &hs[(size_t)b * 8];
        if (start_of(q) < first) first = start_of(q);
        if (q[6] > last) last = q[6];
        if (q[6] < first_end) first_end = q[6];
        if (q[0] <= q[1]) acc[1] += (double)(q[1] - q[0]) * 0.01;                     // 100 MHz wall clock -> us
        for (int k = 2; k <= 6; ++k) acc[k] += (double)(q[k] - q[k - 1]) * 0.01;
        acc[7] += (double)q[7] * 0.01;
    }
    if (hs[(size_t)grid * 24 + (size_t)first_wg * 8] || hs[(size_t)grid * 24 + (size_t)first_wg * 8 + 3]) {      // (a build with NPBNN_EXP_PROLOGUE_STAMPS)
        double px[5] = {0};
        for (int b = first_wg; b < grid; ++b)
            for (int k = 0; k < 5; ++k) px[k] += (double)(hs[(size_t)grid * 24 + (size_t)b * 8 + k] - hs[(size_t)b * 8]) * 0.01;
        double period = 0, pmax = 0;
        int np_ = 0;
        for (int b = first_wg; b < grid; ++b) {
            const unsigned long long prev = hs[(size_t)grid * 24 + (size_t)b * 8 + 5];
            if (prev) { const double d = (double)(hs[(size_t)b * 8] - prev) * 0.01; period += d; if (d > pmax) pmax = d; ++np_; }
        }
        if (np_) fprintf(stderr, "[npbnn eval stamps] persistent launch: start of the pass before -> start of this one, us: mean %.2f, slowest workgroup %.2f\n", period / np_, pmax);
        fprintf(stderr, "[npbnn eval stamps] prologue of wave 0, us after its start: parameters read %.2f, pass descriptor %.2f, image copies requested %.2f, "
                        "first X pieces requested %.2f; end of the pass (sums out, workgroup reported done) %.2f\n", px[0] / nwg, px[1] / nwg, px[2] / nwg, px[3] / nwg, px[4] / nwg);
    }
    double late = 0;
    for (int b = first_wg; b < grid; ++b) late += (double)(start_of(&hs[(size_t)b * 8]) - first) * 0.01;
    fprintf(stderr, "[npbnn eval stamps] wave 0 of a workgroup, mean us: start skew %.2f | issue %.2f  barrier1 %.2f  patch %.2f  tiles %.2f  "
                    "barrier2 %.2f  partials %.2f | tails within tiles %.2f | first start -> first end %.2f, -> last end %.2f\n",
            late / nwg, acc[1] / nwg, acc[2] / nwg, acc[3] / nwg, acc[4] / nwg, acc[5] / nwg, acc[6] / nwg, acc[7] / nwg,
            (double)(first_end - first) * 0.01, (double)(last - first) * 0.01);
}

// diagnostics (NPBNN_STEP_STAMPS): what the step kernel stamped during a batch - [1024][8] phases of a step, rows indexed by the first
// iteration of the pass it decided
void report_step_stamps(const DevBuf<unsigned long long>& stamps) {
    std::vector<unsigned long long> hs(1024 * 8);
    (void)hipMemcpy(hs.data(), stamps, hs.size() * 8, hipMemcpyDeviceToHost);
    double acc[8] = {0};
    int n = 0;
    for (int r = 1; r < 1024; ++r) {
        const unsigned long long* q = &hs[(size_t)r * 8];
        if (!q[0] || !q[6]) continue;
        bool whole = true;          // (a step that skipped a phase - a void pass has nothing to reduce - left an older stamp there)
        for (int k = 1; k <= 6; ++k) whole = whole && q[k] >= q[k - 1];
        if (!whole) continue;
        for (int k = 1; k <= 6; ++k) acc[k] += (double)(q[k] - q[k - 1]) * 0.01;   // 100 MHz wall clock -> us
        ++n;
    }
    if (n) fprintf(stderr, "[npbnn step stamps] prefetch %.2f  reduce %.2f  decide %.2f  commit %.2f  prepare %.2f  finish %.2f us (mean of %d)\n",
                   acc[1] / n, acc[2] / n, acc[3] / n, acc[4] / n, acc[5] / n, acc[6] / n, n);
    // start of a step -> start of the next one (the period of a pass where the step is what the passes wait for), and what of it the
    // step workgroup spent between two steps (waiting for the evaluating workgroups' sums, flag-ordered schedules).  Rows are
    // indexed by the first iteration of the decided pass: in time order
    std::vector<std::pair<unsigned long long, unsigned long long>> se;
    for (int r = 1; r < 1024; ++r) {
        const unsigned long long* q = &hs[(size_t)r * 8];
        if (q[0] && q[6] && q[6] > q[0]) se.push_back({q[0], q[6]});
    }
    std::sort(se.begin(), se.end());
    double period = 0, idle = 0;
    int m = 0;
    for (size_t i = 0; i + 1 < se.size(); ++i) {
        const double d = (double)(se[i + 1].first - se[i].first) * 0.01;
        if (se[i + 1].first < se[i].second || d > 200.0) continue;      // (a row overwritten by a later lap of the table; a batch boundary)
        period += d;
        idle += (double)(se[i + 1].first - se[i].second) * 0.01;
        ++m;
    }
    if (m) fprintf(stderr, "[npbnn step stamps] step start -> next step start %.2f us, of which between steps %.2f us (mean of %d)\n", period / m, idle / m, m);
}

EvalParams make_params(npbnn_ctx* ctx, const Dataset& d) {
    EvalParams p{};
    p.X = ctx->net.l0_f16 ? d.m->X16 : d.m->X;
    p.labels = d.labels;
    p.targets = d.targets;
    p.inst_w = nullptr;
    p.image = ctx->d_image;
    p.n_rows = d.m->n_rows;
    p.n_tiles = d.m->n_tiles;
    p.has_pass = 0;
    p.Fp = ctx->net.l0_f16 ? d.m->Fp16 : d.m->Fp;
    p.net = ctx->net;
    p.lay = layout_for(ctx, d);
    p.cand_slopes = nullptr;
    return p;
}

int check_dataset_for_lik(npbnn_ctx* ctx, const Dataset& d, int lik) {
    if (!d.m->X) return fail(ctx, NPBNN_E_STATE, "no data matrix for this set");
    if (d.m->F != ctx->arch.in_dim)
        return fail(ctx, NPBNN_E_ARG, "data has %d features but the network expects %d", d.m->F, ctx->arch.in_dim);
    if (lik == NPBNN_LIK_CATEGORICAL && !d.labels) return fail(ctx, NPBNN_E_STATE, "categorical likelihood needs labels (npbnn_set_labels_i64)");
    if (lik == NPBNN_LIK_GAUSS || lik_needs_row_scratch(lik)) {
        if (!d.targets) return fail(ctx, NPBNN_E_STATE, "this likelihood needs targets (npbnn_set_targets_f64)");
        if (d.k != ctx->net.k_targets) return fail(ctx, NPBNN_E_ARG, "targets have %d columns, architecture says %d", d.k, ctx->net.k_targets);
    }
    return NPBNN_OK;
}

int rebuild_net(npbnn_ctx* ctx, bool f16) {
    int rc = build_net(ctx, &ctx->arch, f16);
    if (rc) return rc;
    ctx->d_image.reset();
    ctx->d_w2img.reset();
    ctx->d_w2scale.reset();
    if (ctx->wide) return wide_build(ctx, f16);
    wide_free(ctx);
    {   // (one candidate beside a wave with labels and targets)
        npbnn_resident_launch r;
        npbnn_resident_launch_req q{};
        q.has_labels = 1; q.has_targets = 1; q.n_cu = 1; q.lds_limit = (int)ctx->lds_limit; q.want_cand = 1;
        if (npbnn_resident_launch_of(&ctx->rlay, &q, &r) == NPBNN_RESIDENT_NO_FIT)
            return fail(ctx, NPBNN_E_ARG, "network too large: weight image of %d KiB does not fit the %zu KiB LDS of a CU",
                        ctx->net.image_floats * 4 / 1024, ctx->lds_limit / 1024);
    }
    // (room for kMaxCand independent images: npbnn_predict_sets stages that many weight sets per pass)
    if (int rc2 = ctx->d_image.reserve(ctx, (size_t)kMaxCand * ctx->net.image_floats)) return rc2;
    HIP_TRY(ctx, hipMemset(ctx->d_image, 0, (size_t)kMaxCand * ctx->net.image_floats * sizeof(float)));
    // where each packed weight lives in the image (bias column -> bias slot, else its MFMA fragment slot)
    std::vector<int> map((size_t)ctx->n_weights);
    std::vector<float> scale;
    std::vector<float> wscale;
    if (f16) {
        scale.assign((size_t)ctx->n_weights, 1.0f);
        wscale.resize((size_t)round_up(ctx->arch.in_dim, 32));
        HIP_TRY(ctx, hipMemcpy(wscale.data(), ctx->store->wscale, wscale.size() * sizeof(float), hipMemcpyDeviceToHost));
    }
    for (int l = 0; l < ctx->net.n_layers; ++l) {
        const LayerMeta& L = ctx->net.L[l];
        const int ld = L.in_dim + L.has_bias;
        for (int o = 0; o < L.out_dim; ++o)
            for (int j = 0; j < ld; ++j) {
                const size_t wi = (size_t)L.w_off + (size_t)o * ld + j;
                int scale_col;
                map[wi] = npbnn_resident_pos(&ctx->rlay, l, o, j, &scale_col);
                if (scale_col >= 0) scale[wi] = wscale[(size_t)scale_col];
            }
    }
    if (int rc2 = ctx->d_w2img.reserve(ctx, map.size())) return rc2;
    HIP_TRY(ctx, hipMemcpy(ctx->d_w2img, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice));
    if (f16) {
        if (int rc2 = ctx->d_w2scale.reserve(ctx, scale.size())) return rc2;
        HIP_TRY(ctx, hipMemcpy(ctx->d_w2scale, scale.data(), scale.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return NPBNN_OK;
}

double wall_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void launch_pack_weights(npbnn_ctx* ctx, const double* d_w, const double* d_col_override, float* image, int* flags) {
    if (ctx->wide) { wide_pack(ctx, d_w, d_col_override, image, flags); return; }
    const int total = pack_item_count(ctx->net, true);
    hipLaunchKernelGGL(pack_weights_kernel, dim3((total + 255) / 256), dim3(256), 0, ctx->stream, d_w, d_col_override,
                       ctx->n_classw ? ctx->d_classw : nullptr, image, ctx->net, ctx->net.l0_f16 ? ctx->store->wscale : nullptr, flags);
}

int launch_plain_eval(npbnn_ctx* ctx, const LaunchPlan& lp, int which) {
    if (lp.wide && lp.n_cand > 1) return wide_forward(ctx, which, ctx->d_wide_cand, false, false, nullptr, lp.n_cand);
    if (lp.wide) return wide_forward(ctx, which, ctx->d_image, false);
    hipLaunchKernelGGL(lp.fn, dim3(lp.grid), dim3(lp.wpb * 64), lp.lds, ctx->stream, (const EvalParams*)ctx->d_eparams, 0, 1);
    return NPBNN_OK;
}

float* pass_image(npbnn_ctx* ctx, const LaunchPlan& lp, int j) {
    if (!lp.wide) return ctx->d_image + (size_t)j * ctx->net.image_floats;
    return lp.n_cand > 1 ? ctx->d_wide_cand + (size_t)j * ctx->wmeta.image_floats : ctx->d_image.get();
}

void launch_pack_group(npbnn_ctx* ctx, const LaunchPlan& lp, const double* d_w, const double* d_col_override, int g) {
    if (lp.wide) { wide_pack(ctx, d_w, d_col_override, pass_image(ctx, lp, 0), ctx->d_overflow + 1, g); return; }
    for (int j = 0; j < g; ++j)
        launch_pack_weights(ctx, d_w + (size_t)j * ctx->n_weights, d_col_override, pass_image(ctx, lp, j), ctx->d_overflow);
}

// confusion counts: device and pinned host buffers for n_classes x n_classes
int ensure_conf(npbnn_ctx* ctx, int n_classes) {
    const size_t need = (size_t)(n_classes < kResidentMaxWidth ? kResidentMaxWidth : n_classes);
    if (int rc = ctx->d_conf.reserve(ctx, need * need)) return rc;
    return ctx->h_conf.reserve(ctx, need * need);
}

void launch_finalize(npbnn_ctx* ctx) {
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, ctx->stream, (const FinalizeParams*)ctx->d_fparams);
}

}  // namespace npbnn_api

extern "C" void npbnn_set_global_error_(const char* msg) { g_last_error = msg ? msg : ""; }

extern "C" {

int npbnn_abi_version(void) { return NPBNN_ABI_VERSION; }

int npbnn_device_count(int* out) {
    if (!out) return fail(nullptr, NPBNN_E_ARG, "null out");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *out = 0;
        return fail(nullptr, NPBNN_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *out = n;
    return NPBNN_OK;
}

const char* npbnn_last_error(const npbnn_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

int npbnn_create(int device_id, npbnn_ctx** out) {
    if (!out) return fail(nullptr, NPBNN_E_ARG, "null out");
    *out = nullptr;
    int n = 0;
    HIP_TRY(nullptr, hipGetDeviceCount(&n));
    if (device_id < 0 || device_id >= n) return fail(nullptr, NPBNN_E_ARG, "device %d not present (%d devices)", device_id, n);
    HIP_TRY(nullptr, hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, NPBNN_E_ARG, "device %d is %s; this library is built for gfx950 (MI355X) only", device_id, prop.gcnArchName);
    std::unique_ptr<npbnn_ctx> c(new npbnn_ctx());          // (a failure part-way frees what was made)
    c->device = device_id;
    hold_store(c.get(), std::make_shared<FeatureStore>(device_id), false);
    c->n_cu = prop.multiProcessorCount;
    c->lds_limit = 160 * 1024;
    HIP_TRY(nullptr, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(nullptr, hipEventCreate(&c->ev[0]));
    HIP_TRY(nullptr, hipEventCreate(&c->ev[1]));
    // the kernels' parameter blocks: ONE device allocation laid out like its page-locked staging twin, so that a chain batch sends
    // all of them in one copy
    const size_t params_bytes = sizeof(EvalParams) + sizeof(FinalizeParams) + sizeof(ChainParams);
    int rc;
    if ((rc = ensure_conf(c.get(), kResidentMaxWidth)) || (rc = c->d_out.reserve(nullptr, 1)) || (rc = c->d_overflow.reserve(nullptr, 1 + kSetFlags)) ||
        (rc = c->d_params.reserve(nullptr, params_bytes)) || (rc = c->h_params.reserve(nullptr, params_bytes)) || (rc = c->h_out.reserve(nullptr, 1)))
        return rc;
    c->d_eparams = reinterpret_cast<EvalParams*>(c->d_params.get());
    c->d_fparams = reinterpret_cast<FinalizeParams*>(c->d_params + sizeof(EvalParams));
    c->d_cparams = reinterpret_cast<ChainParams*>(c->d_params + sizeof(EvalParams) + sizeof(FinalizeParams));
    *out = c.release();
    return NPBNN_OK;
}

void npbnn_destroy(npbnn_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;        // the buffers with the device current, the store if nobody else holds it, the streams and events last (npbnn_ctx_streams)
}

int npbnn_share_data(npbnn_ctx* ctx, npbnn_ctx* owner) {
    if (!ctx || !owner || ctx == owner) return fail(ctx, NPBNN_E_ARG, "share_data: bad arguments");
    const bool others = !ctx->store_taken && ctx->store.use_count() > 1;      // contexts that took this one's store
    if (others && owner->store == ctx->store) return fail(ctx, NPBNN_E_ARG, "share_data: contexts borrow from each other");
    if (owner->device != ctx->device) return fail(ctx, NPBNN_E_ARG, "share_data: contexts on devices %d and %d", ctx->device, owner->device);
    if (others) return fail(ctx, NPBNN_E_STATE, "share_data: %d other context(s) use this one's matrices", (int)ctx->store.use_count() - 1);
    if (!owner->ds[0].m->X) return fail(ctx, NPBNN_E_STATE, "share_data: the owner has no training matrix");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the owner's fp16-split copies are built now (on its stream) so that those who take its store never have to
    for (int w = 0; w < 2; ++w)
        if (owner->ds[w].m->X && owner->l0_option != NPBNN_L0_F32) {
            int usable = 0;
            int rc = ensure_x16(owner, w, &usable);
            if (rc) { ctx->err = owner->err; return rc; }
        }
    HIP_TRY(ctx, hipStreamSynchronize(owner->stream));
    hold_store(ctx, owner->store, true);
    ctx->arch_set = false;            // (layer-0 layout depends on the data: set_arch again)
    return NPBNN_OK;
}

int npbnn_set_data_f64(npbnn_ctx* ctx, const double* X, int64_t n_rows, int32_t F, int which) {
    return upload_matrix<double>(ctx, X, n_rows, F, which);
}

int npbnn_set_data_f32(npbnn_ctx* ctx, const float* X, int64_t n_rows, int32_t F, int which) {
    return upload_matrix<float>(ctx, X, n_rows, F, which);
}

int npbnn_set_labels_i64(npbnn_ctx* ctx, const int64_t* y, int64_t n_rows, int which) {
    int rc = check_rows(ctx, which, n_rows, "set_labels");
    if (rc) return rc;
    if (!y) return fail(ctx, NPBNN_E_ARG, "set_labels: null labels");
    Dataset& d = ctx->ds[which];
    const size_t n_pad = (size_t)d.m->n_tiles * 16;
    std::vector<int> tmp(n_pad, -1);
    for (int64_t i = 0; i < n_rows; ++i) {
        if (y[i] < 0 || y[i] >= NPBNN_MAX_WIDTH)
            return fail(ctx, NPBNN_E_ARG, "set_labels: label %lld at row %lld outside 0..%d", (long long)y[i], (long long)i, NPBNN_MAX_WIDTH - 1);
        tmp[i] = (int)y[i];
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = d.labels.reserve(ctx, n_pad);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(d.labels, tmp.data(), n_pad * sizeof(int), hipMemcpyHostToDevice));
    return NPBNN_OK;
}

int npbnn_set_targets_f64(npbnn_ctx* ctx, const double* Y, int64_t n_rows, int32_t k, int which) {
    int rc = check_rows(ctx, which, n_rows, "set_targets");
    if (rc) return rc;
    if (!Y || k < 1 || k > NPBNN_MAX_TARGETS) return fail(ctx, NPBNN_E_ARG, "set_targets: need 1..%d target columns, got %d", NPBNN_MAX_TARGETS, k);
    Dataset& d = ctx->ds[which];
    const size_t n_pad = (size_t)d.m->n_tiles * 16;
    std::vector<float> tmp(n_pad * k, 0.0f);
    for (size_t i = 0; i < (size_t)n_rows * k; ++i) tmp[i] = (float)Y[i];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (d.k != k) d.targets.reset();
    rc = d.targets.reserve(ctx, n_pad * k);
    if (rc) return rc;
    d.k = k;
    HIP_TRY(ctx, hipMemcpy(d.targets, tmp.data(), n_pad * k * sizeof(float), hipMemcpyHostToDevice));
    return NPBNN_OK;
}

int npbnn_set_row_weights(npbnn_ctx* ctx, const double* instance_w, int64_t n_rows, const double* class_w, int32_t n_classes) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    Dataset& d = ctx->ds[0];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (instance_w) {
        int rc = check_rows(ctx, 0, n_rows, "set_row_weights");
        if (rc) return rc;
        const size_t n_pad = (size_t)d.m->n_tiles * 16;
        std::vector<float> tmp(n_pad, 0.0f);
        for (int64_t i = 0; i < n_rows; ++i) tmp[i] = (float)instance_w[i];
        rc = d.inst_w.reserve(ctx, n_pad);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpy(d.inst_w, tmp.data(), n_pad * sizeof(float), hipMemcpyHostToDevice));
    } else {
        d.inst_w.reset();
    }
    if (class_w) {
        if (n_classes < 1 || n_classes > NPBNN_MAX_WIDTH) return fail(ctx, NPBNN_E_ARG, "set_row_weights: n_classes=%d", n_classes);
        if (int rc = ctx->d_classw.reserve(ctx, NPBNN_MAX_WIDTH)) return rc;
        HIP_TRY(ctx, hipMemcpy(ctx->d_classw, class_w, (size_t)n_classes * sizeof(double), hipMemcpyHostToDevice));
        ctx->n_classw = n_classes;
    } else {
        ctx->n_classw = 0;
    }
    if (ctx->arch_set && (ctx->n_classw > 0) != (ctx->net.classw_off >= 0))      // the image gains / loses its class-weight block
        return rebuild_net(ctx, ctx->net.l0_f16 != 0);
    return NPBNN_OK;
}

int npbnn_set_arch(npbnn_ctx* ctx, const npbnn_arch* arch) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (!arch) return fail(ctx, NPBNN_E_ARG, "null arch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->arch_set = false;
    const npbnn_arch previous = ctx->arch;
    ctx->arch = *arch;
    ctx->l0_blocks.clear();                      // (a structure belongs to one architecture: npbnn_set_layer_mask after this call)
    int rc = rebuild_net(ctx, false);            // float32 layout first; plan_launch switches to fp16-split when it applies
    if (rc) {
        ctx->arch = previous;
        return rc;
    }
    // buffers sized by the number of weights (or inputs); the device chain's result block is laid out again by its next batch
    ctx->d_wraw.reset();
    ctx->d_colov.reset();
    ctx->h_w.reset();
    ctx->d_mask.reset();
    ctx->d_pscale_w.reset();
    ctx->res_nw = 0;
    if ((rc = ctx->d_wraw.reserve(ctx, (size_t)kMaxCand * ctx->n_weights))) return rc;
    if ((rc = ctx->d_colov.reserve(ctx, (size_t)arch->in_dim))) return rc;
    if ((rc = ctx->h_w.reserve(ctx, (size_t)ctx->n_weights + arch->in_dim))) return rc;
    ctx->arch_set = true;
    return NPBNN_OK;
}

int npbnn_set_layer_mask(npbnn_ctx* ctx, const double* mask_packed) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (!ctx->arch_set) return fail(ctx, NPBNN_E_STATE, "set_layer_mask: call npbnn_set_arch first");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<unsigned char> blocks;
    if (mask_packed) {
        const npbnn_arch& a = ctx->arch;
        const int in = a.in_dim, out = a.out_dim[0], ld = in + (a.has_bias[0] ? 1 : 0);
        const int g16 = (in + 15) / 16, mts = (out + 15) / 16;
        blocks.assign((size_t)mts * g16, 0);
        bool dense = true;
        for (int o = 0; o < out; ++o)
            for (int c = 0; c < in; ++c)
                if (mask_packed[(size_t)o * ld + (a.has_bias[0] ? 1 : 0) + c] != 0.0) blocks[(size_t)(o / 16) * g16 + c / 16] = 1;
        for (unsigned char b : blocks) dense = dense && b != 0;
        if (dense) blocks.clear();
    }
    if (blocks == ctx->l0_blocks) return NPBNN_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->l0_blocks.swap(blocks);
    return rebuild_net(ctx, ctx->net.l0_f16 != 0);
}

int npbnn_set_option(npbnn_ctx* ctx, int option, int value) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (option == NPBNN_OPT_L0_PRECISION) {
        if (value < NPBNN_L0_AUTO || value > NPBNN_L0_F16) return fail(ctx, NPBNN_E_ARG, "set_option: layer-0 precision %d", value);
        ctx->l0_option = value;
        return NPBNN_OK;
    }
    if (option == NPBNN_OPT_FAST_TAILS) {
        ctx->fast_option = value ? 1 : 0;
        return NPBNN_OK;
    }
    if (option == NPBNN_OPT_PERSISTENT) {
        ctx->persist_option = value ? 1 : 0;
        return NPBNN_OK;
    }
    if (option == NPBNN_OPT_WIDE) {
        const int on = value ? 1 : 0;
        if (on != ctx->wide_option) {
            ctx->wide_option = on;
            if (ctx->arch_set) {
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                return rebuild_net(ctx, ctx->net.l0_f16 != 0);
            }
        }
        return NPBNN_OK;
    }
    if (option == NPBNN_OPT_TRAINABLE_SLOPES) {
        const int on = value ? 1 : 0;
        if (on != ctx->slopes_option) {
            ctx->slopes_option = on;
            if (ctx->arch_set) return rebuild_net(ctx, ctx->net.l0_f16 != 0);      // (the image layout changes)
        }
        return NPBNN_OK;
    }
    return fail(ctx, NPBNN_E_ARG, "set_option: unknown option %d", option);
}

int npbnn_get_info(npbnn_ctx* ctx, int what, int* out) {
    if (!ctx || !out) return fail(ctx, NPBNN_E_ARG, "get_info: bad arguments");
    if (what == NPBNN_INFO_L0_F16) { *out = ctx->net.l0_f16; return NPBNN_OK; }
    if (what == NPBNN_INFO_L0_OPTION) { *out = ctx->l0_option; return NPBNN_OK; }
    if (what == NPBNN_INFO_WIDE) { *out = (ctx->arch_set && ctx->wide) ? 1 : 0; return NPBNN_OK; }
    if (what == NPBNN_INFO_F16_MOVED_COLUMNS) { *out = ctx->store->f16_shifted_cols; return NPBNN_OK; }
    if (what == NPBNN_INFO_F16_MAX_MOVE) { *out = ctx->store->f16_max_shift; return NPBNN_OK; }
    if (what == NPBNN_INFO_PDP_ROUTE) { *out = ctx->pdp_route; return NPBNN_OK; }
    if (what == NPBNN_INFO_ALE_ROUTE) { *out = ctx->ale_route; return NPBNN_OK; }
    if (what == NPBNN_INFO_SALIENCY_ROUTE) { *out = ctx->saliency_route; return NPBNN_OK; }
    if (what == NPBNN_INFO_SALIENCY_FOLD_NS) { *out = ctx->saliency_ns; return NPBNN_OK; }
    if (what == NPBNN_INFO_SHAPLEY_ROUTE) { *out = ctx->shapley_route; return NPBNN_OK; }
    if (what == NPBNN_INFO_SHAPLEY_WALK_NS) { *out = ctx->shapley_ns; return NPBNN_OK; }
    if (what == NPBNN_INFO_REPLAY_PASSES) { *out = ctx->replay_passes; return NPBNN_OK; }
    if (what == NPBNN_INFO_REPLAY_MAX_GROUP) { *out = ctx->replay_max_group; return NPBNN_OK; }
    if (what == NPBNN_INFO_CALIBRATION_FINAL_NS) { *out = ctx->calibration_ns; return NPBNN_OK; }
    if (what == NPBNN_INFO_LOO_FINAL_NS) { *out = ctx->loo_ns; return NPBNN_OK; }
    if (what == NPBNN_INFO_GRAD_ROWS_NS || what == NPBNN_INFO_GRAD_FOLD_NS) { *out = ctx->grad_ns[what - NPBNN_INFO_GRAD_ROWS_NS]; return NPBNN_OK; }
    if (what >= NPBNN_INFO_PERMUTE_NS && what <= NPBNN_INFO_CONVERGENCE_FINAL_NS) { *out = ctx->fi_ns[what - NPBNN_INFO_PERMUTE_NS]; return NPBNN_OK; }
    if (ctx->arch_set && ctx->wide && (what == NPBNN_INFO_WAVES_PER_BLOCK || what == NPBNN_INFO_MAX_CANDIDATES || what == NPBNN_INFO_FAST_TAILS)) {
        *out = what == NPBNN_INFO_WAVES_PER_BLOCK ? 4 : what == NPBNN_INFO_MAX_CANDIDATES ? 1 : 0;      // (group passes: one chain per pass; what a replay of stored sets carried: NPBNN_INFO_REPLAY_MAX_GROUP)
        return NPBNN_OK;
    }
    if (what == NPBNN_INFO_N_CU) { *out = ctx->n_cu; return NPBNN_OK; }
    if (what == NPBNN_INFO_TURN_NS_OVERLAPPED || what == NPBNN_INFO_TURN_NS_BETWEEN) {
        *out = (int)(1000.0 * ctx->sched.turn_us[what == NPBNN_INFO_TURN_NS_BETWEEN ? 1 : 0]);
        return NPBNN_OK;
    }
    if (what == NPBNN_INFO_IT_NS_OVERLAPPED || what == NPBNN_INFO_IT_NS_BETWEEN) {
        const double* c = ctx->sched.it_us[what == NPBNN_INFO_IT_NS_BETWEEN ? 1 : 0];      // (short batches - dispatches of 100 - when measured, else long ones)
        *out = (int)(1000.0 * (c[0] > 0.0 ? c[0] : c[1]));
        return NPBNN_OK;
    }
    if (what == NPBNN_INFO_WAVES_PER_BLOCK || what == NPBNN_INFO_MAX_CANDIDATES || what == NPBNN_INFO_FAST_TAILS) {
        // what plan_launch gives a chain pass on the training table: of one candidate (the waves), of as many as fit (the other two)
        npbnn_resident_launch r{};
        r.n_cand = 1;
        if (what == NPBNN_INFO_WAVES_PER_BLOCK || (ctx->arch_set && (what == NPBNN_INFO_FAST_TAILS || ctx->ds[0].m->X)))
            resident_launch(ctx, ctx->ds[0], what == NPBNN_INFO_WAVES_PER_BLOCK ? 1 : kMaxCand, false, what != NPBNN_INFO_WAVES_PER_BLOCK, false, 0, &r);
        *out = what == NPBNN_INFO_WAVES_PER_BLOCK ? r.waves_full : what == NPBNN_INFO_MAX_CANDIDATES ? r.n_cand : r.fast;
        return NPBNN_OK;
    }
    return fail(ctx, NPBNN_E_ARG, "get_info: unknown item %d", what);
}

static int eval_once(npbnn_ctx* ctx, const double* W_packed, const double* act_prm, const double* col_override, double lik_temp,
                     const double* sigma, int which, npbnn_eval_out* out, int64_t* confusion, int force_f32, int* overflowed) {
    const int lik = ctx->net.lik_kind;
    Dataset& d = ctx->ds[which];
    LaunchPlan lp;
    int rc = plan_launch(ctx, which, &lp, force_f32, 1, false, confusion == nullptr, true);
    if (rc) return rc;
    rc = ensure_work_buffers(ctx, lp.n_waves);
    if (rc) return rc;
    rc = stage_weights(ctx, W_packed, act_prm, col_override);
    if (rc) return rc;
    EvalParams p = make_params(ctx, d);
    p.partials = ctx->d_partials;
    p.inst_w = (which == 0) ? d.inst_w : nullptr;
    p.use_classw = (which == 0 && ctx->n_classw > 0) ? 1 : 0;
    const int C = ctx->net.n_out;
    if (confusion) {
        rc = ensure_conf(ctx, C);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_conf, 0, (size_t)C * C * sizeof(unsigned), ctx->stream));
        p.confusion = ctx->d_conf;
    }
    rc = push_eval_params(ctx, p);
    if (rc) return rc;
    rc = launch_plain_eval(ctx, lp, which);
    if (rc) return rc;
    HIP_TRY(ctx, hipGetLastError());
    FinalizeParams f{};
    f.partials = ctx->d_partials;
    f.n_waves = lp.n_waves;
    f.lik_kind = lik;
    f.k_targets = ctx->net.k_targets;
    f.n_rows = d.m->n_rows;
    f.lik_temp = lik_temp;
    f.sigma_given = sigma ? 1 : 0;
    if (sigma)
        for (int j = 0; j < ctx->net.k_targets; ++j) f.sigma[j] = sigma[j];
    f.out = ctx->d_out;
    rc = push_finalize_params(ctx, f);
    if (rc) return rc;
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, ctx->stream, (const FinalizeParams*)ctx->d_fparams);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, sizeof(npbnn_eval_out), hipMemcpyDeviceToHost, ctx->stream));
    if (confusion)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_conf, ctx->d_conf, (size_t)C * C * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    int ovf = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&ovf, ctx->d_overflow, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ovf & kFlagStructure) return fail(ctx, NPBNN_E_ARG, "eval: a layer-0 weight is not zero where the mask given to npbnn_set_layer_mask is");
    *overflowed = ctx->net.l0_f16 && (ovf & kFlagF16Range);
    if (*overflowed) return NPBNN_OK;
    *out = *ctx->h_out;
    if (confusion)
        for (int i = 0; i < C * C; ++i) confusion[i] = (int64_t)ctx->h_conf[i];
    return NPBNN_OK;
}

int npbnn_eval(npbnn_ctx* ctx, const double* W_packed, const double* act_prm, const double* col_override, double lik_temp,
               const double* sigma, int which, npbnn_eval_out* out, int64_t* confusion) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (!out) return fail(ctx, NPBNN_E_ARG, "eval: null out");
    if (which != 0 && which != 1) return fail(ctx, NPBNN_E_ARG, "eval: which must be 0 or 1");
    if (!ctx->arch_set) return fail(ctx, NPBNN_E_STATE, "eval: call npbnn_set_arch first");
    const int lik = ctx->net.lik_kind;
    if (lik == NPBNN_LIK_NONE) return fail(ctx, NPBNN_E_STATE, "eval: architecture was set with NPBNN_LIK_NONE");
    int rc = check_dataset_for_lik(ctx, ctx->ds[which], lik);
    if (rc) return rc;
    if (confusion && lik != NPBNN_LIK_CATEGORICAL) return fail(ctx, NPBNN_E_ARG, "eval: confusion counts need the categorical likelihood");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int overflowed = 0;
    rc = eval_once(ctx, W_packed, act_prm, col_override, lik_temp, sigma, which, out, confusion, 0, &overflowed);
    if (rc) return rc;
    if (overflowed) {   // a scaled layer-0 weight left the fp16 range: this evaluation runs on the exact float32 path
        if (ctx->l0_option == NPBNN_L0_F16) return fail(ctx, NPBNN_E_RANGE, "eval: a layer-0 weight left the fp16 range");
        rc = eval_once(ctx, W_packed, act_prm, col_override, lik_temp, sigma, which, out, confusion, 1, &overflowed);
    }
    return rc;
}

int npbnn_predict(npbnn_ctx* ctx, const double* W_packed, const double* act_prm, const double* col_override, int which,
                  int apply_out_fn, double* out_y) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (!out_y) return fail(ctx, NPBNN_E_ARG, "predict: null out_y");
    if (which != 0 && which != 1) return fail(ctx, NPBNN_E_ARG, "predict: which must be 0 or 1");
    if (!ctx->arch_set) return fail(ctx, NPBNN_E_STATE, "predict: call npbnn_set_arch first");
    Dataset& d = ctx->ds[which];
    int rc = check_dataset_for_lik(ctx, d, NPBNN_LIK_NONE);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int C = ctx->net.n_out;
    const size_t n_el = (size_t)d.m->n_rows * C;
    std::vector<float> tmp(n_el);
    for (int attempt = 0; attempt < 2; ++attempt) {
    LaunchPlan lp;
    rc = plan_launch(ctx, which, &lp, attempt);
    if (rc) return rc;
    rc = stage_weights(ctx, W_packed, act_prm, col_override);
    if (rc) return rc;
    if ((rc = ctx->d_y.reserve(ctx, n_el))) return rc;
    EvalParams p = make_params(ctx, d);
    p.labels = nullptr;
    p.targets = nullptr;
    p.net.lik_kind = NPBNN_LIK_NONE;
    p.y_out = ctx->d_y;
    p.predict_mode = apply_out_fn ? 2 : 1;
    rc = push_eval_params(ctx, p);
    if (rc) return rc;
    rc = launch_plain_eval(ctx, lp, which);
    if (rc) return rc;
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(tmp.data(), ctx->d_y, n_el * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    int ovf = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&ovf, ctx->d_overflow, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ovf & kFlagStructure) return fail(ctx, NPBNN_E_ARG, "predict: a layer-0 weight is not zero where the mask given to npbnn_set_layer_mask is");
    if (!(ctx->net.l0_f16 && (ovf & kFlagF16Range))) break;
    if (ctx->l0_option == NPBNN_L0_F16) return fail(ctx, NPBNN_E_RANGE, "predict: a layer-0 weight left the fp16 range");
    }
    for (size_t i = 0; i < n_el; ++i) out_y[i] = (double)tmp[i];
    return NPBNN_OK;
}

int npbnn_predict_sets(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which, int apply_out_fn,
                       double* out_y) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (!W_sets || !out_y || n_sets < 1) return fail(ctx, NPBNN_E_ARG, "predict_sets: bad arguments");
    if (which != 0 && which != 1) return fail(ctx, NPBNN_E_ARG, "predict_sets: which must be 0 or 1");
    if (!ctx->arch_set) return fail(ctx, NPBNN_E_STATE, "predict_sets: call npbnn_set_arch first");
    Dataset& d = ctx->ds[which];
    int rc = check_dataset_for_lik(ctx, d, NPBNN_LIK_NONE);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t per_set = (size_t)d.m->n_rows * ctx->net.n_out;
    std::vector<float> tmp(kMaxCand * per_set);
    return replay_sets(ctx, "predict_sets", W_sets, act_prm_sets, n_sets, which, apply_out_fn, nullptr, [&](const SetGroup& grp) {
        const size_t n = (size_t)grp.g * per_set;
        HIP_TRY(ctx, hipMemcpyAsync(tmp.data(), grp.y, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        double* dst = out_y + (size_t)grp.s0 * per_set;
        for (size_t i = 0; i < n; ++i) dst[i] = (double)tmp[i];
        return (int)NPBNN_OK;
    });
}

}  // extern "C"

extern "C" {

int npbnn_device_synchronize(int device_id) {
    HIP_TRY(nullptr, hipSetDevice(device_id));
    HIP_TRY(nullptr, hipDeviceSynchronize());
    return NPBNN_OK;
}

int npbnn_pinned_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return fail(nullptr, NPBNN_E_ARG, "pinned_alloc: bad arguments");
    *out = nullptr;
    HIP_TRY(nullptr, hipHostMalloc(out, bytes));
    return NPBNN_OK;
}

void npbnn_pinned_free(void* ptr) {
    if (ptr) (void)hipHostFree(ptr);
}

int npbnn_time_pass(npbnn_ctx* ctx, const double* W_packed, int n_candidates, int iters, double* ms_kernel, int* used_candidates) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (iters < 1 || !ms_kernel || !W_packed) return fail(ctx, NPBNN_E_ARG, "time_pass: bad arguments");
    if (!ctx->arch_set) return fail(ctx, NPBNN_E_STATE, "time_pass: call npbnn_set_arch first");
    const int lik = ctx->net.lik_kind;
    Dataset& d = ctx->ds[0];
    int rc = check_dataset_for_lik(ctx, d, lik);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchPlan lp;
    rc = plan_launch(ctx, 0, &lp, 0, n_candidates < 1 ? kMaxCand : n_candidates, false, true);
    if (rc) return rc;
    rc = ensure_work_buffers(ctx, lp.n_waves);
    if (rc) return rc;
    rc = stage_weights(ctx, W_packed, nullptr, nullptr);
    if (rc) return rc;
    PassDesc pd{};
    pd.t0 = 0;
    pd.n_cand = lp.n_cand;          // every candidate = the staged weights (empty patch lists): same work as a chain pass
    EvalParams p = make_params(ctx, d);
    p.partials = ctx->d_partials;
    p.inst_w = d.inst_w;
    p.use_classw = ctx->n_classw > 0 ? 1 : 0;
    p.has_pass = 1;
    p.pass_desc[0] = pd;
    p.pv = nullptr;
    p.pos = nullptr;
    p.pscale = nullptr;
    p.M = 0;
    DevBuf<unsigned long long> d_stamps;
    if (getenv("NPBNN_EVAL_STAMPS")) {      // diagnostics: per-phase wall-clock stamps of the last launch
        if ((rc = d_stamps.reserve(ctx, (size_t)lp.grid * 32))) return rc;     // [grid][8] wave 0 + [grid][16] per wave + [grid][8] prologue
        HIP_TRY(ctx, hipMemset(d_stamps, 0, (size_t)lp.grid * 32 * sizeof(unsigned long long)));
        p.stamps = d_stamps;
    }
    rc = push_eval_params(ctx, p);
    if (rc) return rc;
    if (lp.wide) {      // the pass of the weight-streamed path: its layers' products + the likelihood kernel, timed together
        const float* img = ctx->d_image;
        if (lp.n_cand > 1) {          // (every candidate = the staged weights, as on the resident path)
            rc = wide_cand_begin(ctx);
            if (rc) return rc;
            img = ctx->d_wide_cand;
        }
        for (int i = 0; i < 3 && !rc; ++i) rc = wide_forward(ctx, 0, img, false, false, nullptr, lp.n_cand);
        HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
        for (int i = 0; i < iters && !rc; ++i) rc = wide_forward(ctx, 0, img, false, false, nullptr, lp.n_cand);
        HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (rc) return rc;
        float msw = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&msw, ctx->ev[0], ctx->ev[1]));
        *ms_kernel = (double)msw / iters;
        if (used_candidates) *used_candidates = lp.n_cand;
        return NPBNN_OK;
    }
    for (int i = 0; i < 3; ++i)
        hipLaunchKernelGGL(lp.fn, dim3(lp.grid), dim3(lp.wpb * 64), lp.lds, ctx->stream, (const EvalParams*)ctx->d_eparams, 0, 1);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    for (int i = 0; i < iters; ++i)
        hipLaunchKernelGGL(lp.fn, dim3(lp.grid), dim3(lp.wpb * 64), lp.lds, ctx->stream, (const EvalParams*)ctx->d_eparams, 0, 1);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipGetLastError());
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    *ms_kernel = (double)ms / iters;
    if (used_candidates) *used_candidates = lp.n_cand;
    if (getenv("NPBNN_TIME_PASS_ONE_BY_ONE")) {      // diagnostics: every launch between events of its own, the stream idle before it (what a profiler's trace shows)
        double sum = 0.0, mn = 1e30, mx = 0.0;
        for (int i = 0; i < iters; ++i) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
            hipLaunchKernelGGL(lp.fn, dim3(lp.grid), dim3(lp.wpb * 64), lp.lds, ctx->stream, (const EvalParams*)ctx->d_eparams, 0, 1);
            HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            float one = 0.f;
            HIP_TRY(ctx, hipEventElapsedTime(&one, ctx->ev[0], ctx->ev[1]));
            sum += one; if (one < mn) mn = one; if (one > mx) mx = one;
        }
        fprintf(stderr, "[npbnn time_pass] %d launches one by one: %.2f us mean (%.2f-%.2f); back to back %.2f us per launch\n", iters, 1e3 * sum / iters, 1e3 * mn,
                1e3 * mx, 1e3 * (double)ms / iters);
    }
    if (const char* ns = getenv("NPBNN_TIME_PASS_STREAMS")) {      // diagnostics: the same independent launches dealt over several streams
        const int n_streams = atoi(ns) > 1 ? (atoi(ns) > 4 ? 4 : atoi(ns)) : 1;
        hipStream_t ss[4];
        for (int i = 0; i < n_streams; ++i) HIP_TRY(ctx, hipStreamCreateWithFlags(&ss[i], hipStreamNonBlocking));
        for (int rep = 0; rep < 2; ++rep) {
            const double t0 = wall_us();
            for (int i = 0; i < iters; ++i)
                hipLaunchKernelGGL(lp.fn, dim3(lp.grid), dim3(lp.wpb * 64), lp.lds, ss[i % n_streams], (const EvalParams*)ctx->d_eparams, 0, 1);
            for (int i = 0; i < n_streams; ++i) HIP_TRY(ctx, hipStreamSynchronize(ss[i]));
            if (rep) fprintf(stderr, "[npbnn time_pass] %d independent launches dealt over %d stream(s): %.2f us per launch (wall clock)\n", iters, n_streams,
                             (wall_us() - t0) / iters);
        }
        for (int i = 0; i < n_streams; ++i) (void)hipStreamDestroy(ss[i]);
    }
    if (d_stamps) report_eval_stamps(d_stamps, lp.grid, lp.wpb, 0);
    return NPBNN_OK;
}

int npbnn_time_wide(npbnn_ctx* ctx, const double* W_packed, int iters, double* ms_layer0, double* ms_pass, int* info) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (iters < 1 || !ms_layer0 || !ms_pass || !W_packed) return fail(ctx, NPBNN_E_ARG, "time_wide: bad arguments");
    if (!ctx->arch_set) return fail(ctx, NPBNN_E_STATE, "time_wide: call npbnn_set_arch first");
    Dataset& d = ctx->ds[0];
    int rc = check_dataset_for_lik(ctx, d, ctx->net.lik_kind);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchPlan lp;
    rc = plan_launch(ctx, 0, &lp, 0, 1, false, true);
    if (rc) return rc;
    if (!lp.wide) return fail(ctx, NPBNN_E_STATE, "time_wide: this network runs on the LDS-resident path");
    rc = ensure_work_buffers(ctx, lp.n_waves);
    if (rc) return rc;
    rc = stage_weights(ctx, W_packed, nullptr, nullptr);
    if (rc) return rc;
    EvalParams p = make_params(ctx, d);
    p.partials = ctx->d_partials;
    p.inst_w = d.inst_w;
    p.use_classw = ctx->n_classw > 0 ? 1 : 0;
    rc = push_eval_params(ctx, p);
    if (rc) return rc;
    int geo[4] = {0, 0, 0, 0};
    for (int only0 = 1; only0 >= 0; --only0) {
        for (int i = 0; i < 3 && !rc; ++i) rc = wide_forward(ctx, 0, ctx->d_image, false, only0 != 0, geo);
        HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
        for (int i = 0; i < iters && !rc; ++i) rc = wide_forward(ctx, 0, ctx->d_image, false, only0 != 0, nullptr);
        HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (rc) return rc;
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        *(only0 ? ms_layer0 : ms_pass) = (double)ms / iters;
    }
    if (info) for (int i = 0; i < 4; ++i) info[i] = geo[i];
    return NPBNN_OK;
}

int npbnn_time_eval(npbnn_ctx* ctx, const double* W_packed, int iters, double* ms_main_kernel, double* ms_total) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (iters < 1 || !ms_main_kernel || !ms_total) return fail(ctx, NPBNN_E_ARG, "time_eval: bad arguments");
    if (!ctx->arch_set) return fail(ctx, NPBNN_E_STATE, "time_eval: call npbnn_set_arch first");
    const int lik = ctx->net.lik_kind;
    Dataset& d = ctx->ds[0];
    int rc = check_dataset_for_lik(ctx, d, lik);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchPlan lp;
    rc = plan_launch(ctx, 0, &lp, 0, 1, false, true, true);      // (the build npbnn_eval runs)
    if (rc) return rc;
    rc = ensure_work_buffers(ctx, lp.n_waves);
    if (rc) return rc;
    rc = stage_weights(ctx, W_packed, nullptr, nullptr);
    if (rc) return rc;
    EvalParams p = make_params(ctx, d);
    p.partials = ctx->d_partials;
    p.inst_w = d.inst_w;
    p.use_classw = ctx->n_classw > 0 ? 1 : 0;
    FinalizeParams f{};
    f.partials = ctx->d_partials;
    f.n_waves = lp.n_waves;
    f.lik_kind = lik;
    f.k_targets = ctx->net.k_targets;
    f.n_rows = d.m->n_rows;
    f.lik_temp = 1.0;
    f.out = ctx->d_out;
    rc = push_eval_params(ctx, p);
    if (rc) return rc;
    rc = push_finalize_params(ctx, f);
    if (rc) return rc;
    // (1) the dominant kernel alone: `iters` back-to-back launches between one pair of events (per-launch event pairs
    //     would add ~4 us of command-processor overhead to each 20 us kernel); includes the ~1.5 us launch boundary
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 3 && !rc; ++i) rc = launch_plain_eval(ctx, lp, 0);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    for (int i = 0; i < iters && !rc; ++i) rc = launch_plain_eval(ctx, lp, 0);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (rc) return rc;
    float burst = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&burst, ctx->ev[0], ctx->ev[1]));
    const double sum = (double)burst;
    // (2) evaluation = eval kernel + finalize
    HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    for (int i = 0; i < iters && !rc; ++i) {
        rc = launch_plain_eval(ctx, lp, 0);
        hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, ctx->stream, (const FinalizeParams*)ctx->d_fparams);
    }
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipGetLastError());
    float tot = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&tot, ctx->ev[0], ctx->ev[1]));
    *ms_main_kernel = sum / iters;
    *ms_total = (double)tot / iters;
    return NPBNN_OK;
}

}  // extern "C"
