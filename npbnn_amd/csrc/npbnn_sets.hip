// The replay of stored weight sets over a resident table (npbnn_sets.hip.h): the one loop behind npbnn_predict_sets and the entries
// that summarise its predictions on the device (np_bnn/BNN_lib.py:375-381, 715-748 run one RunPredict per stored sample).  Sets that
// share their activation slopes travel together, up to kMaxCand per streaming read of X: as many as the resident kernel holds images
// for, and on the weight-streamed path up to kWideMaxCand where the first layer's product is the fused one (one set per pass where it
// is not: more than 64 nodes, a contraction cut into K-slices).  A group whose scaled layer-0 weights leave the fp16 range repeats on the
// exact float32 path - on the weight-streamed path, where the packing reports per set, only the set that left it.  What an entry does
// with a group's float32 predictions is its sink.  NPBNN_INFO_REPLAY_PASSES / _MAX_GROUP: what the last replay launched.
#include "npbnn_stack.hip.h"

#include <cmath>

namespace npbnn_api {

int slope_group_len(const double* act_prm_sets, int n_act, int s0, int n_sets, int cap) {
    int g = 1;
    while (s0 + g < n_sets && g < cap &&
           (!act_prm_sets || n_act == 0 ||
            memcmp(act_prm_sets + (size_t)(s0 + g) * n_act, act_prm_sets + (size_t)s0 * n_act, (size_t)n_act * sizeof(double)) == 0))
        ++g;
    return g;
}

void load_group_slopes(npbnn_ctx* ctx, const double* act_prm_sets, int n_act, int s0) {
    for (int l = 0; l < kMaxLayers; ++l) ctx->net.act_prm[l] = 0.f;
    if (act_prm_sets)
        for (int l = 0; l < n_act; ++l) ctx->net.act_prm[l] = (float)act_prm_sets[(size_t)s0 * n_act + l];
}

int check_stack_budget(npbnn_ctx* ctx, const char* who, int n_sets, long long n_rows, int C, size_t elem_bytes, const char* type) {
    size_t budget = 1ull << 30;        // default budget of a device stack [n_sets][n_rows][out_dim]
    if (const char* e = getenv("NPBNN_HPD_STACK_BYTES")) { const long long v = atoll(e); if (v > 0) budget = (size_t)v; }
    const size_t row_bytes = (size_t)n_sets * C * elem_bytes;
    if ((size_t)n_rows * row_bytes > budget)
        return fail(ctx, NPBNN_E_NOMEM, "%s: the [%d][%lld][%d] %s stack takes %zu bytes, over the budget of %zu "
                    "(NPBNN_HPD_STACK_BYTES); at most %zu rows fit", who, n_sets, n_rows, C, type, (size_t)n_rows * row_bytes, budget,
                    budget / row_bytes);
    return NPBNN_OK;
}

int replay_into_stack(npbnn_ctx* ctx, const char* who, const double* W_sets, const double* act_prm_sets, int n_sets, int which, int apply_out_fn,
                      const SetsTable& t, DevBuf<float>* stack) {
    const int C = ctx->net.n_out;
    int rc = check_stack_budget(ctx, who, n_sets, t.n_rows, C);
    if (rc || (rc = dev_alloc(ctx, *stack, (size_t)n_sets * t.n_rows * C))) return rc;
    return replay_sets(ctx, who, W_sets, act_prm_sets, n_sets, which, apply_out_fn, stack->get(), SetSink());
}

EvalParams predict_params(npbnn_ctx* ctx, const Dataset& d, float* y_out, int apply_out_fn) {
    EvalParams p = make_params(ctx, d);
    p.labels = nullptr;
    p.targets = nullptr;
    p.net.lik_kind = NPBNN_LIK_NONE;
    p.y_out = y_out;
    p.predict_mode = apply_out_fn ? 2 : 1;
    p.weight_sets = 1;
    p.lay = layout_for(ctx, d, true);
    return p;
}

int replay_sets(npbnn_ctx* ctx, const char* who, const double* W_sets, const double* act_prm_sets, int n_sets, int which, int apply_out_fn,
                float* y_stack, const SetSink& sink) {
    Dataset& d = ctx->ds[which];
    const int n_act = ctx->net.n_layers - 1;
    const size_t per_set = (size_t)d.m->n_rows * ctx->net.n_out;
    const size_t wn = (size_t)ctx->n_weights;
    hipStream_t st = ctx->stream;
    int rc;
    if (!y_stack && (rc = ctx->d_y.reserve(ctx, kMaxCand * per_set))) return rc;
    FiTimer tm;
    double pass_ns = 0.0, sink_ns = 0.0;
    std::vector<double> wstage(kMaxCand * wn);
    ctx->replay_passes = 0;
    ctx->replay_max_group = 0;
    int s0 = 0;
    bool alone_f32 = false;        // set s0 left the fp16 range in the pass before (weight-streamed path): it runs alone, on the float32 path
    while (s0 < n_sets) {
        int g = alone_f32 ? 1 : slope_group_len(act_prm_sets, n_act, s0, n_sets, kMaxCand);
        float* y = y_stack ? y_stack + (size_t)s0 * per_set : ctx->d_y.get();
        for (int attempt = alone_f32 ? 1 : 0; attempt < 2; ++attempt) {
            alone_f32 = false;
            LaunchPlan lp;
            rc = plan_launch(ctx, which, &lp, attempt, g, true);
            if (rc) return rc;
            if (lp.n_cand < g) g = lp.n_cand;          // (fewer images fit the LDS, or the product is not the fused one: the rest waits for the next round)
            if (lp.wide) lp.n_cand = g;
            memcpy(wstage.data(), W_sets + (size_t)s0 * wn, (size_t)g * wn * sizeof(double));
            tm.mark(0, st);
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_wraw, wstage.data(), (size_t)g * wn * sizeof(double), hipMemcpyHostToDevice, st));
            load_group_slopes(ctx, act_prm_sets, n_act, s0);
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_overflow, 0, (1 + kSetFlags) * sizeof(int), st));
            launch_pack_group(ctx, lp, ctx->d_wraw, nullptr, g);
            HIP_TRY(ctx, hipGetLastError());
            rc = push_eval_params(ctx, predict_params(ctx, d, y, apply_out_fn));
            if (rc) return rc;
            rc = launch_plain_eval(ctx, lp, which);
            if (rc) return rc;
            HIP_TRY(ctx, hipGetLastError());
            tm.mark(1, st);
            int flags[1 + kSetFlags] = {0};
            HIP_TRY(ctx, hipMemcpyAsync(flags, ctx->d_overflow, sizeof(flags), hipMemcpyDeviceToHost, st));
            // (push_eval_params stages through one pinned slot: the launch that reads it must be in before the next write)
            HIP_TRY(ctx, hipStreamSynchronize(st));
            pass_ns += tm.ns(0, 1);
            ++ctx->replay_passes;
            if (g > ctx->replay_max_group) ctx->replay_max_group = g;
            int ovf = flags[0], bad = -1;              // bad: the first set of the group out of the fp16 range (resident path: one word for the group)
            for (int j = g - 1; j >= 0; --j) {
                ovf |= flags[1 + j];
                if ((lp.wide ? flags[1 + j] : flags[0]) & kFlagF16Range) bad = j;
            }
            if (ovf & kFlagStructure) return fail(ctx, NPBNN_E_ARG, "%s: a layer-0 weight is not zero where the mask given to npbnn_set_layer_mask is", who);
            if (!ctx->net.l0_f16 || bad < 0) break;
            if (ctx->l0_option == NPBNN_L0_F16) return fail(ctx, NPBNN_E_RANGE, "%s: a layer-0 weight left the fp16 range", who);
            if (!lp.wide) continue;                    // resident path: the whole group again on the float32 path
            // weight-streamed path: the sets before it are delivered as computed, it repeats alone, a fresh group follows it
            if (bad > 0) { g = bad; alone_f32 = true; break; }
            g = 1;
        }
        // the group's predictions [g][rows][C] to the entry, before the next group overwrites them
        tm.mark(2, st);
        if (sink && (rc = sink(SetGroup{s0, g, y}))) return rc;
        HIP_TRY(ctx, hipGetLastError());
        tm.mark(3, st);
        if (tm.on) {
            HIP_TRY(ctx, hipStreamSynchronize(st));
            sink_ns += tm.ns(2, 3);
        }
        s0 += g;
    }
    ctx->fi_ns[1] = pass_ns > (double)INT_MAX ? INT_MAX : (int)pass_ns;
    ctx->fi_ns[2] = sink_ns > (double)INT_MAX ? INT_MAX : (int)sink_ns;
    return NPBNN_OK;
}

int fetch_flags_and_totals(npbnn_ctx* ctx, const int* d_flag, const double* d_part, size_t n_q, int n_wg, int* flags, std::vector<double>* totals) {
    hipStream_t st = ctx->stream;
    std::vector<double> h_part(n_q * n_wg);
    HIP_TRY(ctx, hipMemcpyAsync(flags, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    if (!h_part.empty()) HIP_TRY(ctx, hipMemcpyAsync(h_part.data(), d_part, h_part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    totals->assign(n_q, 0.0);
    for (size_t q = 0; q < n_q; ++q)
        for (int w = 0; w < n_wg; ++w) (*totals)[q] += h_part[q * n_wg + w];
    return NPBNN_OK;
}

int open_sets_table(npbnn_ctx* ctx, const char* who, int which, SetsTable* t) {
    if (which != 0 && which != 1) return fail(ctx, NPBNN_E_ARG, "%s: which must be 0 or 1", who);
    if (!ctx->arch_set) return fail(ctx, NPBNN_E_STATE, "%s: call npbnn_set_arch first", who);
    t->d = &ctx->ds[which];
    const int rc = check_dataset_for_lik(ctx, *t->d, NPBNN_LIK_NONE);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    t->n_rows = t->d->m->n_rows;
    t->st = ctx->stream;
    t->n_wg = (int)grid_for(t->n_rows);
    return NPBNN_OK;
}

int check_sigma_sets(npbnn_ctx* ctx, const char* who, const double* sigma_sets, int n_sets, int T) {
    for (size_t i = 0; i < (size_t)n_sets * T; ++i)
        if (!(sigma_sets[i] > 0.0) || !std::isfinite(sigma_sets[i]))
            return fail(ctx, NPBNN_E_ARG, "%s: sigma of set %zu, target %zu is %g; every sigma must be positive and finite", who, i / T, i % T,
                        sigma_sets[i]);
    return NPBNN_OK;
}

int PointOuts::copy_out(npbnn_ctx* ctx, hipStream_t st) const {
    for (int i = 0; i < count; ++i)
        if (s[i].host) HIP_TRY(ctx, hipMemcpyAsync(s[i].host, dev(i), s[i].len * sizeof(double), hipMemcpyDeviceToHost, st));
    return NPBNN_OK;
}

int finish_sets_entry(npbnn_ctx* ctx, const char* who, FiTimer& tm, const int* d_flag, const double* d_part, size_t n_q, int n_wg, int* ns_slot,
                      int n_classes, std::vector<double>* totals) {
    HIP_TRY(ctx, hipGetLastError());
    tm.mark(1, ctx->stream);
    int flags = 0;
    const int rc = fetch_flags_and_totals(ctx, d_flag, d_part, n_q, n_wg, &flags, totals);
    if (rc) return rc;
    *ns_slot = tm.ns(0, 1);
    if (flags & kFlagNaN) return fail(ctx, NPBNN_E_ARG, "%s: a prediction is NaN", who);
    if (n_classes > 0 && (flags & kFlagBadLabel)) return fail(ctx, NPBNN_E_ARG, "%s: a label lies outside [0, %d)", who, n_classes);
    return NPBNN_OK;
}

}  // namespace npbnn_api
