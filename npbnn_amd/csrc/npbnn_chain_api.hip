// Device-resident chains behind the C ABI (include/npbnn_hip.h): npbnn_chain_run, the group pass, the exchange run.
// Host-side orchestration only: uploads, the batch's launches on the chain's stream(s), the result copy.
#define NPBNN_KERNELS_CHAIN
#include "npbnn_ctx.hip.h"

extern "C" int npbnn_comm_allgather_inplace_stream_(npbnn_comm* c, double* d_buf, int count, void* stream);
extern "C" int npbnn_comm_info_(const npbnn_comm* c, int* device, int* rank, int* nranks);
extern "C" void npbnn_comm_abort_(npbnn_comm* c);
extern "C" int npbnn_comm_wait_stream_(npbnn_comm* c, void* stream, const char* what);

namespace {

// ---- a device batch of the chain in three phases: prepare (uploads, parameter blocks, first step), enqueue passes, collect ----
// one block, device and page-locked host twin: [ChainDev | overflow | W | cnt | log u || accepted | logLik' | logPrior'];
// everything before `||` goes up in ONE copy at the start of a batch, the whole block comes back in one at its end
struct ResLayout { size_t w, cnt, logu, acc, llp, lpp, total; };
ResLayout res_layout(size_t kc, size_t wb) {
    const auto up256 = [](size_t v) { return (v + 255) / 256 * 256; };
    ResLayout L;
    L.w = 512;
    L.cnt = L.w + up256(wb);
    L.logu = L.cnt + up256(kc * sizeof(int));
    L.acc = L.logu + up256(kc * sizeof(double));
    L.llp = L.acc + up256(kc);
    L.lpp = L.llp + up256(kc * sizeof(double));
    L.total = L.lpp + up256(kc * sizeof(double));
    return L;
}
constexpr size_t kResFlagWord = 448;           // the block's flag word (kFlag...: ctx->d_chain_ovf), behind the room ChainDev has
static_assert(sizeof(ChainDev) <= kResFlagWord, "ChainDev must fit its slot of the result block");
static_assert(kSpecPartSlots == NPBNN_SCHED_SPEC_PART_SLOTS, "npbnn_sched_plan.h holds the evaluating workgroups against the slots spec_rounds reads");
int res_flags(const npbnn_ctx* ctx) { return *reinterpret_cast<const int*>(ctx->h_res + kResFlagWord); }   // (of the block that has come back)

// what a batch is made from: the caller's arrays, and how the batch is run
struct ChainArgs {
    const npbnn_chain_cfg* cfg;
    const double *W_in, *mask_packed;
    int K, M;
    const int32_t* idx; const double* delta; const int32_t* cnt; const double* log_u;     // the draws
    int seg_len; bool alone_on_device; int group_blocks;                                  // (see chain_prepare)
};

struct ChainBatch {
    LaunchPlan lp;
    ResLayout RL;
    int D = 1, schedule = NPBNN_SCHED_SERIAL, K = 0, M = 0;
    bool overlap = false;
    bool persist = false;                      // persistent form: one launch loops over the passes (device flags order them)
    bool sync = false;                         // overlapped schedule with the launches alternating between two streams (device flags)
    bool spec = false;                         // NPBNN_SCHED_PERSIST_SERIAL: the launch's build with the speculative step
    bool forked = false;                       // sync: the two streams have been made to wait for ctx->stream
    bool step_keeps_image = false;             // weight-streamed path: the step patches the candidate image itself (ChainParams::cand_image)
    bool make_cands = false;                   // weight-streamed path: the candidates are made between step and pass (ChainParams::prep_terms)
    size_t wb = 0;
    int launch = 0;                            // launches enqueued so far (overlapped schedule: the pass parity follows it)
    DevBuf<unsigned long long> d_stamps;       // diagnostics
    DevBuf<unsigned long long> d_estamps;      // diagnostics (NPBNN_EVAL_STAMPS: the evaluating workgroups' phases, last pass of the batch)
    double tw0 = 0.0, tw1 = 0.0;
};

// NPBNN_CHAIN_TIMING=2: synchronise after every stage of a batch's set-up and print what each took (diagnostics: it serialises
// what normally overlaps)
static int stage_timing() { static const int v = getenv("NPBNN_CHAIN_TIMING") ? atoi(getenv("NPBNN_CHAIN_TIMING")) : 0; return v >= 2; }
static void stage_mark(npbnn_ctx* ctx, const char* what, double* t_last) {
    if (!stage_timing()) return;
    (void)hipStreamSynchronize(ctx->stream);
    const double now = wall_us();
    fprintf(stderr, "[npbnn stage] %-28s %.1f us\n", what, now - *t_last);
    *t_last = wall_us();
}

// ---- rows split over ranks (npbnn_set_row_shard) ----
// this rank's record of a pass: per candidate and value in use, the sum of the pass's per-wave partials in the order the step kernel
// itself would add them (lanes take records lane, lane + 64, ... in turn, then a fixed butterfly) - written to the rank's own place in
// the gather buffer [rank][candidate][value]
__global__ void __launch_bounds__(1024) shard_sum_kernel(const double* __restrict__ partials, int n_blocks, int D, int lik_kind, int k_targets,
                                                         double* __restrict__ mine) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int nvals = partial_value_count(lik_kind, k_targets);
    for (int item = wave; item < D * nvals; item += nw) {
        const int j = item / nvals, v = partial_value_index(item % nvals, k_targets);
        const double* src = partials + ((size_t)j * kPartialStride + v) * n_blocks;
        double s = 0.0;
        for (int b = lane; b < n_blocks; b += 64) s += src[b];
        s = butterfly_sum_f64(s);
        if (lane == 0) mine[j * kPartialStride + v] = s;
    }
}
// the gathered records [rank][candidate][value] in the layout the step kernel sums: [candidate][value][rank] (rank order = the order
// of the addition, the same on every rank)
__global__ void __launch_bounds__(256) shard_spread_kernel(const double* __restrict__ gathered, int n_ranks, double* __restrict__ part) {
    const int rec = kMaxCand * kPartialStride;
    for (int i = threadIdx.x; i < rec * n_ranks; i += blockDim.x) {
        const int r = i / rec, e = i % rec;
        part[(size_t)e * n_ranks + r] = gathered[i];
    }
}

// between a pass and its step: every rank's record to every rank, on the chain's stream (RCCL) or through the host (gather callback)
int shard_exchange(npbnn_ctx* ctx, const LaunchPlan& lp, int D) {
    hipStream_t st = ctx->stream;
    const int rec = kMaxCand * kPartialStride;
    hipLaunchKernelGGL(shard_sum_kernel, dim3(1), dim3(1024), 0, st, (const double*)ctx->d_partials, lp.n_waves, D, ctx->net.lik_kind, ctx->net.k_targets,
                       ctx->d_shard_recv + (size_t)ctx->shard_rank * rec);
    if (ctx->shard_n > 1) {
        if (ctx->shard_comm) {
            const int rc = npbnn_comm_allgather_inplace_stream_(ctx->shard_comm, ctx->d_shard_recv, rec, st);
            if (rc) return fail(ctx, NPBNN_E_COMM, "chain_run: the gather of the row shards' sums failed");
        } else {
            double* mine = ctx->h_shard + (size_t)ctx->shard_n * rec;          // (send block behind the receive block)
            HIP_TRY(ctx, hipMemcpyAsync(mine, ctx->d_shard_recv + (size_t)ctx->shard_rank * rec, rec * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            if (ctx->shard_gather(ctx->shard_user, mine, ctx->h_shard, rec) != 0)
                return fail(ctx, NPBNN_E_COMM, "chain_run: the gather callback of the row shards failed");
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_shard_recv, ctx->h_shard, (size_t)ctx->shard_n * rec * sizeof(double), hipMemcpyHostToDevice, st));
        }
    }
    hipLaunchKernelGGL(shard_spread_kernel, dim3(1), dim3(256), 0, st, (const double*)ctx->d_shard_recv, ctx->shard_n, ctx->d_shard_part);
    return NPBNN_OK;
}

// ---- prepare, in stages: check, plan and schedule, reserve, upload, parameter blocks, launch.  Everything goes to ctx->stream. ----
// stage 1: every refusal the arguments and the context's state decide, before anything is reserved or enqueued
int prepare_check(npbnn_ctx* ctx, const ChainArgs& A) {
    const npbnn_chain_cfg* cfg = A.cfg;
    const int K = A.K, M = A.M, lik = ctx->net.lik_kind;
    if (lik == NPBNN_LIK_NONE) return fail(ctx, NPBNN_E_STATE, "chain_run: the architecture has no likelihood");
    if (cfg->prior_kind < 0 || cfg->prior_kind > NPBNN_PRIOR_LAPLACE) return fail(ctx, NPBNN_E_ARG, "chain_run: prior_kind=%d", cfg->prior_kind);
    for (int t = 0; t < K; ++t)
        if (A.cnt[t] < 0 || A.cnt[t] > M) return fail(ctx, NPBNN_E_ARG, "chain_run: cnt[%d]=%d outside 0..%d", t, A.cnt[t], M);
    // (the K * M weight indices are checked on the device, where they are read anyway: gather_pos_kernel)
    const int rc = check_dataset_for_lik(ctx, ctx->ds[0], lik);
    if (rc) return rc;
    if (ctx->shard_n > 0 && (A.group_blocks > 0 || A.seg_len > 0))
        return fail(ctx, NPBNN_E_STATE, "chain_run: a context whose rows are split over ranks runs plain batches only (no group pass, no exchange run)");
    if (cfg->sigma_mult || cfg->hastings) {
        if (!cfg->sigma_mult || !cfg->hastings || lik != NPBNN_LIK_GAUSS)
            return fail(ctx, NPBNN_E_ARG, "chain_run: sigma_mult and hastings go together, with the Gaussian likelihood");
        for (size_t i = 0; i < (size_t)K * ctx->net.k_targets; ++i)
            if (!(cfg->sigma_mult[i] > 0.0)) return fail(ctx, NPBNN_E_ARG, "chain_run: sigma_mult[%zu] is not positive", i);
    }
    if (cfg->prior_scale_w && cfg->prior_kind != NPBNN_PRIOR_UNIFORM)
        for (int i = 0; i < ctx->n_weights; ++i)
            if (!(cfg->prior_scale_w[i] > 0.0)) return fail(ctx, NPBNN_E_ARG, "chain_run: prior_scale_w[%d] is not positive", i);
    if (cfg->slope_idx || cfg->slope_delta) {          // trainable activation slopes
        if (!cfg->slope_idx || !cfg->slope_delta || cfg->n_slopes < 1 || cfg->n_slopes > kMaxLayers || cfg->n_slopes != ctx->net.n_layers - 1)
            return fail(ctx, NPBNN_E_ARG, "chain_run: slope_idx and slope_delta go together, with one slope per hidden layer (got %d for %d layers)",
                        cfg->n_slopes, ctx->net.n_layers);
        if (ctx->net.slope_off < 0) return fail(ctx, NPBNN_E_STATE, "chain_run: trainable slopes need NPBNN_OPT_TRAINABLE_SLOPES");
        if (A.seg_len > 0 || A.group_blocks > 0) return fail(ctx, NPBNN_E_ARG, "chain_run: trainable slopes run in plain batches only");
        for (int t = 0; t < K; ++t)
            if (cfg->slope_idx[t] < 0 || cfg->slope_idx[t] >= cfg->n_slopes) return fail(ctx, NPBNN_E_ARG, "chain_run: slope_idx[%d] out of range", t);
    }
    return NPBNN_OK;
}

// stage 2: the launch, and the schedule its passes run on (npbnn_sched_plan.h: the rule reads neither the plan nor the environment)
int prepare_plan(npbnn_ctx* ctx, const ChainArgs& A, ChainBatch* B) {
    const npbnn_chain_cfg* cfg = A.cfg;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LaunchPlan& lp = B->lp;
    int want_cand = cfg->n_candidates;
    if (want_cand < 1) want_cand = kMaxCand;            // 0 = as many as fit
    if (A.group_blocks > 0) want_cand = 1;
    if (cfg->slope_idx && ctx->wide) want_cand = 1;      // (weight-streamed path: candidates with slopes of their own travel one per pass)
    const int rc = plan_launch(ctx, 0, &lp, cfg->force_f32, want_cand, false, true);
    if (rc) return rc;
    if (lp.wide && A.group_blocks > 0)
        return fail(ctx, NPBNN_E_STATE, "chain_run: a network on the weight-streamed path carries one weight set per pass (no group pass)");
    const int eval_wgs = lp.grid > ctx->n_cu - 1 ? ctx->n_cu - 1 : lp.grid;      // one workgroup of an overlapped launch runs the step: the others share the tiles
    npbnn_sched_req r;
    r.asked = cfg->schedule; r.D = lp.n_cand; r.K = A.K; r.M = A.M; r.eval_wgs = eval_wgs;
    r.alone = A.alone_on_device; r.plain = A.seg_len == 0; r.group = A.group_blocks > 0; r.boundaries_only = ctx->shard_n > 0 || lp.wide;
    r.sync_failed = ctx->sync_failed; r.persist_option = ctx->persist_option != 0;
    r.has_spec_build = lp.fn_spec != nullptr; r.own_slopes = cfg->slope_idx != nullptr; r.no_spec_step = getenv("NPBNN_NO_SPEC_STEP") != nullptr;
    r.prior_fits_spec = cfg->prior_kind == NPBNN_PRIOR_UNIFORM || (cfg->prior_kind == NPBNN_PRIOR_NORMAL && !cfg->prior_scale_w);
    const npbnn_sched_choice c = npbnn_sched_choose(&r, &ctx->sched);
    B->D = lp.n_cand; B->schedule = c.schedule; B->persist = c.persist; B->overlap = c.overlap; B->spec = c.spec;
    B->sync = c.sync && !c.persist;          // (two launch streams to fork and join)
    if (!ctx->stream_e[0]) {      // (with the chain's first batch, whatever its schedule: creating a stream takes milliseconds)
        for (int i = 0; i < 2; ++i) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream_e[i], hipStreamNonBlocking));
    }
    if (B->overlap) lp.grid = lp.n_waves = eval_wgs < 1 ? 1 : eval_wgs;
    if (A.group_blocks > 0) { lp.grid = A.group_blocks; lp.n_waves = A.group_blocks; }
    if (B->spec) lp.fn = lp.fn_spec;       // (the builds that carry spec_rounds)      // prepare the next pass ahead for every outcome
    return NPBNN_OK;
}

// stage 3: room for everything the batch puts on the device (the spec buffers' pass tags are cleared here, before they could repeat)
int prepare_reserve(npbnn_ctx* ctx, const ChainArgs& A, ChainBatch* B) {
    const npbnn_chain_cfg* cfg = A.cfg;
    const int K = A.K, M = A.M;
    const LaunchPlan& lp = B->lp;
    int rc = ensure_work_buffers(ctx, lp.n_waves);
    if (rc) return rc;
    const size_t wb = B->wb = (size_t)ctx->n_weights * sizeof(double);
    if ((size_t)K > ctx->res_k || (size_t)ctx->n_weights != ctx->res_nw) {
        size_t kc = (size_t)K > ctx->res_k ? (size_t)K : ctx->res_k;
        if (kc < kChainMinCapacity) kc = kChainMinCapacity;
        const ResLayout L = res_layout(kc, wb);
        ctx->d_res.reset();
        ctx->h_res.reset();
        ctx->d_mask.reset();        // sized by the number of weights as well
        ctx->res_k = 0; ctx->res_nw = 0;
        if ((rc = ctx->d_res.reserve(ctx, L.total)) || (rc = ctx->h_res.reserve(ctx, L.total))) return rc;
        ctx->res_k = kc; ctx->res_nw = (size_t)ctx->n_weights;
        char* b = ctx->d_res;
        ctx->d_chain = reinterpret_cast<ChainDev*>(b);
        ctx->d_chain_ovf = reinterpret_cast<int*>(b + kResFlagWord);
        ctx->d_wcur = reinterpret_cast<double*>(b + L.w);
        ctx->d_cnt = reinterpret_cast<int*>(b + L.cnt);
        ctx->d_logu = reinterpret_cast<double*>(b + L.logu);
        ctx->d_acc = reinterpret_cast<unsigned char*>(b + L.acc);
        ctx->d_llp = reinterpret_cast<double*>(b + L.llp);
        ctx->d_lpp = reinterpret_cast<double*>(b + L.lpp);
    }
    B->RL = res_layout(ctx->res_k, wb);
    if (A.mask_packed && (rc = ctx->d_mask.reserve(ctx, (size_t)ctx->n_weights))) return rc;
    if ((rc = ctx->d_pv.reserve(ctx, (size_t)2 * kMaxCand * M))) return rc;
    if (B->spec) {
        bool touch_new = false, part_new = false;
        if ((rc = ctx->d_spec.reserve(ctx, 1)) || (rc = ctx->d_spec_pv.reserve(ctx, (size_t)3 * kSpecOutcomes * kMaxCand * M)) ||
            (rc = ctx->d_spec_touch.reserve(ctx, (size_t)kMaxCand * ctx->n_weights * 4, 0, &touch_new)) ||
            (rc = ctx->d_spec_part.reserve(ctx, (size_t)2 * kMaxCand * kPartialStride * kSpecPartSlots * 2, 0, &part_new)))
            return rc;
        if (touch_new || part_new) ctx->spec_gen = 0xf0000000u;         // (forces the clearing below)
        if (ctx->spec_gen + (unsigned)K + 8u >= 0xf0000000u) {   // the batch's pass tags (one per pass, at most K + 1 passes) could repeat
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_spec_touch, 0, ctx->d_spec_touch.size() * sizeof(unsigned), ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_spec_part, 0, ctx->d_spec_part.size() * sizeof(unsigned long long), ctx->stream));
            ctx->spec_gen = 0;
        }
    }
    const size_t need = (size_t)K * M;
    {   // room for K x M draws, and when it grows, for at least kChainMinCapacity iterations of M
        const size_t cap = need > (size_t)kChainMinCapacity * M ? need : (size_t)kChainMinCapacity * M;
        const auto idx_ints = [](size_t n) { return (n * (sizeof(int) + sizeof(double)) + 512) / sizeof(int); };   // (indices, then the deviates: see prepare_upload)
        if ((rc = ctx->d_idx.reserve(ctx, idx_ints(need), idx_ints(cap))) || (rc = ctx->d_pos.reserve(ctx, need, cap)) ||
            (rc = ctx->d_pscale.reserve(ctx, need, cap)))
            return rc;
    }
    ctx->d_delta = reinterpret_cast<double*>(reinterpret_cast<char*>(ctx->d_idx.get()) + (need * sizeof(int) + 255) / 256 * 256);
    const size_t cap = (size_t)K > kChainMinCapacity ? (size_t)K : kChainMinCapacity;     // the optional per-iteration arrays
    if (cfg->sigma_mult && ((rc = ctx->d_smult.reserve(ctx, (size_t)K * NPBNN_MAX_TARGETS, cap * NPBNN_MAX_TARGETS)) || (rc = ctx->d_hast.reserve(ctx, (size_t)K, cap))))
        return rc;
    if (cfg->prior_scale_w && cfg->prior_kind != NPBNN_PRIOR_UNIFORM && (rc = ctx->d_pscale_w.reserve(ctx, (size_t)ctx->n_weights))) return rc;
    if (cfg->slope_idx && ((rc = ctx->d_sidx.reserve(ctx, (size_t)K, cap)) || (rc = ctx->d_sdelta.reserve(ctx, (size_t)K, cap)) || (rc = ctx->d_slopes.reserve(ctx, 1))))
        return rc;
    // Weight-streamed path: the step keeps the candidate image itself while a proposal fits its staged entries (ChainParams::cand_image);
    // wider ones get two launches over all compute units between step and pass - wide_cand_sync - and where those launches run anyway
    // they also MAKE the candidates (values, prior terms: wide_cand_prepare_kernel) - one workgroup's walk over 3 x 2.6 k entries is
    // 24 us of a 37-us step.  Plain batches without slopes of their own only (an exchange run stops a chain at the proposal that
    // leaves the fp16 range: the step must see that flag when it prepares).
    B->step_keeps_image = lp.wide && M <= kWideStepPatchMax && B->D == 1;
    B->make_cands = lp.wide && !B->step_keeps_image && A.seg_len == 0 && !cfg->slope_idx && !getenv("NPBNN_WIDE_STEP_MAKES");
    if (B->make_cands && (rc = ctx->d_prep_terms.reserve(ctx, (size_t)kMaxCand * M))) return rc;
    if (getenv("NPBNN_STEP_STAMPS")) {      // diagnostics: per-phase wall-clock stamps of the step kernel
        if ((rc = B->d_stamps.reserve(ctx, 1024 * 8))) return rc;
        HIP_TRY(ctx, hipMemset(B->d_stamps, 0, 1024 * 8 * sizeof(unsigned long long)));
    }
    if (getenv("NPBNN_EVAL_STAMPS") && A.group_blocks == 0) {
        if ((rc = B->d_estamps.reserve(ctx, (size_t)(lp.grid + 1) * 32))) return rc;
        HIP_TRY(ctx, hipMemset(B->d_estamps, 0, (size_t)(lp.grid + 1) * 32 * sizeof(unsigned long long)));
    }
    return NPBNN_OK;
}

// the state a batch starts from
ChainDev initial_state(const ChainArgs& A) {
    ChainDev init{};                // (counters, flags and done[] start at zero)
    init.logLik = A.cfg->cur_loglik;
    init.logPrior = A.cfg->cur_logprior;
    init.logPrior_rep = A.cfg->cur_logprior;
    for (int j = 0; j < NPBNN_MAX_TARGETS; ++j) init.sigma[j] = A.cfg->cur_sigma[j];
    init.void_launch = -2;
    init.seg_end = (A.seg_len > 0 && A.seg_len < A.K) ? A.seg_len : A.K;
    init.temperature = A.cfg->temperature;
    init.prepared = -1;             // (the first step kernel raises it to 0)
    init.started = -1;
    return init;
}

// stage 4: the draws, the head of the result block, the optional arrays
int prepare_upload(npbnn_ctx* ctx, const ChainArgs& A, const ChainBatch& B, double* t_stage) {
    const npbnn_chain_cfg* cfg = A.cfg;
    const int K = A.K;
    const size_t need = (size_t)K * A.M;
    hipStream_t st = ctx->stream;
    if (A.mask_packed) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_mask, A.mask_packed, B.wb, hipMemcpyHostToDevice, st));
    // indices and deviates: ONE copy when the caller laid them out the way the device holds them (idx, then delta at the next
    // multiple of 256 bytes - npbnn_amd's pre-draw does), else one each
    const size_t idx_bytes = need * sizeof(int), delta_off = (idx_bytes + 255) / 256 * 256;
    if (reinterpret_cast<const char*>(A.delta) == reinterpret_cast<const char*>(A.idx) + delta_off) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_idx, A.idx, delta_off + need * sizeof(double), hipMemcpyHostToDevice, st));
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_idx, A.idx, idx_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_delta, A.delta, need * sizeof(double), hipMemcpyHostToDevice, st));
    }
    stage_mark(ctx, "copy of indices + deviates", t_stage);
    {   // initial chain state, overflow flag, weights and the per-iteration scalars travel together (head of the block)
        const ChainDev init = initial_state(A);
        memset(ctx->h_res, 0, 512);
        memcpy(ctx->h_res, &init, sizeof(ChainDev));
        memcpy(ctx->h_res + B.RL.w, A.W_in, B.wb);
        memcpy(ctx->h_res + B.RL.cnt, A.cnt, (size_t)K * sizeof(int));
        memcpy(ctx->h_res + B.RL.logu, A.log_u, (size_t)K * sizeof(double));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_res, ctx->h_res, B.RL.acc, hipMemcpyHostToDevice, st));
    }
    stage_mark(ctx, "copy of state + weights", t_stage);
    if (cfg->sigma_mult) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_smult, cfg->sigma_mult, (size_t)K * ctx->net.k_targets * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_hast, cfg->hastings, (size_t)K * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (cfg->prior_scale_w && cfg->prior_kind != NPBNN_PRIOR_UNIFORM)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_pscale_w, cfg->prior_scale_w, B.wb, hipMemcpyHostToDevice, st));
    if (cfg->slope_idx) {
        SlopeState init_s{};
        for (int l = 0; l < cfg->n_slopes; ++l) init_s.cur[l] = cfg->cur_slopes[l];
        // (pageable sources: the copies are staged by the runtime before the calls return)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_slopes, &init_s, sizeof(SlopeState), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_sidx, cfg->slope_idx, (size_t)K * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_sdelta, cfg->slope_delta, (size_t)K * sizeof(double), hipMemcpyHostToDevice, st));
    }
    return NPBNN_OK;
}

// stage 5: the two parameter blocks.  What ChainParams c{} leaves at zero: no sigma multipliers, Hastings terms, per-weight prior
// scales, slopes of their own, prepared prior terms or speculative step unless the batch has them
void fill_chain_params(npbnn_ctx* ctx, const ChainArgs& A, const ChainBatch& B, ChainParams& c) {
    const npbnn_chain_cfg* cfg = A.cfg;
    const LaunchPlan& lp = B.lp;
    const bool sharded = ctx->shard_n > 0, f16 = ctx->net.l0_f16 != 0;
    c.st = ctx->d_chain;
    c.pass = reinterpret_cast<PassDesc*>(reinterpret_cast<char*>(ctx->d_eparams) + offsetof(EvalParams, pass_desc));   // inside the evaluation's block
    c.w_cur = ctx->d_wcur;
    c.mask = A.mask_packed ? ctx->d_mask : nullptr;
    c.idx = ctx->d_idx; c.delta = ctx->d_delta; c.cnt = ctx->d_cnt; c.log_u = ctx->d_logu;
    if (cfg->sigma_mult) { c.sigma_mult = ctx->d_smult; c.hastings = ctx->d_hast; }
    c.out_acc = ctx->d_acc; c.out_ll = ctx->d_llp; c.out_lp = ctx->d_lpp;
    c.partials = sharded ? ctx->d_shard_part : ctx->d_partials;
    c.image = ctx->d_image;
    c.cand_image = B.step_keeps_image ? ctx->d_wide_cand : nullptr;
    c.prep_terms = B.make_cands ? ctx->d_prep_terms : nullptr;
    c.pos = ctx->d_pos;
    c.pscale = f16 ? ctx->d_pscale : nullptr;
    c.pv = B.spec ? ctx->d_spec_pv : ctx->d_pv;      // (spec: the first step writes pass 0 into slot (parity 0, outcome 0))
    c.n_weights_spec = ctx->n_weights;
    if (B.spec) {
        c.spec = ctx->d_spec; c.spec_pv = ctx->d_spec_pv; c.spec_touch = ctx->d_spec_touch; c.spec_part = ctx->d_spec_part;
        c.spec_gen = (int)ctx->spec_gen;
        ctx->spec_gen += (unsigned)A.K + 8u;           // (a pass decides at least one iteration)
    }
    c.overflow = ctx->d_chain_ovf;
    c.stamps = B.d_stamps;
    c.K = A.K; c.M = A.M; c.D = B.D;
    c.n_blocks = sharded ? ctx->shard_n : lp.n_waves;      // (row shards: one record per rank, gathered)
    c.stop_on_overflow = A.seg_len > 0 ? 1 : 0;
    c.sync_test_skip = -1;
    if ((B.sync || B.persist) && ctx->debug_sync_skip >= 0) {       // (npbnn_debug_sync_skip_: provoke the time-out of the two-stream schedule, once)
        c.sync_test_skip = ctx->debug_sync_skip;
        ctx->debug_sync_skip = -1;
    }
    c.prior_kind = cfg->prior_kind;
    for (int l = 0; l < kMaxLayers; ++l) {
        c.prior_scale[l] = cfg->prior_scale[l];
        c.half_inv_s2[l] = cfg->prior_scale[l] > 0 ? 0.5 / (cfg->prior_scale[l] * cfg->prior_scale[l]) : 0.0;
    }
    if (cfg->prior_scale_w && cfg->prior_kind != NPBNN_PRIOR_UNIFORM) c.prior_scale_w = ctx->d_pscale_w;
    if (cfg->slope_idx) {
        c.slopes = ctx->d_slopes; c.slope_idx = ctx->d_sidx; c.slope_delta = ctx->d_sdelta;
        c.n_slopes = cfg->n_slopes;
        c.slope_term_in = cfg->slope_term_in_prior ? 1 : 0;
    }
    c.w_bound = cfg->w_bound; c.lik_temp = cfg->lik_temp; c.sigma_given = cfg->sigma_given;
    for (int j = 0; j < NPBNN_MAX_TARGETS; ++j) c.sigma_fixed[j] = cfg->sigma[j];
    c.n_rows = sharded ? ctx->shard_rows_total : ctx->ds[0].m->n_rows;
    c.net = ctx->net;
    c.class_w = ctx->n_classw ? ctx->d_classw : nullptr;
    c.w_scale = f16 ? ctx->store->wscale : nullptr;
}

void fill_eval_params(npbnn_ctx* ctx, const ChainArgs& A, const ChainBatch& B, EvalParams& p) {
    const Dataset& d = ctx->ds[0];
    const LaunchPlan& lp = B.lp;
    const bool f16 = ctx->net.l0_f16 != 0;
    p.partials = ctx->d_partials;
    p.inst_w = d.inst_w;
    p.use_classw = ctx->n_classw > 0 ? 1 : 0;
    p.has_pass = 1;
    if (B.d_estamps) p.stamps = B.d_estamps;
    p.pv = B.spec ? ctx->d_spec_pv : ctx->d_pv;
    p.pos = ctx->d_pos;
    p.pscale = f16 ? ctx->d_pscale : nullptr;
    p.M = A.M;
    p.chain = B.overlap ? ctx->d_cparams : nullptr;
    p.sync_mode = B.spec ? 3 : (B.sync || B.persist) ? 1 : 0;
    // (the persistent overlapped launch: workgroups run up to a pass ahead of each other, so the heavier shares taking turns evens out)
    p.share_rot = (B.persist && !B.spec && A.group_blocks == 0 && lp.grid > 1 && !getenv("NPBNN_NO_SHARE_ROTATION")) ? d.m->n_tiles % lp.grid : 0;
    p.cand_slopes = A.cfg->slope_idx ? &ctx->d_slopes->cand[0][0][0] : nullptr;
}

int prepare_params(npbnn_ctx* ctx, const ChainArgs& A, const ChainBatch& B) {
    const npbnn_chain_cfg* cfg = A.cfg;
    // activation slopes of the batch: fixed ones (ActFun("genReLU", prm=...): cfg->cur_slopes with no slope draws) go into the network
    // description every candidate reads; trainable ones travel per candidate in the weight image (ChainParams::slope_idx)
    for (int l = 0; l < kMaxLayers; ++l)
        ctx->net.act_prm[l] = (!cfg->slope_idx && l < cfg->n_slopes && l < NPBNN_MAX_LAYERS) ? (float)cfg->cur_slopes[l] : 0.f;
    ctx->batch_slopes = cfg->slope_idx != nullptr;
    ChainParams c{};
    fill_chain_params(ctx, A, B, c);
    EvalParams p = make_params(ctx, ctx->ds[0]);
    fill_eval_params(ctx, A, B, p);
    // both parameter blocks in one copy (they sit in one device allocation, laid out like the staging area)
    memcpy(ctx->h_params, &p, sizeof(EvalParams));
    memcpy(ctx->h_params + sizeof(EvalParams) + sizeof(FinalizeParams), &c, sizeof(ChainParams));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_eparams, ctx->h_params, sizeof(EvalParams) + sizeof(FinalizeParams) + sizeof(ChainParams), hipMemcpyHostToDevice,
                                ctx->stream));
    return NPBNN_OK;
}

// stage 6: step (pack the weight image, prepare candidates) -> [eval -> step (decide + prepare)]* ; a pass consumes 1..D iterations, so
// the number of passes is only known on the device
int prepare_launch(npbnn_ctx* ctx, const ChainArgs& A, const ChainBatch& B, double* t_stage) {
    const LaunchPlan& lp = B.lp;
    const bool f16 = ctx->net.l0_f16 != 0;
    const size_t need = (size_t)A.K * A.M;
    hipStream_t st = ctx->stream;
    {   // one launch: image position (and fp16-split scale) of every drawn entry, so that no kernel needs a dependent lookup - indices
        // outside the network are neutralised there and reported when the batch comes back (kFlagBadIndex) - and, in the blocks
        // behind those, the weight image of the state the batch starts from (accepted candidates are committed to it entry by entry)
        const int gather_blocks = (int)((need + 255) / 256), pack_blocks = lp.wide ? 0 : (pack_item_count(ctx->net, true) + 255) / 256;
        PackJob pk;
        pk.w = lp.wide ? nullptr : ctx->d_wcur;      // (weight-streamed path: its own packing kernel, below)
        pk.class_w = ctx->n_classw ? ctx->d_classw : nullptr;
        pk.image = ctx->d_image;
        pk.net = reinterpret_cast<const NetMeta*>(reinterpret_cast<const char*>(ctx->d_cparams) + offsetof(ChainParams, net));
        pk.w_scale = f16 ? ctx->store->wscale : nullptr;
        hipLaunchKernelGGL(gather_pos_kernel, dim3((unsigned)(gather_blocks + pack_blocks)), dim3(256), 0, st, ctx->d_idx, (long long)need, ctx->n_weights,
                           (const int*)ctx->d_w2img, (const float*)(f16 ? ctx->d_w2scale : nullptr), ctx->d_pos,
                           f16 ? ctx->d_pscale : (float*)nullptr, ctx->d_chain_ovf, gather_blocks, pk);
    }
    if (lp.wide) {       // the committed image of the state the batch starts from, and the candidate image as a copy of it
        wide_pack(ctx, ctx->d_wcur, nullptr, ctx->d_image, ctx->d_chain_ovf);
        const int rc = wide_cand_begin(ctx);
        if (rc) return rc;
    }
    stage_mark(ctx, "gather + pack kernel", t_stage);
    hipLaunchKernelGGL(chain_step_kernel, dim3(1), dim3(1024), 0, st, (const ChainParams*)ctx->d_cparams, 1);
    stage_mark(ctx, "first step kernel", t_stage);
    return NPBNN_OK;
}

// seg_len > 0: the chain stops deciding at iteration seg_len until an exchange kernel moves the limit (exchange run)
// alone_on_device: no other chain's launches share the GPU with this batch (the two-stream schedule counts on that)
// group_blocks > 0: the chain is one of a group pass (npbnn_chains_run_batched): one candidate per launch, overlapped schedule,
// its sums come from that many evaluating workgroups of the group's launches
int chain_prepare(npbnn_ctx* ctx, const npbnn_chain_cfg* cfg, const double* W_in, const double* mask_packed, int32_t K, int32_t M,
                  const int32_t* idx, const double* delta, const int32_t* cnt, const double* log_u, int seg_len, ChainBatch* B,
                  bool alone_on_device = true, int group_blocks = 0) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (!cfg || !W_in || K < 1 || M < 1 || !idx || !delta || !cnt || !log_u) return fail(ctx, NPBNN_E_ARG, "chain_run: bad arguments");
    if (!ctx->arch_set) return fail(ctx, NPBNN_E_STATE, "chain_run: call npbnn_set_arch first");
    B->tw0 = wall_us();
    const ChainArgs A{cfg, W_in, mask_packed, K, M, idx, delta, cnt, log_u, seg_len, alone_on_device, group_blocks};
    int rc;
    if ((rc = prepare_check(ctx, A)) || (rc = prepare_plan(ctx, A, B)) || (rc = prepare_reserve(ctx, A, B))) return rc;
    double t_stage = wall_us();
    stage_mark(ctx, "(host set-up so far)", &t_stage);
    if ((rc = prepare_upload(ctx, A, *B, &t_stage)) || (rc = prepare_params(ctx, A, *B))) return rc;
    stage_mark(ctx, "copy of parameter blocks", &t_stage);
    if ((rc = prepare_launch(ctx, A, *B, &t_stage))) return rc;
    B->K = K; B->M = M; B->forked = false; B->launch = 0;
    B->tw1 = wall_us();
    return NPBNN_OK;
}

// flag-ordered overlapped schedule: the launches go to two streams in turn.  Work enqueued on ctx->stream (uploads, the first
// step) must be complete before their first launch (fork), theirs before ctx->stream copies results back (join): both by
// host synchronisation - once a stream has waited for another stream's event, this runtime runs every later launch of the two
// one after the other, which is the very thing the schedule is there to avoid (measured: no overlap at all with event waits)
int chain_fork(npbnn_ctx* ctx, ChainBatch& B) {
    if (!B.sync || B.forked) return NPBNN_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    B.forked = true;
    return NPBNN_OK;
}
int chain_join(npbnn_ctx* ctx, ChainBatch& B) {
    if (!B.sync || !B.forked) return NPBNN_OK;
    for (int i = 0; i < 2; ++i) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream_e[i]));
    B.forked = false;
    return NPBNN_OK;
}

int chain_enqueue(npbnn_ctx* ctx, ChainBatch& B, int n) {
    hipStream_t st = ctx->stream;
    const LaunchPlan& lp = B.lp;
    if (B.persist) {            // ONE launch stands for the n passes: its workgroups loop over them (eval_kernel, n_loop)
        if (n > 0) hipLaunchKernelGGL(lp.fn, dim3(lp.grid + 1), dim3(lp.wpb * 64), lp.lds, st, (const EvalParams*)ctx->d_eparams, B.launch, n);
        B.launch += n;
    } else if (B.sync) {
        int rc = chain_fork(ctx, B);
        if (rc) return rc;
        for (int i = 0; i < n; ++i, ++B.launch) {    // (bit 30: not the last launch of this round - see sync_step_leave)
            if (i == 1) hipLaunchKernelGGL(sync_gate_kernel, dim3(1), dim3(64), 0, ctx->stream_e[B.launch & 1], ctx->d_chain, B.launch - 1);
            hipLaunchKernelGGL(lp.fn, dim3(lp.grid + 1), dim3(lp.wpb * 64), lp.lds, ctx->stream_e[B.launch & 1], (const EvalParams*)ctx->d_eparams,
                               B.launch | (i + 1 < n ? (1 << 30) : 0), 1);
        }
    } else if (B.overlap) {
        for (int i = 0; i < n; ++i, ++B.launch)
            hipLaunchKernelGGL(lp.fn, dim3(lp.grid + 1), dim3(lp.wpb * 64), lp.lds, st, (const EvalParams*)ctx->d_eparams, B.launch, 1);
    } else {
        for (int i = 0; i < n; ++i, ++B.launch) {
            if (lp.wide) {      // the layers' products and the likelihood of the candidate image (kept by the step, or by wide_cand_sync)
                if (B.M > kWideStepPatchMax || B.D > 1) wide_cand_sync(ctx, B.M, B.D, B.make_cands);
                const int rcw = wide_forward(ctx, 0, ctx->d_wide_cand, true, false, nullptr, B.D);
                if (rcw) return rcw;
            } else {
                hipLaunchKernelGGL(lp.fn, dim3(lp.grid), dim3(lp.wpb * 64), lp.lds, st, (const EvalParams*)ctx->d_eparams, 0, 1);
            }
            if (ctx->shard_n > 0) {
                const int rc = shard_exchange(ctx, lp, B.D);
                if (rc) return rc;
            }
            hipLaunchKernelGGL(chain_step_kernel, dim3(1), dim3(1024), 0, st, (const ChainParams*)ctx->d_cparams, 0);
        }
    }
    return NPBNN_OK;
}

// after the result block has come back (h_res): hand the first k_take iterations' outcome to the caller
int chain_finish(npbnn_ctx* ctx, ChainBatch& B, const npbnn_chain_cfg* cfg, double* W_inout, uint8_t* out_accepted, double* out_loglik_prop,
                 double* out_logprior_prop, npbnn_chain_result* result, int k_take, bool exchange_run = false) {
    const ChainDev fin = *reinterpret_cast<const ChainDev*>(ctx->h_res.get());
    npbnn_sched_record_outcome(&ctx->sched, B.schedule, k_take, fin.n_passes + fin.n_void, fin.n_accepted);
    if (B.d_stamps) report_step_stamps(B.d_stamps);
    if (B.d_estamps) report_eval_stamps(B.d_estamps, B.lp.grid + (B.overlap ? 1 : 0), B.lp.wpb, (B.sync || B.persist) ? 1 : 0);
    const int flags = res_flags(ctx);
    if (flags & kFlagStructure) return fail(ctx, NPBNN_E_ARG, "chain_run: a layer-0 weight is not zero where the mask given to npbnn_set_layer_mask is");
    if (flags & kFlagBadIndex) return fail(ctx, NPBNN_E_ARG, "chain_run: a weight index of the batch is outside 0 .. %d (the entry was ignored)", ctx->n_weights - 1);
    const int overflow = (ctx->net.l0_f16 && (flags & kFlagF16Range)) ? 1 : 0;
    if (overflow && !exchange_run)           // W_inout untouched: the caller re-runs this batch with cfg->force_f32 = 1
        return fail(ctx, NPBNN_E_RANGE, "chain_run: a layer-0 weight left the fp16 range during this batch");
    {
        const char* b = ctx->h_res;
        memcpy(W_inout, b + B.RL.w, B.wb);
        memcpy(out_accepted, b + B.RL.acc, (size_t)k_take);
        if (out_loglik_prop) memcpy(out_loglik_prop, b + B.RL.llp, (size_t)k_take * sizeof(double));
        if (out_logprior_prop) memcpy(out_logprior_prop, b + B.RL.lpp, (size_t)k_take * sizeof(double));
    }
    for (int l = 0; l < NPBNN_MAX_LAYERS; ++l) result->slopes[l] = 0.0;
    if (ctx->batch_slopes) {             // (the stream is idle: the result block has just come back)
        SlopeState fs;
        HIP_TRY(ctx, hipMemcpy(&fs, ctx->d_slopes, sizeof(SlopeState), hipMemcpyDeviceToHost));
        for (int l = 0; l < kMaxLayers && l < NPBNN_MAX_LAYERS; ++l) result->slopes[l] = fs.cur[l];
    }
    result->loglik = fin.logLik;
    result->logprior = fin.n_accepted > 0 ? fin.logPrior_rep : cfg->cur_logprior;
    for (int j = 0; j < NPBNN_MAX_TARGETS; ++j) result->sigma[j] = fin.sigma[j];
    result->n_accepted = fin.n_accepted;
    result->n_passes = fin.n_passes;
    result->n_candidates = B.D;
    result->n_void_passes = fin.n_void;
    result->schedule = B.schedule;
    result->temperature = fin.temperature;
    result->iterations_done = k_take;
    result->overflow = overflow;          // (exchange run: the chain stopped before the proposal that overflows)
    return NPBNN_OK;
}

// the multi-chain entries: every job complete, no context twice (`entry`: who asks, for the text)
int check_jobs(const npbnn_chain_job* jobs, int n_jobs, const char* entry) {
    for (int q = 0; q < n_jobs; ++q) {
        const npbnn_chain_job& J = jobs[q];
        if (!J.ctx || !J.cfg || !J.W_inout || !J.result || !J.out_accepted) return fail(J.ctx, NPBNN_E_ARG, "%s: job %d incomplete", entry, q);
        for (int p2 = 0; p2 < q; ++p2)
            if (jobs[p2].ctx == J.ctx) return fail(J.ctx, NPBNN_E_ARG, "%s: jobs %d and %d share a ctx", entry, p2, q);
    }
    return NPBNN_OK;
}

// a failure in the middle of such an entry: job 0's context reports it (`from`: the context that holds the text, if another one does),
// and the first n jobs' streams are drained of what was enqueued for them
void drain_jobs(const npbnn_chain_job* jobs, int n, const npbnn_ctx* from = nullptr) {
    if (from && from != jobs[0].ctx) jobs[0].ctx->err = from->err;
    for (int q = 0; q < n; ++q) (void)hipStreamSynchronize(jobs[q].ctx->stream);
}

}  // namespace

extern "C" {

int npbnn_chain_run(npbnn_ctx* ctx, const npbnn_chain_cfg* cfg, double* W_inout, const double* mask_packed, int32_t K, int32_t M,
                    const int32_t* idx, const double* delta, const int32_t* cnt, const double* log_u, uint8_t* out_accepted,
                    double* out_loglik_prop, double* out_logprior_prop, npbnn_chain_result* result) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (!result || !out_accepted) return fail(ctx, NPBNN_E_ARG, "chain_run: bad arguments");
    static const bool timing = getenv("NPBNN_CHAIN_TIMING") != nullptr;     // diagnostics: host wall clock per phase
    ChainBatch B;
    int rc = chain_prepare(ctx, cfg, W_inout, mask_packed, K, M, idx, delta, cnt, log_u, 0, &B);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    int t_done = 0, n_rounds = 0;
    const ChainDev* now = reinterpret_cast<const ChainDev*>(ctx->h_res.get());
    while (t_done < K) {       // launch the least number of passes that can finish, look at the counter, repeat if short
        ++n_rounds;
        const double ta = timing ? wall_us() : 0.0;
        const int n_launch = npbnn_sched_passes(K - t_done, B.D, B.persist, B.overlap, ctx->sched.its_per_pass, 1.0);
        double t_stage = wall_us();
        rc = chain_enqueue(ctx, B, n_launch);
        if (!rc) rc = chain_join(ctx, B);
        if (rc) return rc;
        HIP_TRY(ctx, hipGetLastError());
        stage_mark(ctx, "passes", &t_stage);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_res, ctx->d_res, B.RL.total, hipMemcpyDeviceToHost, st));   // state + results, one copy
        stage_mark(ctx, "copy of the results", &t_stage);
        const double tb = timing ? wall_us() : 0.0;
        if (ctx->shard_comm && ctx->shard_n > 1) {      // (collectives in the stream: a bounded wait - a peer that is gone must not hang this rank)
            if (npbnn_comm_wait_stream_(ctx->shard_comm, st, "the row-sharded chain batch") != 0)
                return fail(ctx, NPBNN_E_COMM, "chain_run: the row-sharded batch did not complete (a peer failed?)");
        } else {
            HIP_TRY(ctx, hipStreamSynchronize(st));
        }
        if (timing) {
            const double tc = wall_us();
            fprintf(stderr, "[npbnn chain timing]   round %d: %d launches enqueued in %.0f us, waited %.0f us, t=%d of %d\n", n_rounds, n_launch, tb - ta,
                    tc - tb, reinterpret_cast<const ChainDev*>(ctx->h_res.get())->t, K);
        }
        if (now->aborted) {         // a device-side wait of the flag-ordered schedule timed out: nothing was decided after it
            ctx->sync_failed = true;
            return fail(ctx, NPBNN_E_SYNC, "chain_run: the flag-ordered overlapped schedule timed out at t=%d; retry on one stream", now->t);
        }
        if (now->t < t_done || (now->t == t_done && !B.overlap))
            return fail(ctx, NPBNN_E_STATE, "chain_run: the device chain made no progress (t=%d)", now->t);
        if (now->t == t_done && n_rounds > 64) return fail(ctx, NPBNN_E_STATE, "chain_run: the device chain is stuck at t=%d", now->t);
        t_done = now->t;
    }
    const double tw2 = wall_us();
    rc = chain_finish(ctx, B, cfg, W_inout, out_accepted, out_loglik_prop, out_logprior_prop, result, K);
    if (rc) return rc;
    npbnn_sched_record_timing(&ctx->sched, B.schedule, B.persist, K, n_rounds, result->n_passes + result->n_void_passes, tw2 - B.tw1);
    if (timing && ctx->d_spec && B.schedule == NPBNN_SCHED_PERSIST_SERIAL) {
        SpecState hs;
        if (hipMemcpy(&hs, ctx->d_spec, sizeof hs, hipMemcpyDeviceToHost) == hipSuccess && hs.rounds > 0)
            fprintf(stderr, "[npbnn chain timing]   step rounds %d: touch %.2f  candidates %.2f  descriptors %.2f  wait for the pass %.2f  decide+publish %.2f  "
                            "commit %.2f us per round\n", hs.rounds, hs.ticks[0] * 0.01 / hs.rounds, hs.ticks[1] * 0.01 / hs.rounds, hs.ticks[2] * 0.01 / hs.rounds,
                    hs.ticks[3] * 0.01 / hs.rounds, hs.ticks[4] * 0.01 / hs.rounds, hs.ticks[5] * 0.01 / hs.rounds);
    }
    if (timing)
        fprintf(stderr, "[npbnn chain timing] K=%d passes=%d (+%d void, %s) rounds=%d: setup %.0f us, passes %.0f us (%.2f us/pass), results %.0f us\n", K,
                result->n_passes, result->n_void_passes, B.overlap ? "overlapped" : "serial", n_rounds, B.tw1 - B.tw0, tw2 - B.tw1,
                (tw2 - B.tw1) / (result->n_passes > 0 ? result->n_passes : 1), wall_us() - tw2);
    return NPBNN_OK;
}


int npbnn_chains_run_batched(npbnn_chain_job* jobs, int32_t n_jobs, int32_t K) {
    if (!jobs || n_jobs < 2 || n_jobs > kMaxCand || K < 1) return fail(nullptr, NPBNN_E_ARG, "chains_run_batched: 2..%d chains, K >= 1", kMaxCand);
    npbnn_ctx* ctx0 = jobs[0].ctx;
    if (!ctx0) return fail(nullptr, NPBNN_E_ARG, "chains_run_batched: job 0 has no context");
    int force_f32 = 0, rc = check_jobs(jobs, n_jobs, "chains_run_batched");
    if (rc) return rc;
    for (int q = 0; q < n_jobs; ++q) {
        const npbnn_chain_job& J = jobs[q];
        if (!J.ctx->arch_set) return fail(J.ctx, NPBNN_E_STATE, "chains_run_batched: job %d: call npbnn_set_arch first", q);
        // replicas of one model over the same resident matrix: same device, same X, same network shape, same likelihood
        const npbnn_ctx* a = ctx0;
        const npbnn_ctx* b = J.ctx;
        if (b->device != a->device || b->ds[0].m->X != a->ds[0].m->X || b->ds[0].m->n_rows != a->ds[0].m->n_rows || b->n_weights != a->n_weights ||
            memcmp(&b->arch, &a->arch, sizeof(npbnn_arch)) != 0 || b->l0_blocks != a->l0_blocks || (b->n_classw > 0) != (a->n_classw > 0) ||
            (b->ds[0].inst_w != nullptr) != (a->ds[0].inst_w != nullptr))
            return fail(J.ctx, NPBNN_E_ARG, "chains_run_batched: job %d is not a replica of job 0 (same device, shared feature matrix "
                                            "(npbnn_share_data), same architecture and likelihood)", q);
        force_f32 |= J.cfg->force_f32;
    }
    HIP_TRY(ctx0, hipSetDevice(ctx0->device));
    Dataset& d0 = ctx0->ds[0];
    rc = check_dataset_for_lik(ctx0, d0, ctx0->net.lik_kind);
    if (rc) return rc;
    // the group's launch: one candidate per chain, the evaluating workgroups share the tiles, one step workgroup per chain
    LaunchPlan lpG;
    rc = plan_launch(ctx0, 0, &lpG, force_f32, n_jobs, false, true);
    if (rc) return rc;
    if (lpG.n_cand != n_jobs)
        return fail(ctx0, NPBNN_E_ARG, "chains_run_batched: %d weight images do not fit a compute unit's LDS together (%d do)", n_jobs, lpG.n_cand);
    int G = lpG.grid;
    if (G > ctx0->n_cu - n_jobs) G = ctx0->n_cu - n_jobs;
    if (G < 1) G = 1;
    std::vector<ChainBatch> B(n_jobs);
    std::vector<npbnn_chain_cfg> cfgs(n_jobs);
    for (int q = 0; q < n_jobs; ++q) {
        const npbnn_chain_job& J = jobs[q];
        cfgs[q] = *J.cfg;
        cfgs[q].force_f32 = force_f32;
        rc = chain_prepare(J.ctx, &cfgs[q], J.W_inout, J.mask_packed, K, J.M, J.idx, J.delta, J.cnt, J.log_u, 0, &B[q], false, G);
        if (rc) {
            drain_jobs(jobs, q + 1, J.ctx);
            return rc;
        }
        if ((J.ctx->net.l0_f16 != 0) != (ctx0->net.l0_f16 != 0)) {
            drain_jobs(jobs, q + 1);
            return fail(ctx0, NPBNN_E_STATE, "chains_run_batched: the chains ended up on different layer-0 paths");
        }
    }
    hipStream_t st = ctx0->stream;
    for (int q = 1; q < n_jobs; ++q) {          // the other chains' preparation (their own streams) before the first group launch
        npbnn_ctx* c = jobs[q].ctx;
        if (!c->ev_x) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_x, hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->ev_x, c->stream));
        HIP_TRY(ctx0, hipStreamWaitEvent(st, c->ev_x, 0));
    }
    if ((rc = ctx0->d_gparams.reserve(ctx0, 1)) || (rc = ctx0->h_gparams.reserve(ctx0, 1))) return rc;
    {
        EvalParams g = make_params(ctx0, d0);
        g.partials = nullptr;
        g.inst_w = d0.inst_w;
        g.use_classw = ctx0->n_classw > 0 ? 1 : 0;
        g.has_pass = 0;
        g.group_n = n_jobs;
        for (int q = 0; q < n_jobs; ++q) {
            npbnn_ctx* c = jobs[q].ctx;
            GroupSlot& S = g.group[q];
            S.chain = c->d_cparams;
            S.pass = reinterpret_cast<const PassDesc*>(reinterpret_cast<const char*>(c->d_eparams) + offsetof(EvalParams, pass_desc));
            S.image = c->d_image;
            S.pv = c->d_pv;
            S.pos = c->d_pos;
            S.pscale = c->net.l0_f16 ? c->d_pscale : nullptr;
            S.partials = c->d_partials;
            S.M = jobs[q].M;
        }
        memcpy(ctx0->h_gparams, &g, sizeof g);
        HIP_TRY(ctx0, hipMemcpyAsync(ctx0->d_gparams, ctx0->h_gparams, sizeof g, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(ctx0, hipFuncSetAttribute(reinterpret_cast<const void*>(lpG.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lpG.lds));
    // a launch decides at most one iteration per chain and loses one to every accept (the pass in flight is void): what the chains'
    // last acceptance rates say is needed, then look and repeat if some chain is short
    int launch = 0, rounds = 0;
    std::vector<int> t_done(n_jobs, 0);
    for (;;) {
        int rem = 0;
        double acc = 0.0;
        for (int q = 0; q < n_jobs; ++q) {
            if (K - t_done[q] > rem) rem = K - t_done[q];
            const double a = jobs[q].ctx->sched.accept_rate < 0 ? 0.3 : jobs[q].ctx->sched.accept_rate;
            if (a > acc) acc = a;
        }
        if (rem == 0) break;
        if (++rounds > 64) return fail(ctx0, NPBNN_E_STATE, "chains_run_batched: the chains are stuck");
        const int n = npbnn_sched_passes_group(rem, acc);
        for (int i = 0; i < n; ++i, ++launch)
            hipLaunchKernelGGL(lpG.fn, dim3(G + n_jobs), dim3(lpG.wpb * 64), lpG.lds, st, (const EvalParams*)ctx0->d_gparams, launch, 1);
        HIP_TRY(ctx0, hipGetLastError());
        for (int q = 0; q < n_jobs; ++q) {
            npbnn_ctx* c = jobs[q].ctx;
            HIP_TRY(c, hipMemcpyAsync(c->h_res, c->d_res, B[q].RL.total, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(ctx0, hipStreamSynchronize(st));
        for (int q = 0; q < n_jobs; ++q) {
            const ChainDev* now = reinterpret_cast<const ChainDev*>(jobs[q].ctx->h_res.get());
            if (now->t < t_done[q]) return fail(jobs[q].ctx, NPBNN_E_STATE, "chains_run_batched: chain %d went backwards (t=%d)", q, now->t);
            t_done[q] = now->t;
        }
    }
    for (int q = 0; q < n_jobs; ++q)            // (nothing is handed back unless every chain's batch is good: the caller repeats the
        if (jobs[q].ctx->net.l0_f16 && (res_flags(jobs[q].ctx) & kFlagF16Range))      // whole group)
            return fail(ctx0, NPBNN_E_RANGE, "chains_run_batched: a layer-0 weight of chain %d left the fp16 range during this batch", q);
    for (int q = 0; q < n_jobs; ++q) {
        const npbnn_chain_job& J = jobs[q];
        rc = chain_finish(J.ctx, B[q], &cfgs[q], J.W_inout, J.out_accepted, J.out_loglik_prop, J.out_logprior_prop, J.result, K);
        if (rc) {
            if (J.ctx != ctx0) ctx0->err = J.ctx->err;
            return rc;
        }
    }
    return NPBNN_OK;
}

int npbnn_chains_run_exchange(npbnn_comm* comm, npbnn_chain_job* jobs, int32_t n_jobs, int32_t n_chains, int32_t seg_len, int32_t n_seg,
                              const int32_t* swap_j, const int32_t* swap_k, const double* swap_logu, double launch_slack,
                              double* out_records, int32_t* out_segments_done) {
    if (!jobs || n_jobs < 1 || n_jobs > 64 || seg_len < 1 || n_seg < 1 || !swap_j || !swap_k || !swap_logu || !out_segments_done)
        return fail(nullptr, NPBNN_E_ARG, "chains_run_exchange: bad arguments");
    if ((long long)seg_len * n_seg > (1 << 24)) return fail(nullptr, NPBNN_E_ARG, "chains_run_exchange: %d x %d iterations in one call", n_seg, seg_len);
    int device = -1, rank = 0, world = 1;
    if (comm) {
        int rc = npbnn_comm_info_(comm, &device, &rank, &world);
        if (rc) return rc;
    }
    if (n_chains != world * n_jobs)
        return fail(nullptr, NPBNN_E_ARG, "chains_run_exchange: %d chains on %d ranks x %d jobs (every rank must hold the same number)", n_chains, world, n_jobs);
    if (int rc = check_jobs(jobs, n_jobs, "chains_run_exchange")) return rc;
    for (int q = 0; q < n_jobs; ++q) {
        const npbnn_chain_job& J = jobs[q];
        if (device < 0) device = J.ctx->device;
        if (J.ctx->device != device) return fail(J.ctx, NPBNN_E_ARG, "chains_run_exchange: job %d is on device %d, the others on %d", q, J.ctx->device, device);
        if (J.chain_id != rank + world * q) return fail(J.ctx, NPBNN_E_ARG, "chains_run_exchange: job %d holds chain %d, expected %d", q, J.chain_id, rank + world * q);
    }
    for (int s = 0; s < n_seg; ++s)
        if (swap_j[s] < 0 || swap_j[s] >= n_chains || swap_k[s] < 0 || swap_k[s] >= n_chains)
            return fail(jobs[0].ctx, NPBNN_E_ARG, "chains_run_exchange: swap %d names chains %d, %d of %d", s, swap_j[s], swap_k[s], n_chains);
    if (!(launch_slack > 0.0)) launch_slack = 1.25;       // (< 1 starves the segments on purpose: tests of the shortfall path)
    const int K = seg_len * n_seg;
    npbnn_ctx* ctx0 = jobs[0].ctx;
    HIP_TRY(ctx0, hipSetDevice(device));
    const auto up256 = [](size_t v) { return (v + 255) / 256 * 256; };
    // per-ctx exchange block; the records live in job 0's and are shared
    struct XLayout { size_t sj, sk, su, state, rec, cold, total; };
    std::vector<XLayout> XL(n_jobs);
    std::vector<ChainBatch> B(n_jobs);
    const size_t rec_bytes = (size_t)n_seg * n_chains * kRecDoubles * sizeof(double);
    int rc_prepare = NPBNN_OK;       // first failure of this rank before anything is enqueued (the ranks agree on it below)
    auto size_exchange_block = [&](int q) -> int {
        npbnn_ctx* ctx = jobs[q].ctx;
        XLayout& L = XL[q];
        L.sj = 256;
        L.sk = L.sj + up256((size_t)n_seg * sizeof(int));
        L.su = L.sk + up256((size_t)n_seg * sizeof(int));
        L.state = L.su + up256((size_t)n_seg * sizeof(double));
        L.rec = L.state + up256((size_t)n_seg * NPBNN_XSTATE_DOUBLES * sizeof(double));
        L.cold = L.rec + (q == 0 ? up256(rec_bytes) : 0);
        L.total = L.cold + (jobs[q].out_cold_w ? up256((size_t)n_seg * ctx->n_weights * sizeof(double)) : 0);
        static_assert(sizeof(ExchangeParams) <= 256, "ExchangeParams must fit its slot");
        int rc = ctx->d_xbuf.reserve(ctx, L.total, L.total + L.total / 2);
        if (!rc) rc = ctx->h_xbuf.reserve(ctx, L.total, L.total + L.total / 2);
        if (rc) return rc;
        if (!ctx->ev_x) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_x, hipEventDisableTiming));
        return NPBNN_OK;
    };
    for (int q = 0; q < n_jobs && !rc_prepare; ++q) {
        rc_prepare = size_exchange_block(q);
        if (rc_prepare && jobs[q].ctx != ctx0) ctx0->err = jobs[q].ctx->err;
    }
    double* d_rec = rc_prepare ? nullptr : reinterpret_cast<double*>(ctx0->d_xbuf + XL[0].rec);
    // Everything that can fail on this rank alone (bad draws, a weight outside the fp16 range, allocation) is checked BEFORE the
    // first collective is enqueued, and the ranks agree on the outcome (one host-side all-gather): either every rank enqueues
    // its in-place all-gathers, or none does.
    for (int q = 0; q < n_jobs && !rc_prepare; ++q) {
        const npbnn_chain_job& J = jobs[q];
        npbnn_ctx* ctx = J.ctx;
        int rc = chain_prepare(ctx, J.cfg, J.W_inout, J.mask_packed, K, J.M, J.idx, J.delta, J.cnt, J.log_u, seg_len, &B[q], n_jobs == 1);
        if (rc) {
            drain_jobs(jobs, q + 1, ctx);
            rc_prepare = rc;
            break;
        }
        const XLayout& L = XL[q];
        ExchangeParams x{};
        x.rec = d_rec;
        x.swap_j = reinterpret_cast<const int*>(ctx->d_xbuf + L.sj);
        x.swap_k = reinterpret_cast<const int*>(ctx->d_xbuf + L.sk);
        x.swap_logu = reinterpret_cast<const double*>(ctx->d_xbuf + L.su);
        x.snap_state = reinterpret_cast<double*>(ctx->d_xbuf + L.state);
        x.snap_w = J.out_cold_w ? reinterpret_cast<double*>(ctx->d_xbuf + L.cold) : nullptr;
        x.world = world;
        x.per_rank = n_jobs;
        x.n_seg = n_seg;
        x.seg_len = seg_len;
        x.my_slot = rank * n_jobs + q;
        x.n_weights = ctx->n_weights;
        memset(ctx->h_xbuf, 0, 256);
        memcpy(ctx->h_xbuf, &x, sizeof x);
        memcpy(ctx->h_xbuf + L.sj, swap_j, (size_t)n_seg * sizeof(int));
        memcpy(ctx->h_xbuf + L.sk, swap_k, (size_t)n_seg * sizeof(int));
        memcpy(ctx->h_xbuf + L.su, swap_logu, (size_t)n_seg * sizeof(double));
        if (hipMemcpyAsync(ctx->d_xbuf, ctx->h_xbuf, L.state, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            (x.snap_w && hipMemsetAsync(ctx->d_xbuf + L.cold, 0, (size_t)n_seg * ctx->n_weights * sizeof(double), ctx->stream) != hipSuccess))
            rc_prepare = fail(ctx0, NPBNN_E_HIP, "chains_run_exchange: staging the exchange block of job %d failed", q);
    }
    if (comm && world > 1) {
        std::vector<double> ok_all((size_t)world, 0.0);
        const double ok_mine = rc_prepare == NPBNN_OK ? 1.0 : 0.0;
        int rc = npbnn_comm_allgather_f64(comm, &ok_mine, 1, ok_all.data());
        if (rc) {
            ctx0->err = npbnn_last_error(nullptr);
            drain_jobs(jobs, n_jobs);
            return rc;
        }
        int bad_rank = -1;
        for (int r = 0; r < world; ++r)
            if (ok_all[(size_t)r] != 1.0 && bad_rank < 0) bad_rank = r;
        if (bad_rank >= 0) {
            drain_jobs(jobs, n_jobs);
            if (rc_prepare) return rc_prepare;
            return fail(ctx0, NPBNN_E_COMM, "chains_run_exchange: rank %d could not prepare its chains; nothing was enqueued on any rank", bad_rank);
        }
    } else if (rc_prepare) {
        return rc_prepare;
    }
    HIP_TRY(ctx0, hipMemsetAsync(d_rec, 0, rec_bytes, ctx0->stream));
    if (n_jobs > 1) {      // the other chains' first record must not overtake the clearing of the shared block
        HIP_TRY(ctx0, hipEventRecord(ctx0->ev_x, ctx0->stream));
        for (int q = 1; q < n_jobs; ++q) HIP_TRY(jobs[q].ctx, hipStreamWaitEvent(jobs[q].ctx->stream, ctx0->ev_x, 0));
    }
    const int rec_per_rank = n_jobs * kRecDoubles;
    std::vector<hipStream_t> xs(n_jobs);        // stream the exchange kernels of a job run on
    for (int s = 0; s < n_seg; ++s) {
        for (int q = 0; q < n_jobs; ++q) {
            npbnn_ctx* ctx = jobs[q].ctx;
            int rc = chain_enqueue(ctx, B[q], npbnn_sched_passes_segment(seg_len, B[q].D, B[q].overlap, ctx->sched.its_per_pass, launch_slack));
            if (rc) {       // the peers have this interval's collective in flight: it must not pair with anything else we issue
                if (ctx != ctx0) ctx0->err = ctx->err;
                if (comm && world > 1) npbnn_comm_abort_(comm);
                (void)hipDeviceSynchronize();
                return rc;
            }
            // two-stream schedule (one chain on this GPU): the exchange kernels follow the interval's LAST launch on its stream -
            // by then the other stream's launches are through as well (the last step waited for them) - and the next interval's
            // first launch, which goes to the other stream, waits behind a gate for exchange_apply_kernel's hand-over.  No host
            // synchronisation, no stream events.
            xs[q] = B[q].sync ? ctx->stream_e[(B[q].launch - 1) & 1] : ctx->stream;
            hipLaunchKernelGGL(exchange_pack_kernel, dim3(1), dim3(64), 0, xs[q], (const ChainParams*)ctx->d_cparams,
                               (const ExchangeParams*)ctx->d_xbuf.get(), s);
            if (q > 0) {
                HIP_TRY(ctx, hipEventRecord(ctx->ev_x, ctx->stream));
                HIP_TRY(ctx0, hipStreamWaitEvent(ctx0->stream, ctx->ev_x, 0));
            }
        }
        if (comm) {
            int rc = npbnn_comm_allgather_inplace_stream_(comm, d_rec + (size_t)s * n_chains * kRecDoubles, rec_per_rank, xs[0]);
            if (rc) {
                ctx0->err = npbnn_last_error(nullptr);
                if (world > 1) npbnn_comm_abort_(comm);
                drain_jobs(jobs, n_jobs);
                return rc;
            }
        }
        if (n_jobs > 1) {
            HIP_TRY(ctx0, hipEventRecord(ctx0->ev_x, ctx0->stream));
            for (int q = 1; q < n_jobs; ++q) HIP_TRY(jobs[q].ctx, hipStreamWaitEvent(jobs[q].ctx->stream, ctx0->ev_x, 0));
        }
        for (int q = 0; q < n_jobs; ++q) {
            npbnn_ctx* ctx = jobs[q].ctx;
            hipLaunchKernelGGL(exchange_apply_kernel, dim3(1), dim3(1024), 0, xs[q], (const ChainParams*)ctx->d_cparams,
                               (const ExchangeParams*)ctx->d_xbuf.get(), s, B[q].launch, B[q].overlap ? 1 : 0);
            if (B[q].sync && s + 1 < n_seg)
                hipLaunchKernelGGL(sync_gate_exchanged_kernel, dim3(1), dim3(64), 0, ctx->stream_e[B[q].launch & 1], ctx->d_chain, s + 1);
        }
    }
    for (int q = 0; q < n_jobs; ++q) {
        int rc = chain_join(jobs[q].ctx, B[q]);
        if (rc) return rc;
    }
    for (int q = 0; q < n_jobs; ++q) {
        npbnn_ctx* ctx = jobs[q].ctx;
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_res, ctx->d_res, B[q].RL.total, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_xbuf + XL[q].state, ctx->d_xbuf + XL[q].state, XL[q].total - XL[q].state, hipMemcpyDeviceToHost, ctx->stream));
    }
    for (int q = 0; q < n_jobs; ++q) {
        if (comm && world > 1) {       // these streams wait for collectives: a peer that has gone must not hang this rank (wait_stream)
            int rc = npbnn_comm_wait_stream_(comm, jobs[q].ctx->stream, "chains_run_exchange");
            if (rc) {
                ctx0->err = npbnn_last_error(nullptr);
                (void)hipDeviceSynchronize();           // (the communicator was aborted: its kernels leave, the streams drain)
                return rc;
            }
        } else {
            HIP_TRY(jobs[q].ctx, hipStreamSynchronize(jobs[q].ctx->stream));
        }
    }
    int seg_done = -1;
    for (int q = 0; q < n_jobs; ++q) {
        const ChainDev* fin = reinterpret_cast<const ChainDev*>(jobs[q].ctx->h_res.get());
        if (fin->aborted) jobs[q].ctx->sync_failed = true;     // (the chain stopped at a valid state; the records show it as short)
        if (seg_done < 0) seg_done = fin->seg_idx;
        if (fin->seg_idx != seg_done) return fail(ctx0, NPBNN_E_STATE, "chains_run_exchange: chains disagree on the exchanges done (%d, %d)", seg_done, fin->seg_idx);
        if (fin->t < seg_done * seg_len || fin->t > K) return fail(ctx0, NPBNN_E_STATE, "chains_run_exchange: chain %d is at iteration %d after %d exchanges", q, fin->t, seg_done);
    }
    for (int q = 0; q < n_jobs; ++q) {
        const npbnn_chain_job& J = jobs[q];
        npbnn_ctx* ctx = J.ctx;
        const ChainDev* fin = reinterpret_cast<const ChainDev*>(ctx->h_res.get());
        int rc = chain_finish(ctx, B[q], J.cfg, J.W_inout, J.out_accepted, J.out_loglik_prop, J.out_logprior_prop, J.result, fin->t, true);
        if (rc) return rc;
        if (J.out_state) memcpy(J.out_state, ctx->h_xbuf + XL[q].state, (size_t)n_seg * NPBNN_XSTATE_DOUBLES * sizeof(double));
        if (J.out_cold_w) memcpy(J.out_cold_w, ctx->h_xbuf + XL[q].cold, (size_t)n_seg * ctx->n_weights * sizeof(double));
    }
    if (out_records) {     // device order (rank-major) -> chain order
        const double* h_rec = reinterpret_cast<const double*>(ctx0->h_xbuf + XL[0].rec);
        for (int s = 0; s < n_seg; ++s)
            for (int i = 0; i < n_chains; ++i) {
                const int slot = (i % world) * n_jobs + i / world;
                memcpy(out_records + ((size_t)s * n_chains + i) * kRecDoubles, h_rec + ((size_t)s * n_chains + slot) * kRecDoubles,
                       kRecDoubles * sizeof(double));
            }
    }
    *out_segments_done = seg_done;
    return NPBNN_OK;
}

int npbnn_set_row_shard(npbnn_ctx* ctx, npbnn_comm* comm, npbnn_gather_fn gather, void* user, int32_t rank, int32_t n_ranks, int64_t n_rows_total) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (n_ranks == 0) {
        ctx->shard_n = 0;
        ctx->shard_comm = nullptr;
        ctx->shard_gather = nullptr;
        return NPBNN_OK;
    }
    if (n_ranks < 0 || n_ranks > 4096 || rank < 0 || rank >= n_ranks || n_rows_total < 1)
        return fail(ctx, NPBNN_E_ARG, "set_row_shard: rank %d of %d, %lld rows in all", rank, n_ranks, (long long)n_rows_total);
    if (n_ranks > 1 && !comm && !gather) return fail(ctx, NPBNN_E_ARG, "set_row_shard: %d ranks need a communicator or a gather callback", n_ranks);
    if (comm) {
        int device = -1, crank = -1, cworld = 0;
        if (npbnn_comm_info_(comm, &device, &crank, &cworld) != 0) return fail(ctx, NPBNN_E_COMM, "set_row_shard: the communicator is not usable");
        if (crank != rank || cworld != n_ranks || device != ctx->device)
            return fail(ctx, NPBNN_E_ARG, "set_row_shard: communicator is rank %d of %d on device %d, asked for rank %d of %d on device %d", crank, cworld,
                        device, rank, n_ranks, ctx->device);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t rec = (size_t)kMaxCand * kPartialStride;
    ctx->d_shard_recv.reset();
    ctx->d_shard_part.reset();
    ctx->h_shard.reset();
    int rc = ctx->d_shard_recv.reserve(ctx, rec * n_ranks);
    if (!rc) rc = ctx->d_shard_part.reserve(ctx, rec * n_ranks);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemset(ctx->d_shard_recv, 0, rec * n_ranks * sizeof(double)));       // (values not in use stay zero)
    HIP_TRY(ctx, hipMemset(ctx->d_shard_part, 0, rec * n_ranks * sizeof(double)));
    if ((rc = ctx->h_shard.reserve(ctx, rec * (n_ranks + 1)))) return rc;
    memset(ctx->h_shard, 0, rec * (n_ranks + 1) * sizeof(double));
    ctx->shard_n = n_ranks;
    ctx->shard_rank = rank;
    ctx->shard_rows_total = n_rows_total;
    ctx->shard_comm = comm;
    ctx->shard_gather = comm ? nullptr : gather;
    ctx->shard_user = user;
    ctx->sched.its_per_pass = 0.0;    // (the ranks must agree on the number of launches: start from the same history)
    ctx->sched.accept_rate = -1.0;
    return NPBNN_OK;
}

// diagnostics (not part of the ABI): in the next batch of this context that runs on the two-stream schedule, the step workgroup of
// launch `launch` never reports back - every wait behind it must time out cleanly (tests of that path)
int npbnn_debug_sync_skip_(npbnn_ctx* ctx, int launch) {
    if (!ctx) return NPBNN_E_ARG;
    ctx->debug_sync_skip = launch;
    return NPBNN_OK;
}

// diagnostics (not part of the ABI): the weight image as it stands in device memory
int npbnn_debug_image_(npbnn_ctx* ctx, float* out, int n) {
    if (!ctx || !out) return NPBNN_E_ARG;
    if (n > ctx->net.image_floats) n = ctx->net.image_floats;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, ctx->d_image, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return n;
}

}  // extern "C"
