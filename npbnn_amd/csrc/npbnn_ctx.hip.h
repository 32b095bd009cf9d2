// Host-side state of a chain context and the helpers the translation units of the C ABI share
// (npbnn_capi.hip: contexts, data, architecture, evaluation, prediction, timing hooks; npbnn_chain_api.hip: device-resident
// chains, group passes, exchange runs; npbnn_general.hip: the general device chain).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "npbnn_buf.hip.h"
#include "npbnn_hip.h"
#include "npbnn_kernels.hip.h"
#include "npbnn_sched_plan.h"

using namespace npbnn;
using npbnn_api::DevBuf;
using npbnn_api::PinnedBuf;

// the evaluation-kernel instantiations live in npbnn_eval_inst_*.hip (compiled in parallel)
namespace npbnn {
eval_fn_t pick_eval_mti8_cat(int mt0, int f16);
eval_fn_t pick_eval_mti8_gauss(int mt0, int f16);
eval_fn_t pick_eval_mti8_gen(int mt0, int f16);
eval_fn_t pick_eval_d1_cat(int mt0, int f16);
eval_fn_t pick_eval_d1_gauss(int mt0, int f16);
eval_fn_t pick_eval_d1_gen(int mt0, int f16);
eval_fn_t pick_eval_d2_cat(int mt0, int f16);
eval_fn_t pick_eval_d2_gauss(int mt0, int f16);
eval_fn_t pick_eval_d3_cat(int mt0, int f16);
eval_fn_t pick_eval_d3_gauss(int mt0, int f16);
// the fast builds (eval_kernel<..., FAST = true>): nullptr where there is none (more than kFastMaxMT0 tiles in layer 0)
eval_fn_t pick_eval_d1_cat_fast(int mt0, int f16);
eval_fn_t pick_eval_d1_cat_plain(int mt0, int f16);      // (plain evaluations: no chain pass)
eval_fn_t pick_eval_d1_cat_spec(int mt0, int f16);       // (NPBNN_SCHED_PERSIST_SERIAL: with the outcome-speculative step; nullptr where none)
eval_fn_t pick_eval_d1_gauss_spec(int mt0, int f16);
eval_fn_t pick_eval_d3_cat_spec(int mt0, int f16);
eval_fn_t pick_eval_d3_gauss_spec(int mt0, int f16);
eval_fn_t pick_eval_d1_gauss_plain(int mt0, int f16);
eval_fn_t pick_eval_d1_gauss_fast(int mt0, int f16);
eval_fn_t pick_eval_d2_cat_fast(int mt0, int f16);
eval_fn_t pick_eval_d2_gauss_fast(int mt0, int f16);
eval_fn_t pick_eval_d3_cat_fast(int mt0, int f16);
eval_fn_t pick_eval_d3_gauss_fast(int mt0, int f16);
}

// lk: likelihood class of the build (npbnn::lik_class); the float64 row-wise class has single-candidate builds only
static inline eval_fn_t npbnn_pick_eval_kernel(int mt0, int mti, int f16, int n_cand, int lk, bool fast = false, bool blocked = false, bool plain = false) {
    using namespace npbnn;
    if (fast) {
        const bool g = lk == kLikGauss;
        if (blocked) f16 = 2;                 // (npbnn_resident_fast_ok: block structure only on the fp16-split path)
        if (n_cand <= 1 && plain) return g ? pick_eval_d1_gauss_plain(mt0, f16) : pick_eval_d1_cat_plain(mt0, f16);
        if (n_cand <= 1) return g ? pick_eval_d1_gauss_fast(mt0, f16) : pick_eval_d1_cat_fast(mt0, f16);
        if (n_cand == 2) return g ? pick_eval_d2_gauss_fast(mt0, f16) : pick_eval_d2_cat_fast(mt0, f16);
        return g ? pick_eval_d3_gauss_fast(mt0, f16) : pick_eval_d3_cat_fast(mt0, f16);
    }
    if (mti != 1) return lk == kLikGen ? pick_eval_mti8_gen(mt0, f16) : lk == kLikGauss ? pick_eval_mti8_gauss(mt0, f16) : pick_eval_mti8_cat(mt0, f16);
    if (lk == kLikGen) return pick_eval_d1_gen(mt0, f16);
    const bool g = lk == kLikGauss;
    if (n_cand <= 1) return g ? pick_eval_d1_gauss(mt0, f16) : pick_eval_d1_cat(mt0, f16);
    if (n_cand == 2) return g ? pick_eval_d2_gauss(mt0, f16) : pick_eval_d2_cat(mt0, f16);
    return g ? pick_eval_d3_gauss(mt0, f16) : pick_eval_d3_cat(mt0, f16);
}

namespace npbnn_api {

// One feature matrix as the device holds it: the float32 table and its fp16-split copies, built lazily on the device.
struct FeatureTable {
    DevBuf<float> X;
    int64_t n_rows = 0;
    int n_tiles = 0;
    int F = 0, Fp = 0;
    DevBuf<float> X16;         // fp16-split copy, row stride Fp16 floats
    int Fp16 = 0;
    int f16_state = 0;         // 0 not built, 1 usable, -1 not representable (inf/NaN or outside the fp16 range), -2 representable but
                               // too coarse for some column: its entries span too many powers of two for a pair of fp16 numbers,
                               // -3 a table under another table's scales whose scaled entries are large enough for a weight's
                               // absolute floor to show (ensure_x16, kF16FloorSum)
    int f16_worst_col = -1;    // column with the largest (max entry error / mean |entry|) of the fp16 pair, and that ratio
    double f16_worst_ratio = 0.0;
    double f16_floor_sum = 0.0;    // sum over columns of what the scaled column maximum exceeds 1 by (a table that did not give the scales: ensure_x16)
    DevBuf<float> X16w;        // the fp16-split copy in the weight-streamed path's piece order (split_x_tiled_kernel), built when a
                               // network on that path first asks for it
};

// The training and test matrices with the fp16-split path's scales: what npbnn_share_data shares.  Every context holds one through a
// shared_ptr: the context that uploaded it and those that took it from another context alike, all on one device.  It goes, with that
// device current, when its last holder lets go.
struct FeatureStore {
    explicit FeatureStore(int device_id) : device(device_id) {}
    ~FeatureStore() { (void)hipSetDevice(device); }      // (the buffers are freed after this body)
    FeatureTable table[2];
    DevBuf<float> xscale;          // per-feature power-of-two scales of the fp16-split path (from the training matrix)
    DevBuf<float> wscale;
    int scale_F = 0;
    int f16_shifted_cols = 0;      // columns whose scale was moved up (heavy tails: ensure_scales) and the largest such move (powers of two)
    int f16_max_shift = 0;
    const int device;
};

// A table as one context sees it: the matrices in the store it holds, and what it alone keeps for them.
struct Dataset {
    FeatureTable* m = nullptr;    // store->table[which] of the context (hold_store)
    DevBuf<int> labels;
    DevBuf<float> targets;
    DevBuf<float> inst_w;
    int k = 0;
    std::vector<int> perm_cols;   // npbnn_permute_columns: the columns of X (and of its split copies) that hold permuted values now ...
    DevBuf<float> perm_saved;     // ... and those columns as npbnn_set_data left them, [perm_cols.size()][n_rows]
};

}  // namespace npbnn_api
using npbnn_api::Dataset;
using npbnn_api::FeatureStore;
using npbnn_api::FeatureTable;

// The streams and events of a context.  A base of npbnn_ctx: they are destroyed after every buffer the context owns.
struct npbnn_ctx_streams {
    hipStream_t stream = nullptr;
    hipStream_t stream_e[2] = {nullptr, nullptr};   // flag-ordered overlapped chain schedule: the launches alternate between these two
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipEvent_t ev_x = nullptr;
    npbnn_ctx_streams() = default;
    npbnn_ctx_streams(const npbnn_ctx_streams&) = delete;
    npbnn_ctx_streams& operator=(const npbnn_ctx_streams&) = delete;
    ~npbnn_ctx_streams() {
        for (hipEvent_t e : {ev_x, ev[0], ev[1]})
            if (e) (void)hipEventDestroy(e);
        for (hipStream_t s : {stream_e[0], stream_e[1], stream})
            if (s) (void)hipStreamDestroy(s);
    }
};

struct npbnn_ctx : npbnn_ctx_streams {
    int device = 0;
    int n_cu = 256;
    size_t lds_limit = 160 * 1024;
    std::string err;
    // The feature matrices, possibly shared with other contexts (npbnn_share_data): never null.  store_taken: this context took the
    // store from another one - it builds no row-major split copy in it and moves no column of it, whoever else still holds it.
    std::shared_ptr<FeatureStore> store;
    bool store_taken = false;
    Dataset ds[2];
    DevBuf<double> d_classw;
    int n_classw = 0;
    bool arch_set = false;
    npbnn_arch arch{};
    NetMeta net{};
    npbnn_resident_layout rlay{};  // the resident image's layout behind `net` (npbnn_resident_plan.h: what the launch rule reads); unused on the weight-streamed path
    int n_weights = 0;
    int mt0_template = 1;
    int l0_option = 0;             // NPBNN_L0_AUTO / _F32 / _F16
    int fast_option = 1;           // NPBNN_OPT_FAST_TAILS
    int slopes_option = 0;         // NPBNN_OPT_TRAINABLE_SLOPES: the image holds a slot per hidden layer for the activation slope
    DevBuf<SlopeState> d_slopes;    // trainable slopes of the device chain (npbnn_chain_cfg.slope_idx ...)
    DevBuf<int> d_sidx;             // pre-drawn slope entries ...
    DevBuf<double> d_sdelta;        // ... and steps
    bool batch_slopes = false;      // the batch in flight carries slopes (chain_finish reads them back)
    int persist_option = 1;        // NPBNN_OPT_PERSISTENT
    const void* attr_fn = nullptr; // kernel whose dynamic-LDS limit was raised last, and to what
    size_t attr_lds = 0;
    // layer-0 block structure (npbnn_set_layer_mask): which (16-node tile, 16-feature group) blocks of the mask hold a nonzero;
    // empty = dense
    std::vector<unsigned char> l0_blocks;      // [mt][ceil(in_dim / 16)]
    DevBuf<int> d_overflow;         // [1 + kSetFlags]: the flag word of a launch, then one per weight set of a replay group
    // parameter blocks of the kernels: device copies (kernels take a pointer) + pinned host staging, both laid out
    // EvalParams | FinalizeParams | ChainParams
    DevBuf<char> d_params;
    EvalParams* d_eparams = nullptr;       // (view into d_params)
    FinalizeParams* d_fparams = nullptr;   // (view into d_params)
    ChainParams* d_cparams = nullptr;      // (view into d_params)
    PinnedBuf<char> h_params;
    DevBuf<float> d_w2scale;
    // device work buffers
    DevBuf<double> d_wraw;         // packed float64 weights
    DevBuf<double> d_colov;        // column override (in_dim doubles)
    DevBuf<float> d_image;         // float32 fragment image
    DevBuf<int> d_w2img;           // packed-weight index -> image float index
    DevBuf<double> d_partials;
    DevBuf<unsigned> d_conf;       // [classes][classes], classes >= kResidentMaxWidth (ensure_conf)
    DevBuf<npbnn_eval_out> d_out;
    DevBuf<float> d_y;
    // pinned host staging
    PinnedBuf<double> h_w;
    PinnedBuf<npbnn_eval_out> h_out;
    PinnedBuf<unsigned> h_conf;
    // device-resident chain.  d_res / h_res: one block [ChainDev | overflow flag | W_cur | accepted | logLik' | logPrior'] so that a
    // single copy brings the whole outcome of a batch to the (pinned) host side; d_chain ... d_lpp point into it.  res_k, res_nw:
    // the iterations and weights it is laid out for (0: lay it out again)
    DevBuf<char> d_res;
    PinnedBuf<char> h_res;
    size_t res_k = 0, res_nw = 0;
    int* d_chain_ovf = nullptr;    // (view into d_res)
    npbnn_sched_hist sched = NPBNN_SCHED_HIST_INIT;   // what the chain's batches ran on and cost: the history their schedule goes by (npbnn_sched_plan.h)
    double* d_wcur = nullptr;      // (view into d_res)
    DevBuf<double> d_pv;           // [2][kMaxCand][M] proposed values of the candidates in flight
    // NPBNN_SCHED_PERSIST_SERIAL (spec_round): outcome-speculative preparation
    DevBuf<SpecState> d_spec;
    DevBuf<double> d_spec_pv;      // [3][kSpecOutcomes][kMaxCand][M]
    DevBuf<unsigned> d_spec_touch; // [kMaxCand][n_weights][4] touch tables: pass tag (cleared before it could repeat), -, value
    DevBuf<unsigned long long> d_spec_part;   // [2][kMaxCand][kPartialStride][256][2] the workgroups' sums of a pass as tagged word pairs (npbnn_chain.hip.h, SpecPart)
    unsigned spec_gen = 0;         // pass tags handed out so far
    // rows split over the ranks of a communicator (npbnn_set_row_shard): the records of partial sums are gathered before every step
    int shard_n = 0, shard_rank = 0;
    long long shard_rows_total = 0;
    npbnn_comm* shard_comm = nullptr;
    npbnn_gather_fn shard_gather = nullptr;
    void* shard_user = nullptr;
    DevBuf<double> d_shard_recv;   // [shard_n][kMaxCand][kPartialStride]: this rank's record at its own place, the peers' after the gather
    DevBuf<double> d_shard_part;   // [kMaxCand][kPartialStride][shard_n]: the same in the layout the step kernel sums
    PinnedBuf<double> h_shard;     // as d_shard_recv, + this rank's record (host-staged gather)
    DevBuf<double> d_mask;
    ChainDev* d_chain = nullptr;   // (view into d_res)
    DevBuf<int> d_idx;             // the batch's weight indices, then (d_delta) its deviates
    double* d_delta = nullptr;     // (view into d_idx)
    DevBuf<int> d_pos;
    DevBuf<float> d_pscale;
    int* d_cnt = nullptr;          // (view into d_res)
    double* d_logu = nullptr;      // (view into d_res)
    unsigned char* d_acc = nullptr;   // (view into d_res)
    double* d_llp = nullptr;       // (view into d_res)
    double* d_lpp = nullptr;       // (view into d_res)
    DevBuf<EvalParams> d_gparams;     // parameter block of a group pass led by this context (npbnn_chains_run_batched)
    PinnedBuf<EvalParams> h_gparams;  // its page-locked staging twin
    DevBuf<double> d_pscale_w;     // [n_weights] per-weight prior scales of the current batch (npbnn_chain_cfg.prior_scale_w)
    DevBuf<double> d_smult;        // [K][NPBNN_MAX_TARGETS] sigma multipliers, [K] Hastings terms (regression with an estimated error parameter)
    DevBuf<double> d_hast;
    // exchange run (npbnn_chains_run_exchange): [ExchangeParams | swap_j | swap_k | swap_logu || state | records | cold weights]
    DevBuf<char> d_xbuf;
    PinnedBuf<char> h_xbuf;
    bool sync_failed = false;      // a wait timed out once: the schedule stays off for this context
    int debug_sync_skip = -1;      // npbnn_debug_sync_skip_ (diagnostics, not part of the ABI)
    int fi_ns[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // NPBNN_FI_TIMING: device time of the last npbnn_permute_columns, of the passes / accumulation / final
                                   // kernel of the last npbnn_predict_sets_summary, and of the last npbnn_predict_sets_support's,
                                   // npbnn_predict_sets_lppd's, npbnn_predict_sets_uncertainty's and npbnn_predict_sets_convergence's final kernels (NPBNN_INFO_PERMUTE_NS ...;
                                   // every entry that goes through replay_sets, npbnn_sets.hip.h, leaves its passes and sinks in [1], [2])
    int calibration_ns = 0;        // NPBNN_FI_TIMING: the last npbnn_predict_sets_calibration's final kernel (NPBNN_INFO_CALIBRATION_FINAL_NS; fi_ns is full)
    int loo_ns = 0;                // NPBNN_FI_TIMING: the last npbnn_predict_sets_loo's psis_kernel (NPBNN_INFO_LOO_FINAL_NS)
    std::shared_ptr<void> grad_work; // npbnn_loglik_grad's device buffers, kept between calls (GradWork, npbnn_grad.hip); freed when a table
                                     // is replaced (forget_rows) and with the context
    int grad_ns[2] = {0, 0};       // NPBNN_FI_TIMING: the last npbnn_loglik_grad's phase 1 and phase 2 (NPBNN_INFO_GRAD_ROWS_NS, NPBNN_INFO_GRAD_FOLD_NS)
    int replay_passes = 0, replay_max_group = 0;  // the last replay_sets: passes over X (float32 repeats included), most sets in one (NPBNN_INFO_REPLAY_*)
    int pdp_route = 0;             // route of the last npbnn_predict_pdp: 1 grid-batched kernel, 2 per grid point (NPBNN_INFO_PDP_ROUTE)
    int ale_route = 0;             // route of the last npbnn_predict_ale: 1 both edges from one read of X, 2 per edge; 0 none, or refused (NPBNN_INFO_ALE_ROUTE)
    int saliency_route = 0;        // route of the last npbnn_predict_saliency: 1 phase 1 in registers, 2 the plain kernel; 0 none, or refused (NPBNN_INFO_SALIENCY_ROUTE)
    int saliency_ns = 0;           // NPBNN_FI_TIMING: the last npbnn_predict_saliency's fold and reduce kernels (NPBNN_INFO_SALIENCY_FOLD_NS)
    int shapley_route = 0;         // route of the last npbnn_predict_shapley: 1 the walks in registers, 2 the plain kernels; 0 none, or refused (NPBNN_INFO_SHAPLEY_ROUTE)
    int shapley_ns = 0;            // NPBNN_FI_TIMING: the last npbnn_predict_shapley's walk kernels (NPBNN_INFO_SHAPLEY_WALK_NS)
    // weight-streamed path (npbnn_wide.hip): the network does not fit a compute unit's LDS (or NPBNN_OPT_WIDE asks for it)
    bool wide = false;
    int wide_option = 0;           // NPBNN_OPT_WIDE: 0 when the resident path cannot hold the network, 1 always
    WideMeta wmeta{};
    // Sizes: d_wide_cand and d_wide_cs by the network alone (wide_build); d_prep_terms by the widest proposal (chain_prepare);
    // the fp16-split copy FeatureTable::X16w by its own table (built by wide_plan, freed with the table); d_wide_act by the largest table a plan
    // was made for (wide_plan: rows x widest layer, and npbnn_wide_slice_room for the K-slices), which wide_forward checks every launch against.
    DevBuf<float> d_wide_cand;     // candidate image of a device chain (the committed image with the pending proposal patched in)
    DevBuf<float> d_wide_act[3];   // hidden activations [rows][16 * tiles], ping-pong between layers; [2]: the K-slices' sums
    DevBuf<double> d_prep_terms;   // [kMaxCand][M] prior terms of the pending candidates' entries (ChainParams::prep_terms)
    DevBuf<WideCandState> d_wide_cs;   // what the candidate image's last patch covered (wide proposals: wide_cand_sync)
    std::set<const void*> wide_lds_raised;   // kernels of the weight-streamed path whose dynamic-LDS limit was raised (wide_forward)
};

static_assert(sizeof(EvalParams) % 8 == 0 && sizeof(FinalizeParams) % 8 == 0, "parameter blocks are laid out back to back");

namespace npbnn_api {

constexpr int kWideMaxCand = 3;                // weight sets a fused pass of the weight-streamed path carries at most
static_assert(kWideMaxCand <= kMaxCand, "d_y, the staged weights and the per-set flag words are sized for kMaxCand sets per pass");
constexpr int kSetFlags = kMaxCand;            // per-set flag words behind ctx->d_overflow[0] (launch_pack_group)
constexpr int kMinResidentWaves = 4;           // fewer waves than this beside the weight image: the network runs on the weight-streamed path
constexpr int kWideStepPatchMax = 2048;      // widest proposal whose candidate image the step workgroup keeps by itself (weight-streamed path)
constexpr size_t kChainMinCapacity = 2048;    // iterations the per-batch chain buffers are sized for at least (allocation is slow)

int fail(npbnn_ctx* ctx, int code, const char* fmt, ...);

#define HIP_TRY(ctx, call)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(ctx, NPBNN_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                    \
    } while (0)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

struct LaunchPlan {
    eval_fn_t fn;
    eval_fn_t fn_spec;       // the same launch's build with the outcome-speculative step (NPBNN_SCHED_PERSIST_SERIAL), or nullptr
    int n_cand;
    int grid, wpb;
    size_t lds;
    int n_waves;
    bool fast;
    bool wide = false;       // weight-streamed path: no single kernel - wide_forward launches the layers' products and the likelihood
};

// ---- weight-streamed path (npbnn_wide.hip) ----
// rc, lay: what npbnn_resident_layout_of said of the network on this layer-0 layout
bool wide_needed(const npbnn_ctx* ctx, const npbnn_arch* a, int rc, const npbnn_resident_layout& lay);
int wide_build(npbnn_ctx* ctx, bool f16);
void wide_free(npbnn_ctx* ctx);
// predict: a predicting launch - its weight sets are independent (stored samples that share their slopes), not a chain's candidates
int wide_plan(npbnn_ctx* ctx, int which, LaunchPlan* lp, int want_cand = 1, bool predict = false);
// n_sets > 1: the sets d_w + j * n_weights into the images image + j * wmeta.image_floats, what set j reports into flags[j]
void wide_pack(npbnn_ctx* ctx, const double* d_w, const double* d_col_override, float* image, int* flags, int n_sets = 1);
// the forward pass + likelihood of the weights in `image` on the ctx stream; the launch's EvalParams must be in ctx->d_eparams.
// chain_pass: a pass of a device chain (the kernels leave at once when the chain's batch is through; candidate slopes from the chain)
// only_layer0: stop behind the first layer's product (timing hook); info: that product's geometry, or nullptr
int wide_forward(npbnn_ctx* ctx, int which, const float* image, bool chain_pass, bool only_layer0 = false, int* info = nullptr, int n_cand = 1);
int wide_cand_begin(npbnn_ctx* ctx);     // start of a chain batch: candidate image = committed image, nothing patched
void wide_cand_sync(npbnn_ctx* ctx, int M, int n_cand, bool make_them);   // before a pass of a chain with wide proposals: candidate image = committed image + the pending proposal
int ensure_conf(npbnn_ctx* ctx, int n_classes);
// one evaluation launch of a plan on the ctx stream (resident: the plan's kernel; weight-streamed: wide_forward on the committed image,
// or on the lp.n_cand images of pass_image when the plan carries several sets)
int launch_plain_eval(npbnn_ctx* ctx, const LaunchPlan& lp, int which);
// The weight image of set j of a pass of independent weight sets (EvalParams::weight_sets): resident path d_image + j * net.image_floats;
// weight-streamed path the candidate images, or the committed image when the plan carries one set.
float* pass_image(npbnn_ctx* ctx, const LaunchPlan& lp, int j);
// The g sets d_w + j * n_weights (device, float64) packed into the images of a pass (on the weight-streamed path lp.n_cand == g).  Flags:
// resident path all sets into ctx->d_overflow[0]; weight-streamed path set j into ctx->d_overflow[1 + j] (kSetFlags words: a set out of
// the fp16 range repeats alone).  The caller zeroes them.
void launch_pack_group(npbnn_ctx* ctx, const LaunchPlan& lp, const double* d_w, const double* d_col_override, int g);

WaveLayout layout_for(const npbnn_ctx* ctx, const Dataset& d, bool predict_only = false);
int ensure_x16(npbnn_ctx* ctx, int which, int* usable);
int rebuild_net(npbnn_ctx* ctx, bool f16);
// lik_only: the caller wants the likelihood terms and nothing else from the launch (no statistics, no predictions)
// plain: the launch is a plain evaluation - no pass descriptor, no chain (the builds without that code)
int plan_launch(npbnn_ctx* ctx, int which, LaunchPlan* lp, int force_f32 = 0, int want_cand = 1, bool predict_only = false, bool lik_only = false,
                bool plain = false);
int ensure_work_buffers(npbnn_ctx* ctx, int n_waves);
int stage_weights(npbnn_ctx* ctx, const double* W, const double* act_prm, const double* col_override);
int push_eval_params(npbnn_ctx* ctx, const EvalParams& p);
int push_finalize_params(npbnn_ctx* ctx, const FinalizeParams& f);
int push_chain_params(npbnn_ctx* ctx, const ChainParams& c);
EvalParams make_params(npbnn_ctx* ctx, const Dataset& d);
void report_eval_stamps(const DevBuf<unsigned long long>& stamps, int grid, int wpb, int first_wg);
void report_step_stamps(const DevBuf<unsigned long long>& stamps);
int check_dataset_for_lik(npbnn_ctx* ctx, const Dataset& d, int lik);
double wall_us();
// launches of kernels that live in npbnn_capi.hip, for the other translation units: the weight image of device-resident float64
// weights (col_override may be nullptr) into `image`, and the reduction of the partial sums of the last evaluation
void launch_pack_weights(npbnn_ctx* ctx, const double* d_w, const double* d_col_override, float* image, int* flags);
void launch_finalize(npbnn_ctx* ctx);

}  // namespace npbnn_api
using namespace npbnn_api;
