/*
 * npbnn_hip.h — C ABI of the MI355X (gfx950) backend for npBNN's MCMC hot path.
 *
 * The reference (dsilvestro/npBNN, np_bnn 0.1.23) is pure Python and has no
 * FFI of its own; its boundary for this path is the Python call surface.  Each
 * entry point below names the reference function(s) it replaces (file:line
 * relative to the upstream repository root).  INTEGRATION.md shows the ctypes
 * stub a maintainer would add on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success or a negative NPBNN_E_* code; the
 *     message is available from npbnn_last_error(ctx) (ctx may be NULL for
 *     errors raised before a context exists);
 *   - the caller owns every host buffer and may free it as soon as the call
 *     returns; the library owns all device memory for the lifetime of the ctx;
 *   - one ctx = one chain = one HIP stream on one device; a ctx is not
 *     thread-safe, distinct ctxs are independent;
 *   - host matrices are dense row-major; weights are float64 as in the
 *     reference and are converted to float32 on the device; the per-row
 *     arithmetic is float32, every cross-row sum is float64 with a fixed
 *     reduction order (results are run-to-run identical).
 */
#ifndef NPBNN_HIP_H
#define NPBNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NPBNN_ABI_VERSION 1
#define NPBNN_MAX_LAYERS 8      /* weight matrices per network                    */
#define NPBNN_MAX_WIDTH 4096    /* max nodes of any hidden/output layer (layers of more than 128 nodes, and networks whose
                                   weights do not fit a compute unit's LDS, run on the weight-streamed path) */
#define NPBNN_MAX_TARGETS 16    /* max target columns for the Gaussian/count liks */
#define NPBNN_XSTATE_DOUBLES (4 + NPBNN_MAX_TARGETS)   /* doubles per exchange in npbnn_chain_job.out_state */

enum {
    NPBNN_OK = 0,
    NPBNN_E_ARG = -1,       /* bad argument / unsupported shape      */
    NPBNN_E_STATE = -2,     /* call order (e.g. eval before set_arch) */
    NPBNN_E_HIP = -3,       /* a HIP runtime call failed              */
    NPBNN_E_NOMEM = -4,
    NPBNN_E_COMM = -5,      /* RCCL failure                           */
    NPBNN_E_RANGE = -6,     /* value outside the fp16-split range      */
    NPBNN_E_SYNC = -7,      /* a device-side wait of NPBNN_SCHED_OVERLAP2 timed out */
    NPBNN_E_INTERNAL = -8   /* the library's own plan and its buffers disagree (a bug: the launch is refused) */
};

/* activation kinds — ActFun.activate selection, np_bnn/BNN_lib.py:50-87 */
enum { NPBNN_ACT_RELU = 0, NPBNN_ACT_LEAKY = 1, NPBNN_ACT_SWISH = 2, NPBNN_ACT_TANH = 3 };

/* output functions — np_bnn/BNN_lib.py:166-182 */
enum {
    NPBNN_OUT_SOFTMAX = 0,        /* SoftMax              :166-168 */
    NPBNN_OUT_IDENTITY = 1,       /* RegressTransform     :174-175 */
    NPBNN_OUT_SOFTPLUS_HALF = 2   /* RegressTransformError:177-182 */
};

/* likelihood kinds — np_bnn/BNN_lib.py:100-143 and np_bnn/BNN_lik.py:5-66 */
enum {
    NPBNN_LIK_CATEGORICAL = 0,     /* calc_likelihood                  BNN_lib.py:100-121 */
    NPBNN_LIK_GAUSS = 1,           /* calc_likelihood_regression       BNN_lib.py:123-131, sigma given or
                                      empirical (np.std of residuals, BNN_env.py:475-476) */
    NPBNN_LIK_GAUSS_PRED_SIGMA = 2,/* calc_likelihood_regression_error BNN_lib.py:134-143 */
    NPBNN_LIK_POISSON = 3,         /* poi_likelihood                   BNN_lik.py:5-14    */
    NPBNN_LIK_NEGBIN = 4,          /* negbin_likelihood                BNN_lik.py:16-30   */
    NPBNN_LIK_NEGBIN2D = 5,        /* negbin_likelihood2d              BNN_lik.py:33-49   */
    NPBNN_LIK_NEGBIN_BASE10 = 6,   /* negbin_likelihood_base10         BNN_lik.py:55-66   */
    NPBNN_LIK_NONE = 7             /* forward only                                         */
};

/* prior kinds — npBNN.__init__/calc_prior, np_bnn/BNN_env.py:135-150,180-194 */
enum { NPBNN_PRIOR_UNIFORM = 0, NPBNN_PRIOR_NORMAL = 1, NPBNN_PRIOR_CAUCHY = 2, NPBNN_PRIOR_LAPLACE = 3 };

enum { NPBNN_TRAIN = 0, NPBNN_TEST = 1 };

typedef struct npbnn_ctx npbnn_ctx;

/* Network description.  Layer l has a weight matrix out_dim[l] x (in_l + has_bias[l])
 * with the bias in COLUMN 0 (init_weight_prm, np_bnn/BNN_mcmc.py:9-25;
 * MatrixMultiplicationD, np_bnn/BNN_lib.py:154-162); in_0 = in_dim, in_l = out_dim[l-1].
 * Packed weights = the layer matrices concatenated, each row-major. */
typedef struct {
    int32_t n_layers;
    int32_t in_dim;
    int32_t out_dim[NPBNN_MAX_LAYERS];
    int32_t has_bias[NPBNN_MAX_LAYERS];
    int32_t act_kind;       /* hidden layers; the last layer has no activation (BNN_lib.py:253) */
    int32_t out_kind;
    int32_t lik_kind;
    int32_t n_targets;      /* k target columns (Gaussian / count likelihoods), else 0 */
    int32_t final_act;      /* 1: the activation also follows the last layer (RunHiddenLayer on its own, BNN_lib.py:190-191) */
} npbnn_arch;

/* Result of one evaluation.  sum_r / sum_r2 are the per-column residual moments
 * (targets - prediction) from which sigma, the Gaussian log-likelihood and the MSE
 * statistics (CalcAccuracyRegression / CalcLabelAccuracyRegression, BNN_lib.py:195-201)
 * all derive. */
typedef struct {
    double loglik;                       /* includes lik_temp */
    double sigma[NPBNN_MAX_TARGETS];     /* sigma actually used (given or empirical) */
    double sum_r[NPBNN_MAX_TARGETS];
    double sum_r2[NPBNN_MAX_TARGETS];
    int64_t n_rows;
} npbnn_eval_out;

/* ---- lifecycle ------------------------------------------------------------------ */
int npbnn_abi_version(void);
int npbnn_device_count(int* out);
int npbnn_create(int device_id, npbnn_ctx** out);
void npbnn_destroy(npbnn_ctx* ctx);
const char* npbnn_last_error(const npbnn_ctx* ctx);

/* ---- resident data: replaces npBNN._data/_labels/_test_data/_test_labels living in host
 * numpy arrays and being copied every iteration (tmp = bnn_obj._data + 0, BNN_env.py:388) ---- */
int npbnn_set_data_f64(npbnn_ctx* ctx, const double* X, int64_t n_rows, int32_t n_features, int which);
int npbnn_set_data_f32(npbnn_ctx* ctx, const float* X, int64_t n_rows, int32_t n_features, int which);
/* The chains of one run (MC3 replicates the model per chain, np_bnn/BNN_mc3.py:55-58) hold the same feature matrices: `ctx` uses
 * the device copies `owner` holds - training and test matrices, their fp16-split copies and scales - instead of uploading its
 * own (labels / targets / row weights stay per context: set them afterwards, then npbnn_set_arch).  Same device only.  The
 * matrices live until the last context that uses them is destroyed or given data of its own: they outlive the owner, whose
 * context npbnn_destroy frees at once.  npbnn_set_data on an owner while others use its matrices is an error. */
int npbnn_share_data(npbnn_ctx* ctx, npbnn_ctx* owner);

int npbnn_set_labels_i64(npbnn_ctx* ctx, const int64_t* y, int64_t n_rows, int which);
int npbnn_set_targets_f64(npbnn_ctx* ctx, const double* Y, int64_t n_rows, int32_t k, int which);
/* instance_weight / class_weight of calc_likelihood (BNN_lib.py:100-121); NULL clears. Train set only. */
int npbnn_set_row_weights(npbnn_ctx* ctx, const double* instance_w, int64_t n_rows,
                          const double* class_w, int32_t n_classes);
int npbnn_set_arch(npbnn_ctx* ctx, const npbnn_arch* arch);
/* Block structure of the first layer: `mask_packed` is the 0/1 mask of the network in packed-weight order (create_mask,
 * np_bnn/BNN_lib.py:16-47; npBNN.apply_mask, np_bnn/BNN_env.py:259-267; re-applied to every proposal, :461-462), or NULL for a
 * dense first layer.  Only its layer-0 part is looked at: blocks of 16 nodes x 16 features (32 on the fp16-split path) in which
 * the mask is all zero get no storage in the device's weight image and no matrix-core work - block_bnns.py's layouts (groups of
 * consecutive features wired to a few nodes each) shrink to their diagonal.  The caller promises that every weight it passes
 * from now on is zero where the mask is (the sampler's proposals are: BNN_env.py:462); a weight that is not fails the call that
 * brought it with NPBNN_E_ARG.  Results are the dense ones bit for bit.  After npbnn_set_arch; cleared by the next one. */
int npbnn_set_layer_mask(npbnn_ctx* ctx, const double* mask_packed);

/* ---- options / introspection.
 * NPBNN_OPT_L0_PRECISION selects how the first layer's product X.W0^T (MatrixMultiplicationD, BNN_lib.py:154-162; float64
 * np.dot in the reference) is computed:
 *   NPBNN_L0_F32   float32 matrix cores (v_mfma_f32_16x16x4_f32), bit-exact float32 fused-multiply-add chain;
 *   NPBNN_L0_F16   "fp16-split": every x and w is held as a pair of fp16 numbers (high + low part, ~22 significant bits,
 *                  features scaled per column by a power of two), three fp16 matrix-core products accumulated in float32;
 *                  same HBM bytes as float32, 5x less matrix-core time;
 *   NPBNN_L0_AUTO  fp16-split whenever the data and weights are representable (finite, in range), else float32; an
 *                  evaluation whose weights leave the fp16 range is transparently repeated in float32 (default). */
/* NPBNN_OPT_FAST_TAILS (default 1): launches that want nothing but the likelihood of a 2- or 3-layer network whose later layers
 * have <= 16 nodes (the layer loop of MCMC.mh_step, np_bnn/BNN_env.py:449-473, on every BASELINE shape) run on builds of the
 * evaluation kernel with the layer loop, the activation and the epilogue resolved at compile time; 0 keeps every launch on
 * the general build (same results bit for bit; for A/B timing).  NPBNN_INFO_FAST_TAILS: 1 when such launches would take them. */
/* NPBNN_OPT_PERSISTENT (default 1): npbnn_chain_run with cfg->schedule = NPBNN_SCHED_AUTO may pick NPBNN_SCHED_PERSIST for a chain
 * that has its GPU to itself; 0 keeps the automatic choice on kernel boundaries (NPBNN_SCHED_OVERLAP / _SERIAL). */
/* NPBNN_OPT_TRAINABLE_SLOPES (default 0): 1 reserves a slot per hidden layer in the weight image for the activation slope, so that the
 * candidates of a chain pass can each carry their own (npbnn_chain_cfg.slope_idx ...); such a network runs on the general builds. */
/* NPBNN_OPT_WIDE (default 0): the weight-streamed path.  A network runs on it BY ITSELF when a layer has more than 128 nodes or when its
 * weights would leave a compute unit's LDS fewer than 4 waves beside them (the reference's default n_nodes = [50, 5], np_bnn/BNN_env.py:20,
 * from ~700 features on, [32, 8] from ~980 (first layers of one or two output tiles leave it below eight waves); MatrixMultiplicationD, np_bnn/BNN_lib.py:154-162, takes any shape): every layer is then a
 * tiled matrix product whose operands both stream through LDS, weights from images resident in HBM (widths up to NPBNN_MAX_WIDTH, images
 * up to 2 GiB); a chain pass carries up to three candidates where the pass is one fused launch (narrow networks on many rows), else
 * one.  Same results as the resident path to rounding (not bit for bit: another order of float32 additions); the envelope and the
 * rates either side of the switch are in DESIGN.md 4.4.  1 = every network runs on it
 * (A/B timing, tests).  NPBNN_INFO_WIDE: 1 when the architecture set last runs on it.
 * NPBNN_INFO_F16_MOVED_COLUMNS / _F16_MAX_MOVE: the fp16-split copy scales every column by a power of two taken from its largest entry;
 * heavy-tailed columns (typical entries many powers of two below the largest) get that scale moved up so that the pair keeps their
 * typical entries (the largest entry then lies below 2^move instead of below 1; the weights' scale moves the other way): how many
 * columns of the training matrix were moved, and the largest move in powers of two (<= 12).  Valid once a launch has built the copy. */
enum { NPBNN_OPT_L0_PRECISION = 1, NPBNN_OPT_FAST_TAILS = 2, NPBNN_OPT_PERSISTENT = 3, NPBNN_OPT_TRAINABLE_SLOPES = 4, NPBNN_OPT_WIDE = 5 };
enum { NPBNN_L0_AUTO = 0, NPBNN_L0_F32 = 1, NPBNN_L0_F16 = 2 };
/* NPBNN_INFO_TURN_NS_OVERLAPPED / _BETWEEN: what NPBNN_SCHED_AUTO last measured for one launch turn (a pass, decided or void) of the
 * two persistent forms, in nanoseconds (0: never run on this context); NPBNN_INFO_IT_NS_OVERLAPPED / _BETWEEN: what an ITERATION of a
 * batch cost on each of them - the figure NPBNN_SCHED_AUTO compares, kept apart for batches of fewer than 256 iterations (reported
 * here when measured) and longer ones.  NPBNN_INFO_MAX_CANDIDATES: weight sets one pass over the
 * data can carry for this network (1-3: what fits a compute unit's LDS, and two from three layer-0 output tiles on) - the
 * candidates of a speculative chain pass, the chains of a group pass (npbnn_chains_run_batched), the sets of npbnn_predict_sets.  On the
 * weight-streamed path it answers 1 (the group pass carries one chain there), while a replay of stored sets carries up to three per
 * read of X wherever the first layer's product takes the rest of the pass along (at most 64 nodes, one K-slice) and one elsewhere:
 * NPBNN_INFO_REPLAY_PASSES: passes over X the last replay of stored sets launched (npbnn_predict_sets and the entries that summarise
 * it), float32 repeats included; NPBNN_INFO_REPLAY_MAX_GROUP: the most sets one of those passes carried.  Both paths write them.
 * NPBNN_INFO_L0_OPTION: the NPBNN_OPT_L0_PRECISION in force (NPBNN_L0_*).  A caller that repeats a chain batch after NPBNN_E_RANGE
 * with cfg->force_f32 = 1 asks it first: under NPBNN_L0_F16 the error stands, as it does for npbnn_eval and npbnn_chain_run_general. */
enum { NPBNN_INFO_L0_F16 = 1, NPBNN_INFO_WAVES_PER_BLOCK = 2, NPBNN_INFO_N_CU = 3, NPBNN_INFO_FAST_TAILS = 4,
       NPBNN_INFO_TURN_NS_OVERLAPPED = 5, NPBNN_INFO_TURN_NS_BETWEEN = 6, NPBNN_INFO_MAX_CANDIDATES = 7,
       NPBNN_INFO_IT_NS_OVERLAPPED = 8, NPBNN_INFO_IT_NS_BETWEEN = 9, NPBNN_INFO_WIDE = 10,
       NPBNN_INFO_F16_MOVED_COLUMNS = 11, NPBNN_INFO_F16_MAX_MOVE = 12, NPBNN_INFO_PDP_ROUTE = 13,
       /* with NPBNN_FI_TIMING=1 in the environment (HIP events; 0 otherwise): device time in nanoseconds of the last
        * npbnn_permute_columns (restore, gather and the patch of the split copies), and of the last npbnn_predict_sets_summary's
        * evaluation passes (weight packing included), accumulation launches and final kernel; npbnn_predict_sets_support leaves its
        * passes and accumulation in the same two slots and its own final kernel in NPBNN_INFO_SUPPORT_FINAL_NS; npbnn_predict_sets_lppd
        * does the same with NPBNN_INFO_LPPD_FINAL_NS (and leaves 0 in its three slots when it refuses a call before any launch), and
        * npbnn_predict_sets_uncertainty with NPBNN_INFO_UNCERTAINTY_FINAL_NS (likewise), and npbnn_predict_sets_convergence with
        * NPBNN_INFO_CONVERGENCE_FINAL_NS (its diagnostic and summary kernels; likewise), and npbnn_predict_sets_calibration with
        * NPBNN_INFO_CALIBRATION_FINAL_NS (likewise; a slot of its own after the options' and the replay's).  npbnn_predict_sets and npbnn_predict_sets_hpd
        * run the same replay, so after them NPBNN_INFO_SUMMARY_PASS_NS / _ACC_NS describe that call: its passes, and the copies to the
        * host (npbnn_predict_sets) or nothing (npbnn_predict_sets_hpd, whose groups write straight into its stack) */
       NPBNN_INFO_PERMUTE_NS = 14, NPBNN_INFO_SUMMARY_PASS_NS = 15, NPBNN_INFO_SUMMARY_ACC_NS = 16, NPBNN_INFO_SUMMARY_FINAL_NS = 17,
       NPBNN_INFO_SUPPORT_FINAL_NS = 18, NPBNN_INFO_LPPD_FINAL_NS = 19, NPBNN_INFO_UNCERTAINTY_FINAL_NS = 20,
       NPBNN_INFO_CONVERGENCE_FINAL_NS = 21,
       NPBNN_INFO_REPLAY_PASSES = 22, NPBNN_INFO_REPLAY_MAX_GROUP = 23, NPBNN_INFO_L0_OPTION = 24,
       NPBNN_INFO_CALIBRATION_FINAL_NS = 25,
       /* the route that served the last npbnn_predict_ale (1 or 2; 0 before any call, and after one that was refused) */
       NPBNN_INFO_ALE_ROUTE = 26,
       /* the route that served the last npbnn_predict_saliency (1 or 2; 0 before any call, and after one that was refused), and with
        * NPBNN_FI_TIMING=1 the device time in nanoseconds of its phase 2: the fold and reduce kernels of every launch (0 otherwise) */
       NPBNN_INFO_SALIENCY_ROUTE = 27, NPBNN_INFO_SALIENCY_FOLD_NS = 28,
       /* the route that served the last npbnn_predict_shapley (1 or 2; 0 before any call, and after one that was refused), and with
        * NPBNN_FI_TIMING=1 the device time in nanoseconds of its walk kernels (0 otherwise) */
       NPBNN_INFO_SHAPLEY_ROUTE = 29, NPBNN_INFO_SHAPLEY_WALK_NS = 30,
       /* with NPBNN_FI_TIMING=1 the device time in nanoseconds of the last npbnn_predict_sets_loo's final kernel (0 otherwise, and
        * after a call refused before any launch); its passes and its log-likelihood launches are in NPBNN_INFO_SUMMARY_PASS_NS / _ACC_NS */
       NPBNN_INFO_LOO_FINAL_NS = 31,
       /* with NPBNN_FI_TIMING=1 the device time in nanoseconds of the last npbnn_loglik_grad's phase 1 (one thread per row) and of its
        * phase 2 (the products over the rows and the reduce kernel), over every chunk (0 otherwise, and after a refused call) */
       NPBNN_INFO_GRAD_ROWS_NS = 32, NPBNN_INFO_GRAD_FOLD_NS = 33 };
int npbnn_set_option(npbnn_ctx* ctx, int option, int value);
int npbnn_get_info(npbnn_ctx* ctx, int what, int* out);

/* ---- one proposal evaluation: replaces the per-layer RunHiddenLayer loop + output function +
 * likelihood of MCMC.mh_step (BNN_env.py:449-473, 485-491) and of MCMC.__init__ (:299-319).
 *   W_packed     float64 packed weights (mask / indicators already applied by the caller, :461-464)
 *   act_prm      per-hidden-layer slope for NPBNN_ACT_LEAKY (ActFun._prm, BNN_lib.py:84-85) or NULL
 *   col_override length in_dim or NULL: entries that are not NaN replace that feature column by the
 *                given constant (data_transform_obj.transform, BNN_env.py:14-17)
 *   sigma        k values, or NULL = empirical sigma (BNN_env.py:475-476); Gaussian likelihood only
 *   confusion    n_classes x n_classes int64 [true label][argmax] or NULL; CalcAccuracy,
 *                CalcLabelAccuracy and CalcLabelFreq (BNN_lib.py:203-233) are functions of it */
int npbnn_eval(npbnn_ctx* ctx, const double* W_packed, const double* act_prm,
               const double* col_override, double lik_temp, const double* sigma, int which,
               npbnn_eval_out* out, int64_t* confusion);

/* ---- predictions: replaces RunPredict / RunPredictInd (BNN_lib.py:245-272).
 * out_y is n_rows x out_dim[last] float64; apply_out_fn=0 returns the last layer's pre-output values. */
int npbnn_predict(npbnn_ctx* ctx, const double* W_packed, const double* act_prm,
                  const double* col_override, int which, int apply_out_fn, double* out_y);

/* Posterior prediction: n_sets stored weight vectors (W_sets [n_sets][n_weights], act_prm_sets [n_sets][n_layers-1] or NULL)
 * against the resident matrix `which`; up to three sets share one streaming read of X.  out_y: [n_sets][n_rows][out_dim].
 * Replaces the loop over RunPredict of get_posterior_cat_prob (np_bnn/BNN_lib.py:375-381; also predictBNN :430, feature_importance
 * :504-597, get_posterior_est :715-748), which copies and re-reads the feature matrix once per posterior sample. */
int npbnn_predict_sets(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which, int apply_out_fn,
                       double* out_y);

/* Partial dependence: replaces the loop over grid points and stored samples of get_pdp (np_bnn/BNN_pdp.py).  For each of n_grid
 * points the focal columns (focal[n_focal]) read as grid[g][0..n_focal-1], then the columns col_override gives (in_dim entries,
 * NaN = none: data_transform_obj, which applies after the grid values and so wins on a focal column) read as that constant.
 * out_mean [n_grid][n_rows][out_dim]: per grid point and row, the prediction averaged over the n_sets stored weight vectors
 * (W_sets and act_prm_sets as in npbnn_predict_sets).  NPBNN_INFO_PDP_ROUTE tells which route served the last call:
 *   1  grid-batched kernel (networks on the LDS-resident path with narrow layers): one read of X per group of sets computes layer 0
 *      with the focal columns at 0; each grid point adds its shift sum_f grid[g][f] * W0[:, f] and runs the later layers;
 *   2  one pass of the evaluation kernels per (grid point, set), the grid values folded into layer 0's bias like col_override.
 * Sums over the sets run in a fixed order (deterministic results).  NPBNN_PDP_PER_GRID=1 (environment) forces route 2.
 * Route 1's envelope, for in_dim F and layer widths out_dim[0] = H0, out_dim[1], ..., out_dim[n_layers - 1]; a network on the
 * LDS-resident path that meets all four limits takes route 1, every other one route 2 (tests/test_hip_pdp_envelope.py holds both
 * sides of each limit to the float64 oracle).  With H0P = 32 when H0 <= 32, else 64:
 *   a  H0 <= 64;
 *   b  round_up(F, 16) * H0P * 4 bytes <= 64 KiB: one set's first layer in LDS (F <= 512 when H0 <= 32, F <= 256 above);
 *   c  out_dim[l] <= 32 for every l >= 1, and out_dim[0] <= 32 as well when n_layers == 1 (the outputs stay in 32 registers);
 *   d  (64 / H0P) * T * 4 bytes <= 32 KiB, T = sum over l >= 1 of round_up(out_dim[l], 4) + out_dim[l] * round_up(out_dim[l-1], 8):
 *      the later layers of the 64 / H0P sets of one launch in LDS (after H0 = 32, three layers of 32 and 4 outputs have T = 3300
 *      and fit, four layers of 32 have T = 4356 and do not).
 * These figures are constants of the code (kPdp* in npbnn_pdp.hip), chosen for register and LDS room, not measured cross-over points. */
int npbnn_predict_pdp(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, const int32_t* focal, int32_t n_focal,
                      const double* grid, int32_t n_grid, const double* col_override, int which, int apply_out_fn, double* out_mean);

/* Accumulated local effects (Apley & Zhu 2020) of one feature column, per stored weight set; np_bnn has no counterpart.  The n_bins + 1
 * edges (finite, strictly increasing) cut the column `focal` into n_bins bins: a row belongs to the first bin k = 1 .. n_bins whose
 * upper edge edges[k] is not below its entry - float32 entry against the edge rounded to float32 - and to the last bin when it lies
 * above every edge; entries at or below edges[0] fall into bin 1.  out_counts [n_bins]: the rows of each bin.  out_effect
 * [n_sets][n_bins][out_dim]: per set and bin, the mean over the bin's rows of (the prediction with the focal column at edges[k]) minus
 * (the prediction with it at edges[k - 1]); 0 for a bin without rows.  The edges enter in float64, as npbnn_predict_pdp's grid values
 * do, and col_override applies after them as it does there: with the focal column overridden every effect is 0.  The running sums
 * over the bins and their centring are the caller's (npbnn_amd/ale.py).  NPBNN_INFO_ALE_ROUTE tells which route served the call:
 *   1  networks inside npbnn_predict_pdp's route-1 envelope (limits a - d above): one read of X per group of sets computes layer 0
 *      with the focal column at 0, and each row adds the shifts of its own bin's two edges;
 *   2  one pass of the evaluation kernels per (edge, group of sets), the edge folded into layer 0's bias; after the pass at edge k its
 *      predictions are added to bin k's sums and taken from bin k + 1's.
 * Sums over rows run per workgroup of 256 rows in row order, then over the workgroups in a fixed order, in float64, without
 * floating-point atomics: the same input gives the same bits.  NPBNN_ALE_PER_EDGE=1 (environment) forces route 2.  NPBNN_E_ARG, before any launch:
 * a null W_sets, edges, out_counts or out_effect, n_sets < 1, n_bins outside 1 .. 1024, focal outside 0 .. in_dim - 1, edges that
 * are not finite or not strictly increasing. */
int npbnn_predict_ale(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int32_t focal, const double* edges,
                      int32_t n_bins, const double* col_override, int which, int apply_out_fn, int64_t* out_counts, double* out_effect);

/* Input-gradient saliency of the stored weight sets; np_bnn has no counterpart.  With G[s][i][c][j] = d f_s(x~_i)_c / d x_ij - x~_i the row i
 * of the resident matrix `which` after col_override, f the network's output (through the output function with apply_out_fn = 1, the last
 * layer's values with 0) - the three outputs, each [n_sets][out_dim][in_dim], are means over the n rows:
 *   out_mean  (1/n) sum_i G      the average marginal effect
 *   out_abs   (1/n) sum_i |G|    the saliency
 *   out_sq    (1/n) sum_i G^2    the rows' spread
 * A column col_override gives a constant has gradient 0, exactly.  The chain rule runs over the code of the forward pass: ReLU 1 for
 * z > 0, else 0; leaky slope for z < 0, else 1, each set with its own slope per layer (act_prm_sets as in npbnn_predict_sets);
 * swish s (1 + z (1 - s)), s = sigma(z); tanh 1 - t^2; the last layer's activation where arch.final_act is set; softmax p_c (delta_ck -
 * p_k); softplus-half sigma(z_c) on the outputs c >= out_dim / 2; biases contribute nothing.  G never leaves the device and is never
 * stored whole.  A launch has two phases over a chunk of rows: phase 1, one thread per row, runs forward and then, per output, back to
 * layer 0's pre-activation, D[c][row][h] = d f_c / d z0_h; phase 2 forms G = D_c W0^T per tile of 32 rows x 32 features on the float32
 * matrix instruction and folds it at once.  NPBNN_INFO_SALIENCY_ROUTE tells which phase 1 served the call:
 *   1  networks inside npbnn_predict_pdp's route-1 envelope (limits a - d above): layer 0 from a weight image in LDS, one read of X per
 *      group of sets, the later layers in registers;
 *   2  every other network the library takes (layers up to NPBNN_MAX_WIDTH, any in_dim, the weight-streamed path's): a plain kernel
 *      with runtime widths whose activations live in a device scratch.  NPBNN_SALIENCY_PLAIN=1 (environment) forces it, and so does
 *      NPBNN_FORCE_WIDE=1.
 * Both read the float32 matrix only: NPBNN_OPT_L0_PRECISION plays no part, and there is no fp16-range repeat.  Sums over rows run in
 * float32 inside one tile of 32 rows at most, from there on in float64: in row order over a wave's 256 rows, then over the waves in a
 * fixed order, without floating-point atomics: the same input gives the same bits on every call.  D and the partial sums have a byte
 * budget (128 MiB; NPBNN_SALIENCY_SCRATCH_BYTES in the environment overrides it): a larger table runs in chunks of rows.
 * NPBNN_E_ARG, before any launch: a null W_sets, out_mean, out_abs or out_sq, n_sets < 1, a table without rows.  NPBNN_E_STATE without
 * npbnn_set_arch or without data on `which`. */
int npbnn_predict_saliency(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, const double* col_override, int which,
                           int apply_out_fn, double* out_mean, double* out_abs, double* out_sq);

/* ---- the log-likelihood and its gradient with respect to the WEIGHTS.  np_bnn has no counterpart: it takes a starting point trained
 * elsewhere (get_weights_from_tensorflow_model, np_bnn/BNN_lib.py:601-624); npbnn_amd/gradient.py builds map_estimate on this entry.
 * Arguments as npbnn_eval's.  With z the last layer's values of row i of the resident matrix `which` after col_override (after the
 * activation where arch.final_act is set),
 *   out->loglik = sum_i l_i        out_grad [n_weights] = sum_i d l_i / d W
 * out_grad in packed-weight order: the layer matrices concatenated, each row-major, the bias in column 0 where the layer has one.
 *   NPBNN_LIK_CATEGORICAL      l_i = lik_temp w_i log softmax(z)_{y_i};  d l_i / d z_c = lik_temp w_i (delta(c, y_i) - p_c).  w_i: the
 *                              instance weight times the class weight of y_i, each 1 where npbnn_set_row_weights gave none, as
 *                              npbnn_eval applies them: on the training table only.
 *   NPBNN_LIK_GAUSS            l_i = lik_temp sum_t norm.logpdf(y_it, z_t, sigma_t);  d l_i / d z_t = lik_temp (y_it - z_t) / sigma_t^2.
 *                              sigma (k values) is required: NULL, the empirical sigma, is NPBNN_E_ARG.  out->sigma, sum_r and sum_r2
 *                              are filled as npbnn_eval fills them.
 *   NPBNN_LIK_GAUSS_PRED_SIGMA mu = z[:k], s = softplus(z[k:]), l_i = lik_temp sum_t norm.logpdf(y_it, mu_t, s_t);
 *                              d l / d z_t = lik_temp (y - mu) / s^2,  d l / d z_{k+t} = lik_temp ((y - mu)^2 / s^3 - 1 / s) sigmoid(z_{k+t}).
 * The count likelihoods and NPBNN_LIK_NONE are refused with NPBNN_E_ARG.  Below the outputs the chain rule is npbnn_predict_saliency's:
 * every activation's derivative on the branch the forward pass takes, the last layer's where arch.final_act is set, the slopes from
 * act_prm.  With delta_l the derivative with respect to layer l's pre-activation and h_(l-1) that layer's input (the row of X for
 * l = 0), d l_i / d W_l = delta_l h_(l-1)^T; a bias column receives sum_i delta_l; a column of layer 0 whose feature col_override
 * replaces by the constant c_j receives c_j times layer 0's bias sum - the derivative of what the forward pass computes.  The
 * derivative with respect to the slopes is not returned.
 * One route, every network the library takes at runtime widths, in two phases over a chunk of rows.  Phase 1, one thread per row:
 * forward from the float32 blocks of npbnn_predict_saliency's route 2, the row's log-likelihood term, and the backward pass of that
 * scalar down to layer 0; every layer's values and deltas stay in a device scratch, layer 0's delta row-major.  Phase 2: the products
 * whose reduction dimension is the rows - layer 0's [H0 x rows] [rows x in_dim] against X itself on v_mfma_f32_32x32x2_f32, a wave
 * per slot of rows, 32 hidden units and up to 128 features; the later layers in a plain kernel.  Sums over rows run in float32
 * inside one slot of 256 rows (kGradSlotRows), from there on as float64 partials in device memory that a reduce kernel adds in a
 * fixed order; lik_temp multiplies the float64 totals.  No floating-point atomics: the same input gives the same bits on every
 * call.  It reads the float32 matrix only: NPBNN_OPT_L0_PRECISION plays no part and there is no fp16-range repeat.  Scratch and
 * partials have a byte budget (128 MiB; NPBNN_GRAD_SCRATCH_BYTES in the environment overrides it): a larger table runs in chunks
 * of rows (npbnn_attrib_grad_of).  With NPBNN_FI_TIMING=1 the device time of phase 1 goes to NPBNN_INFO_GRAD_ROWS_NS and that of
 * phase 2, the reduce kernel included, to NPBNN_INFO_GRAD_FOLD_NS (0 otherwise, and after a refused call).  The context keeps the
 * call's device buffers - up to the scratch budget, and the float32 blocks - for the next call; npbnn_set_data and npbnn_share_data
 * free them, npbnn_destroy too.  Measured on an MI355X (tools/time_grad.py; the entry and, in a run of their own, the two phases
 * as medians of 200 calls, in two fresh processes):
 * 100k x 256, [32, 8], 10 classes 0.64-0.65 ms a call (phase 1 0.34, phase 2 0.17), 1M x 64, [16, 4], 2 Gaussian targets
 * 1.18-1.20 ms (0.56, 0.56); npbnn_eval of the same weights 0.08-0.09 and 0.10-0.11 ms, the definition in numpy 80-82 and 320-341 ms.  Against float64
 * (tests/test_hip_grad.py): the largest error is 0.23 of a bar of 16 times the larger of a float32 restatement's distance and
 * 2^-24 sum_i |delta_i| |h_i|, per layer; the log-likelihood within a relative 3.3e-8.
 * NPBNN_E_ARG before any launch: a null W_packed, out or out_grad, `which` not 0 or 1, a table without rows, a likelihood other
 * than the three, NPBNN_LIK_GAUSS without sigma, NPBNN_LIK_GAUSS_PRED_SIGMA with out_dim other than 2 k, targets of another width;
 * after the launches: a label outside [0, out_dim).  NPBNN_E_STATE: no npbnn_set_arch, no data, labels or targets on `which`, or a
 * row-sharded context (npbnn_set_row_shard).  A refused call leaves out and out_grad untouched.  Non-finite results are returned
 * as they are. */
int npbnn_loglik_grad(npbnn_ctx* ctx, const double* W_packed, const double* act_prm, const double* col_override, double lik_temp,
                      const double* sigma, int which, npbnn_eval_out* out, double* out_grad);

/* Permutation-sampling Shapley attributions of single rows, per stored weight set; np_bnn has no counterpart.  f_s is the network of set s
 * (through the output function with apply_out_fn = 1, the last layer's values with 0), x_e row rows[e] of the resident matrix `which`, b row
 * bg_rows[.] of the resident matrix `which_bg`, both after col_override.  A player is a group of columns: player_of [in_dim] names every
 * column's player (NULL: column j is player j, and n_players must be in_dim).  Each row of perms [n_perm][n_players] is a permutation pi of
 * the players.  A walk (s, e, b, pi) starts at b and at step k sets every column of player pi[k] to x_e's value;
 *   phi_walk[pi[k]][c] = f_s(after step k)_c - f_s(before step k)_c,   phi[s][e][p][c] = mean over the n_bg n_perm walks of phi_walk[p][c],
 * so sum_p phi[s][e][p][c] = f_s(x_e)_c - mean_b f_s(b)_c for any permutations, and with all n_players! of them phi is the exact
 * interventional Shapley value over the background rows.  A player whose columns are all overridden is exactly 0.  The outputs:
 *   out_mean  [n_explain][n_players][C]           mean over the sets of phi
 *   out_sq    [n_explain][n_players][C]           mean over the sets of phi^2
 *   out_abs   [n_sets][n_players][C]              mean over the explained rows of |phi|
 *   out_fx    [n_sets][n_explain][C]              f_s(x_e), one direct forward pass
 *   out_base  [n_sets][C]                         mean_b f_s(b)
 *   out_phi   [n_sets][n_explain][n_players][C]   phi itself, or NULL: not wanted.  NPBNN_E_NOMEM when it is over its byte budget (256 MiB;
 *             NPBNN_SHAPLEY_PHI_BYTES in the environment overrides it); the message names the largest n_explain that fits.
 * The tables, the hybrid rows and the walks' differences stay on the device.  A step moves layer 0's pre-activation by W0[:, j] (x_ej - b_j)
 * per column of its player and runs the later layers again.  A lane owns one explained row and the 64 lanes of a wave share (set, b, pi);
 * z0(b) is computed once per (set, b).  The W = n_bg n_perm walks, b-major, are cut into n_split runs of consecutive walks, one wave each;
 * n_split depends on the sizes, the device's compute units and the scratch budget below: another budget or device gives other splits, so the
 * same values to rounding, not the same bits.  NPBNN_INFO_SHAPLEY_ROUTE tells which kernels served the call:
 *   1  networks inside npbnn_predict_pdp's route-1 envelope (limits a - d above): the set's transposed first layer in LDS, z0 in registers,
 *      the later layers in registers from LDS broadcasts;
 *   2  every other network the library takes: plain kernels with runtime widths whose z0 and activations live in a device scratch
 *      [unit][value][lane].  NPBNN_SHAPLEY_PLAIN=1 (environment) forces it, and so does NPBNN_FORCE_WIDE=1.
 * Both read the float32 matrix only: NPBNN_OPT_L0_PRECISION plays no part, and there is no fp16-range repeat.  Arithmetic is float32 inside a
 * walk, the difference of two float32 predictions included.  Every sum is float64: a wave adds its walks' differences in walk order, the
 * splits are added in split order, the sets in set order, the rows of |phi| per thread in row order, then over the workgroup and the chunks in
 * a fixed order; out_base is the float64 mean of the float32 f_s(b).  No floating-point atomics: the same input gives the same bits on every
 * call.  The waves' partial sums (and route 2's scratch) have a byte budget (128 MiB; NPBNN_SHAPLEY_SCRATCH_BYTES in the environment overrides
 * it): a larger job runs in chunks of explained rows, and launches of fewer sets.  With NPBNN_FI_TIMING=1 the device time of the walk kernels
 * goes to NPBNN_INFO_SHAPLEY_WALK_NS (an int: it ends at 2147 ms).  Measured on an MI355X (tools/time_shapley.py, tests/test_hip_shapley.py -s;
 * NOTES 8.14): config 2's shapes, 100 sets, 64 rows x 4 backgrounds x 2 permutations 21.4 ms against 600.5 ms through a table of hybrid rows and
 * npbnn_predict_sets; 256 x 20 x 8 1584 ms under the default budget, whose 102 waves at once bound it, 114.8 ms under 4 GiB; largest error
 * against float64 1.9e-06 of an array's largest entry on either route.  NPBNN_E_ARG, before any launch: a null required pointer; n_sets, n_explain, n_bg, n_perm or n_players
 * below 1; a row index outside its table; a player_of entry outside 0 .. n_players - 1; a player without a column; a row of perms that is not
 * a permutation.  NPBNN_E_STATE without npbnn_set_arch or without data on either table.  A refused call leaves the outputs untouched. */
int npbnn_predict_shapley(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, const double* col_override, int which,
                          const int64_t* rows, int32_t n_explain, int which_bg, const int64_t* bg_rows, int32_t n_bg, const int32_t* player_of,
                          int32_t n_players, const int32_t* perms, int32_t n_perm, int apply_out_fn, double* out_mean, double* out_sq,
                          double* out_abs, double* out_fx, double* out_base, double* out_phi);

/* Posterior credible intervals: calcHPD (np_bnn/BNN_lib.py:286-302) applied to every (row, output) of the n_sets stored samples'
 * predictions, as its summary code does once per row (np_bnn/BNN_plot.py:73-75).  The sets replay as in npbnn_predict_sets, but
 * each group writes its float32 predictions into a device stack [n_sets][n_rows][out_dim] that never leaves the device; one HPD
 * launch then reads it once.  out_mean / out_lo / out_hi [n_rows][out_dim]: the mean over the sets (float64 sum) and the bounds of
 * the narrowest window holding nIn = round(level * n_sets) values (round half to even), the first one among equally narrow ones;
 * widths in float64 from the float32 values, so the bounds are calcHPD's on the float64 array npbnn_predict_sets returns.
 * NPBNN_E_ARG: more than 16384 sets, level outside (0, 1), nIn < 2, or a prediction that is NaN or infinite.  NPBNN_E_NOMEM: the
 * stack is over its byte budget (1 GiB; NPBNN_HPD_STACK_BYTES in the environment overrides it), the message names the largest row
 * count that fits. */
int npbnn_predict_sets_hpd(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which, int apply_out_fn,
                           double level, double* out_mean, double* out_lo, double* out_hi);

/* Permutation importance (feature_importance, np_bnn/BNN_lib.py:504-597) without leaving the device.
 *
 * npbnn_permute_columns replaces the copy of the feature matrix and the shuffle of some of its columns at the top of
 * get_posterior_cat_prob (np_bnn/BNN_lib.py:364-371) and the upload that would follow: column cols[j] of the resident matrix `which`
 * reads X0[perm[p][r]][cols[j]] in row r, X0 being the matrix as npbnn_set_data_* left it; p = 0 for every column when n_perm == 1
 * (the block moves as a whole, :371), p = j when n_perm == n_cols (every column by its own permutation, :368-369).  perm:
 * [n_perm][n_rows] int64 row indices.  A call first puts back the columns the previous call moved (the library keeps those columns
 * alone, n_rows x n_cols floats); n_cols == 0 or perm == NULL only puts them back.  The fp16-split copies are patched in the moved
 * columns under the column scales they were built with (a column's largest entry does not move with its rows).
 * NPBNN_E_STATE: the matrix is borrowed (npbnn_share_data) or other contexts borrow it.  NPBNN_E_ARG: a column outside the matrix
 * or named twice, n_perm not in {1, n_cols}, or a row index outside [0, n_rows) (found on the device before anything is written:
 * the matrix stays as it was).  npbnn_set_data_* drops the saved columns. */
int npbnn_permute_columns(npbnn_ctx* ctx, int which, const int32_t* cols, int32_t n_cols, const int64_t* perm, int32_t n_perm);

/* Summary of the n_sets stored samples' predictions on the resident matrix `which`, and its confusion table: the loop over
 * RunPredict and the summary of get_posterior_cat_prob (np_bnn/BNN_lib.py:375-392) and CalcAccuracy's argmax against the labels
 * (:203-209), with nothing but the results leaving the device.  The sets replay as in npbnn_predict_sets; each group's float32
 * predictions are folded into a device accumulator before the next group overwrites them.
 *   mode 0  out_summary[r][c] = share of the sets whose largest prediction in row r is class c, the first such class (:382-390);
 *   mode 1  out_summary[r][c] = mean of the sets' predictions, the float32 values added in float64 in set order (:391-392).
 * out_summary: [n_rows][out_dim] float64, or NULL.  labels: [n_rows] int64 in [0, out_dim), or NULL; out_confusion:
 * [out_dim][out_dim] int64, [label][argmax of the summary row, the first class among equal ones], or NULL (labels and
 * out_confusion go together; out_summary and out_confusion both NULL is an error).  NPBNN_E_ARG also for a prediction that is
 * NaN and for a label outside the classes. */
int npbnn_predict_sets_summary(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which,
                               int apply_out_fn, int mode, const int64_t* labels, double* out_summary, int64_t* out_confusion);

/* Confidence thresholds and Bayes-factor support of the n_sets stored samples' summary on the resident matrix `which`: what
 * get_posterior_threshold's sweep (np_bnn/BNN_lib.py:640-671, get_accuracy_threshold :627-637), CalcTP / CalcFP (:305-317),
 * CalcTP_BF / CalcFP_BF (:320-337) and turn_low_pp_instances_to_nan (:674-679) compute from it, in one pass.  The sets replay and
 * accumulate exactly as in npbnn_predict_sets_summary (same mode, same quotient q = accumulator / n_sets, same first argmax k* of the
 * quotient); with p = q[k*] per row:
 *   out_cube   int64 [n_thresholds + 1][out_dim][out_dim]: cell [b][label][k*] counts the rows with exactly b thresholds strictly
 *              below p (p > t in float64 against thresholds[], which must ascend).  The rows retained at thresholds[i] are the bins
 *              b > i; summed over b the cube is npbnn_predict_sets_summary's confusion table.
 *   out_bf     int64 [n_bf + 1][2], with prior_summary [n_rows][out_dim] (else both NULL, n_bf 0): cell [b][k* == label] counts the rows
 *              with exactly b of bf_thresholds[] strictly below (p / (1e-10 + 1 - p)) / (r / (1e-10 + 1 - r)), r = prior_summary[row][k*].
 *   out_summary [n_rows][out_dim] float64 or NULL: the summary; with a cutoff (pointer, or NULL for none) the rows where p > *cutoff
 *              is false are NaN in every class.  out_keep uint8 [n_rows] or NULL: 1 where p > *cutoff (1 everywhere without one).
 * labels [n_rows] int64 in [0, out_dim) are required.  NPBNN_E_ARG before any launch: thresholds or bf_thresholds not ascending or NaN,
 * a NaN cutoff; after the pass: a prediction that is NaN, a label outside the classes. */
int npbnn_predict_sets_support(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which, int apply_out_fn,
                               int mode, const int64_t* labels, const double* thresholds, int32_t n_thresholds, const double* prior_summary,
                               const double* bf_thresholds, int32_t n_bf, const double* cutoff, int64_t* out_cube, int64_t* out_bf,
                               double* out_summary, uint8_t* out_keep);

/* Log pointwise predictive density and WAIC of the n_sets stored samples on the resident matrix `which`, from the per-row terms of the
 * reference's own likelihoods, unweighted and untempered: ll[s][i] = log(prediction[i, label_i]) (calc_likelihood,
 * np_bnn/BNN_lib.py:100-121, the summand of :121) for NPBNN_LIK_CATEGORICAL, and sum over the target columns t of
 * norm.logpdf(y[i][t], mu[i][t], sigma[s][t]) (calc_likelihood_regression, :123-131) for NPBNN_LIK_GAUSS; predictions as the loop over
 * RunPredict gives them per stored sample (:375-381, 715-748).  The [n_sets][n_rows] matrix is never built: the sets replay as in
 * npbnn_predict_sets_summary with the pre-output values left on the device, and each group is folded into float64 per-row
 * accumulators (the log-softmax is taken from the float32 logits in float64, not as the log of a float32 probability).
 *   lppd_i    = logsumexp_s ll[s][i] - log n_sets          mean_ll_i = mean_s ll[s][i]
 *   p_waic_i  = var_s ll[s][i], ddof 1 (0 for one set)     ll_sample[s] = sum_i ll[s][i]
 * lik_kind: NPBNN_LIK_CATEGORICAL (softmax output; labels from npbnn_set_labels_i64 on `which`) or NPBNN_LIK_GAUSS (identity output;
 * targets from npbnn_set_targets_f64, as many columns as the network has outputs; sigma_sets [n_sets][n_targets], every entry
 * positive and finite; NULL for CATEGORICAL); the predicted-sigma and count likelihoods are refused.  out_lppd_i / out_mean_ll_i /
 * out_pwaic_i: [n_rows] each, any may be NULL; out_ll_sample [n_sets] or NULL; out_totals[3] (required): sum_i lppd_i, sum_i mean_ll_i,
 * sum_i p_waic_i - elpd_waic = out_totals[0] - out_totals[2], WAIC = -2 elpd_waic.  Every cross-row sum is made of per-workgroup
 * float64 partials added in a fixed order: two calls return the same bits, however the sets are grouped.  NPBNN_E_ARG before any
 * evaluation: another lik_kind, NULL out_totals, sigma_sets missing or holding a non-positive or non-finite entry, targets of another
 * width, a label outside [0, out_dim); NPBNN_E_STATE: no labels / targets on `which`.  NPBNN_E_ARG after the passes: a prediction that
 * is NaN. */
int npbnn_predict_sets_lppd(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which, int lik_kind,
                            const double* sigma_sets, double* out_lppd_i, double* out_mean_ll_i, double* out_pwaic_i,
                            double* out_ll_sample, double out_totals[3]);

/* Posterior uncertainty decomposition of the n_sets stored samples on the resident matrix `which`: the uncertainty of a prediction
 * split into the part the data cannot remove (aleatoric) and the part that comes from the posterior over the weights (epistemic).
 * The reference has no such function; the predictions are what the loop over RunPredict gives per stored sample
 * (np_bnn/BNN_lib.py:375-381, 715-748) under the output function of ctx's architecture (out_kind), S = n_sets, float64 throughout:
 *   NPBNN_OUT_SOFTMAX (SoftMax, :166-171), p_s = softmax(z_s) of a row's pre-output values z_s, C = out_dim:
 *     out_mean [n_rows][C]   mean_prob = (1/S) sum_s p_s
 *     out_total [n_rows]     predictive entropy -sum_k m_k log m_k of mean_prob, in nats (a term with m_k = 0 is 0)
 *     out_aleatoric [n_rows] expected entropy (1/S) sum_s H(p_s), H(p_s) = lse(z_s) - sum_k p_sk z_sk - never log(softmax): a
 *                            probability that underflows contributes 0
 *     out_epistemic [n_rows] mutual information max(0, predictive - expected entropy); exactly 0 for one set
 *     out_totals[3]          the sums over the rows of the three per-row quantities, in that order
 *   NPBNN_OUT_IDENTITY (RegressTransform, :174-175; T = out_dim, mu_s = z_s) and NPBNN_OUT_SOFTPLUS_HALF (RegressTransformError,
 *   :177-182; out_dim = 2 T, mu_s = z_s[:T], sigma_s = logaddexp(0, z_s[T:])):
 *     out_mean [n_rows][T]      mean_s mu_s
 *     out_epistemic [n_rows][T] (1/S) sum_s (mu_s - mean)^2 (ddof 0: the law of total variance of the mixture), from sums shifted by
 *                               the first set's mu; exactly 0 for one set
 *     out_aleatoric [n_rows][T] (1/S) sum_s sigma_s^2, and out_total [n_rows][T] = epistemic + aleatoric: NPBNN_OUT_SOFTPLUS_HALF only.
 *                               The identity output predicts no sigma - the caller adds the mean of its samples' squared error
 *                               parameters, which does not depend on the row - and both pointers must be NULL under it.
 *     out_totals[4][T]          the sums over the rows of mean, total, aleatoric, epistemic per target (total and aleatoric: 0 under
 *                               NPBNN_OUT_IDENTITY)
 * Every pointwise output may be NULL (it is then not copied from the device); out_totals is required.  No labels or targets are read.
 * The sets replay as in npbnn_predict_sets_lppd, the pre-output values left on the device in float32 and widened before any exp or
 * log; each group is folded into float64 per-row accumulators in set order, and every cross-row sum is made of per-workgroup float64
 * partials added in a fixed order: two calls return the same bits, however the sets are grouped.  Before any launch: NPBNN_E_ARG for
 * n_sets < 1, NULL W_sets or out_totals, `which` not 0 or 1, an odd out_dim under NPBNN_OUT_SOFTPLUS_HALF, out_total or out_aleatoric
 * given under NPBNN_OUT_IDENTITY; NPBNN_E_STATE without npbnn_set_arch or without data on `which`.  NPBNN_E_ARG after the passes: a
 * prediction that is NaN. */
int npbnn_predict_sets_uncertainty(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which,
                                   double* out_mean, double* out_total, double* out_aleatoric, double* out_epistemic, double* out_totals);

/* Posterior calibration of the n_sets stored samples on the resident matrix `which`: whether the probabilities the posterior mean
 * reports can be believed, against the labels (npbnn_set_labels_i64) or targets (npbnn_set_targets_f64) set on `which`.  The reference
 * has no such function; the predictions are what the loop over RunPredict gives per stored sample (np_bnn/BNN_lib.py:245-256) under
 * the output function of ctx's architecture (SoftMax, RegressTransform, RegressTransformError, np_bnn/BNN_lib.py:166-182), S = n_sets,
 * float64 throughout, the sets folded in set order.  B = n_bins in 1..64.
 *   NPBNN_OUT_SOFTMAX, m = (1/S) sum_s softmax(z_s) of a row's pre-output values z_s (accumulated as
 *   npbnn_predict_sets_uncertainty accumulates it), C = out_dim:
 *     out_pred [n_rows]    k*, the first argmax of m            out_point0 [n_rows]  confidence = m[k*]
 *     out_point1 [n_rows]  brier = sum_k (m_k - [k == label])^2  out_point2 [n_rows]  nll = -log m[label]; +inf when m[label] is 0 (a
 *                                                                                    value, not an error)
 *     out_counts [2][B]    count, n_correct of the reliability table: the rows, and the rows with k* == label, per bin
 *                          min(B - 1, floor(confidence B)) - a confidence of exactly 1 falls in the last bin
 *     out_bin_sums [B]     sum_confidence: the sum of the confidences of a bin's rows
 *     out_totals[3]        the sums over the rows of brier, nll and (k* == label)
 *   NPBNN_OUT_IDENTITY (T = out_dim, mu_s = z_s, sigma_s = sigma_sets[s], required, every entry positive and finite) and
 *   NPBNN_OUT_SOFTPLUS_HALF (out_dim = 2 T, mu_s = z_s[:T], sigma_s = logaddexp(0, z_s[T:]); sigma_sets must be NULL), y the targets
 *   [n_rows][T] as the device keeps them (float32); levels[n_levels], n_levels in 0..16, each strictly inside (0, 1):
 *     out_point0 [n_rows][T]  pit = (1/S) sum_s Phi((y - mu_s) / sigma_s), Phi(u) = 0.5 erfc(-u / sqrt 2): the probability integral
 *                             transform under the posterior predictive mixture
 *     out_point1 [n_rows][T]  mean = K + (1/S) sum_s (mu_s - K), K the first set's mu
 *     out_point2 [n_rows][T]  sq_err = (y - mean)^2
 *     out_counts [T][B + n_levels]  per target pit_hist[B], the rows per bin min(B - 1, floor(pit B)), then covered[n_levels], the
 *                             rows with |pit - 0.5| <= level / 2 (the target lies inside the mixture's central interval of that level)
 *     out_totals[2][T]        the sums over the rows of sq_err and of pit per target
 *   out_pred and out_bin_sums must be NULL under regression; under NPBNN_OUT_SOFTMAX the levels are checked and play no part.
 * Every pointwise output (out_point0..2, out_pred) may be NULL (it is then not copied from the device); out_counts and out_totals are
 * required, and out_bin_sums under NPBNN_OUT_SOFTMAX.  The sets replay as in npbnn_predict_sets_uncertainty, the pre-output values left
 * on the device in float32 and widened before any exp, log or erfc.  The integer tables are exact; every cross-row floating-point sum
 * is made of per-workgroup float64 partials added in a fixed order: two calls return the same bits, however the sets are grouped.
 * Before any evaluation: NPBNN_E_ARG for n_sets < 1, NULL W_sets or required outputs, `which` not 0 or 1, n_bins outside 1..64,
 * n_levels outside 0..16, a level outside (0, 1), sigma_sets missing, non-positive or non-finite under NPBNN_OUT_IDENTITY or given
 * under the other two kinds, an odd out_dim under NPBNN_OUT_SOFTPLUS_HALF, targets of another width than T, a label outside
 * [0, out_dim), out_bin_sums or out_pred given under regression; NPBNN_E_STATE without npbnn_set_arch, without data on `which`, or
 * without labels / targets on `which`.  NPBNN_E_ARG after the passes: a prediction that is NaN.  A call refused before any
 * evaluation leaves 0 in its three timing slots (NPBNN_INFO_SUMMARY_PASS_NS, _ACC_NS, NPBNN_INFO_CALIBRATION_FINAL_NS). */
int npbnn_predict_sets_calibration(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which,
                                   const double* sigma_sets, int32_t n_bins, const double* levels, int32_t n_levels,
                                   double* out_point0, double* out_point1, double* out_point2,
                                   int64_t* out_pred, int64_t* out_counts, double* out_bin_sums, double* out_totals);

/* Convergence diagnostics of the n_sets stored samples in function space: split R-hat and effective sample size of every (row, output)
 * of their predictions on the resident matrix `which`.  The reference leaves convergence to a trace viewer on the logged weights; for
 * a network those are the wrong quantity (hidden units permute and rescale without changing the function).  The sets are n_chains
 * chains of N = n_sets / n_chains draws each, chain-major (set s = j * N + t); npbnn_op_convergence (below) has the definition.  The sets
 * replay as in npbnn_predict_sets_hpd into a float32 device stack [n_sets][n_rows][out_dim] that never leaves the device, under the
 * same byte budget (1 GiB; NPBNN_HPD_STACK_BYTES in the environment overrides it; NPBNN_E_NOMEM names the largest row count that fits);
 * one diagnostic launch then reads it once, float64 from the float32 values: the results are the definition's on the float64 array
 * npbnn_predict_sets returns.  The grid depends on n_rows * out_dim alone: however the replay groups the sets, two calls return the
 * same bits.
 *   out_rhat / out_ess  [n_rows][out_dim], or NULL: they then never leave the device
 *   out_summary         [out_dim][4] (required), per output over the rows: the largest rhat, the smallest ess, the number of columns
 *                       with rhat > rhat_threshold, the number of constant columns - reduced on the device in a fixed order.  NaNs
 *                       (constant columns) take no part in the largest / smallest, which are NaN when every column is constant.
 * NPBNN_E_ARG before any launch: NULL W_sets or out_summary, `which` not 0 or 1, a NaN threshold, n_sets not a multiple of n_chains,
 * n_chains outside [1, 64], fewer than 8 draws per chain, more than 16384 sets; NPBNN_E_STATE without npbnn_set_arch or without data
 * on `which`.  NPBNN_E_ARG after the passes: a prediction that is NaN or infinite.  A call refused before any launch leaves 0 in its
 * three timing slots. */
int npbnn_predict_sets_convergence(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int32_t n_chains,
                                   int which, int apply_out_fn, double rhat_threshold, double* out_rhat, double* out_ess,
                                   double* out_summary);

/* The posterior predictive distribution of the n_sets stored samples on the resident matrix `which`, per (row, target): its quantiles,
 * its mean and its continuous ranked probability score against targets given in the call.  The reference has no such function: its
 * summary code takes calcHPD of the predicted means (np_bnn/BNN_plot.py:73-75), an interval that leaves the noise term out.  The
 * predictive distribution of a cell is the mixture (1/S) sum_s N(mu_s, sigma_s^2), S = n_sets; npbnn_op_mixture (below) has the
 * definitions.  The kind follows the output function of ctx's architecture:
 *   NPBNN_OUT_IDENTITY       T = out_dim, mu_s = the set's prediction, sigma_s = sigma_sets[s][t]; sigma_sets [n_sets][T] is required,
 *                            every entry positive and finite (the per-sample sigma of the Gaussian likelihood)
 *   NPBNN_OUT_SOFTPLUS_HALF  out_dim = 2 T, the sets replay with the output function applied: a row of a set's predictions holds T
 *                            means followed by T sigmas (RegressTransformError, np_bnn/BNN_lib.py:177); sigma_sets must be NULL
 * and every other kind is refused.  The sets replay as in npbnn_predict_sets_hpd into a float32 device stack [n_sets][n_rows][out_dim]
 * that never leaves the device, under the same byte budget (1 GiB; NPBNN_HPD_STACK_BYTES in the environment overrides it;
 * NPBNN_E_NOMEM names the largest row count that fits); the kernels read mu and sigma where they lie in it and widen them to float64:
 * the results are the definitions' values on the float64 array npbnn_predict_sets returns.
 *   probs [n_probs]      n_probs in 0..16, each with min(p, 1 - p) >= 1e-12, in any order
 *   targets              [n_rows][T] float64, or NULL (out_crps and out_totals are then NULL too); passed here and not taken from
 *                        npbnn_set_targets_f64, which keeps float32.  Given, at least one of out_crps and out_totals is.
 *   out_quantile         [n_probs][n_rows][T]; NULL exactly when n_probs == 0
 *   out_mean             [n_rows][T], or NULL
 *   out_crps             [n_rows][T], or NULL
 *   out_totals           [T], or NULL: the sum of crps over the rows per target, made of per-workgroup float64 partials added in a
 *                        fixed order
 * The bits of a cell's result depend on its S values alone, and the grids on n_rows and T: two calls return the same bits however the
 * replay groups the sets.  The CRPS costs S (S - 1) / 2 pair terms per cell.  NPBNN_E_ARG before any launch: NULL W_sets, n_sets < 1 or
 * above 16384, more than 16 probabilities or one out of range, probs / out_quantile that do not go together, nothing asked for,
 * out_crps or out_totals without targets or targets without either, a target that is NaN or infinite, `which` not 0 or 1, an output
 * kind other than the two, an odd out_dim under NPBNN_OUT_SOFTPLUS_HALF, sigma_sets missing, non-positive or non-finite under
 * NPBNN_OUT_IDENTITY or given under NPBNN_OUT_SOFTPLUS_HALF; NPBNN_E_STATE without npbnn_set_arch or without data on `which`.
 * NPBNN_E_ARG after the passes: a prediction that is NaN or infinite, or a predicted sigma that is not positive and finite - a
 * softplus that underflowed to 0 in float32 is a refusal, not a division.  A refused call leaves the outputs untouched. */
int npbnn_predict_sets_predictive(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which,
                                  const double* sigma_sets, const double* probs, int32_t n_probs, const double* targets,
                                  double* out_quantile, double* out_mean, double* out_crps, double* out_totals);

/* Pareto-smoothed importance-sampling leave-one-out cross-validation (PSIS-LOO; Vehtari, Gelman, Gabry 2017; Vehtari et al. 2024) of
 * the n_sets stored samples on the resident matrix `which`, against the labels (NPBNN_LIK_CATEGORICAL) or targets (NPBNN_LIK_GAUSS,
 * sigma_sets [n_sets][out_dim]) set on it; lik_kind, sigma_sets and the per-row terms ll[s][i] as in npbnn_predict_sets_lppd, every
 * other kind refused in the same words.  The sets replay as there (pre-output float32 values, grouping without effect on a bit); each
 * group's ll goes into a float64 device matrix [n_sets][n_rows], and one launch of the kernel of npbnn_op_psis (below, which has the
 * definition) reads it once.  2 <= n_sets <= 16384.  The matrix is budgeted like the stack of npbnn_predict_sets_hpd: n_sets * n_rows * 8
 * bytes against 1 GiB (NPBNN_HPD_STACK_BYTES in the environment overrides it); NPBNN_E_NOMEM before any allocation names the rows that
 * fit, and the caller goes block by block of rows (a row's results depend on its own column alone).
 *   out_elpd, out_lppd, out_k   [n_rows] each: elpd_loo_i, lppd_i and the Pareto shape k of the row (+inf where the tail holds four
 *                               values or fewer: plain importance sampling)
 *   out_log_lik_sample          [n_sets], or NULL: sum_i ll[s][i], from per-workgroup float64 partials added in a fixed order
 *   out_log_lik                 [n_sets][n_rows], or NULL: the matrix itself
 * Every summation order is fixed: two calls return the same bytes.  NPBNN_E_ARG before the device is touched: NULL W_sets or outputs,
 * n_sets < 2 or above 16384, a lik_kind that is not served, sigma_sets that does not go with it or is not positive and finite, an
 * output function that does not go with the likelihood, targets of another width; NPBNN_E_STATE without npbnn_set_arch, data, labels
 * or targets.  NPBNN_E_ARG before any evaluation: a label outside [0, out_dim); after the passes: a prediction that is NaN or a
 * log-likelihood that is not finite.  A call refused before any evaluation leaves 0 in NPBNN_INFO_SUMMARY_PASS_NS, _ACC_NS and
 * NPBNN_INFO_LOO_FINAL_NS. */
int npbnn_predict_sets_loo(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which, int lik_kind,
                           const double* sigma_sets, double* out_elpd, double* out_lppd, double* out_k, double* out_log_lik_sample,
                           double* out_log_lik);

/* ---- timing hook for bench.py: launches the evaluation kernels `iters` times on the ctx stream
 * with weights already resident and returns the mean duration of the dominant kernel (HIP events
 * around each launch) and of the whole evaluation, in milliseconds. */
int npbnn_time_eval(npbnn_ctx* ctx, const double* W_packed, int iters, double* ms_main_kernel,
                    double* ms_total);

/* ---- device-resident Metropolis-Hastings iterations: replaces K consecutive calls of MCMC.mh_step
 * (np_bnn/BNN_env.py:381-532) on its default path - UpdateNormal proposals (np_bnn/BNN_mcmc.py:57-69), masks
 * (BNN_env.py:461-462), prior (npBNN.calc_prior, BNN_env.py:180-194), accept test (BNN_env.py:493-494) - with the
 * chain state resident on the GPU.  The host pre-draws the K iterations' random numbers from the very numpy Generator
 * stream the reference consumes (npbnn_host_predraw in libnpbnn_host.so) and passes them here:
 *   idx[t*M + j]   flat index into the packed weights of the j-th perturbed entry of iteration t, or -1 (skipped)
 *   delta[t*M + j] the normal deviate added to that entry;  cnt[t] entries are used in row t
 *   log_u[t]       log of the uniform draw of the accept test
 * W_inout holds the current weights on entry and the chain's weights after K iterations on return. */
typedef struct {
    int32_t prior_kind;                        /* NPBNN_PRIOR_* */
    double prior_scale[NPBNN_MAX_LAYERS];      /* npBNN._prior_scale, one per layer */
    double w_bound;                            /* reflection bound, INFINITY for none */
    double temperature;                        /* MCMC._temperature */
    double lik_temp;                           /* MCMC._lik_temp */
    int32_t sigma_given;                       /* Gaussian likelihood: 1 = use sigma[], 0 = empirical sigma */
    double sigma[NPBNN_MAX_TARGETS];           /* on entry: sigma for proposals when sigma_given */
    double cur_loglik, cur_logprior;           /* state of the chain on entry (MCMC._logLik / _logPrior) */
    double cur_sigma[NPBNN_MAX_TARGETS];       /* npBNN._error_prm on entry */
    int32_t force_f32;                         /* 1: run this batch on the float32 layer-0 path (after NPBNN_E_RANGE) */
    int32_t n_candidates;                      /* proposals evaluated per pass over X (speculative Metropolis-Hastings: iteration t and
                                                  t+1.. assuming the earlier ones are rejected; the chain is unchanged); 0 = as many
                                                  as fit (<= 3), 1 = strictly one evaluation per iteration */
    int32_t schedule;                          /* NPBNN_SCHED_AUTO / _SERIAL (evaluate a pass, decide it, evaluate the next) / _OVERLAP
                                                  (decide pass L-1 inside the launch that evaluates pass L, which was prepared assuming
                                                  pass L-1 rejects; a pass overtaken by an accept is dropped) / _OVERLAP2 (below).
                                                  The same chain whichever runs.  _AUTO: overlapped while fewer than ~37 % of the
                                                  iterations of the previous batch were accepted (75 % of the passes of 3) - as _PERSIST for a chain alone on
                                                  its GPU (NPBNN_OPT_PERSISTENT), else _OVERLAP - and _SERIAL above that; _OVERLAP2
                                                  only runs when asked for by name. */
    int32_t reserved_;
    /* regression with an estimated error parameter (BNN_env.py:435-442: every proposal multiplies sigma by pre-drawn factors,
     * multiplier_proposal_vector, BNN_mcmc.py:101-113): sigma_mult[t*n_targets + q] is the factor of target column q at iteration
     * t (1.0 = untouched), hastings[t] the proposal's Hastings term sum(log m).  The proposal of iteration t is evaluated with
     * sigma' = current sigma * factors (cur_sigma on entry; result->sigma on return), which becomes the chain's sigma when the
     * proposal is accepted.  NULL: sigma as sigma_given / sigma[] say. */
    const double* sigma_mult;
    const double* hastings;
    /* hyper-priors with one scale per input node or per weight (npBNN.sample_prior_scale, BNN_env.py:196-221: hyper_p = 2, 3):
     * the scale of every packed weight (n_weights values, layer matrices concatenated row-major like the weights), or NULL for
     * one scale per layer (prior_scale[] above).  Constant over the call: the Gibbs step that redraws them runs between calls. */
    const double* prior_scale_w;
    /* trainable activation slopes (ActFun(trainable=True), BNN_env.py:416-421,502-503; needs NPBNN_OPT_TRAINABLE_SLOPES): every
     * iteration first proposes new slopes from the accepted ones - UpdateNormal1D(acc_prm, d = 0.05, n = 1, bounds [0, 1]): entry
     * slope_idx[t] moves by slope_delta[t], reflected at 0 and 1 - evaluates its proposal with them, adds
     * log(r) * -sum(slopes') * r (r = 10) to the proposal's log prior and keeps them when the proposal is accepted.
     * cur_slopes: the accepted slopes on entry (result->slopes on return; n_slopes = hidden layers); slope_term_in_prior: 1 when
     * cur_logprior already holds that term for cur_slopes (it does after the chain's first accepted proposal: MCMC.__init__ computes
     * its prior without it, BNN_env.py:374).  slope_idx NULL: FIXED slopes (ActFun("genReLU", prm=...), BNN_lib.py:84-85) - the
     * n_slopes values of cur_slopes are the slopes of the hidden layers for every proposal of the batch (n_slopes = 0: none, slope 0). */
    const int32_t* slope_idx;
    const double* slope_delta;
    double cur_slopes[NPBNN_MAX_LAYERS];
    int32_t n_slopes;
    int32_t slope_term_in_prior;
} npbnn_chain_cfg;
#define NPBNN_SCHED_AUTO 0
#define NPBNN_SCHED_SERIAL 1
#define NPBNN_SCHED_OVERLAP 2
#define NPBNN_SCHED_OVERLAP2 3         /* the overlapped schedule with the launches alternating between two streams: the next launch's
                                         workgroups take the compute units over as the previous launch drains; what a kernel boundary
                                         guaranteed is guaranteed by device-side flags (release / acquire at agent scope).  A wait that
                                         times out ends the batch with NPBNN_E_SYNC (state untouched: retry with NPBNN_SCHED_OVERLAP).
                                         Opt-in: it counts on the two streams having hardware queues of their own and on nothing else
                                         sharing the GPU, neither of which HIP guarantees; a chain that shares its GPU runs _OVERLAP */

#define NPBNN_SCHED_PERSIST 4          /* the overlapped schedule as ONE persistent launch per batch round: every workgroup loops over
                                         the passes, a workgroup that has finished pass L goes straight on to pass L + 1 (no kernel
                                         boundary, no second stream, no launch gap), ordered by the same device-side flags as
                                         _OVERLAP2.  Needs every workgroup of the launch resident (grid <= compute units, the chain
                                         alone on its GPU); every wait is bounded: NPBNN_E_SYNC leaves the state untouched (retry
                                         with NPBNN_SCHED_OVERLAP; the library does so by itself and keeps the context off this schedule afterwards). */

#define NPBNN_SCHED_PERSIST_SERIAL 5   /* for chains that move: one persistent launch like _PERSIST, but a pass is DECIDED before the next one
                                         starts (evaluate pass L, decide it, evaluate pass L + 1 from the state it left - the order of the
                                         reference's loop, np_bnn/BNN_env.py:449-494), so no pass is ever evaluated from a state an accept
                                         has replaced.  The evaluating workgroups wait a few microseconds for the step workgroup between
                                         passes instead of a kernel boundary, a step kernel and a second boundary.  Same conditions,
                                         same bounded waits and the same fallback as _PERSIST.  _AUTO picks it over _PERSIST when the
                                         previous batch accepted more than ~7 % of its proposals. */

typedef struct {
    double loglik, logprior;                   /* state after the K iterations */
    double sigma[NPBNN_MAX_TARGETS];
    int64_t n_accepted;
    int32_t n_passes;                          /* passes over X used for the K iterations */
    int32_t n_candidates;                      /* candidates per pass actually used */
    int32_t n_void_passes;                     /* overlapped schedule: passes dropped because the pass before them accepted */
    int32_t schedule;                          /* schedule actually used (NPBNN_SCHED_SERIAL / _OVERLAP / _OVERLAP2) */
    double temperature;                        /* MCMC._temperature after the iterations (changes in an exchange run only) */
    int32_t iterations_done;                   /* K for npbnn_chain_run; an exchange run may stop a chain earlier (see below) */
    int32_t overflow;                          /* exchange run: 1 = the chain stopped before a proposal that leaves the fp16 range of the
                                                  layer-0 path (continue it with npbnn_chain_run, cfg->force_f32 = 1) */
    double slopes[NPBNN_MAX_LAYERS];           /* accepted activation slopes after the iterations (cfg->n_slopes of them) */
} npbnn_chain_result;

int npbnn_chain_run(npbnn_ctx* ctx, const npbnn_chain_cfg* cfg, double* W_inout, const double* mask_packed,
                    int32_t K, int32_t M, const int32_t* idx, const double* delta, const int32_t* cnt,
                    const double* log_u, uint8_t* out_accepted, double* out_loglik_prop, double* out_logprior_prop,
                    npbnn_chain_result* result);

/* ---- the general device chain: K iterations of MCMC.mh_step (np_bnn/BNN_env.py:381-532) for the sampler settings whose proposal is
 * more than a list of perturbed weights - the other proposal kernels (UpdateUniform np_bnn/BNN_mcmc.py:86-96: perturbations drawn from
 * numpy's global stream; UpdateFixedNormal :27-42: values replaced, Hastings term from every draw; UpdateNormalNormalized :71-82: the
 * perturbed layer divided by its sum), weight indicators (BNN_env.py:460,464: layer 0 multiplied by 0/1 indicators, flipped by
 * UpdateBinomial, BNN_mcmc.py:98-99, in the iterations that do not perturb layer 0; their Bernoulli prior, BNN_env.py:190-193) and
 * feature indicators (BNN_env.py:424-433: a switched-off feature reads as its mean, data_transform_obj :9-17).  Every iteration the
 * device builds the full candidate (weights, indicators, override, log prior in full, Hastings term), packs its weight image,
 * evaluates it (one pass over X) and decides it; nothing returns to the host in between.  All random numbers are pre-drawn by the
 * caller, in the reference's order, from the streams the reference uses:
 *   idx / val / cnt   per iteration the UNIQUE weights the proposal touches (the last draw of a position wins, as numpy's indexed
 *                     assignment does) and, per entry, the perturbation to add (NPBNN_PROP_NORMAL / _UNIFORM / _NORMAL_NORMALIZED) or
 *                     the value to install (NPBNN_PROP_FIXED_NORMAL)
 *   h_idx / h_val / h_fac / h_cnt   NPBNN_PROP_FIXED_NORMAL: EVERY draw - weight, drawn value, 0.5 / d^2 of its proposal width - for
 *                     the Hastings term sum(logpdf(old) - logpdf(drawn))
 *   layer_mask[t]     bit l: layer l was perturbed at iteration t (NPBNN_PROP_NORMAL_NORMALIZED renormalises those layers)
 *   ind_*             weight indicators: ind_inout the current 0/1 matrix of layer 0 (in / out), the flips of iteration t are
 *                     ind_pos[ind_ptr[t] .. ind_ptr[t+1])
 *   find_*            feature indicators likewise; find_use[t] = 1 where the override applies (iterations after adapt_stop)
 * cfg as for npbnn_chain_run (schedule, n_candidates, slopes unused: one candidate per pass, decided before the next). */
enum { NPBNN_PROP_NORMAL = 0, NPBNN_PROP_UNIFORM = 1, NPBNN_PROP_FIXED_NORMAL = 2, NPBNN_PROP_NORMAL_NORMALIZED = 3 };
typedef struct {
    int32_t proposal_kind;
    int32_t M;                                 /* capacity per iteration of the entry lists */
    const int32_t* idx;
    const double* val;
    const int32_t* cnt;
    const int32_t* h_idx;
    const double* h_val;
    const double* h_fac;
    const int32_t* h_cnt;
    const int32_t* layer_mask;
    double* ind_inout;                         /* or NULL: no weight indicators */
    const int32_t* ind_ptr;
    const int32_t* ind_pos;
    double prior_ind1;                         /* npBNN._prior_ind1 */
    int32_t has_indicator_prior;               /* npBNN._freq_indicator > 0 */
    int32_t reserved_;
    double* find_inout;                        /* or NULL: no feature indicators */
    const double* feature_means;
    const int32_t* find_ptr;
    const int32_t* find_pos;
    const int32_t* find_use;
} npbnn_general_cfg;
int npbnn_chain_run_general(npbnn_ctx* ctx, const npbnn_chain_cfg* cfg, const npbnn_general_cfg* gcfg, double* W_inout,
                            const double* mask_packed, int32_t K, const double* log_u, uint8_t* out_accepted,
                            double* out_loglik_prop, double* out_logprior_prop, npbnn_chain_result* result);

/* ---- stand-alone operators on host arrays (float64): the reference's call-surface helpers when user code calls them on an
 * explicit matrix instead of through the sampler.  Each call uploads, runs one device kernel and downloads.
 *   npbnn_op_activation  relu_f / leaky_relu_f / swish_f / tanh_f (BNN_lib.py:50-66); kind 4 = SoftPlus (:170-172); in place
 *   npbnn_op_output      SoftMax / RegressTransformError on the rows of a matrix (BNN_lib.py:166-182); in place; ind < 0: cols/2
 *   npbnn_op_likelihood  calc_likelihood* (BNN_lib.py:100-143) and the BNN_lik.py plug-ins on a prediction matrix
 *   npbnn_op_confusion   argmax predictions -> [true][predicted] counts and predicted-class counts
 *                        (CalcAccuracy / CalcLabelAccuracy / CalcLabelFreq, BNN_lib.py:203-233)
 *   npbnn_op_sse         per-column sum of squared errors, link 0 identity / 1 exp / 2 10^x
 *                        (CalcAccuracyRegression, CalcLabelAccuracyRegression BNN_lib.py:195-201; *_acc BNN_lik.py:81-99) */
int npbnn_op_activation(int device, int kind, double prm, double* inout, int64_t n);
int npbnn_op_output(int device, int out_kind, double* inout, int64_t rows, int32_t cols, int32_t ind);
int npbnn_op_likelihood(int device, int lik_kind, const double* pred, int64_t rows, int32_t cols, const int64_t* labels,
                        const double* targets, int32_t k, const double* inst_w, const double* class_w, int32_t n_class_w,
                        double lik_temp, const double* sigma, double* out);
int npbnn_op_confusion(int device, const double* pred, int64_t rows, int32_t cols, const int64_t* labels, int64_t* conf,
                       int64_t* pred_counts);
int npbnn_op_sse(int device, const double* pred, const double* targets, int64_t rows, int32_t cols_pred, int32_t k, int link,
                 double* out_per_col);

/* npbnn_op_hpd: calcHPD (np_bnn/BNN_lib.py:286-302) of each of n_cols columns, column c's n_samples values at
 * values[s * col_stride + c] (value_type NPBNN_VALUE_F64 or NPBNN_VALUE_F32; window widths are computed in that type, as upstream
 * computes them in the type of its input).  out_lo / out_hi [n_cols]: the bounds of the first narrowest window holding
 * nIn = round(level * n_samples) sorted values (round half to even).  NPBNN_E_ARG: more than 16384 samples, level outside (0, 1),
 * nIn < 2, or a value that is NaN or infinite. */
#define NPBNN_VALUE_F64 0
#define NPBNN_VALUE_F32 1
int npbnn_op_hpd(int device, const void* values, int value_type, int64_t n_samples, int64_t n_cols, int64_t col_stride, double level,
                 double* out_lo, double* out_hi);

/* npbnn_op_psis: PSIS-LOO of each of n_cols columns of log-likelihoods, column i's n_samples = S values ll_s at
 * values[s * col_stride + i] (value_type NPBNN_VALUE_F64 or NPBNN_VALUE_F32), 2 <= S <= 16384, every value finite.  All arithmetic
 * is float64.  Per column:
 *   x_s   = -ll_s - max_t(-ll_t)                              (log importance ratios, the largest 0)
 *   M     = ceil(min(S / 5, 3 sqrt(S)));   cut = max((M + 1)-th largest x, log(DBL_MIN));   ecut = exp(cut)
 *   tail  = the x_s > cut (strictly), ascending x_(1) <= ... <= x_(n); n may be below M under ties, or 0
 *   n <= 4:  k = +inf and every log weight lw_s = x_s (plain importance sampling)
 *   n >  4:  t_j = exp(x_(j)) - ecut; (k, sigma) = gpdfit(t); the j-th smallest tail value gets
 *            lw = min(log(sigma * expm1(-k * log1p(-p_j)) / k + ecut), 0), p_j = (j - 0.5) / n (k == 0: -sigma * log1p(-p_j) for the
 *            quotient); lw_s = x_s outside the tail
 *   elpd_loo_i = logsumexp_s(lw_s + ll_s) - logsumexp_s(lw_s)  (each with its maximum taken out first)
 *   lppd_i     = logsumexp_s(ll_s) - log S
 * gpdfit is Zhang and Stephens (2009) with the weakly informative prior of loo / ArviZ, on t ascending of length n:
 *   m = 30 + floor(sqrt(n));  b_q = (1 - sqrt(m / (q - 0.5))) / (3 t[floor(n / 4 + 0.5) - 1]) + 1 / t[n - 1], q = 1..m
 *   k_q = mean_j log1p(-b_q t_j);  L_q = n (log(-b_q / k_q) - k_q - 1);  w_q = 1 / sum_r exp(L_r - L_q)
 *   the q with w_q >= 10 * 2^-52 are kept and renormalised;  b = sum_q b_q w_q;  k' = mean_j log1p(-b t_j)
 *   sigma = -k' / b;  k = (n k' + 5) / (n + 10)
 * out_elpd, out_lppd, out_k [n_cols].  The bits of a column's results depend on its values alone.  NPBNN_E_ARG: S outside the
 * limits, or a value that is NaN or infinite.  n_cols == 0 returns at once. */
int npbnn_op_psis(int device, const void* values, int value_type, int64_t n_samples, int64_t n_cols, int64_t col_stride, double* out_elpd,
                  double* out_lppd, double* out_k);

/* npbnn_op_convergence: split R-hat and effective sample size of each of n_cols columns, column c's values at
 * values[s * col_stride + c] (value_type NPBNN_VALUE_F64 or NPBNN_VALUE_F32).  All arithmetic is float64.  A column is M = n_chains
 * chains of N = n_draws draws each, chain-major: sample s = j * N + t; 1 <= M <= 64, N >= 8, M * N <= 16384.  Each chain is split
 * into halves of n = N / 2 draws (rounded down), t in [0, n) and t in [N - n, N): the middle draw of an odd N is dropped; m = 2 M
 * split chains.  For each split chain k:
 *   mu_k = (1/n) sum x          d = x - mu_k          acov_k(t) = (1/n) sum_{i < n - t} d_i d_{i+t}          s2_k = acov_k(0) n / (n - 1)
 * (two passes, mean then centred sums: never the one-pass sum-of-squares form).  Over the split chains:
 *   W = mean_k s2_k       Bn = sum_k (mu_k - mean mu)^2 / (m - 1)       varp = W (n - 1) / n + Bn       rhat = sqrt(varp / W)
 *   rho(0) = 1            rho(t) = 1 - (W - mean_k acov_k(t)) / varp
 * Effective sample size: P_0 = rho(0) + rho(1); for k = 1, 2, ... while 2k + 1 <= n - 1: P_k = rho(2k) + rho(2k + 1), stop at the
 * first P_k < 0 (that pair is not added), otherwise P_k = min(P_k, P_{k-1}) is added;
 *   tau = max(-1 + 2 sum P_k, 1 / log10(m n))          ess = m n / tau
 * No rank normalisation, no tail ESS, no lag cap.  out_rhat / out_ess [n_cols].  A column with W == 0 (every split chain constant)
 * has rhat = ess = NaN; this is not an error.  NPBNN_E_ARG: the limits above, or a value that is NaN or infinite. */
int npbnn_op_convergence(int device, const void* values, int value_type, int32_t n_chains, int32_t n_draws, int64_t n_cols,
                         int64_t col_stride, double* out_rhat, double* out_ess);

/* npbnn_op_mixture: quantiles, mean and continuous ranked probability score of n_cols Gaussian mixtures.  Cell c has n_samples = S
 * components, 1 <= S <= 16384, mu_s at mu[s * col_stride + c] (value_type NPBNN_VALUE_F64 or NPBNN_VALUE_F32) and sigma_s
 *   sigma_cols == 0       at sigma[s * col_stride + c], sigma of mu's type and layout
 *   sigma_cols == T >= 1  at sigma[s * T + c % T], sigma float64 [n_samples][T]: the per-sample sigma of the Gaussian likelihood
 * every mu finite and every sigma positive and finite.  All arithmetic is float64:
 *   F(x)       = (1/S) sum_s Phi((x - mu_s) / sigma_s),  Phi(u) = 0.5 erfc(-u / sqrt 2)
 *   quantile_p = the x with F(x) = p (F is continuous and strictly increasing: x is unique)
 *   mean       = K + (1/S) sum_s (mu_s - K), K = mu_1 (as npbnn_predict_sets_calibration forms it)
 *   A(m, v)    = 2 sqrt(v) phi(m / sqrt v) + m erf(m / sqrt(2 v))      (= E|N(m, v)|; both terms are >= 0)
 *   crps(y)    = (1/S) sum_s A(y - mu_s, sigma_s^2)
 *                - (1/(2 S^2)) [sum_s 2 sigma_s / sqrt(pi) + 2 sum_{s<t} A(mu_s - mu_t, sigma_s^2 + sigma_t^2)]
 * The quantile is a safeguarded Newton search (bisection whenever a Newton step leaves the bracket) from the bracket of the
 * components' own p-quantiles, widened while an end is on the wrong side, run until the bracket cannot narrow or 200 passes over S are
 * spent; for p > 0.5 on the upper tail, sum erfc(+u) against 1 - p.  The end of the last bracket with the smaller residual is returned: with
 * delta = (S + 8) 2^-53, |F(q) - p| <= 4 delta max(p, 1 - p) or q lies within 4 ulp of the root (F may pass the first bound within
 * one ulp of x).  The CRPS costs S (S - 1) / 2 pair terms per cell; with T1 and T2 / 2 its two non-negative parts,
 * |crps - exact| <= (64 + ceil(S (S - 1) / 128)) 2^-53 (T1 + T2 / 2).  The bits of a cell's result depend on its values and on S alone.
 *   probs [n_probs]   n_probs in 0..16, each with min(p, 1 - p) >= 1e-12, in any order
 *   out_quantile      [n_probs][n_cols]; NULL exactly when n_probs == 0
 *   out_mean          [n_cols], or NULL
 *   y, out_crps       [n_cols] both, or both NULL; y finite
 * NPBNN_E_ARG, before the device is touched: more than 16384 samples, more than 16 probabilities or one out of range, nothing asked
 * for, y without out_crps or the reverse, a mu or y that is NaN or infinite, a sigma that is not positive and finite. */
int npbnn_op_mixture(int device, const void* mu, const void* sigma, int value_type, int64_t n_samples, int64_t n_cols, int64_t col_stride,
                     int32_t sigma_cols, const double* probs, int32_t n_probs, const double* y, double* out_quantile, double* out_mean,
                     double* out_crps);

/* ---- MC3 temperature-swap exchange over RCCL (xGMI inside a node): replaces the multiprocessing pool
 * round trip of whole pickled chains in MC3.run_mcmc (np_bnn/BNN_mc3.py:94-112), of which the swap
 * decision only reads two scalars per chain.  One communicator per process / GPU; host buffers in and out.
 * Errors are reported through npbnn_last_error(NULL). */
typedef struct npbnn_comm npbnn_comm;
int npbnn_comm_unique_id(char out[128]);                                  /* rank 0; ship the bytes to every rank */
int npbnn_comm_init(int device_id, int rank, int nranks, const char id[128], npbnn_comm** out);
int npbnn_comm_allgather_f64(npbnn_comm* comm, const double* send, int count, double* recv /* nranks*count */);
int npbnn_comm_bcast_i64(npbnn_comm* comm, int64_t* buf, int count, int root);
void npbnn_comm_destroy(npbnn_comm* comm);
/* Which RCCL does this process run?  runtime_version: ncclGetVersion() of the library that is mapped (e.g. 22707), header_version:
 * NCCL_VERSION_CODE of the rccl.h this library was compiled against, path: the file the mapped library came from.
 * npbnn_comm_init refuses to start when the two differ in major.minor (a process that loaded another librccl.so.1 first - the one
 * bundled with a PyTorch wheel - would otherwise run this library's calls on it).  (No reference counterpart: BNN_mc3.py has no
 * communication library.) */
int npbnn_comm_runtime(int* runtime_version, int* header_version, char* path, int path_cap);
/* hipDeviceSynchronize on `device_id`: everything enqueued on that GPU by this process has completed (bench.py brackets its timed
 * region with it, next to a barrier of the communicator). */
int npbnn_device_synchronize(int device_id);

/* ---- one chain over several GPUs: the ROWS of the training matrix split over the processes of `comm` (rank r holds a contiguous
 * share as its ordinary training set), every process running the same chain from the same draws.  The reference evaluates the
 * likelihood of a proposal as one sum over all rows (np_bnn/BNN_lib.py:100-143 called from MCMC.mh_step, BNN_env.py:467-491); here a
 * pass leaves one record of partial sums per candidate on every rank (log-likelihood sum or residual moments), the records are
 * all-gathered - ncclAllGather on the chain's stream, kMaxCand x 33 doubles per rank - and every rank adds them in RANK ORDER and
 * takes the same decision: the chains stay bit-identical without another word between the ranks.  n_rows_total replaces the local
 * row count wherever the likelihood needs N (the empirical sigma of a regression).  After this call npbnn_chain_run runs on kernel
 * boundaries (NPBNN_SCHED_SERIAL: pass, gather, step) whatever schedule is asked for; npbnn_eval / npbnn_predict keep returning the
 * LOCAL rows' sums (the host adds what it needs across ranks: npbnn_amd/rowshard.py).  npbnn_chain_run_general, the batched and the
 * exchange runs refuse a sharded context.
 *   comm != NULL: the gather is enqueued on the stream (RCCL).  comm == NULL, gather != NULL: host-staged - the record comes to the
 *   host, gather(user, send, recv, count) must fill recv[n_ranks][count] (rank order) and return 0, the result goes back; the form
 *   the CPU-launched rehearsals use (processes that share one GPU cannot form an RCCL communicator).  n_ranks == 1: no gather.
 *   n_ranks == 0 switches sharding off. */
typedef int (*npbnn_gather_fn)(void* user, const double* send, double* recv, int32_t count);
int npbnn_set_row_shard(npbnn_ctx* ctx, npbnn_comm* comm, npbnn_gather_fn gather, void* user, int32_t rank, int32_t n_ranks,
                        int64_t n_rows_total);

/* ---- exchange run: the chains of an MC3 run (np_bnn/BNN_mc3.py:87-126) advance n_seg swap intervals of seg_len iterations with
 * the temperature swaps between them done on the GPU: replaces n_seg rounds of  pool.map(run_single_mcmc) -> read
 * [logPost, temperature] of every chain -> swap the temperatures of chains j, k when
 *   (logPost_k - logPost_j) * T_j + (logPost_j - logPost_k) * T_k >= log u           (BNN_mc3.py:99-112)
 * Everything is enqueued on the chains' streams: after the launches of a segment every chain writes its record, the records
 * are all-gathered in place (RCCL on the stream when `comm` spans several processes; chains of this process meet through
 * events), every chain applies the decision to its own temperature and starts the next segment.  No host round trip per
 * segment.  The swap proposals (swap_j, swap_k: chain ids; swap_logu) are pre-drawn by the caller from the stream the
 * reference's parent process draws from, identically on every rank.
 *   chain i lives on rank i % nranks as job i / nranks of that rank; n_chains = nranks * n_jobs; K = n_seg * seg_len rows per job.
 * The number of passes a segment needs is only known on the device; each segment is given launch_slack (1.25 if <= 0) times
 * the expected number.  If some chain has not finished a segment when it is exchanged (or stopped before an fp16 overflow), every
 * chain on every rank sees it in the records and stops at that exchange: *out_segments_done < n_seg, each job's
 * result->iterations_done says how far its chain got (its state and outputs are valid up to there), and the caller
 * finishes that segment with npbnn_chain_run and a host-side swap.
 * Failures between ranks: what can fail on one rank alone (its draws, its weights, its memory) is checked before anything is
 * enqueued, and the ranks agree on the outcome through one host-side all-gather of `comm` - on an error every rank returns one
 * (the failing rank its own, the others NPBNN_E_COMM) with nothing of the run in flight.  An error after that point (a launch or
 * a collective that fails in the middle of the run) aborts `comm` on the failing rank, so that its peers' pending collectives end
 * with an error instead of pairing with unrelated ones: the handle is dead afterwards (every call on it returns NPBNN_E_COMM);
 * destroy it and start again with a new one.
 *   out_records[s][i] = {logPost, temperature (before swap s), 1.0 if chain i had finished segment s, iterations done}
 *   job.out_state[s]  = {logLik, logPrior, temperature, iterations done, sigma[NPBNN_MAX_TARGETS]} of the chain after exchange s
 *                       (NPBNN_XSTATE_DOUBLES per exchange; sigma = the regression error parameter, BNN_env.py:500-501, which the
 *                       logger writes with the cold chain's row, :611-612)
 *   job.out_cold_w[s] = its weights at exchange s if it is the cold chain (temperature 1) afterwards (the logger's sample,
 *                       BNN_mc3.py:118-122); untouched otherwise */
typedef struct {
    npbnn_ctx* ctx;
    const npbnn_chain_cfg* cfg;
    double* W_inout;
    const double* mask_packed;
    int32_t M, chain_id;
    const int32_t* idx;
    const double* delta;
    const int32_t* cnt;
    const double* log_u;
    uint8_t* out_accepted;
    double* out_loglik_prop;                   /* or NULL */
    double* out_logprior_prop;                 /* or NULL */
    double* out_state;                         /* [n_seg][NPBNN_XSTATE_DOUBLES] or NULL */
    double* out_cold_w;                        /* [n_seg][n_weights] or NULL */
    npbnn_chain_result* result;
} npbnn_chain_job;
int npbnn_chains_run_exchange(npbnn_comm* comm /* NULL: the chains of this process only */, npbnn_chain_job* jobs, int32_t n_jobs,
                              int32_t n_chains, int32_t seg_len, int32_t n_seg, const int32_t* swap_j, const int32_t* swap_k,
                              const double* swap_logu, double launch_slack, double* out_records /* [n_seg][n_chains][4] */,
                              int32_t* out_segments_done);

/* ---- group pass: 2 or 3 chains of one model (the per-chain replicas MC3 makes, np_bnn/BNN_mc3.py:55-75: same data, same network)
 * that live on ONE GPU advance K iterations each, every launch evaluating one proposal PER CHAIN against a single streaming
 * read of the feature matrix: replaces n_jobs calls of MCMC.mh_step per iteration, each with its own copy of and pass over X
 * (BNN_mc3.py:80-85 through a pool of processes).  Candidate slot j of a launch belongs to chain j - its committed weight image
 * patched with its own pre-drawn perturbation - and its sums go to that chain's step, which runs in a workgroup of its own inside
 * the same launch while the next proposals are evaluated (the overlapped schedule of npbnn_chain_run, one candidate per chain:
 * a chain that accepts loses the one proposal that was in flight).  Every slot does useful work whatever the acceptance rate,
 * where a single chain's speculative candidates are wasted after its first accept of a pass.  Each chain is exactly the chain
 * npbnn_chain_run gives it (same decisions; its log-likelihood sums are formed from a different number of workgroup partials, so
 * they may differ in the last bits).  The jobs are filled in as for npbnn_chains_run_exchange (chain_id, out_state, out_cold_w
 * unused); the contexts must share their feature matrix (npbnn_share_data) and have the same architecture, mask and likelihood.
 * NPBNN_E_ARG when n_jobs weight images do not fit the LDS of a compute unit together; NPBNN_E_RANGE as npbnn_chain_run. */
int npbnn_chains_run_batched(npbnn_chain_job* jobs, int32_t n_jobs, int32_t K);

/* timing hook for a speculative chain pass: the evaluation kernel with n_candidates weight sets (0 = as many as fit),
 * `iters` back-to-back launches between one pair of HIP events on the ctx stream; mean milliseconds per launch */
int npbnn_time_pass(npbnn_ctx* ctx, const double* W_packed, int n_candidates, int iters, double* ms_kernel, int* used_candidates);

/* timing hook for the weight-streamed path (NPBNN_INFO_WIDE): `iters` back-to-back passes between one pair of HIP events - ms_pass:
 * all of a pass's launches (the layers' products, the likelihood kernel); ms_layer0: the first layer's product alone (with the
 * reduction of its K-slices, when it is cut into any) - the contraction over the feature matrix, the kernel the matrix cores'
 * roofline is quoted for.  info[0..3]: rows x outputs of a workgroup's block of that product, its K-slices, its workgroups.
 * NPBNN_E_STATE when the architecture set last runs on the LDS-resident path. */
int npbnn_time_wide(npbnn_ctx* ctx, const double* W_packed, int iters, double* ms_layer0, double* ms_pass, int* info);

/* page-locked host memory for the per-batch inputs of npbnn_chain_run (idx / delta / cnt / log_u): arrays drawn straight into
 * such memory are uploaded asynchronously at link speed instead of through the driver's bounce buffer.  (The reference has no
 * counterpart: its draws never leave the host, np_bnn/BNN_mcmc.py:57-69.) */
int npbnn_pinned_alloc(size_t bytes, void** out);
void npbnn_pinned_free(void* ptr);

#ifdef __cplusplus
}
#endif
#endif /* NPBNN_HIP_H */
