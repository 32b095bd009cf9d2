/*
 * npbnn_attrib_plan.h — the work plan of the attribution entries (npbnn_predict_pdp, npbnn_predict_ale, npbnn_predict_saliency,
 * npbnn_predict_shapley) as arithmetic on plain numbers: route 1's envelope and block shapes (npbnn_attrib_route_of), and per entry
 * how a job is cut into groups of prepared sets, launches of sets and chunks of rows, outputs or grid points under its byte budgets,
 * with the element count of every device buffer that cut needs (npbnn_attrib_sal_of, npbnn_attrib_shap_of, npbnn_attrib_pdp_g_chunk,
 * npbnn_attrib_ale_of), and the cut of npbnn_loglik_grad's table into chunks of rows (npbnn_attrib_grad_of: it runs on saliency's
 * route-2 blocks; tests/test_host_grad_plan.py).  Nothing here touches the GPU, the environment or a context: the entries read those, fill a request, allocate
 * by the plan's counts and loop by the plan's numbers.  Plain C, so that the host library (npbnn_host.c) exports the same rule the HIP
 * library runs by, for the CPU tests of it (tests/test_host_attrib_plan.py).
 */
#ifndef NPBNN_ATTRIB_PLAN_H
#define NPBNN_ATTRIB_PLAN_H

#include <limits.h>

#include "npbnn_resident_plan.h"   /* NPBNN_PLAN_FN, kMaxLayers */

static const int kPdpRows = 256;                       /* rows of a workgroup of route 1's kernels (one per thread) */
static const int kPdpTail = 32;                        /* widest later layer (and output) route 1 takes */
static const int kPdpMaxH0 = 64;                       /* widest first layer route 1 takes */
static const long long kPdpW0Lds = 64 * 1024;          /* LDS bytes for one set's first-layer weights (Fp x H0P floats) */
static const long long kPdpTailLds = 32 * 1024;        /* LDS bytes for the later layers of the sets of one launch */
static const int kSalWaveRows = 256;                   /* rows a wave of sal_fold_kernel folds: eight tiles of 32 */
static const int kShapWavesPerCu = 8;                  /* waves the splits of the walks aim at, per compute unit */

NPBNN_PLAN_FN int attrib_round_up(int v, int m) { return (v + m - 1) / m * m; }
NPBNN_PLAN_FN long long attrib_min(long long a, long long b) { return a < b ? a : b; }
NPBNN_PLAN_FN long long attrib_max(long long a, long long b) { return a > b ? a : b; }
/* a count that a budget of `bytes` holds at `each` bytes apiece, between 1 and `all` */
NPBNN_PLAN_FN long long attrib_fit(long long bytes, long long each, long long all) { return attrib_max(1, attrib_min(all, bytes / attrib_max(each, 1))); }

/* ---- route 1: the envelope and the float32 blocks of a set ----------------------------------------------------------------- */

/* what pdp_prep_kernel turns a set's float64 weights into */
typedef struct PdpPrep {
    int F, Fp, H0, H0P, hb0, n_layers, n_grid, wn, tail_floats;
    int l_in[NPBNN_MAX_LAYERS], l_out[NPBNN_MAX_LAYERS], l_hb[NPBNN_MAX_LAYERS], l_woff[NPBNN_MAX_LAYERS], t_inp[NPBNN_MAX_LAYERS],
        t_off[NPBNN_MAX_LAYERS];
} PdpPrep;

enum { NPBNN_ATTRIB_PDP = 0, NPBNN_ATTRIB_SALIENCY = 1, NPBNN_ATTRIB_SHAPLEY = 2 };   /* (partial dependence and ALE plan alike) */

typedef struct npbnn_attrib_route_req {
    const npbnn_arch* arch;
    int n_weights;       /* packed weights of a set */
    int Fp;              /* floats of a row of the table on the device */
    int n_points;        /* shifted biases per set: grid points, bin edges, or 1 */
    int streamed;        /* the library streams this network's weights by itself */
    int route1_off;      /* the entry's environment switch forces route 2 */
    int entry;           /* NPBNN_ATTRIB_* */
} npbnn_attrib_route_req;

typedef struct npbnn_attrib_route {
    PdpPrep q;
    int fits;            /* the network is inside route 1's envelope (include/npbnn_hip.h) and route 1 is not switched off */
    int route;           /* 1 or 2 */
    int H0P;             /* floats of a row of layer 0's blocks.  Route 1: 32 or 64.  Saliency's and Shapley's route 2 read the same
                            blocks at H0 rounded up to 32; partial dependence's and ALE's route 2 read none */
    int NS;              /* sets of a launch whose layer-0 sums a thread keeps in registers (NS H0P = 64 floats); 1 on saliency's route 2 */
    int sum_w, max_w;    /* the layers' widths added, and the widest */
    long long set_bytes; /* a set's float32 blocks: first layer, one bias point, later layers, slopes */
    long long lds_bytes; /* dynamic LDS of a route-1 launch of NS sets: one first-layer image and the sets' later layers */
} npbnn_attrib_route;

static inline void npbnn_attrib_route_of(const npbnn_attrib_route_req* n, npbnn_attrib_route* r) {
    const npbnn_arch* a = n->arch;
    const int F = a->in_dim, L = a->n_layers, H0 = a->out_dim[0];
    PdpPrep* q = &r->q;
    int woff, toff = 0;
    r->H0P = H0 <= 32 ? 32 : 64;
    r->NS = 64 / r->H0P;
    r->fits = !n->streamed && !n->route1_off && H0 <= kPdpMaxH0 && (long long)n->Fp * r->H0P * 4 <= kPdpW0Lds;
    q->F = F; q->Fp = n->Fp; q->H0 = H0; q->hb0 = a->has_bias[0]; q->n_layers = L; q->n_grid = n->n_points; q->wn = n->n_weights;
    woff = H0 * (F + q->hb0);
    r->sum_w = r->max_w = H0;
    for (int l = 1; l < L; ++l) {
        q->l_in[l] = a->out_dim[l - 1];
        q->l_out[l] = a->out_dim[l];
        q->l_hb[l] = a->has_bias[l];
        q->l_woff[l] = woff;
        woff += q->l_out[l] * (q->l_in[l] + q->l_hb[l]);
        q->t_inp[l] = attrib_round_up(q->l_in[l], 8);
        q->t_off[l] = toff;
        toff += attrib_round_up(q->l_out[l], 4) + q->l_out[l] * q->t_inp[l];
        if (q->l_out[l] > kPdpTail) r->fits = 0;
        r->sum_w += q->l_out[l];
        r->max_w = (int)attrib_max(r->max_w, q->l_out[l]);
    }
    q->tail_floats = toff;
    if (L == 1 && H0 > kPdpTail) r->fits = 0;
    if ((long long)r->NS * q->tail_floats * 4 > kPdpTailLds) r->fits = 0;
    r->route = r->fits ? 1 : 2;
    if (r->route == 2 && n->entry != NPBNN_ATTRIB_PDP) {
        r->H0P = attrib_round_up(H0, 32);
        if (n->entry == NPBNN_ATTRIB_SALIENCY) r->NS = 1;
    }
    q->H0P = r->H0P;
    r->set_bytes = ((long long)n->Fp * r->H0P + (long long)n->n_points * r->H0P + q->tail_floats + kMaxLayers) * 4;
    r->lds_bytes = ((long long)n->Fp * r->H0P + (long long)r->NS * q->tail_floats) * 4;
}

/* sets whose blocks are prepared at a time: more are prepared group after group, into the same buffers */
NPBNN_PLAN_FN int npbnn_attrib_prep_sets(long long set_bytes, int n_sets, long long prep_bytes) { return (int)attrib_fit(prep_bytes, set_bytes, n_sets); }

/* ---- saliency ------------------------------------------------------------------------------------------------------------ */

typedef struct npbnn_attrib_sal_req {
    const npbnn_attrib_route* r;
    int C, F;
    long long n_rows;
    int n_sets;
    long long scratch_bytes;   /* D, the partials and phase 1's scratches */
    long long prep_bytes;      /* the float32 blocks */
} npbnn_attrib_sal_req;

typedef struct npbnn_attrib_sal {
    int rows_cap;        /* rows of a chunk: a multiple of 256 */
    int n_c;             /* outputs of a launch (route 1: all of them) */
    int n_slot_cap;      /* waves of sal_fold_kernel per (set, output) of a launch */
    int pairs_cap;       /* (set, output) pairs of a launch */
    int prep_sets;
    int Fq;              /* F rounded up to phase 2's feature tiles of 32 */
    int a_off[NPBNN_MAX_LAYERS];   /* route 2: layer l's first unit in the activation and factor scratches */
    long long row_fixed, row_pair; /* scratch bytes per row of a chunk: independent of the launch's pairs, and per pair */
    long long n_D, n_part, n_fac, n_act, n_g;   /* elements of the buffers (D, fac, act, g float; part double) */
    long long lds_bytes; /* route 1's dynamic LDS */
} npbnn_attrib_sal;

static inline void npbnn_attrib_sal_of(const npbnn_attrib_sal_req* s, npbnn_attrib_sal* p) {
    const npbnn_attrib_route* r = s->r;
    const int L = r->q.n_layers, C = s->C;
    long long rows_cap;
    const long long rows_all = (s->n_rows + kSalWaveRows - 1) / kSalWaveRows * kSalWaveRows;
    p->Fq = attrib_round_up(s->F, 32);
    /* Scratch bytes per row of a chunk: what does not depend on the outputs of a launch (route 1: the later layers' factors; route 2:
     * activations, factors and two gradients), and per (set, output) of a launch D's H0P floats and the row's share of a wave's partials */
    p->row_fixed = r->route == 1 ? (long long)L * kPdpTail * 4 : (long long)(2 * r->sum_w + 2 * r->max_w) * 4;
    p->row_pair = (long long)r->H0P * 4 + (3 * (long long)p->Fq * 8 + kSalWaveRows - 1) / kSalWaveRows;
    p->n_c = C;
    rows_cap = s->scratch_bytes / (p->row_fixed + (long long)r->NS * C * p->row_pair) / kSalWaveRows * kSalWaveRows;
    if (rows_cap < kSalWaveRows) {
        rows_cap = kSalWaveRows;
        if (r->route == 2) {                               /* (route 1's pairs of a launch are 64 at most: they stay together) */
            const long long per_row = s->scratch_bytes / kSalWaveRows;
            p->n_c = (int)attrib_max(1, attrib_min(C, per_row > p->row_fixed ? (per_row - p->row_fixed) / p->row_pair : 0));
        }
    }
    rows_cap = attrib_min(attrib_min(rows_cap, rows_all), 1ll << 24);      /* (a chunk's row indices are ints) */
    p->rows_cap = (int)rows_cap;
    p->n_slot_cap = (int)(rows_cap / kSalWaveRows);
    p->pairs_cap = r->NS * p->n_c;
    p->prep_sets = npbnn_attrib_prep_sets(r->set_bytes, s->n_sets, s->prep_bytes);
    for (int l = 0, off = 0; l < L; ++l) {
        p->a_off[l] = off;
        off += l == 0 ? r->q.H0 : r->q.l_out[l];
    }
    p->n_D = (long long)p->pairs_cap * rows_cap * r->H0P;
    p->n_part = (long long)p->pairs_cap * p->n_slot_cap * 3 * p->Fq;
    p->n_fac = r->route == 1 ? rows_cap * L * kPdpTail : rows_cap * r->sum_w;
    p->n_act = r->route == 1 ? 0 : rows_cap * r->sum_w;
    p->n_g = r->route == 1 ? 0 : rows_cap * 2 * r->max_w;
    p->lds_bytes = r->lds_bytes;
}

/* ---- weight gradient of the log-likelihood (npbnn_loglik_grad) ------------------------------------------------------------- */

static const int kGradSlotRows = 256;                  /* rows whose products are added in float32: a workgroup of phase 1, a wave of phase 2 */
static const int kGradLikTerms = 1 + 2 * NPBNN_MAX_TARGETS;   /* per slot: the log-likelihood terms, then every target's sum_r and sum_r2 */

typedef struct npbnn_attrib_grad_req {
    const npbnn_attrib_route* r;   /* the plan of saliency's route 2: one set, one bias point */
    int n_weights;
    long long n_rows;
    long long scratch_bytes;       /* phase 1's scratches and the partials */
} npbnn_attrib_grad_req;

typedef struct npbnn_attrib_grad {
    int rows_cap;        /* rows of a chunk: a multiple of kGradSlotRows */
    int n_slot_cap;      /* slots of a chunk */
    int n_chunks;
    int n_tot;           /* doubles of a slot's partials: the packed weights, layer 0's H0P bias sums, kGradLikTerms */
    int bsum_off, lik_off;         /* where the last two start in a slot's partials */
    int a_off[NPBNN_MAX_LAYERS];   /* layer l's first unit in the scratches [unit][row] */
    long long row_bytes;           /* scratch bytes per row of a chunk, its share of a slot's partials included */
    long long n_act, n_fac, n_dl, n_D0, n_part, n_acc;   /* elements of the buffers (act, fac, dl, D0 float; part, acc double) */
} npbnn_attrib_grad;

static inline void npbnn_attrib_grad_of(const npbnn_attrib_grad_req* s, npbnn_attrib_grad* p) {
    const npbnn_attrib_route* r = s->r;
    const int L = r->q.n_layers;
    long long rows_cap;
    const long long rows_all = (s->n_rows + kGradSlotRows - 1) / kGradSlotRows * kGradSlotRows;
    p->bsum_off = s->n_weights;
    p->lik_off = s->n_weights + r->H0P;
    p->n_tot = p->lik_off + kGradLikTerms;
    /* per row: every unit's value, derivative factor and delta, layer 0's delta once more row-major, and 1 / 256 of a slot's partials */
    p->row_bytes = ((long long)3 * r->sum_w + r->H0P) * 4 + ((long long)p->n_tot * 8 + kGradSlotRows - 1) / kGradSlotRows;
    rows_cap = s->scratch_bytes / p->row_bytes / kGradSlotRows * kGradSlotRows;
    rows_cap = attrib_min(attrib_min(attrib_max(rows_cap, kGradSlotRows), rows_all), 1ll << 24);   /* (a chunk's row indices are ints) */
    p->rows_cap = (int)rows_cap;
    p->n_slot_cap = (int)(rows_cap / kGradSlotRows);
    p->n_chunks = (int)((s->n_rows + rows_cap - 1) / rows_cap);
    for (int l = 0, off = 0; l < L; ++l) {
        p->a_off[l] = off;
        off += l == 0 ? r->q.H0 : r->q.l_out[l];
    }
    p->n_act = p->n_fac = p->n_dl = rows_cap * r->sum_w;
    p->n_D0 = rows_cap * r->H0P;
    p->n_part = (long long)p->n_slot_cap * p->n_tot;
    p->n_acc = p->n_tot;
}

/* ---- Shapley ------------------------------------------------------------------------------------------------------------- */

enum { NPBNN_ATTRIB_OK = 0, NPBNN_ATTRIB_E_PHI = 1, NPBNN_ATTRIB_E_WALKS = 2 };

typedef struct npbnn_attrib_shap_req {
    const npbnn_attrib_route* r;
    int C, P, n_explain, n_bg, n_perm, n_sets, n_cu;
    int want_phi;              /* the caller asks for every set's phi */
    long long scratch_bytes;   /* the walks' partials (and route 2's scratches) */
    long long prep_bytes;      /* the float32 blocks */
    long long phi_bytes;       /* every set's phi on the device */
} npbnn_attrib_shap_req;

typedef struct npbnn_attrib_shap {
    int refusal;         /* NPBNN_ATTRIB_E_PHI: phi is over its budget, phi_rows_fit explained rows would fit; NPBNN_ATTRIB_E_WALKS:
                            `walks` are more than INT_MAX.  Nothing else is filled in then */
    long long phi_rows_fit, walks;
    int W;               /* walks per explained row and set: n_bg n_perm */
    int n_split;         /* waves that share the walks of a block of 64 rows */
    int rb_cap;          /* blocks of 64 explained rows of a chunk */
    int nsl;             /* sets of a launch */
    int e_cap, b_cap;    /* rows the transposed explained and background rows have room for */
    int prep_sets;
    int bg_blocks, ex_blocks;   /* workgroups of a direct launch over the background rows, and over a chunk at most */
    long long unit_bytes;       /* a unit - one wave of the walk kernel - in partials and, on route 2, scratch */
    long long scr_unit;         /* route 2: floats of a unit's scratch */
    long long scr_units;        /* route 2: the units of the larger of a walk launch and a direct launch */
    long long n_xeT, n_xbT, n_z0b, n_fx, n_fb, n_part, n_mean, n_abs, n_phi, n_scr;   /* elements of the buffers */
    long long lds_bytes;        /* route 1's dynamic LDS: one set's first-layer image and later layers */
} npbnn_attrib_shap;

static inline int npbnn_attrib_shap_of(const npbnn_attrib_shap_req* s, npbnn_attrib_shap* p) {
    const npbnn_attrib_route* r = s->r;
    const long long PC = (long long)s->P * s->C, E = s->n_explain;
    long long max_units, n_rb_all, want;
    p->refusal = NPBNN_ATTRIB_OK;
    p->phi_rows_fit = 0;
    p->walks = (long long)s->n_bg * s->n_perm;
    if (s->want_phi) {
        p->phi_rows_fit = s->phi_bytes / (s->n_sets * PC * 8);
        if (E > p->phi_rows_fit) return p->refusal = NPBNN_ATTRIB_E_PHI;
    }
    if (p->walks > INT_MAX) return p->refusal = NPBNN_ATTRIB_E_WALKS;
    p->W = (int)p->walks;
    /* A unit is one wave of the walk kernel: 64 rows x one split of the W walks.  Its partials take PC x 64 doubles, on route 2 its
     * scratch (H0 + 2 max_w + C) x 64 floats more.  The splits aim at kShapWavesPerCu waves per compute unit over all the sets and
     * rows; the budget then bounds the row blocks of a chunk, and the sets of a launch. */
    p->scr_unit = r->route == 2 ? (long long)(r->q.H0 + 2 * r->max_w + s->C) * 64 : 0;
    p->unit_bytes = PC * 64 * 8 + p->scr_unit * 4;
    max_units = attrib_max(1, s->scratch_bytes / p->unit_bytes);
    n_rb_all = (E + 63) / 64;
    want = (long long)kShapWavesPerCu * s->n_cu / (n_rb_all * s->n_sets);
    p->n_split = (int)attrib_max(1, attrib_min(attrib_min(p->walks, want), max_units));
    p->rb_cap = (int)attrib_max(1, attrib_min(attrib_min(n_rb_all, max_units / p->n_split), 1 << 16));
    /* (a launch's sets are its grid's second dimension) */
    p->nsl = (int)attrib_max(1, attrib_min(attrib_min(s->n_sets, max_units / ((long long)p->n_split * p->rb_cap)), 65535));
    p->e_cap = p->rb_cap * 64;
    p->b_cap = attrib_round_up(s->n_bg, 64);
    p->bg_blocks = (s->n_bg + 255) / 256;
    p->ex_blocks = (p->e_cap + 255) / 256;
    p->prep_sets = npbnn_attrib_prep_sets(r->set_bytes, s->n_sets, s->prep_bytes);
    /* route 2's scratch units: a walk launch's nsl x rb_cap x n_split waves, a direct launch's nsl x 4 x workgroups */
    p->scr_units = p->nsl * attrib_max((long long)p->rb_cap * p->n_split, 4 * attrib_max(p->bg_blocks, p->ex_blocks));
    p->n_xeT = (long long)r->q.Fp * p->e_cap;
    p->n_xbT = (long long)r->q.Fp * p->b_cap;
    p->n_z0b = (long long)p->prep_sets * s->n_bg * r->H0P;
    p->n_fx = s->n_sets * E * s->C;
    p->n_fb = (long long)s->n_sets * s->n_bg * s->C;
    p->n_part = (long long)p->nsl * p->rb_cap * p->n_split * PC * 64;
    p->n_mean = 2 * PC * E;
    p->n_abs = s->n_sets * PC;
    p->n_phi = s->want_phi ? s->n_sets * PC * E : 0;
    p->n_scr = r->route == 2 ? p->scr_units * p->scr_unit : 0;
    p->lds_bytes = ((long long)r->q.Fp * r->H0P + r->q.tail_floats) * 4;
    return NPBNN_ATTRIB_OK;
}

/* ---- partial dependence and accumulated local effects ---------------------------------------------------------------------- */

/* grid points whose float32 accumulator [grid points][rows][outputs] a budget holds: larger grids run in chunks of grid points,
 * each chunk one more read of X per group of sets */
NPBNN_PLAN_FN int npbnn_attrib_pdp_g_chunk(int n_grid, long long n_rows, int C, long long acc_bytes) {
    return (int)attrib_fit(acc_bytes, n_rows * C * 4, n_grid);
}

typedef struct npbnn_attrib_ale {
    int n_wg;            /* workgroups of 256 rows the table takes */
    int wg_chunk;        /* ... and of a launch: the per-workgroup partials [sets of a launch][workgroups][bins][outputs] float64 are
                            held to a budget */
    int stride;          /* floats between two rows' differences in LDS (odd: the rows' writes fall into different banks) */
    int stage_floats;    /* LDS floats before the tails: the first-layer image, later the differences and the rows' bins */
    long long n_part;    /* doubles of the partials; route 2's: [sets of a pass][workgroups][2][outputs] */
    long long lds_bytes; /* dynamic LDS of ale_kernel */
} npbnn_attrib_ale;

static inline void npbnn_attrib_ale_of(const npbnn_attrib_route* r, int K, int C, long long n_rows, long long part_bytes, npbnn_attrib_ale* a) {
    a->n_wg = (int)((n_rows + kPdpRows - 1) / kPdpRows);
    a->stride = C | 1;
    a->stage_floats = (int)attrib_max(r->q.Fp * r->H0P, kPdpRows * (a->stride + 1));
    a->wg_chunk = (int)attrib_fit(part_bytes, (long long)r->NS * K * C * 8, a->n_wg);
    a->n_part = r->route == 1 ? (long long)a->wg_chunk * r->NS * K * C : (long long)kMaxCand * a->n_wg * 2 * C;
    a->lds_bytes = ((long long)a->stage_floats + (long long)r->NS * r->q.tail_floats) * 4;
}

#endif
