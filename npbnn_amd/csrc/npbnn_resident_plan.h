/*
 * npbnn_resident_plan.h — the LDS-resident path as arithmetic on plain numbers: the bounds its kernels are built for, where a
 * network's weights sit in the LDS image (npbnn_resident_layout_of, npbnn_resident_pos), how many bytes the choice between the two
 * paths holds against a compute unit's LDS (npbnn_resident_path_bytes), and how a pass is launched (npbnn_resident_launch_of).
 * Nothing here touches the GPU, the environment or a context: the callers (build_net, rebuild_net, plan_launch and npbnn_get_info of
 * npbnn_capi.hip, wide_needed of npbnn_wide.hip) read those and fill a request.  Plain C, so that the host library (npbnn_host.c)
 * exports the same rule the HIP library runs by, for the CPU tests of it (tests/test_host_resident_plan.py).
 */
#ifndef NPBNN_RESIDENT_PLAN_H
#define NPBNN_RESIDENT_PLAN_H

#include "npbnn_hip.h"

/* the build bounds are constant expressions in the HIP units (__launch_bounds__(max_waves_for(...))) and plain functions under gcc */
#ifdef __HIPCC__
#define NPBNN_PLAN_FN __host__ __device__ constexpr
#else
#define NPBNN_PLAN_FN static inline
#endif

/* ---- the build bounds ------------------------------------------------------------------------------------------------------ */

#ifndef NPBNN_RING
#define NPBNN_RING 4
#endif
#ifndef NPBNN_FAST3_WAVES
#define NPBNN_FAST3_WAVES 12
#endif
#define NPBNN_RESIDENT_MAX_MT 8                /* (an array bound below: kMaxMT) */
static const int kMaxLayers = NPBNN_MAX_LAYERS;
/* The LDS-resident path (eval_kernel) holds layers of up to kResidentMaxWidth nodes; wider ones - up to NPBNN_MAX_WIDTH - run on the
 * weight-streamed path (npbnn_wide.hip.h), as does any network whose image does not fit a compute unit's LDS. */
static const int kResidentMaxWidth = 16 * NPBNN_RESIDENT_MAX_MT;
static const int kMaxMT = NPBNN_RESIDENT_MAX_MT;   /* 16-unit tiles per layer of the resident path */
static const int kRing = NPBNN_RING;               /* X ring slots (1 KiB each) per wave; kRing-1 pieces stay in flight */
static const int kMaxCand = 3;                     /* candidates evaluated per pass over X by a speculative chain */
static const int kFastMaxMT0 = 4;                  /* fast builds exist for layer 0 of up to 16 * kFastMaxMT0 nodes */
static const int kFastLayers = 3;                  /* networks of up to this many layers have shape-specialised tails */
/* The fast Gaussian builds are for <= kFastGaussTargets target columns (every BASELINE regression shape: 1 or 2): all of them
 * belong to the lanes of the first quarter (kq = 0) and the moments of columns 2 and 3 of a lane, 8 float64 registers per
 * candidate that the general build carries through the whole kernel, are never touched. */
static const int kFastGaussTargets = 2;
/* likelihood class a build's epilogue is for (eval_kernel, LK) */
static const int kLikCat = 0, kLikGauss = 1, kLikGen = 2;

/* Per-wave row-aux slots (labels / instance weights / targets of a 16-row tile, fetched ahead of the tile's X pieces).  Their
 * number and size depend on the data set and the network: the host lays them out (WaveLayout) and hands the numbers to the
 * kernel, so that nothing is reserved that a run does not use - at config 2 this is what lets a 13th wave fit the LDS. */
typedef struct WaveLayout {
    int aux_slots;   /* 2 when the ring never holds pieces of more than the next tile, else 4 (a power of two) */
    int aux_sz;      /* bytes per slot */
    int off_w;       /* instance weights inside a slot (labels, when present, sit at 0) */
    int off_t;       /* targets inside a slot */
    int wave_lds;    /* bytes of LDS per wave: ring + slots (+ row scratch of the float64 row-wise likelihoods) */
} WaveLayout;
/* likelihoods that combine several outputs of one row (predicted sigma, count data) exchange them through 1 KiB of LDS */
NPBNN_PLAN_FN int lik_needs_row_scratch(int lik_kind) {
    return lik_kind >= NPBNN_LIK_GAUSS_PRED_SIGMA && lik_kind <= NPBNN_LIK_NEGBIN_BASE10;
}
NPBNN_PLAN_FN int lik_class(int lik_kind) {
    return lik_needs_row_scratch(lik_kind) ? kLikGen : (lik_kind == NPBNN_LIK_GAUSS ? kLikGauss : kLikCat);
}
NPBNN_PLAN_FN WaveLayout make_wave_layout(int labels, int inst_w, int k_targets, int kt0, int lik_kind) {
    WaveLayout L = {0, 0, 0, 0, 0};
    L.off_w = labels ? 64 : 0;
    L.off_t = L.off_w + (inst_w ? 64 : 0);
    L.aux_sz = L.off_t + 64 * k_targets;
    L.aux_slots = kt0 >= kRing ? 2 : 4;
    L.wave_lds = kRing * 1024 + L.aux_slots * L.aux_sz + (lik_needs_row_scratch(lik_kind) ? 1024 : 0);
    return L;
}
/* software-pipelined layer 0 (the fragments of K-step s+1 are read from LDS while the MFMAs of step s run): builds whose two
 * fragment sets fit the register budget of their launch bounds
 * (two candidates: one tile - or, in the fast builds of dense first layers, three and four: 158 registers, nothing spilled, the
 * reference's default [50, 5] +3-5 %; with two tiles the second fragment set does not fit, nor in the other builds of three and more) */
NPBNN_PLAN_FN int pipelined_l0(int mt0, int mti, int f16, int d, int fast_dense) {
    return f16 && mti == 1 && ((d == 3 && mt0 <= 2) || (d == 2 && (mt0 <= 1 || (fast_dense && (mt0 == 3 || mt0 == 4)))) || (d == 1 && mt0 <= 2));
}
/* candidates per pass a layer-0 width is built for: three sets of accumulators and tails side by side spill INSIDE the tile loop from
 * three output tiles on (tools/check_hot_loop_spills.sh; measured on 100k x 64, hidden [50, 5]: 30.3 us for three candidates
 * against 18.1 us for two, chain 65-81 k against 91 k it/s) - the launch rule asks for no more, and no such build is instantiated */
NPBNN_PLAN_FN int max_cand_for(int mt0) { return mt0 <= 2 ? 3 : 2; }
/* waves per workgroup a build is compiled for: more candidates keep more accumulators and weight fragments alive.  The
 * three-candidate categorical build of the narrow networks (the chain kernel of config 2) fits 128 VGPRs, i.e. 13 waves:
 * with 24-25 tiles per workgroup that is two rounds of tiles per wave instead of three for some.
 * The fast three-candidate builds take 12 (three per SIMD, 168 registers): with all three tails unrolled side by side 128 spill. */
NPBNN_PLAN_FN int max_waves_for(int mt0, int mti, int f16, int d, int lk, int fast) {
    return mti != 1 ? 8 : d == 1 ? 16 : d == 2 ? (fast ? 12 : 14) : fast ? (NPBNN_FAST3_WAVES) : (lk == kLikCat && pipelined_l0(mt0, mti, f16, d, 0)) ? 13 : 11;
}

/* ---- the image layout ------------------------------------------------------------------------------------------------------ */

typedef struct LayerMeta {
    int kt;        /* 16-wide k tiles of the input dimension */
    int mt;        /* 16-wide tiles of the output dimension */
    int frag_off;  /* float offset of the fragment block in the image */
    int bias_off;  /* float offset of the padded bias (16*mt floats) */
    int in_dim, out_dim, has_bias;
    int w_off;     /* double offset of the layer matrix in the packed weights */
    /* Narrow hidden layers (one output tile, not the last layer): unit u sits at position 4 (u % 4) + u / 4 of the tile instead of u
     * (tile_pos).  A lane (row n, k-group kq) holds positions 4 kq + i in register i, and the next layer's i-th float32 MFMA contracts
     * the positions {i, 4 + i, 8 + i, 12 + i}: with the units transposed like this the first ceil(out / 4) registers hold all of them,
     * and the next layer skips the MFMAs of the others - they would multiply the zeros of the padding (in_live of that layer). */
    int out_perm;  /* this layer's units are placed like that */
    int in_live;   /* float32 MFMAs per input tile this layer needs (4 unless the layer before it has out_perm) */
} LayerMeta;
NPBNN_PLAN_FN int tile_pos(int u) { return 4 * (u & 3) + (u >> 2); }      /* (its own inverse: a 4 x 4 transpose) */
/* where layer-0 unit o sits in an image of `rows` units per tile (NetMeta::l0_rows) */
NPBNN_PLAN_FN int l0_pos_of_unit(int o, int rows) { return (o / rows) * 16 + o % rows; }
/* Image positions (ChainParams::pos).  Bit 31: an fp16-split entry - the low bits are the index of the high part in 2-byte halves, the
 * low part 512 halves behind it, or, with kPosCompact (bit 30), 32 * l0_rows halves.  kSkipPos: no position (outside the block structure) */
static const int kPosCompact = 0x40000000;
static const int kSkipPos = 0x7fffffff;

typedef struct npbnn_resident_req {
    const npbnn_arch* arch;
    int f16;                           /* layer 0 on the fp16-split path */
    const unsigned char* l0_blocks;    /* npbnn_set_layer_mask: [layer-0 tiles][ceil(in_dim / 16)], nonzero where the mask holds anything; NULL: dense */
    int has_classw;                    /* class weights ride in the image */
    int slopes_option;                 /* NPBNN_OPT_TRAINABLE_SLOPES: a slot per hidden layer for the candidates' activation slopes */
    int no_pad_mask, no_l1_f16, no_tile_perm, no_compact_rows;      /* the A/B switches NPBNN_NO_PAD_MASK ... are set */
} npbnn_resident_req;

typedef struct npbnn_resident_layout {
    int n_layers, l0_f16;
    int lik_kind, k_targets, final_act;      /* (of the request: what the launch rule reads besides the layout) */
    LayerMeta L[NPBNN_MAX_LAYERS];
    int l0_begin[NPBNN_RESIDENT_MAX_MT], l0_end[NPBNN_RESIDENT_MAX_MT], l0_base[NPBNN_RESIDENT_MAX_MT];   /* NetMeta's, as the rest */
    int l0_rows, l1_f16, pad_masked, classw_off, slope_off;
    int block_floats;                  /* the layers' fragment and bias blocks alone, before the optional slots */
    int image_floats, n_weights;
} npbnn_resident_layout;

enum { NPBNN_RESIDENT_OK = 0, NPBNN_RESIDENT_E_ARG = -1,
       NPBNN_RESIDENT_NOT_HELD = 1,    /* a layer wider than kResidentMaxWidth, or blocks past 2^28 floats: the weight-streamed path's */
       NPBNN_RESIDENT_NO_FIT = 2,      /* launch rule: the image and one wave do not fit the LDS */
       NPBNN_RESIDENT_FEW_WAVES = 3 }; /* launch rule: fewer than four waves beside the image */

/* The image of the network `r` describes.  (Kinds and target counts are npbnn_set_arch's to check; here only what the arithmetic needs.) */
static inline int npbnn_resident_layout_of(const npbnn_resident_req* r, npbnn_resident_layout* y) {
    const npbnn_arch* a = r ? r->arch : 0;
    if (!a || !y || a->n_layers < 1 || a->n_layers > NPBNN_MAX_LAYERS || a->in_dim < 1) return NPBNN_RESIDENT_E_ARG;
    for (int l = 0; l < a->n_layers; ++l) if (a->out_dim[l] < 1) return NPBNN_RESIDENT_E_ARG;
    for (int l = 0; l < a->n_layers; ++l) if (a->out_dim[l] > kResidentMaxWidth) return NPBNN_RESIDENT_NOT_HELD;
    const int f16 = r->f16 ? 1 : 0, dense = r->l0_blocks == 0;
    y->n_layers = a->n_layers;
    y->l0_f16 = f16;
    y->lik_kind = a->lik_kind;
    y->k_targets = a->n_targets;
    y->final_act = a->final_act ? 1 : 0;
    /* softmax / categorical heads: padding outputs are masked through their bias (see NetMeta::pad_masked) */
    y->pad_masked = (!y->final_act && (a->out_kind == NPBNN_OUT_SOFTMAX || a->lik_kind == NPBNN_LIK_CATEGORICAL) && !r->no_pad_mask) ? 1 : 0;
    {   /* layer 1 on fp16-split products (NetMeta::l1_f16) */
        int narrow_later = a->n_layers >= 2;
        for (int l = 1; l < a->n_layers; ++l) narrow_later = narrow_later && a->out_dim[l] <= 16;
        y->l1_f16 = (f16 && narrow_later && a->act_kind == NPBNN_ACT_TANH && a->out_dim[0] > 16 && !a->final_act && !r->no_l1_f16) ? 1 : 0;
    }
    long long off = 0, woff = 0;
    int in = a->in_dim;
    y->l0_rows = 16;
    for (int l = 0; l < a->n_layers; ++l) {
        const int out = a->out_dim[l];
        LayerMeta* L = &y->L[l];
        L->in_dim = in;
        L->out_dim = out;
        L->has_bias = a->has_bias[l] ? 1 : 0;
        L->kt = (l == 0 && f16) ? 2 * ((in + 31) / 32) : (in + 15) / 16;   /* 1-KiB pieces (16 rows x 64 B) per tile */
        L->mt = (out + 15) / 16;
        L->frag_off = (int)off;
        L->bias_off = 0;
        L->out_perm = (l >= 1 && l + 1 < a->n_layers && L->mt == 1 && !r->no_tile_perm) ? 1 : 0;
        L->in_live = (l >= 1 && y->L[l - 1].out_perm) ? (y->L[l - 1].out_dim + 3) / 4 : 4;
        if (l == 0) {
            /* K-units of the layer-0 loop (32 features on the fp16-split path, 16 on the float32 one); per output tile the hull of
             * the units in which the mask has anything (the whole layer when no structure was declared) */
            const int g16 = (in + 15) / 16, per_unit = f16 ? 2 : 1, units = f16 ? (in + 31) / 32 : g16;
            long long slots = 0;
            for (int mt = 0; mt < kMaxMT; ++mt) { y->l0_begin[mt] = 0; y->l0_end[mt] = 0; y->l0_base[mt] = 0; }
            for (int mt = 0; mt < L->mt; ++mt) {
                int b = 0, e = units;
                if (!dense) {
                    b = units; e = 0;
                    for (int g = 0; g < g16; ++g)
                        if (r->l0_blocks[(size_t)mt * g16 + g]) { const int u = g / per_unit; if (u < b) b = u; if (u + 1 > e) e = u + 1; }
                    if (e <= b) { b = 0; e = 0; }
                }
                y->l0_begin[mt] = b; y->l0_end[mt] = e; y->l0_base[mt] = (int)slots;
                slots += e - b;
            }
            /* rows per tile in the image (NetMeta::l0_rows): a dense fp16-split first layer of three or more tiles whose width is not a
             * multiple of 16 is stored without its padding rows (the builds for one and two tiles - every BASELINE shape - keep 16)
             * (never a network of one matrix: its first layer's positions are the outputs' - the predictions and the likelihood read
             * output c at position c, and there is no layer 1 whose weights could meet the moved units.  Until this was excluded, one
             * matrix of 33 or more outputs, not a multiple of 16, gave its outputs in the image's order: found by the partial-dependence
             * envelope test's 33-output case on route 2, wrong by 0.2 in a probability) */
            if (f16 && dense && a->n_layers >= 2 && L->mt >= 3 && out % 16 != 0 && !r->no_compact_rows)
                y->l0_rows = (out + L->mt - 1) / L->mt;
            off += slots * (f16 ? 32 * y->l0_rows : 256);
        } else if (l == 1 && y->l1_f16) {
            off += ((y->L[0].mt + 1) / 2) * 512;      /* a high and a low block of 256 floats per K-step */
        } else {
            off += (long long)L->kt * L->mt * 256;
        }
        L->w_off = (int)woff;
        woff += (long long)out * (in + L->has_bias);
        in = out;
        if (off >= (1ll << 28) || woff >= (1ll << 31)) return NPBNN_RESIDENT_NOT_HELD;
    }
    for (int l = 0; l < a->n_layers; ++l) {
        y->L[l].bias_off = (int)off;
        off += 16 * y->L[l].mt;
    }
    y->block_floats = (int)off;
    y->classw_off = -1;
    if (r->has_classw) {                /* class weights ride in the image only when there are any */
        y->classw_off = (int)off;
        off += kResidentMaxWidth;
    }
    y->slope_off = -1;
    if (r->slopes_option) {             /* a slot per hidden layer for the candidates' activation slopes (filled in LDS by a chain pass) */
        y->slope_off = (int)off;
        off += kMaxLayers;
    }
    y->image_floats = (int)((off + 63) / 64 * 64);   /* a multiple of 256 B (the LDS copies of several candidates sit back to back) */
    y->n_weights = (int)woff;
    return NPBNN_RESIDENT_OK;
}

/* Where packed weight (layer l, output o, column j of its row: column 0 is the bias where the layer has one) lives in the image: the
 * bias slot, its MFMA fragment slot, or kSkipPos outside the block structure (such a weight is always 0).  *scale_col: on the
 * fp16-split layer 0 the input column whose scale the entry is stored under, else -1. */
static inline int npbnn_resident_pos(const npbnn_resident_layout* y, int l, int o, int j, int* scale_col) {
    const LayerMeta* L = &y->L[l];
    const int in_perm = l >= 1 && y->L[l - 1].out_perm;      /* (a permuted layer has a single tile: o, c < 16) */
    const int rows = y->l0_rows;                             /* (layer 0's units per tile in this image) */
    *scale_col = -1;
    if (L->has_bias && j == 0) return L->bias_off + (L->out_perm ? tile_pos(o) : (l == 0 && rows < 16) ? l0_pos_of_unit(o, rows) : o);
    int c = in_perm ? tile_pos(j - L->has_bias) : j - L->has_bias;
    if (l == 1 && rows < 16) c = l0_pos_of_unit(c, rows);    /* (the position layer 0 leaves that unit at) */
    int mt = o / 16;
    const int u = L->out_perm ? tile_pos(o) : o % 16;
    if (l == 0 && y->l0_f16) {
        mt = o / rows;
        const int ur = o % rows, ks = c / 32, kg = (c % 32) / 8, jj = c % 8;
        *scale_col = c;
        if (ks < y->l0_begin[mt] || ks >= y->l0_end[mt]) return kSkipPos;
        const int slot = y->l0_base[mt] + ks - y->l0_begin[mt];
        const int half_index = 2 * L->frag_off + ((slot * 2) * (4 * rows) + kg * rows + ur) * 8 + jj;
        return (int)(0x80000000u | (rows < 16 ? (unsigned)kPosCompact : 0u) | (unsigned)half_index);
    }
    const int kt = c / 16, kq = (c % 16) / 4, sidx = c % 4;
    if (l == 0) {
        if (kt < y->l0_begin[mt] || kt >= y->l0_end[mt]) return kSkipPos;
        return L->frag_off + ((y->l0_base[mt] + kt - y->l0_begin[mt]) * 64 + kq * 16 + u) * 4 + sidx;
    }
    if (l == 1 && y->l1_f16) {          /* (layer 0 is not permuted: c is the unit; scale stays 1) */
        const int q = kt / 2, e = 4 * (kt & 1) + sidx;
        return (int)(0x80000000u | (unsigned)(2 * L->frag_off + ((q * 2) * 64 + kq * 16 + u) * 8 + e));
    }
    return L->frag_off + ((kt * L->mt + mt) * 64 + kq * 16 + u) * 4 + sidx;
}

/* What the choice between the two paths (wide_needed) holds against a compute unit's LDS: bytes of one candidate's layer blocks, class
 * weights where there are any, kMaxLayers + 64 floats for the slopes slot and the rounding, `waves` waves whose table is taken to have
 * labels and row weights, and the flag word. */
static inline long long npbnn_resident_path_bytes(const npbnn_resident_layout* y, int has_classw, int waves) {
    const long long floats = (long long)y->block_floats + (has_classw ? kResidentMaxWidth : 0) + kMaxLayers + 64;
    return floats * 4 + (long long)waves * make_wave_layout(1, 1, y->k_targets, y->L[0].kt, y->lik_kind).wave_lds + 64;
}

/* ---- the launch plan ------------------------------------------------------------------------------------------------------- */

typedef struct npbnn_resident_launch_req {
    int has_labels, has_row_w, has_targets, n_tiles;      /* what the table has */
    int n_cu, lds_limit, want_cand;
    int predict_only;      /* a predicting launch (no likelihood) */
    int lik_only;          /* the caller wants the likelihood terms and nothing else (no statistics, no predictions) */
    int plain;             /* a plain evaluation: no pass descriptor, no chain */
    int fast_option;       /* NPBNN_OPT_FAST_TAILS */
    int waves_override;    /* NPBNN_WAVES (A/B switch), 0: none */
} npbnn_resident_launch_req;

typedef struct npbnn_resident_launch {
    int refusal;           /* NPBNN_RESIDENT_OK, _NO_FIT (waves is 0) or _FEW_WAVES */
    int n_cand, waves_full, waves, grid, lds_bytes;      /* waves_full: before the thin-second-round rule and the override */
    int mti, lk, fast, blocked, want_spec;               /* the build: eval_kernel's MTI, LK and FAST; blocked: layer 0 skips something;
                                                            want_spec: the launch also wants the build with the speculative step */
    WaveLayout lay;
} npbnn_resident_launch;

/* widest later layer in tiles: 1 selects the MTI = 1 builds */
static inline int npbnn_resident_inner_tiles(const npbnn_resident_layout* y) {
    int mti = 1;
    for (int l = 1; l < y->n_layers; ++l)
        if (y->L[l].mt > mti) mti = y->L[l].mt;
    if (y->n_layers == 1) mti = y->L[0].mt;        /* the single layer's tiles are also the final tiles */
    return mti;
}
/* does layer 0 skip anything (some output tile without weights in some K-unit)? */
static inline int npbnn_resident_l0_blocked(const npbnn_resident_layout* y) {
    const int units = y->l0_f16 ? y->L[0].kt / 2 : y->L[0].kt;
    for (int mt = 0; mt < y->L[0].mt; ++mt)
        if (y->l0_begin[mt] != 0 || y->l0_end[mt] != units) return 1;
    return 0;
}
/* May a launch that wants nothing but the likelihood terms run on the fast builds (eval_kernel, FAST)?  2 or 3 layers, later
 * layers of <= 16 nodes, layer 0 of <= 16 * kFastMaxMT0, categorical (padding outputs masked through the bias) or Gaussian
 * likelihood, no row or class weights, no activation after the last layer. */
static inline int npbnn_resident_fast_ok(const npbnn_resident_layout* y, const npbnn_resident_launch_req* q) {
    const int blocked = npbnn_resident_l0_blocked(y);
    if (!q->fast_option || npbnn_resident_inner_tiles(y) != 1 || y->n_layers < 2 || y->n_layers > kFastLayers || y->L[0].mt > kFastMaxMT0) return 0;
    if (y->final_act || q->has_row_w || y->classw_off >= 0 || y->slope_off >= 0) return 0;
    if (blocked && !y->l0_f16) return 0;          /* (the fast builds for block-structured layers are fp16-split ones) */
    if (y->lik_kind == NPBNN_LIK_CATEGORICAL) return y->pad_masked != 0 && q->has_labels;
    return y->lik_kind == NPBNN_LIK_GAUSS && q->has_targets && y->k_targets <= (blocked ? 1 : kFastGaussTargets);
}

static inline int npbnn_resident_launch_of(const npbnn_resident_layout* y, const npbnn_resident_launch_req* q, npbnn_resident_launch* p) {
    if (!y || !q || !p || q->want_cand < 1 || q->n_tiles < 0 || q->n_cu < 1 || q->lds_limit < 1 || q->waves_override < 0) return NPBNN_RESIDENT_E_ARG;
    const int mt0 = y->L[0].mt, predict_only = q->predict_only != 0;
    p->mti = npbnn_resident_inner_tiles(y) == 1 ? 1 : 8;
    p->lk = predict_only ? kLikCat : lik_class(y->lik_kind);
    p->lay = make_wave_layout(q->has_labels, q->has_row_w, q->has_targets ? y->k_targets : 0, y->L[0].kt, predict_only ? NPBNN_LIK_NONE : y->lik_kind);
    p->blocked = npbnn_resident_l0_blocked(y);
    p->fast = q->lik_only && !predict_only && npbnn_resident_fast_ok(y, q);
    /* speculative passes: as many candidates as still leave >= 8 waves per workgroup (only the MTI = 1 builds have them) */
    int n_cand = (p->mti == 1 && (predict_only || !lik_needs_row_scratch(y->lik_kind))) ? q->want_cand : 1;
    if (n_cand > kMaxCand) n_cand = kMaxCand;
    if (n_cand > max_cand_for(mt0)) n_cand = max_cand_for(mt0);
    int w = 0;
    long long need = 0;
    for (;; --n_cand) {
        /* waves per block such that the fragment images + per-wave rings fit the CU's LDS, + 64: the flag word of the device-side waits */
        for (w = max_waves_for(mt0, p->mti, y->l0_f16, n_cand, p->lk, p->fast); w >= 1; --w) {      /* (from the launch bound of the build in use) */
            need = (long long)n_cand * y->image_floats * 4 + (long long)w * p->lay.wave_lds;
            if (need + 64 <= q->lds_limit) break;
        }
        if (n_cand == 1 || w >= 8) break;
    }
    p->n_cand = n_cand;
    p->waves_full = p->waves = w;
    p->want_spec = p->fast && !q->plain && !predict_only && !p->blocked && (n_cand == 1 || n_cand == 3);
    p->grid = 0;
    p->lds_bytes = 0;
    if (w == 0) return p->refusal = NPBNN_RESIDENT_NO_FIT;
    /* A thin second round of tiles: when a workgroup's share is just over one tile per wave (config 5 with three candidates: 12.25
     * tiles for 12 waves) the leftover tile runs alone after the others are through - a lone wave streams X at a ring's worth per
     * memory latency.  Two waves fewer spread the leftovers over several SIMDs and give the first round less contention: measured
     * 36.4 -> 33.4 us per pass there (9 or 10 waves; 11: 35.0, 8: 35.0, 7: 41.9); single-candidate launches and shares of two rounds
     * or more are best at the build's full count (config 2: 30.6 us at 12 waves, 31.3 at 10). */
    const double share = (double)q->n_tiles / (double)q->n_cu;
    if (n_cand > 1 && share > (double)w && share < 1.25 * (double)w && w - 2 >= 8) w -= 2;
    if (q->waves_override >= 1 && q->waves_override <= p->waves_full) w = q->waves_override;
    p->waves = w;
    /* (the tile schedule of eval_kernel needs a wave on every SIMD of the compute unit: networks that leave fewer run on the
     * weight-streamed path - wide_needed - and a data set whose row-aux slots push a launch below that is refused rather than mis-summed) */
    if (w < 4) return p->refusal = NPBNN_RESIDENT_FEW_WAVES;
    p->grid = (q->n_tiles + w - 1) / w;
    if (p->grid > q->n_cu) p->grid = q->n_cu;     /* persistent: one workgroup per CU */
    if (p->grid < 1) p->grid = 1;
    p->lds_bytes = (int)((long long)n_cand * y->image_floats * 4 + (long long)w * p->lay.wave_lds) + 64;   /* (the flag word behind the images and the rings) */
    return p->refusal = NPBNN_RESIDENT_OK;
}

#endif
