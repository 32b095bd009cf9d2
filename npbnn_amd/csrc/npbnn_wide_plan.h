/*
 * npbnn_wide_plan.h — the launch arithmetic of the weight-streamed path that sizes device buffers: which tiling a layer's product
 * takes (cfg_for in npbnn_wide.hip) and into how many K-slices its contraction is cut (slices_for), and from those the floats the
 * K-slices' sums of a pass over a table need (npbnn_wide_slice_room).  Plain C, so that the host library (npbnn_host.c) exports the
 * same rule the HIP library plans and launches by: wide_plan sizes the slice buffer with it, wide_forward checks every launch
 * against what it sized.
 */
#ifndef NPBNN_WIDE_PLAN_H
#define NPBNN_WIDE_PLAN_H

#include <stdlib.h>

#define NPBNN_WIDE_N_CFG 6
#define NPBNN_WIDE_MAX_SLICES 8        /* K-slices a layer's contraction is cut into at most */

/* row tiles / output tiles of a workgroup's block per tiling (the xt, wt of npbnn_wide.hip's g_cfg, in its order) */
static const int npbnn_wide_cfg_xt[NPBNN_WIDE_N_CFG] = {16, 16, 16, 8, 8, 16};
static const int npbnn_wide_cfg_wt[NPBNN_WIDE_N_CFG] = {16, 8, 4, 4, 2, 16};

/* the tiling of a layer of `mt` 16-output tiles on `n_row_tiles` 16-row tiles: by its width; tables of few rows take the 128-row
 * blocks (more workgroups).  NPBNN_WIDE_CFG=<index> forces one. */
static inline int npbnn_wide_cfg_index(int mt, int n_row_tiles, int n_cu) {
    const char* e = getenv("NPBNN_WIDE_CFG");
    if (e) { const int v = atoi(e); if (v >= 0 && v < NPBNN_WIDE_N_CFG) return v; }
    if (mt > 8) return 0;
    if (mt > 4) return 1;
    if (mt > 2) return (n_row_tiles + 15) / 16 < n_cu / 2 ? 3 : 2;
    return 4;
}

/* K-slices of a layer's product on tiling `cfg`: while the blocks of the output do not fill the chip and a slice keeps a contraction
 * worth its prologue (`units`: 32-wide K-units).  NPBNN_WIDE_SLICES=<n> forces a count, within 1..min(8, units). */
static inline int npbnn_wide_slices(int cfg, int n_row_tiles, int mt, int units, int n_cu) {
    const int xt = npbnn_wide_cfg_xt[cfg], wt = npbnn_wide_cfg_wt[cfg];
    const int n_rb = (n_row_tiles + xt - 1) / xt, n_cb = (mt + wt - 1) / wt;
    int n_sl = 1;
    const char* e = getenv("NPBNN_WIDE_SLICES");
    if (e) n_sl = atoi(e);
    else while (n_sl < NPBNN_WIDE_MAX_SLICES && n_rb * n_cb * (n_sl + 1) <= n_cu && units / (n_sl + 1) >= 8) ++n_sl;
    if (n_sl > NPBNN_WIDE_MAX_SLICES) n_sl = NPBNN_WIDE_MAX_SLICES;
    if (n_sl > units) n_sl = units;
    if (n_sl < 1) n_sl = 1;
    return n_sl;
}

/* floats of the K-slices' sums a pass of the network (`n_layers` layers of out_dim[l] nodes behind in_dim features) over a table of
 * n_rows rows needs: the most any layer cut into more than one slice writes, slices x [16 row tiles][16 mt] (0: no layer is cut).
 * (Counts every layer, also those a pass leaves to the fused end or the tail kernel: room to spare, never too little.) */
static inline long long npbnn_wide_slice_room(int n_layers, const int* out_dim, int in_dim, long long n_rows, int n_cu) {
    const long long n_row_tiles = (n_rows + 15) / 16;
    long long room = 0;
    int in = in_dim;
    for (int l = 0; l < n_layers; ++l) {
        const int mt = (out_dim[l] + 15) / 16, units = (in + 31) / 32;
        const int cfg = npbnn_wide_cfg_index(mt, (int)n_row_tiles, n_cu);
        const int n_sl = npbnn_wide_slices(cfg, (int)n_row_tiles, mt, units, n_cu);
        const long long r = n_sl > 1 ? n_sl * n_row_tiles * 16 * (16ll * mt) : 0;
        if (r > room) room = r;
        in = out_dim[l];
    }
    return room;
}

#endif
