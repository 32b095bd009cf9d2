/*
 * npbnn_stack_plan.h — the tile rule of the column kernels over a sample stack [S][n_cols] (npbnn_hpd.hip, npbnn_convergence.hip,
 * npbnn_predictive.hip; launch_stack_kernel, npbnn_stack.hip.h) as arithmetic on plain numbers: a workgroup of kStackThreads threads
 * takes a tile of adjacent columns (or cells) into LDS.  Nothing here touches the GPU, the environment or a context.  Plain C, so
 * that the host library (npbnn_host.c) exports the rule the HIP library launches by, for the CPU tests of it
 * (tests/test_host_stack_plan.py).
 */
#ifndef NPBNN_STACK_PLAN_H
#define NPBNN_STACK_PLAN_H

#include "npbnn_resident_plan.h"   /* NPBNN_PLAN_FN */

static const int kStackThreads = 256, kStackWaves = 256 / 64;
static const int kStackMaxSamples = 16384;
static const int kStackMaxTile = 64;                   /* columns of a workgroup at most */
static const long long kStackTileLds = 80 * 1024;      /* LDS a tile may take when it holds more than one column (two per CU) */
static const long long kMixMaxLds = 160 * 1024;        /* a single staged column may take the whole LDS */

typedef struct npbnn_stack_tile {
    int tile, log2tile;  /* columns of a workgroup, a power of two */
    long long lds_bytes; /* dynamic LDS of a launch; 0 when the tile is not staged */
    long long blocks;    /* workgroups: n_cols / tile, rounded up */
    int staged;          /* the tile goes into LDS (0: one column over max_col_bytes, read from where it lies) */
} npbnn_stack_tile;

/* col_bytes: one column (or cell, all its planes) as it is staged, pitch included; max_col_bytes: the most a single column may take.
 * The tile doubles while twice the columns stay within kStackMaxTile, within kStackTileLds bytes and within the columns there are. */
NPBNN_PLAN_FN npbnn_stack_tile npbnn_stack_tile_of(long long col_bytes, long long n_cols, long long max_col_bytes) {
    npbnn_stack_tile t = {1, 0, 0, 0, 0};
    for (; t.tile < kStackMaxTile && 2 * t.tile * col_bytes <= kStackTileLds && 2 * t.tile <= n_cols; t.tile *= 2) ++t.log2tile;
    t.staged = t.tile * col_bytes <= max_col_bytes;      /* (a tile of more than one column is within kStackTileLds) */
    t.lds_bytes = t.staged ? t.tile * col_bytes : 0;
    t.blocks = (n_cols + t.tile - 1) / t.tile;
    return t;
}

#endif
