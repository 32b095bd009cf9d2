"""CPU checks of the tile rule of the column kernels over a sample stack (npbnn_amd/csrc/npbnn_stack_plan.h, exported by
libnpbnn_host.so as npbnn_host_stack_tile; hpd_kernel, convergence_kernel and the two mixture kernels size their dynamic LDS and
their grids by the same header).

The plan is held against a restatement of the rule in Python over sample counts, value widths, planes and column counts, against
the shapes the GPU suites' docstrings speak of, and against what the kernels rely on whatever the case: a power-of-two tile of at
most 64 columns, a tile of more than one column within 80 KiB, never more than the 160 KiB of LDS, one workgroup per tile.

Three columns make a tile of two and one column a tile of one at every sample count at which two columns fit the 80 KiB; past
that (a column of more than 40 KiB: S > 10239 float32 values in one plane) the LDS bound comes first and three columns are three
tiles of one, which is asserted as well."""
import ctypes as C
import itertools
import os

import pytest

from npbnn_amd import predraw

MAX_TILE, TILE_LDS, MAX_LDS = 64, 80 * 1024, 160 * 1024
SAMPLES = (1, 2, 7, 63, 64, 65, 100, 257, 512, 1000, 1023, 1024, 1025, 4096, 5000, 10239, 10240, 16383, 16384)
COLS = (1, 2, 3, 63, 64, 65, 129, 100000)


class Tile(C.Structure):
    """npbnn_stack_tile"""
    _fields_ = [("tile", C.c_int), ("log2tile", C.c_int), ("lds_bytes", C.c_longlong), ("blocks", C.c_longlong), ("staged", C.c_int)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(predraw.HOST_LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(predraw.HOST_LIB_PATH)
    lib.npbnn_host_stack_tile.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.POINTER(Tile)]
    return lib


def plan(lib, col_bytes, n_cols, max_col=MAX_LDS):
    t = Tile()
    assert lib.npbnn_host_stack_tile(col_bytes, n_cols, max_col, C.byref(t)) == 0
    return t


def rule(col_bytes, n_cols, max_col=MAX_LDS):
    """the tile loop as the three units used to write it, each for itself: (tile, lds_bytes, staged)"""
    tile = 1
    while tile < MAX_TILE and 2 * tile * col_bytes <= TILE_LDS and 2 * tile <= n_cols:
        tile *= 2
    staged = tile * col_bytes <= max_col
    return tile, tile * col_bytes if staged else 0, staged


def pitch_of(kernel, s):
    """values of a staged column: HPD pads to the next power of two, plus one; the others take S | 1"""
    return (1 << (s - 1).bit_length()) + 1 if kernel == "hpd" else s | 1


def test_plan_matches_the_rule_and_what_the_kernels_rely_on(lib):
    n = 0
    for kernel, s, width, planes, n_cols in itertools.product(("hpd", "column"), SAMPLES, (4, 8), (1, 2), COLS):
        if kernel == "hpd" and planes == 2:
            continue
        col_bytes = pitch_of(kernel, s) * width * planes
        t = plan(lib, col_bytes, n_cols)
        tile, lds, staged = rule(col_bytes, n_cols)
        case = (kernel, s, width, planes, n_cols)
        assert (t.tile, t.lds_bytes, bool(t.staged)) == (tile, lds, staged), case
        assert t.tile == 1 << t.log2tile and 1 <= t.tile <= MAX_TILE, case
        assert t.tile == 1 or t.tile * col_bytes <= TILE_LDS, case
        assert t.lds_bytes <= MAX_LDS, case
        assert bool(t.staged) == (t.lds_bytes > 0) and t.lds_bytes in (0, t.tile * col_bytes), case
        assert t.blocks == -(-n_cols // t.tile) and t.tile <= max(n_cols, 1), case
        if n_cols == 1:
            assert t.tile == 1, case
        if n_cols == 3:
            assert t.tile == (2 if 2 * col_bytes <= TILE_LDS else 1), case
        # (HPD and convergence have no unstaged route: one plane of the widest column they accept fits)
        assert planes == 2 or t.staged, case
        n += 1
    assert n == 2 * len(SAMPLES) * 2 * len(COLS) + len(SAMPLES) * 2 * len(COLS)


PINNED = [
    # kernel, value bytes, planes, S, column or cell bytes, tile, lds_bytes, staged
    ("column", 4, 1, 100, 404, 64, 64 * 404, 1),
    ("column", 8, 1, 1023, 8184, 8, 8 * 8184, 1),
    ("column", 4, 1, 512, 2052, 32, 32 * 2052, 1),
    ("column", 4, 1, 4096, 16388, 4, 4 * 16388, 1),
    ("hpd", 4, 1, 1000, 4100, 16, 65600, 1),
    ("hpd", 8, 1, 16384, 131080, 1, 131080, 1),
    ("column", 4, 2, 16384, 131080, 1, 131080, 1),
    ("column", 8, 2, 16384, 262160, 1, 0, 0),
]


@pytest.mark.parametrize("kernel,width,planes,s,col_bytes,tile,lds,staged", PINNED)
def test_pinned_shapes(lib, kernel, width, planes, s, col_bytes, tile, lds, staged):
    assert pitch_of(kernel, s) * width * planes == col_bytes
    for n_cols in (200, 100000):
        t = plan(lib, col_bytes, n_cols)
        assert (t.tile, t.log2tile, t.lds_bytes, t.staged) == (tile, tile.bit_length() - 1, lds, staged)
        assert t.blocks == -(-n_cols // tile)


def test_tiles_the_gpu_suites_speak_of(lib):
    # tests/test_hip_convergence.py: 153 columns of 100 float32 values in tiles of 64: two full, one of 25; 85 of 1023 float64 in tiles
    # of 8, the last of 5; 391 of 512 float32 in tiles of 32, the last of 7; 34 of 4096 in tiles of 4, the last of 2
    for s, width, n_cols, tile, last in ((100, 4, 153, 64, 25), (1023, 8, 85, 8, 5), (512, 4, 391, 32, 7), (4096, 4, 34, 4, 2)):
        t = plan(lib, (s | 1) * width, n_cols)
        assert (t.tile, t.blocks, n_cols - (t.blocks - 1) * t.tile) == (tile, -(-n_cols // tile), last)
    # the single-column limit is the caller's: under a smaller one the same column is not staged
    assert plan(lib, 131080, 5, 128 * 1024).staged == 0 and plan(lib, 131080, 5, 128 * 1024).lds_bytes == 0
    assert plan(lib, 8, 0).blocks == 0
    assert lib.npbnn_host_stack_tile(0, 5, MAX_LDS, C.byref(Tile())) == -1 and lib.npbnn_host_stack_tile(8, 5, MAX_LDS, None) == -1
