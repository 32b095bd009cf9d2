"""CPU checks of the LDS-resident path's host arithmetic (npbnn_amd/csrc/npbnn_resident_plan.h, exported by libnpbnn_host.so as
npbnn_host_resident_*; the HIP library lays out its weight image, places every packed weight and plans every pass by the same header).

Two wrong answers came out of this arithmetic before it could be run without a GPU: launches of one to three waves summed a quarter to
three quarters of the rows, and one-matrix networks of 33 or more outputs came back in the image's order.  The invariants below are the
ones those broke, swept over the shapes the rule distinguishes; the literal figures are the ones the project's documents state."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import test_host_eval_builds as builds
from npbnn_amd import _capi, predraw

MAX_LAYERS, MAX_MT, MAX_CAND = 8, 8, 3
LDS_LIMIT, N_CU = 163840, 256
SKIP, COMPACT, F16_BIT = 0x7fffffff, 0x40000000, 0x80000000
OK, E_ARG, NOT_HELD, NO_FIT, FEW_WAVES = 0, -1, 1, 2, 3
CAT, GAUSS, POISSON = _capi.LIK_CATEGORICAL, _capi.LIK_GAUSS, _capi.LIK_POISSON
SWITCHES = ("no_pad_mask", "no_l1_f16", "no_tile_perm", "no_compact_rows")
LAUNCH_FIELDS = ("has_labels", "has_row_w", "has_targets", "n_tiles", "n_cu", "lds_limit", "want_cand", "predict_only", "lik_only", "plain",
                 "fast_option", "waves_override")
# a chain pass on a labelled table of 6 250 tiles that asks for as many candidates as fit
LAUNCH_DEFAULT = dict(has_labels=1, has_row_w=0, has_targets=0, n_tiles=6250, n_cu=N_CU, lds_limit=LDS_LIMIT, want_cand=3, predict_only=0,
                      lik_only=1, plain=0, fast_option=1, waves_override=0)


class LayerMeta(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("kt", "mt", "frag_off", "bias_off", "in_dim", "out_dim", "has_bias", "w_off", "out_perm", "in_live")]


class Layout(C.Structure):
    """npbnn_resident_layout"""
    _fields_ = ([(n, C.c_int) for n in ("n_layers", "l0_f16", "lik_kind", "k_targets", "final_act")] + [("L", LayerMeta * MAX_LAYERS)] +
                [(n, C.c_int * MAX_MT) for n in ("l0_begin", "l0_end", "l0_base")] +
                [(n, C.c_int) for n in ("l0_rows", "l1_f16", "pad_masked", "classw_off", "slope_off", "block_floats", "image_floats", "n_weights")])


class Launch(C.Structure):
    """npbnn_resident_launch"""
    _fields_ = [(n, C.c_int) for n in ("refusal", "n_cand", "waves_full", "waves", "grid", "lds_bytes", "mti", "lk", "fast", "blocked", "want_spec",
                                       "aux_slots", "aux_sz", "off_w", "off_t", "wave_lds")]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(predraw.HOST_LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(predraw.HOST_LIB_PATH)
    i32p = C.POINTER(C.c_int32)
    lib.npbnn_host_resident_layout.argtypes = [C.POINTER(_capi.Arch), i32p, C.c_char_p, C.POINTER(Layout)]
    lib.npbnn_host_resident_map.argtypes = [C.POINTER(Layout), i32p, i32p]
    lib.npbnn_host_resident_path_bytes.argtypes = [C.POINTER(Layout), C.c_int, C.c_int]
    lib.npbnn_host_resident_path_bytes.restype = C.c_longlong
    lib.npbnn_host_resident_launch.argtypes = [C.POINTER(Layout), i32p, C.POINTER(Launch)]
    return lib


@pytest.fixture(autouse=True)
def _library_rule(monkeypatch):
    for name in list(os.environ):
        if name.startswith("NPBNN_"):
            monkeypatch.delenv(name)


def make_arch(dims, in_dim, bias=1, act=_capi.ACT_TANH, out=_capi.OUT_SOFTMAX, lik=CAT, n_targets=0, final_act=0):
    a = _capi.Arch()
    a.n_layers, a.in_dim = len(dims), in_dim
    for l, d in enumerate(dims):
        a.out_dim[l] = d
        a.has_bias[l] = bias if isinstance(bias, int) else bias[l]
    a.act_kind, a.out_kind, a.lik_kind, a.n_targets, a.final_act = act, out, lik, n_targets, final_act
    return a


def layout_of(lib, arch, f16=1, blocks=None, classw=0, slopes=0, **switches):
    """(code, Layout) of the rule; blocks: [layer-0 tiles][ceil(in_dim / 16)] array of 0 / 1, or None."""
    assert set(switches) <= set(SWITCHES)
    opts = (C.c_int32 * 7)(f16, classw, slopes, *[int(switches.get(s, 0)) for s in SWITCHES])
    y = Layout()
    raw = None if blocks is None else np.ascontiguousarray(blocks, dtype=np.uint8).tobytes()
    return lib.npbnn_host_resident_layout(C.byref(arch), opts, raw, C.byref(y)), y


def launch_of(lib, y, **kw):
    assert set(kw) <= set(LAUNCH_FIELDS), kw
    r = dict(LAUNCH_DEFAULT, **kw)
    req = (C.c_int32 * len(LAUNCH_FIELDS))(*[int(r[f]) for f in LAUNCH_FIELDS])
    p = Launch()
    rc = lib.npbnn_host_resident_launch(C.byref(y), req, C.byref(p))
    if rc != E_ARG:
        assert rc == p.refusal
    return rc, p


def map_of(lib, y):
    pos = np.zeros(y.n_weights, dtype=np.int32)
    col = np.zeros(y.n_weights, dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    assert lib.npbnn_host_resident_map(C.byref(y), pos.ctypes.data_as(i32p), col.ctypes.data_as(i32p)) == OK
    return pos.astype(np.int64) & 0xffffffff, col


def block_table(width, in_dim, n_blocks):
    """create_mask's structure as npbnn_set_layer_mask sees it: n_blocks equal runs of inputs, each wired to its share of the nodes."""
    g16, mt = (in_dim + 15) // 16, (width + 15) // 16
    per = [width // n_blocks] * n_blocks
    per[-1] += width - sum(per)
    node_block = np.repeat(np.arange(n_blocks), per)
    feat_block = np.minimum(np.arange(in_dim) // max(in_dim // n_blocks, 1), n_blocks - 1)
    t = np.zeros((mt, g16), dtype=np.uint8)
    for o in range(width):
        for g in np.unique(np.nonzero(feat_block == node_block[o])[0] // 16):
            t[o // 16, g] = 1
    return t


# ---- a. values the project states ------------------------------------------------------------------------------------------------

def test_the_default_network_on_256_features(lib):
    """[50, 5] and 7 classes: 13 rows per layer-0 tile and a 57-KB image, two candidates per pass at 10 waves; with 16 rows a 70-KB
    image and one candidate (tests/test_hip_compact_rows.py asserts the 2 on the device)."""
    a = make_arch([50, 5, 7], 256)
    rc, y = layout_of(lib, a)
    assert rc == OK and (y.l0_rows, y.image_floats, y.image_floats * 4) == (13, 14720, 58880)
    rc, p = launch_of(lib, y, n_tiles=76)
    assert rc == OK and (p.n_cand, p.waves_full) == (2, 10)
    rc, y = layout_of(lib, a, no_compact_rows=1)
    assert rc == OK and (y.l0_rows, y.image_floats) == (16, 17792)
    rc, p = launch_of(lib, y, n_tiles=76)
    assert rc == OK and p.n_cand == 1


def test_config_2(lib):
    """[32, 8, 10], tanh, 256 features, 100 000 rows on 256 compute units, fast tails, three candidates wanted."""
    rc, y = layout_of(lib, make_arch([32, 8, 10], 256))
    assert rc == OK and (y.image_floats, y.l1_f16) == (9024, 1)
    rc, p = launch_of(lib, y, n_tiles=6250)
    assert rc == OK and (p.n_cand, p.waves, p.waves_full, p.lds_bytes, p.grid, p.fast) == (3, 12, 12, 159040, 256, 1)


def test_config_5(lib):
    """512 features in 8 blocks of 64 inputs by 4 nodes, 50 000 rows: each output tile spans half the K-units; a workgroup's share is
    12.2 tiles, so the 12 waves are thinned to 10."""
    rc, y = layout_of(lib, make_arch([32, 8, 10], 512), blocks=block_table(32, 512, 8))
    assert rc == OK and (list(y.l0_begin[:2]), list(y.l0_end[:2]), list(y.l0_base[:2])) == ([0, 8], [8, 16], [0, 8])
    assert y.image_floats == 9024
    rc, p = launch_of(lib, y, n_tiles=3125)
    assert rc == OK and (p.n_cand, p.waves_full, p.waves, p.lds_bytes, p.blocked, p.fast) == (3, 12, 10, 150592, 1, 1)


@pytest.mark.parametrize("n_out", [33, 45, 50])
def test_one_matrix_networks_keep_16_rows(lib, n_out):
    rc, y = layout_of(lib, make_arch([n_out], 40))
    assert rc == OK and y.l0_rows == 16


# ---- the sweep of b and d ----------------------------------------------------------------------------------------------------------

def sweep():
    """Networks over first-layer widths 1..128: 1-4 layers, both bias settings, both layer-0 layouts, with and without a block table,
    the four switches, feature counts on both sides of 16 and 32.  Deterministic: each width takes a different corner of the rest."""
    rs = np.random.default_rng(20)
    feats = (5, 15, 16, 17, 31, 32, 33, 40, 70)
    later = (1, 3, 5, 16, 17, 33)
    out = []
    for w in range(1, 129):
        for rep in range(6):
            n_layers = 1 + (w + rep) % 4
            dims = [w] + [int(later[(w + rep + i) % len(later)]) for i in range(n_layers - 1)]
            in_dim = int(feats[(w + 2 * rep) % len(feats)])
            f16, bias = (w + rep) % 2, [int(b) for b in rs.integers(0, 2, n_layers)] if rep % 3 else rep // 3
            sw = {s: int(b) for s, b in zip(SWITCHES, rs.integers(0, 2, 4))} if rep >= 2 else {}
            blocks = None
            if rep in (1, 4):
                mt, g16 = (w + 15) // 16, (in_dim + 15) // 16
                blocks = (rs.random((mt, g16)) < 0.5).astype(np.uint8)
                blocks[rs.integers(0, mt), rs.integers(0, g16)] = 1
            act = _capi.ACT_TANH if (w + rep) % 3 else _capi.ACT_RELU
            out.append(dict(dims=dims, in_dim=in_dim, f16=f16, bias=bias, blocks=blocks, sw=sw, act=act, classw=rep == 5, slopes=rep == 3))
    return out


SWEEP = sweep()


def hull(blocks, mt, in_dim, f16):
    """Per output tile the K-units [begin, end) in which the table has anything - restated from the kernels' contract (NetMeta)."""
    units = (in_dim + 31) // 32 if f16 else (in_dim + 15) // 16
    if blocks is None:
        return [(0, units)] * mt
    out = []
    for t in range(mt):
        u = np.nonzero(blocks[t])[0] // (2 if f16 else 1)
        out.append((int(u.min()), int(u.max()) + 1) if len(u) else (0, 0))
    return out


def decode(y, l, pos, hulls):
    """(output position, column position) the kernels read a fragment entry of layer l at: how eval_kernel's lanes index the image."""
    L = y.L[l]
    if l == 0 and y.l0_f16:
        rows = y.l0_rows
        rel = (pos & 0x3fffffff) - 2 * L.frag_off
        jj, t = rel % 8, rel // 8
        ur, kg, slot = t % rows, (t // rows) % 4, t // (8 * rows)
        tile = np.searchsorted(np.array(list(y.l0_base[:L.mt]) + [10 ** 9]), slot, side="right") - 1
        # (empty tiles share their base with the next one: the last tile with that base holds the slot)
        ks = slot - np.array(y.l0_base[:L.mt])[tile] + np.array(y.l0_begin[:L.mt])[tile]
        return 16 * tile + ur, 32 * ks + 8 * kg + jj
    if l == 1 and y.l1_f16:
        rel = (pos & 0x3fffffff) - 2 * L.frag_off
        e, t = rel % 8, rel // 8
        u, kq, q = t % 16, (t // 16) % 4, t // 128
        return u, 16 * (2 * q + e // 4) + 4 * kq + e % 4
    rel = pos - L.frag_off
    sidx, t = rel % 4, rel // 4
    u, kq, blk = t % 16, (t // 16) % 4, t // 64
    if l == 0:
        tile = np.searchsorted(np.array(list(y.l0_base[:L.mt]) + [10 ** 9]), blk, side="right") - 1
        kt = blk - np.array(y.l0_base[:L.mt])[tile] + np.array(y.l0_begin[:L.mt])[tile]
        return 16 * tile + u, 16 * kt + 4 * kq + sidx
    return 16 * (blk % L.mt) + u, 16 * (blk // L.mt) + 4 * kq + sidx


def parent_path_bytes(c, waves, honour_switches=False):
    """resident_lds_bytes of npbnn_wide.hip as it stood before the rule moved into the header (it knew no switch)."""
    dims, in_dim, f16, blocks = c["dims"], c["in_dim"], c["f16"], c["blocks"]
    no_compact = honour_switches and c["sw"].get("no_compact_rows", 0)
    no_l1 = honour_switches and c["sw"].get("no_l1_f16", 0)
    l1_f16 = bool(f16 and len(dims) >= 2 and all(d <= 16 for d in dims[1:]) and c["act"] == _capi.ACT_TANH and dims[0] > 16 and not no_l1)
    off, i = 0, in_dim
    for l, o in enumerate(dims):
        mt = (o + 15) // 16
        if l == 0:
            units = (i + 31) // 32 if f16 else (i + 15) // 16
            rows = 16
            if f16 and blocks is None and len(dims) >= 2 and mt >= 3 and o % 16 and not no_compact:
                rows = (o + mt - 1) // mt
            slots = mt * units if blocks is None else sum(e - b for b, e in hull(blocks, mt, i, f16))
            off += slots * (32 * rows if f16 else 256)
        elif l == 1 and l1_f16:
            off += ((dims[0] + 15) // 16 + 1) // 2 * 512
        else:
            off += (i + 15) // 16 * mt * 256
        off += 16 * mt
        i = o
    if c["classw"]:
        off += 128
    off += MAX_LAYERS + 64
    kt0 = 2 * ((in_dim + 31) // 32) if f16 else (in_dim + 15) // 16
    ring = 4
    aux = 64 + 64                                   # labels and row weights assumed, no targets in the sweep
    wave_lds = ring * 1024 + (2 if kt0 >= ring else 4) * aux
    return off * 4 + waves * wave_lds + 64


def sweep_layout(lib, c):
    a = make_arch(c["dims"], c["in_dim"], bias=c["bias"], act=c["act"])
    rc, y = layout_of(lib, a, f16=c["f16"], blocks=c["blocks"], classw=int(c["classw"]), slopes=int(c["slopes"]), **c["sw"])
    assert rc == OK, c
    return y


# ---- b. map invariants -----------------------------------------------------------------------------------------------------------

def test_every_weight_has_its_place(lib):
    for c in SWEEP:
        y = sweep_layout(lib, c)
        dims, f16 = c["dims"], c["f16"]
        assert y.n_weights == sum(o * (i + b) for o, i, b in zip(dims, [c["in_dim"]] + dims[:-1], [y.L[l].has_bias for l in range(len(dims))]))
        assert y.block_floats <= y.image_floats and y.image_floats % 64 == 0
        pos, col = map_of(lib, y)
        hulls = hull(c["blocks"], y.L[0].mt, c["in_dim"], f16)
        assert [(y.l0_begin[t], y.l0_end[t]) for t in range(y.L[0].mt)] == hulls, c
        halves = []                                                     # every 2-byte half of the image a weight is written to
        out_pos_prev = None
        for l, o_dim in enumerate(dims):
            L = y.L[l]
            ld = L.in_dim + L.has_bias
            p = pos[L.w_off:L.w_off + o_dim * ld].reshape(o_dim, ld)
            sc = col[L.w_off:L.w_off + o_dim * ld].reshape(o_dim, ld)
            frag_end = y.L[l + 1].frag_off if l + 1 < len(dims) else y.L[0].bias_off
            if L.has_bias:
                b = p[:, 0]
                assert np.all((b >= L.bias_off) & (b < L.bias_off + 16 * L.mt)), (c, l)
                assert np.all(sc[:, 0] == -1)
                halves += [2 * b, 2 * b + 1]
            w = p[:, L.has_bias:]
            o_idx, c_idx = np.meshgrid(np.arange(o_dim), np.arange(L.in_dim), indexing="ij")
            skipped = w == SKIP
            if l == 0:
                rows = y.l0_rows if f16 else 16
                assert rows == 16 or (f16 and c["blocks"] is None and not c["sw"].get("no_compact_rows") and len(dims) >= 2 and L.mt >= 3 and o_dim % 16)
                tile, unit = o_idx // rows, c_idx // (32 if f16 else 16)
                lo, hi = np.array([h[0] for h in hulls])[tile], np.array([h[1] for h in hulls])[tile]
                assert np.array_equal(skipped, (unit < lo) | (unit >= hi)), (c, "skip positions")
                assert np.all(sc[:, L.has_bias:] == (c_idx if f16 else -1))
            else:
                assert not skipped.any() and np.all(sc == -1)
            live = w[~skipped]
            split = (live & F16_BIT) != 0
            assert live.size == 0 or (split.all() == bool((l == 0 and f16) or (l == 1 and y.l1_f16)) and (split.all() or not split.any())), (c, l)
            if split.any():
                assert np.all(((live & COMPACT) != 0) == (l == 0 and y.l0_rows < 16))
                hi_half = live & 0x3fffffff
                lo_half = hi_half + np.where(live & COMPACT, 32 * y.l0_rows, 512)
                for h in (hi_half, lo_half):
                    assert np.all((h >= 2 * L.frag_off) & (h < 2 * frag_end)), (c, l)
                halves += [hi_half, lo_half]
            else:
                assert np.all((live >= L.frag_off) & (live < frag_end)), (c, l)
                halves += [2 * live, 2 * live + 1]
            # where the kernels read these entries: rows are this layer's output positions, columns the positions of its input
            out_pos, col_pos = decode(y, l, live, hulls)
            per_unit = np.full(o_dim, -1)
            per_unit[o_idx[~skipped]] = out_pos
            assert np.all(per_unit[o_idx[~skipped]] == out_pos), (c, l, "one output position per unit")
            if L.has_bias:
                known = per_unit >= 0
                assert np.all((p[:, 0] - L.bias_off)[known] == per_unit[known]), (c, l, "bias slot and fragment row")
                per_unit = p[:, 0] - L.bias_off
            want_col = c_idx[~skipped] if l == 0 else out_pos_prev[c_idx[~skipped]]
            known = want_col >= 0
            assert np.all(col_pos[known] == want_col[known]), (c, l, "the column layer %d's unit was left at" % (l - 1))
            if l + 1 == len(dims):
                known = per_unit >= 0
                assert np.all(per_unit[known] == np.arange(o_dim)[known]), (c, "output c at position c")
            out_pos_prev = per_unit
        allh = np.concatenate([np.ravel(h) for h in halves])
        assert allh.min() >= 0 and allh.max() < 2 * y.block_floats, c
        assert len(np.unique(allh)) == len(allh), (c, "two weights share a place")


def test_one_matrix_outputs_stay_in_place(lib):
    """The shape of the 33-output bug by itself: every bias and every fragment row of a one-matrix network sits at its unit's index."""
    for n_out, f16, bias in itertools.product((33, 45, 50, 127), (0, 1), (0, 1)):
        rc, y = layout_of(lib, make_arch([n_out], 40, bias=bias), f16=f16)
        pos, _ = map_of(lib, y)
        p = pos.reshape(n_out, 40 + bias)
        if bias:
            assert np.array_equal(p[:, 0] - y.L[0].bias_off, np.arange(n_out))
        out_pos, col_pos = decode(y, 0, p[:, bias:], None)
        assert np.array_equal(out_pos, np.repeat(np.arange(n_out)[:, None], 40, 1)) and np.array_equal(col_pos[0], np.arange(40))


# ---- d. the path switch ----------------------------------------------------------------------------------------------------------

def test_the_path_switch_sees_what_it_saw(lib):
    """wide_needed compares npbnn_resident_path_bytes with the LDS limit.  With NPBNN_NO_COMPACT_ROWS and NPBNN_NO_L1_F16 clear it is the
    parent's resident_lds_bytes on the whole sweep, at every wave count the switch asks about; with one of them set it is that
    formula with the switch honoured, as build_net honours it."""
    n_plain = 0
    for c in SWEEP:
        y = sweep_layout(lib, c)
        plain = not (c["sw"].get("no_compact_rows") or c["sw"].get("no_l1_f16"))
        n_plain += plain
        for waves in (4, 8):
            got = lib.npbnn_host_resident_path_bytes(C.byref(y), int(c["classw"]), waves)
            assert got == parent_path_bytes(c, waves, honour_switches=True), c
            if plain:
                assert got == parent_path_bytes(c, waves), c
                assert (got > LDS_LIMIT) == (parent_path_bytes(c, waves) > LDS_LIMIT)
    assert n_plain > len(SWEEP) // 3          # (a third of the sweep sets no switch at all, a quarter of the rest neither of these two)
    # shapes on both sides of the limit, targets in the wave layout included
    for dims, f, lik, k in (([32, 8, 10], 1024, CAT, 0), ([32, 8, 10], 2048, CAT, 0), ([128, 128, 16], 512, GAUSS, 16), ([100, 20, 3], 600, GAUSS, 3)):
        for f16 in (0, 1):
            rc, y = layout_of(lib, make_arch(dims, f, lik=lik, n_targets=k, out=_capi.OUT_IDENTITY if lik == GAUSS else 0), f16=f16)
            c = dict(dims=dims, in_dim=f, f16=f16, blocks=None, sw={}, act=_capi.ACT_TANH, classw=0)
            kt0 = y.L[0].kt
            extra = 4 * (2 if kt0 >= 4 else 4) * 64 * k
            assert lib.npbnn_host_resident_path_bytes(C.byref(y), 0, 4) == parent_path_bytes(c, 4) + extra


# ---- c. launch invariants --------------------------------------------------------------------------------------------------------

def launch_layouts(lib):
    out = [layout_of(lib, make_arch([50, 5, 7], 256))[1], layout_of(lib, make_arch([32, 8, 10], 256))[1],
           layout_of(lib, make_arch([32, 8, 10], 512), blocks=block_table(32, 512, 8))[1],
           layout_of(lib, make_arch([32, 8, 10], 1024), f16=0)[1], layout_of(lib, make_arch([100, 20, 5], 256))[1],
           layout_of(lib, make_arch([61, 16, 4], 256), f16=0)[1], layout_of(lib, make_arch([45], 40))[1],
           layout_of(lib, make_arch([16, 4, 2], 700, lik=GAUSS, out=_capi.OUT_IDENTITY, n_targets=2))[1],
           layout_of(lib, make_arch([50, 5, 3], 64, lik=GAUSS, out=_capi.OUT_IDENTITY, n_targets=3), classw=0, slopes=1)[1],
           layout_of(lib, make_arch([20, 6, 1], 30, lik=POISSON, out=_capi.OUT_IDENTITY, n_targets=1))[1],
           layout_of(lib, make_arch([128, 128, 16], 300, lik=GAUSS, out=_capi.OUT_IDENTITY, n_targets=16))[1]]
    out += [sweep_layout(lib, c) for c in SWEEP[::64]]
    return out


def test_every_plan_can_run(lib):
    lib.npbnn_host_resident_max_waves.argtypes = [C.c_int] * 6
    tables = ((1, 0, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 1, 1))
    tiles = (1, 7, 256, 257, 2049, 3125, 6250, 100000)
    modes = ((0, 1, 0), (0, 1, 1), (0, 0, 1), (1, 0, 0), (0, 0, 0))            # predict_only, lik_only, plain
    seen = {OK: 0, NO_FIT: 0, FEW_WAVES: 0}
    thinned = 0
    for y in launch_layouts(lib):
        mt0 = y.L[0].mt
        for (lab, rw, tg), (pred, lik_only, plain), fast_opt in itertools.product(tables, modes, (0, 1)):
            # (what npbnn_get_info(NPBNN_INFO_MAX_CANDIDATES) asks: the chain pass, nothing forced)
            _, info = launch_of(lib, y, has_labels=lab, has_row_w=rw, has_targets=tg, fast_option=fast_opt)
            for n_tiles, want, over in itertools.product(tiles, (1, 2, 3), (0, 3, 4, 9)):
                rc, p = launch_of(lib, y, has_labels=lab, has_row_w=rw, has_targets=tg, n_tiles=n_tiles, want_cand=want, predict_only=pred,
                                  lik_only=lik_only, plain=plain, fast_option=fast_opt, waves_override=over)
                what = (y.image_floats, lab, rw, tg, pred, lik_only, plain, fast_opt, n_tiles, want, over)
                assert rc in seen, what
                seen[rc] += 1
                top = lib.npbnn_host_resident_max_waves(mt0, p.mti, y.l0_f16, p.n_cand, p.lk, p.fast)
                assert 1 <= p.n_cand <= min(want, MAX_CAND, lib.npbnn_host_resident_max_cand(mt0)), what
                assert p.n_cand == 1 or p.waves_full >= 8, what
                assert p.waves_full <= top, what
                if lik_only and not pred and want == 3:
                    assert (p.n_cand, p.fast) == (info.n_cand, info.fast), what
                if rc == NO_FIT:
                    assert p.waves_full == 0 and y.image_floats * 4 + p.wave_lds + 64 > LDS_LIMIT, what
                    continue
                assert p.n_cand * y.image_floats * 4 + p.waves_full * p.wave_lds + 64 <= LDS_LIMIT, what
                assert (rc == FEW_WAVES) == (p.waves < 4), what
                if rc == FEW_WAVES:
                    continue
                assert 4 <= p.waves <= p.waves_full, what
                assert p.lds_bytes == p.n_cand * y.image_floats * 4 + p.waves * p.wave_lds + 64 <= LDS_LIMIT, what
                assert 1 <= p.grid <= N_CU and p.grid == min(N_CU, -(-n_tiles // p.waves)), what
                if 1 <= over <= p.waves_full:
                    assert p.waves == over, what
                elif p.waves != p.waves_full:
                    thinned += 1
                    share = n_tiles / N_CU
                    assert p.n_cand > 1 and p.waves_full < share < 1.25 * p.waves_full and p.waves == p.waves_full - 2 >= 8, what
                else:
                    share = n_tiles / N_CU
                    assert not (p.n_cand > 1 and p.waves_full < share < 1.25 * p.waves_full and p.waves_full >= 10), what
                assert p.fast in (0, 1) and (not p.fast or (lik_only and not pred and fast_opt and not rw)), what
                assert p.want_spec == int(p.fast and not plain and not p.blocked and p.n_cand in (1, 3)), what
    assert seen[OK] and seen[FEW_WAVES] and seen[NO_FIT] and thinned


# ---- e. which build ----------------------------------------------------------------------------------------------------------------

def test_every_plan_names_an_instantiated_build(lib):
    """The shapes tests/test_hip_chain_oracle.py runs its resident cases on, on both layer-0 layouts and with 1-3 candidates wanted: the
    (MTI, D, LK, FAST, SPEC, CHAIN, BLK, MT0) the launch rule selects is one the instantiation files emit - and, asked for what the
    case asks, the case's own."""
    emitted = builds.all_builds()
    n_own = 0
    for case in builds.gpu.CASES:
        lik = {"cat": CAT, "gauss": GAUSS, "pois": POISSON}[case["lik"]]
        f = 256 if case["blk"] else 12
        k = 0 if lik == CAT else (1 if case["blk"] or lik == POISSON else 2)
        n_out = 5 if lik == CAT else k
        for width in (16 * case["mt0"], 16 * case["mt0"] - 3):
            a = make_arch([width, 40 if case["mti"] == 8 else 6, n_out], f, lik=lik, n_targets=k, out=0 if lik == CAT else _capi.OUT_IDENTITY)
            blocks = block_table(width, f, 4) if case["blk"] else None
            for f16, want, plain in itertools.product((0, 1), (1, 2, 3), (0, 1)):
                rc, y = layout_of(lib, a, f16=f16, blocks=blocks)
                assert rc == OK
                rc, p = launch_of(lib, y, has_labels=lik == CAT, has_targets=lik != CAT, n_tiles=(case["rows"] + 15) // 16, want_cand=want,
                                  plain=plain, fast_option=case["fast"])
                assert rc == OK, (case["key"], width, f16)
                # (npbnn_pick_eval_kernel: the builds without the chain's code are single-candidate fast ones)
                key = (p.mti, p.n_cand, p.lk, p.fast, 0, 0 if (plain and p.fast and p.n_cand == 1) else 1, int(p.fast and p.blocked), y.L[0].mt)
                assert key in emitted, (case["key"], width, f16, want, plain, key)
                if p.want_spec and want in (1, 3):
                    assert key[:4] + (1, 1) + key[6:] in emitted, (case["key"], key)
                own = (f16 == (case["l0"] != "f32") and want == case["d"] and plain == (case["advance"] == "mh_step"))
                if own:
                    n_own += 1
                    want_key = case["key"][:4] + (0,) + case["key"][5:]          # (the spec builds ride beside the launch's own build)
                    if not case["key"][5] and not p.fast:
                        continue
                    assert key == want_key, (case["key"], width, key)
    assert n_own == 2 * len(builds.gpu.CASES)


# ---- f. bad arguments --------------------------------------------------------------------------------------------------------------

def test_bad_arguments(lib):
    good = make_arch([32, 8, 10], 256)
    assert layout_of(lib, good)[0] == OK
    y = Layout()
    opts = (C.c_int32 * 7)(1, 0, 0, 0, 0, 0, 0)
    assert lib.npbnn_host_resident_layout(None, opts, None, C.byref(y)) == E_ARG
    assert lib.npbnn_host_resident_layout(C.byref(good), None, None, C.byref(y)) == E_ARG
    assert lib.npbnn_host_resident_layout(C.byref(good), opts, None, None) == E_ARG
    for bad in (make_arch([], 256), make_arch([32, 8, 10], 0), make_arch([32, 0, 10], 256), make_arch([-1], 256)):
        assert layout_of(lib, bad)[0] == E_ARG
    nine = make_arch([8] * 8, 16)
    nine.n_layers = 9
    assert layout_of(lib, nine)[0] == E_ARG
    assert layout_of(lib, make_arch([129, 5], 256))[0] == NOT_HELD          # (the weight-streamed path's)
    assert layout_of(lib, make_arch([32, 4096, 5], 256))[0] == NOT_HELD
    y = layout_of(lib, good)[1]
    for bad in (dict(want_cand=0), dict(n_cu=0), dict(lds_limit=0), dict(n_tiles=-1), dict(waves_override=-1)):
        assert launch_of(lib, y, **bad)[0] == E_ARG
    assert lib.npbnn_host_resident_launch(None, (C.c_int32 * 12)(*[1] * 12), C.byref(Launch())) == E_ARG
    assert lib.npbnn_host_resident_launch(C.byref(y), None, C.byref(Launch())) == E_ARG
    assert lib.npbnn_host_resident_map(None, None, None) == E_ARG
    assert lib.npbnn_host_resident_path_bytes(None, 0, 4) == -1
