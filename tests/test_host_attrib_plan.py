"""CPU checks of the attribution entries' work plan (npbnn_amd/csrc/npbnn_attrib_plan.h, exported by libnpbnn_host.so as
npbnn_host_attrib_*; npbnn_predict_pdp, npbnn_predict_ale, npbnn_predict_saliency and npbnn_predict_shapley choose their route, cut
their jobs and size their device buffers by the same header).

The tests replay the entries' loops from the plan's numbers and assert what the kernels rely on: every (set, row, output) - and for
Shapley every walk - is covered exactly once, every index a launch can form lies inside the buffer the plan sized for it, the bytes
stay within the budget down to the floor, and grids, int products and dynamic LDS stay within their limits.  The literal figures are
the ones the case tables (tests/saliency_cases.py, shapley_cases.py, pdp_cases.py, ale_cases.py) run under on the GPU.

One thing the budget invariant of Shapley's route 2 leaves out on purpose: a direct launch owns four scratch units per workgroup of 256
rows whatever the budget says (npbnn_attrib_shap.scr_units is the larger of the two launches'), so under a budget of a few units the
scratch takes more than the budget's share.  The sizes are checked against what the launches index, not against the budget."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import ale_cases
import pdp_cases
import saliency_cases
import shapley_cases
from npbnn_amd import _capi, predraw

MAX_LAYERS, MAX_CAND, N_CU = 8, 3, 256
INT_MAX = 2 ** 31 - 1
PDP, SALIENCY, SHAPLEY = 0, 1, 2
E_PHI, E_WALKS = 1, 2
ROWS, TAIL, WAVE_ROWS = 256, 32, 256
BIG = 1 << 40                                    # a budget that holds everything
SAL_SCRATCH, SHAP_SCRATCH = 128 << 20, 128 << 20  # the entries' defaults
_I8 = C.c_int * MAX_LAYERS
_LL = C.c_longlong


class Prep(C.Structure):
    """PdpPrep"""
    _fields_ = ([(n, C.c_int) for n in ("F", "Fp", "H0", "H0P", "hb0", "n_layers", "n_grid", "wn", "tail_floats")] +
                [(n, _I8) for n in ("l_in", "l_out", "l_hb", "l_woff", "t_inp", "t_off")])


class Route(C.Structure):
    """npbnn_attrib_route"""
    _fields_ = ([("q", Prep)] + [(n, C.c_int) for n in ("fits", "route", "H0P", "NS", "sum_w", "max_w")] +
                [(n, _LL) for n in ("set_bytes", "lds_bytes")])


class Sal(C.Structure):
    """npbnn_attrib_sal"""
    _fields_ = ([(n, C.c_int) for n in ("rows_cap", "n_c", "n_slot_cap", "pairs_cap", "prep_sets", "Fq")] + [("a_off", _I8)] +
                [(n, _LL) for n in ("row_fixed", "row_pair", "n_D", "n_part", "n_fac", "n_act", "n_g", "lds_bytes")])


class Shap(C.Structure):
    """npbnn_attrib_shap"""
    _fields_ = ([("refusal", C.c_int)] + [(n, _LL) for n in ("phi_rows_fit", "walks")] +
                [(n, C.c_int) for n in ("W", "n_split", "rb_cap", "nsl", "e_cap", "b_cap", "prep_sets", "bg_blocks", "ex_blocks")] +
                [(n, _LL) for n in ("unit_bytes", "scr_unit", "scr_units", "n_xeT", "n_xbT", "n_z0b", "n_fx", "n_fb", "n_part", "n_mean", "n_abs",
                                    "n_phi", "n_scr", "lds_bytes")])


class Ale(C.Structure):
    """npbnn_attrib_ale"""
    _fields_ = [(n, C.c_int) for n in ("n_wg", "wg_chunk", "stride", "stage_floats")] + [(n, _LL) for n in ("n_part", "lds_bytes")]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(predraw.HOST_LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(predraw.HOST_LIB_PATH)
    i64p = C.POINTER(C.c_int64)
    lib.npbnn_host_attrib_route.argtypes = [C.POINTER(_capi.Arch), C.POINTER(C.c_int32), C.POINTER(Route)]
    lib.npbnn_host_attrib_saliency.argtypes = [C.POINTER(Route), i64p, C.POINTER(Sal)]
    lib.npbnn_host_attrib_shapley.argtypes = [C.POINTER(Route), i64p, C.POINTER(Shap)]
    lib.npbnn_host_attrib_pdp_g_chunk.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int64]
    lib.npbnn_host_attrib_ale.argtypes = [C.POINTER(Route), C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(Ale)]
    return lib


def cdiv(a, b):
    return -(-a // b)


def route_of(lib, dims, features, entry, n_points=1, bias=1, streamed=0, off=0):
    """the route of a network of layer widths ``dims`` (the outputs last) on a table of ``features`` columns"""
    a = _capi.Arch()
    a.n_layers, a.in_dim = len(dims), features
    flags = [bias] * len(dims) if isinstance(bias, int) else list(bias)
    n_w, n_in = 0, features
    for l, d in enumerate(dims):
        a.out_dim[l], a.has_bias[l] = d, flags[l]
        n_w += d * (n_in + flags[l])
        n_in = d
    req = (C.c_int32 * 6)(n_w, cdiv(features, 16) * 16, n_points, streamed, off, entry)
    r = Route()
    assert lib.npbnn_host_attrib_route(C.byref(a), req, C.byref(r)) == 0
    assert r.route == (1 if r.fits else 2) and r.q.wn == n_w and r.q.H0P == r.H0P
    return r


def saliency_of(lib, r, c, features, rows, sets, scratch=SAL_SCRATCH, prep=BIG):
    p = Sal()
    assert lib.npbnn_host_attrib_saliency(C.byref(r), (C.c_int64 * 6)(c, features, rows, sets, scratch, prep), C.byref(p)) == 0
    return p


def shapley_of(lib, r, c, players, explain, n_bg, n_perm, sets, scratch=SHAP_SCRATCH, prep=BIG, phi=BIG, want_phi=1, n_cu=N_CU):
    p = Shap()
    rc = lib.npbnn_host_attrib_shapley(C.byref(r), (C.c_int64 * 11)(c, players, explain, n_bg, n_perm, sets, n_cu, want_phi, scratch, prep, phi),
                                       C.byref(p))
    assert rc == p.refusal
    return p


def case_dims(case):
    return list(case["nodes"]) + [case["n_out"]]


def case_route(lib, case, entry, off_names, n_points=1):
    env = dict(case["env"])
    return route_of(lib, case_dims(case), case["features"], entry, n_points, bias=pdp_cases._bias_flags(case["bias"], len(case_dims(case))),
                    streamed=int(env.get("NPBNN_FORCE_WIDE") == "1"), off=int(any(env.get(n) == "1" for n in off_names)))


# ---- route 1's envelope ------------------------------------------------------------------------------------------------------------

def test_envelope_edges_match_the_case_tables(lib):
    """the route every case table fixes by hand, for every case whose path the library does not choose by itself (the 700-feature
    cases stream their weights on their own: that choice is npbnn_resident_plan.h's)"""
    tables = [(pdp_cases.ENVELOPE, PDP, ("NPBNN_PDP_PER_GRID",)), (ale_cases.CASES, PDP, ("NPBNN_ALE_PER_EDGE",)),
              (saliency_cases.CASES, SALIENCY, ("NPBNN_SALIENCY_PLAIN",)), (shapley_cases.CASES, SHAPLEY, ("NPBNN_SHAPLEY_PLAIN",))]
    seen = set()
    for table, entry, off in tables:
        for name, case in table.items():
            if case["features"] >= 700:
                continue
            assert case_route(lib, case, entry, off).route == case["route"], (entry, name)
            seen.add(name)
    assert {"h0_64", "h0_65", "later_32", "later_33", "outputs_32", "outputs_33", "lds_tail_3300", "lds_tail_4356", "lds_h0_32_f512",
            "lds_h0_32_f513", "lds_h0_48_f256", "lds_h0_48_f257", "one_matrix_33_outputs"} <= seen


@pytest.mark.parametrize("entry", [PDP, SALIENCY, SHAPLEY])
def test_route_shapes(lib, entry):
    for h0, later, depth, c, f in itertools.product((1, 31, 32, 33, 63, 64, 65, 130), (31, 32, 33), (1, 2, 3, 5), (1, 5, 32, 33), (40, 256, 513)):
        dims = ([h0] + [later] * (depth - 2) + [c]) if depth > 1 else [c]
        r = route_of(lib, dims, f, entry, bias=[l % 2 for l in range(len(dims))])
        q, h = r.q, dims[0]
        inside = (h <= 64 and q.Fp * (32 if h <= 32 else 64) * 4 <= 65536 and all(d <= TAIL for d in dims[1:]) and (depth > 1 or h <= TAIL)
                  and (2 if h <= 32 else 1) * q.tail_floats * 4 <= 32768)
        assert bool(r.fits) == inside, dims
        assert r.sum_w == sum(dims) and r.max_w == max(dims)
        if r.fits:
            assert r.H0P == (32 if h <= 32 else 64) and r.NS * r.H0P == 64
            assert r.lds_bytes <= (64 + 32) * 1024
        elif entry != PDP:
            assert r.H0P == cdiv(h, 32) * 32 and (r.NS == 1 or entry == SHAPLEY)
        assert r.H0P >= h or (entry == PDP and not r.fits)
        assert q.Fp * r.H0P < INT_MAX and q.n_grid * r.H0P < INT_MAX
        # the later layers' blocks follow each other without overlap; the packed weights end at n_weights
        off = 0
        for l in range(1, depth):
            assert q.t_off[l] == off and q.t_inp[l] % 8 == 0 and q.t_inp[l] >= q.l_in[l] == dims[l - 1] and q.l_out[l] == dims[l]
            off += cdiv(dims[l], 4) * 4 + dims[l] * q.t_inp[l]
        assert off == q.tail_floats
        last = depth - 1
        assert (q.l_woff[last] + dims[last] * (dims[last - 1] + q.l_hb[last]) if depth > 1 else h * (f + q.hb0)) == q.wn
        assert r.set_bytes == 4 * (q.Fp * r.H0P + r.H0P + q.tail_floats + MAX_LAYERS)
    # the two switches
    assert route_of(lib, [20, 6, 5], 40, entry).route == 1
    assert route_of(lib, [20, 6, 5], 40, entry, streamed=1).route == 2 and route_of(lib, [20, 6, 5], 40, entry, off=1).route == 2


# ---- saliency ----------------------------------------------------------------------------------------------------------------------

def replay_saliency(r, p, c, features, rows, sets):
    """the loops of npbnn_predict_saliency; returns the launches as (group's first set, set of the group, sets, row0, rows, c0, outputs)"""
    L, H0P, R = r.q.n_layers, r.H0P, p.rows_cap
    widths = [r.q.H0] + [r.q.l_out[l] for l in range(1, L)]
    seen = np.zeros((sets, rows, c), dtype=np.int32)
    launches = []
    assert R % WAVE_ROWS == 0 and R >= WAVE_ROWS and p.n_slot_cap == R // WAVE_ROWS and p.pairs_cap == r.NS * p.n_c and p.Fq == cdiv(features, 32) * 32
    assert 1 <= p.n_c <= c and 1 <= p.prep_sets <= sets
    assert [p.a_off[l] for l in range(L)] == [sum(widths[:l]) for l in range(L)]
    for g0 in range(0, sets, p.prep_sets):
        ng = min(p.prep_sets, sets - g0)
        for s0 in range(0, ng, r.NS):
            n_set = min(r.NS, ng - s0)
            for row0 in range(0, rows, R):
                n = min(R, rows - row0)
                wgs, n_slot = cdiv(n, ROWS), cdiv(n, WAVE_ROWS)
                for c0 in range(0, c, p.n_c):
                    nc = min(p.n_c, c - c0)
                    n_sc = n_set * nc
                    launches.append((g0, s0, n_set, row0, n, c0, nc))
                    seen[g0 + s0:g0 + s0 + n_set, row0:row0 + n, c0:c0 + nc] += 1
                    # phase 1: the last element a thread of the launch writes (threads past the chunk's rows write nothing)
                    if r.route == 1:
                        assert nc == c
                        assert (((n_set - 1) * c + c - 1) * R + n - 1) * H0P + H0P <= p.n_D
                        assert (wgs - 1) * L * TAIL * ROWS + ((L - 1) * TAIL + TAIL - 1) * ROWS + ROWS <= p.n_fac
                        assert wgs * L * TAIL * ROWS < INT_MAX
                    else:
                        assert n_set == 1 and ((nc - 1) * R + n - 1) * H0P + H0P <= p.n_D
                        assert (p.a_off[L - 1] + widths[-1] - 1) * R + n <= min(p.n_fac, p.n_act)
                        assert (2 * r.max_w - 1) * R + n <= p.n_g
                    # phase 2: sal_fold_kernel reads whole rows of D up to the chunk's last, writes a partial per (pair, wave, sum, feature)
                    assert ((n_sc - 1) * R + n - 1) * H0P + H0P <= p.n_D
                    assert ((n_sc - 1) * n_slot + n_slot - 1) * 3 * p.Fq + 3 * p.Fq <= p.n_part
                    assert n_sc <= p.pairs_cap and n_slot <= p.n_slot_cap
                    assert max(cdiv(p.Fq, 128), n_sc) <= 65535 and n_sc * 3 * p.Fq < INT_MAX
    assert np.all(seen == 1)
    assert R * H0P < INT_MAX and R <= 1 << 24
    return launches


def saliency_bytes(p):
    return 4 * (p.n_D + p.n_fac + p.n_act + p.n_g) + 8 * p.n_part


def test_saliency_cut_sweep(lib):
    nets = [[20, 6], [32, 32], [33, 9], [64, 6], [65, 6], [130, 40], [20, 33], [31, 32, 12, 9], []]
    n_checked = 0
    for hidden, c, rows, sets in itertools.product(nets, (1, 5, 32, 33), (1, 255, 256, 257, 2111), (1, 2, 3, 7)):
        r = route_of(lib, hidden + [c], 40, SALIENCY)
        whole = saliency_of(lib, r, c, 40, rows, sets, scratch=BIG)
        assert whole.rows_cap == cdiv(rows, WAVE_ROWS) * WAVE_ROWS and whole.n_c == c and whole.prep_sets == sets
        row_all = whole.row_fixed + r.NS * c * whole.row_pair
        floor = WAVE_ROWS * (whole.row_fixed + (r.NS * c if r.route == 1 else 1) * whole.row_pair)
        budgets = (BIG, 3 * WAVE_ROWS * row_all, 2 * WAVE_ROWS * row_all - 1, WAVE_ROWS * row_all, WAVE_ROWS * row_all - 1,
                   WAVE_ROWS * (whole.row_fixed + 2 * whole.row_pair), floor, floor - 1, 1)
        for scratch, prep in itertools.product(budgets, (BIG, 3 * r.set_bytes, r.set_bytes, 1)):
            p = saliency_of(lib, r, c, 40, rows, sets, scratch, prep)
            replay_saliency(r, p, c, 40, rows, sets)
            spent = saliency_bytes(p)
            if scratch >= floor:
                assert spent <= scratch, (hidden, c, rows, scratch)
            else:
                assert p.rows_cap == WAVE_ROWS and p.pairs_cap == (r.NS * c if r.route == 1 else 1) and spent == floor
            assert p.prep_sets == max(1, min(sets, prep // r.set_bytes))
            if r.route == 1:
                assert p.lds_bytes == r.lds_bytes <= (64 + 32) * 1024
            n_checked += 1
    assert n_checked > 20000


def test_saliency_figures_of_the_case_tables(lib):
    # scratch_in_chunks: 900 000 bytes hold 522 rows of 1724 bytes: chunks of 512, five of them for 2111 rows
    case = saliency_cases.CASES["scratch_in_chunks"]
    r = case_route(lib, case, SALIENCY, ("NPBNN_SALIENCY_PLAIN",))
    p = saliency_of(lib, r, 5, 40, 2111, 3, scratch=int(dict(case["env"])["NPBNN_SALIENCY_SCRATCH_BYTES"]))
    assert (r.route, r.NS, p.row_fixed, p.row_pair) == (1, 2, 3 * 32 * 4, 32 * 4 + 6) and p.row_fixed + 2 * 5 * p.row_pair == 1724
    assert (p.rows_cap, p.n_c) == (512, 5)
    assert [n for _, s0, _, _, n, _, _ in replay_saliency(r, p, 5, 40, 2111, 3) if s0 == 0] == [512, 512, 512, 512, 63]
    # route2_outputs_in_chunks: a row costs 1128 fixed bytes plus 390 per output; 520 000 / 256 leave 2031: two outputs a launch
    case = saliency_cases.CASES["route2_outputs_in_chunks"]
    assert case["nodes"] == (65, 6) and case["rows"] == 300 and dict(case["env"]) == {"NPBNN_SALIENCY_SCRATCH_BYTES": "520000"}
    r = case_route(lib, case, SALIENCY, ("NPBNN_SALIENCY_PLAIN",))
    p = saliency_of(lib, r, 5, 40, 300, 3, scratch=520000)
    assert (r.route, r.NS, r.H0P, p.row_fixed, p.row_pair) == (2, 1, 96, 1128, 390)
    assert (p.rows_cap, p.n_c) == (256, 2)
    assert [(n, nc) for _, s0, _, _, n, _, nc in replay_saliency(r, p, 5, 40, 300, 3) if s0 == 0] == [(256, 2), (256, 2), (256, 1), (44, 2), (44, 2), (44, 1)]


@pytest.mark.parametrize("table,entry", [(saliency_cases, SALIENCY), (shapley_cases, SHAPLEY)])
def test_groups_of_three_prepared_sets(lib, table, entry):
    """the sets_7_* cases under a prep budget of three sets' blocks: groups of 3, 3 and 1 sets; on H0P = 32 saliency's second launch of
    a group holds one set where the whole job's second launch holds two"""
    for base, h0p in (("sets_7_two_a_launch", 32), ("sets_7_one_a_launch", 64)):
        case = table.CASES[base + "_in_groups"]
        off = "NPBNN_SALIENCY_PLAIN" if entry == SALIENCY else "NPBNN_SHAPLEY_PLAIN"
        r = case_route(lib, case, entry, (off,))
        env = dict(case["env"])
        prep = int(env["NPBNN_SALIENCY_PREP_BYTES" if entry == SALIENCY else "NPBNN_SHAPLEY_PREP_BYTES"])
        assert r.route == 1 and r.H0P == h0p and prep == 3 * r.set_bytes and len(env) == 1
        assert {k: v for k, v in case.items() if k not in ("name", "seed", "env", "reroute")} == \
               {k: v for k, v in table.CASES[base].items() if k not in ("name", "seed", "env", "reroute")}
        if entry == SALIENCY:
            p = saliency_of(lib, r, 5, 40, 300, 7, prep=prep)
            sets = [(g0, s0, n) for g0, s0, n, _, _, _, _ in replay_saliency(r, p, 5, 40, 300, 7)]
            want = [(0, 0, 2), (0, 2, 1), (3, 0, 2), (3, 2, 1), (6, 0, 1)] if h0p == 32 else [(g, s, 1) for g in (0, 3) for s in range(3)] + [(6, 0, 1)]
            assert p.prep_sets == 3 and sets == want
        else:
            p = shapley_of(lib, r, 5, 40, 70, 3, 4, 7, prep=prep)
            assert p.prep_sets == 3 and p.nsl == 7 and p.e_cap == 128
            assert [g for g, *_ in replay_shapley(r, p, 5, 40, 70, 3, 4, 7)[0]] == [0, 3, 6]


# ---- Shapley -----------------------------------------------------------------------------------------------------------------------

def replay_shapley(r, p, c, players, explain, n_bg, n_perm, sets):
    """the loops of npbnn_predict_shapley; returns the walk launches as (group's first set, set of the group, sets, e0, rows, row
    blocks) and the gathers of explained rows as (group's first set, e0)"""
    pc, h0p, w = players * c, r.H0P, n_bg * n_perm
    assert p.W == p.walks == w and 1 <= p.n_split <= w and 1 <= p.rb_cap and 1 <= p.nsl <= min(sets, 65535) and 1 <= p.prep_sets <= sets
    assert p.e_cap == 64 * p.rb_cap and p.b_cap == cdiv(n_bg, 64) * 64 and p.bg_blocks == cdiv(n_bg, 256) and p.ex_blocks == cdiv(p.e_cap, 256)
    assert p.rb_cap * p.n_split < INT_MAX and p.e_cap < INT_MAX
    # every walk belongs to exactly one split
    cuts = [q * w // p.n_split for q in range(p.n_split + 1)]
    assert cuts[0] == 0 and cuts[-1] == w and all(b > a for a, b in zip(cuts, cuts[1:]))
    assert p.n_xeT == r.q.Fp * p.e_cap and p.n_xbT == r.q.Fp * p.b_cap
    assert p.n_fx == sets * explain * c and p.n_fb == sets * n_bg * c and p.n_mean == 2 * pc * explain and p.n_abs == sets * pc
    seen = np.zeros((sets, explain), dtype=np.int32)
    launches, gathers = [], []

    def direct(ns, n):
        # one thread per row; wave (set of the launch, 64 rows) owns scratch unit (set x workgroups + workgroup) x 4 + wave
        assert ns <= 65535
        if r.route == 2:
            assert ((ns - 1) * cdiv(n, 256) + cdiv(n, 256) - 1) * 4 + 3 < p.scr_units

    for g0 in range(0, sets, p.prep_sets):
        ng = min(p.prep_sets, sets - g0)
        for s0 in range(0, ng, p.nsl):
            ns = min(p.nsl, ng - s0)
            direct(ns, n_bg)
            assert ((s0 + ns - 1) * n_bg + n_bg - 1) * h0p + h0p <= p.n_z0b
        for e0 in range(0, explain, p.e_cap):
            rows = min(p.e_cap, explain - e0)
            if g0 == 0 or p.e_cap < explain:
                gathers.append((g0, e0))
            n_rb = cdiv(rows, 64)
            assert n_rb <= p.rb_cap
            for s0 in range(0, ng, p.nsl):
                ns = min(p.nsl, ng - s0)
                direct(ns, rows)
                units = ns * n_rb * p.n_split
                assert units * pc * 64 <= p.n_part and cdiv(n_rb * p.n_split, 4) < INT_MAX
                if r.route == 2:
                    assert units <= p.scr_units
                launches.append((g0, s0, ns, e0, rows, n_rb))
                seen[g0 + s0:g0 + s0 + ns, e0:e0 + rows] += 1
    assert np.all(seen == 1)
    # the rows in d_xeT are the chunk's whenever a walk launch reads them: one chunk stays, more chunks are gathered before every use
    if p.e_cap < explain:
        assert len(gathers) == len({(g, e) for g, _, _, e, _, _ in launches})
    else:
        assert gathers == [(0, 0)]
    if r.route == 2:
        assert p.scr_unit == (r.q.H0 + 2 * r.max_w + c) * 64 and p.n_scr == p.scr_units * p.scr_unit
    else:
        assert p.scr_unit == 0 and p.n_scr == 0 and p.lds_bytes == 4 * (r.q.Fp * h0p + r.q.tail_floats) <= (64 + 32) * 1024
    return launches, gathers


def test_shapley_cut_sweep(lib):
    nets = [[20, 6], [32, 32], [33, 9], [64, 6], [65, 6], [130, 40], [20, 33], [31, 32, 12, 9], []]
    n_checked = 0
    for hidden, c, explain, sets in itertools.product(nets, (1, 5, 32, 33), (1, 63, 64, 65, 255, 257, 1000), (1, 2, 7)):
        r = route_of(lib, hidden + [c], 40, SHAPLEY)
        for players, (n_bg, n_perm) in itertools.product((1, 7, 40), ((1, 1), (3, 4), (300, 1))):
            unit = shapley_of(lib, r, c, players, explain, n_bg, n_perm, sets, scratch=BIG).unit_bytes
            assert unit == players * c * 64 * 8 + (4 * 64 * (r.q.H0 + 2 * r.max_w + c) if r.route == 2 else 0)
            for scratch, prep in itertools.product((BIG, 64 * unit, 5 * unit, 2 * unit, 2 * unit - 1, unit, unit - 1, 1), (BIG, 3 * r.set_bytes, 1)):
                p = shapley_of(lib, r, c, players, explain, n_bg, n_perm, sets, scratch, prep)
                assert p.refusal == 0
                replay_shapley(r, p, c, players, explain, n_bg, n_perm, sets)
                # the walk launch's units - partials and, on route 2, scratch - within the budget, or one unit at the floor
                units = p.nsl * p.rb_cap * p.n_split
                assert units * unit <= scratch or units == 1
                assert p.prep_sets == max(1, min(sets, prep // r.set_bytes))
                # the splits aim at eight waves per compute unit over the whole job, the walks and the budget allowing
                want = 8 * N_CU // (cdiv(explain, 64) * sets)
                assert p.n_split == max(1, min(n_bg * n_perm, want, scratch // unit))
                n_checked += 1
    assert n_checked > 20000


def test_shapley_refusals(lib):
    r = route_of(lib, [20, 6, 5], 40, SHAPLEY)
    per_row = 3 * 40 * 5 * 8
    p = shapley_of(lib, r, 5, 40, 70, 3, 4, 3, phi=per_row * 10)
    assert p.refusal == E_PHI and p.phi_rows_fit == 10
    assert shapley_of(lib, r, 5, 40, 10, 3, 4, 3, phi=per_row * 10).refusal == 0
    assert shapley_of(lib, r, 5, 40, 70, 3, 4, 3, phi=per_row * 10, want_phi=0).refusal == 0
    p = shapley_of(lib, r, 5, 40, 70, 1 << 16, 1 << 15, 3, want_phi=0)
    assert p.refusal == E_WALKS and p.walks == 1 << 31
    assert shapley_of(lib, r, 5, 40, 70, 1 << 16, (1 << 15) - 1, 3, want_phi=0).refusal == 0
    # (out_phi over its budget is reported first, as the entry always has)
    assert shapley_of(lib, r, 5, 40, 70, 1 << 16, 1 << 15, 3, phi=1).refusal == E_PHI


def test_shapley_figures_of_the_case_tables(lib):
    # scratch_in_chunks: a wave's partials take 40 x 5 x 64 x 8 = 102 400 bytes; 250 000 bytes hold two, which go to the splits of the
    # walks: a chunk is one block of 64 rows, five of them for 257 rows, one set a launch
    case = shapley_cases.CASES["scratch_in_chunks"]
    r = case_route(lib, case, SHAPLEY, ("NPBNN_SHAPLEY_PLAIN",))
    p = shapley_of(lib, r, 5, 40, 257, 3, 4, 3, scratch=int(dict(case["env"])["NPBNN_SHAPLEY_SCRATCH_BYTES"]))
    assert (r.route, p.unit_bytes, p.n_split, p.rb_cap, p.nsl, p.e_cap) == (1, 102400, 2, 1, 1, 64)
    launches, _ = replay_shapley(r, p, 5, 40, 257, 3, 4, 3)
    assert [(e0, n) for _, s0, _, e0, n, _ in launches if s0 == 0] == [(0, 64), (64, 64), (128, 64), (192, 64), (256, 1)]
    assert all(ns == 1 for _, _, ns, _, _, _ in launches) and len(launches) == 15
    # route2_scratch_in_chunks: a unit costs 102 400 + 101 120 bytes, so two fit: two splits, one block of rows, one set, two chunks
    case = shapley_cases.CASES["route2_scratch_in_chunks"]
    assert case["nodes"] == (130, 40) and case["n_explain"] == 70 and dict(case["env"]) == {"NPBNN_SHAPLEY_SCRATCH_BYTES": "450000"}
    r = case_route(lib, case, SHAPLEY, ("NPBNN_SHAPLEY_PLAIN",))
    p = shapley_of(lib, r, 5, 40, 70, 3, 4, 3, scratch=450000)
    assert (r.route, r.H0P, 4 * p.scr_unit, p.unit_bytes) == (2, 160, 101120, 102400 + 101120)
    assert (p.n_split, p.rb_cap, p.nsl) == (2, 1, 1)
    assert p.scr_units == 4                       # (the direct launch's four waves of a workgroup, over the walk launch's two)
    launches, _ = replay_shapley(r, p, 5, 40, 70, 3, 4, 3)
    assert [(e0, n) for _, s0, _, e0, n, _ in launches if s0 == 0] == [(0, 64), (64, 6)]


# ---- partial dependence and accumulated local effects ------------------------------------------------------------------------------

def test_pdp_grid_chunks(lib):
    for n_grid, rows, c in itertools.product((1, 3, 50), (1, 300, 100000), (1, 5, 33)):
        for budget in (BIG, 3 * rows * c * 4, rows * c * 4 * 2 - 1, rows * c * 4, rows * c * 4 - 1, 1):
            g = lib.npbnn_host_attrib_pdp_g_chunk(n_grid, rows, c, budget)
            assert g == max(1, min(n_grid, budget // (rows * c * 4)))
            assert g * rows * c * 4 <= budget or g == 1
    # pdp_cases' chunks_of_one_grid_point: an accumulator of one grid point, three chunks for a grid of three
    case = pdp_cases.ENVELOPE["chunks_of_one_grid_point"]
    budget = int(dict(case["env"])["NPBNN_PDP_ACC_BYTES"])
    assert budget == 300 * 5 * 4 and lib.npbnn_host_attrib_pdp_g_chunk(case["grid"][2], case["rows"], case["n_out"], budget) == 1
    assert lib.npbnn_host_attrib_pdp_g_chunk(case["grid"][2], case["rows"], case["n_out"], 512 << 20) == 3


def ale_of(lib, r, k, c, rows, budget):
    a = Ale()
    assert lib.npbnn_host_attrib_ale(C.byref(r), k, c, rows, budget, C.byref(a)) == 0
    return a


def test_ale_workgroup_chunks(lib):
    for hidden, c, k, rows in itertools.product(([20, 6], [40, 6], [65, 6], []), (1, 5, 32), (1, 7, 1024), (1, 256, 257, 2111)):
        r = route_of(lib, hidden + [c], 40, PDP, n_points=k + 1)
        wg_bytes = r.NS * k * c * 8
        for budget in (BIG, 3 * wg_bytes, 2 * wg_bytes - 1, wg_bytes, wg_bytes - 1, 1):
            a = ale_of(lib, r, k, c, rows, budget)
            assert a.n_wg == cdiv(rows, ROWS) and a.stride == c | 1 and 1 <= a.wg_chunk <= a.n_wg
            if r.route == 2:
                assert a.n_part == MAX_CAND * a.n_wg * 2 * c
                continue
            assert a.wg_chunk * wg_bytes <= budget or a.wg_chunk == 1
            # ale_kernel: a workgroup's partials [set of the launch][workgroup][bin][output]; its stage holds the first-layer image, then
            # 256 rows' differences at the stride and their bins
            assert ((r.NS - 1) * a.wg_chunk + a.wg_chunk - 1) * k * c + k * c <= a.n_part
            assert a.stage_floats >= max(r.q.Fp * r.H0P, ROWS * a.stride + ROWS)
            assert a.lds_bytes == 4 * (a.stage_floats + r.NS * r.q.tail_floats) <= (64 + 32) * 1024
    # ale_cases' partials_in_chunks: the partials of one workgroup (two sets x 7 bins x 5 outputs), nine launches per group of sets
    case = ale_cases.CASES["partials_in_chunks"]
    budget = int(dict(case["env"])["NPBNN_ALE_PART_BYTES"])
    r = case_route(lib, case, PDP, ("NPBNN_ALE_PER_EDGE",), n_points=8)
    a = ale_of(lib, r, 7, 5, case["rows"], budget)
    assert budget == 2 * 7 * 5 * 8 and (r.route, r.NS, a.n_wg, a.wg_chunk) == (1, 2, 9, 1)
    assert ale_of(lib, r, 7, 5, case["rows"], 256 << 20).wg_chunk == 9
