"""Shapley attributions on the GPU (npbnn_predict_shapley, bn.get_shapley) against the float64 restatement of
tests/shapley_cases.py on the rows the device holds, over both routes: the walks in registers from a weight image in LDS
(NPBNN_INFO_SHAPLEY_ROUTE 1) and the plain kernels (2).  The error of an output array is max|device - float64| / max|float64| over
the case; the bars are shapley_cases.TOL and, for the efficiency identity on the device's own outputs, TOL_EFFICIENCY.
tests/test_host_shapley.py checks on the host that the references tell a wrong kernel from a right one."""
import numpy as np
import pytest

import npbnn_amd as bn
import shapley_cases as sh
from npbnn_amd import _capi as capi

pytestmark = pytest.mark.gpu

OUT_KINDS = {"softmax": capi.OUT_SOFTMAX, "identity": capi.OUT_IDENTITY, "softplus_half": capi.OUT_SOFTPLUS_HALF}
_shared = {}


def _case_data(name):
    """inputs and float64 reference of a case, computed once"""
    if name not in _shared:
        case = sh.CASES[name]
        inp = sh.inputs(case)
        _shared[name] = (case, inp, sh.reference(case, inp))
    return _shared[name]


def _context(case, inp):
    ctx = bn.HipContext()
    ctx.set_data(inp["x"])
    if inp["x_test"] is not None:
        ctx.set_data(inp["x_test"], capi.TEST)
    ctx.set_arch_from_weights(inp["weights"][0], inp["x"].shape[1], bn.ActFun(fun=case["fun"], trainable=case["trainable"]).device_kind(),
                              OUT_KINDS[case["out"]], capi.LIK_NONE)
    return ctx


def _call(ctx, case, inp, want_phi=True):
    return ctx.predict_shapley(inp["weights"], inp["rows"], inp["bg_rows"], inp["perms"], player_of=None if inp["groups"] is None else inp["player_of"],
                               act_prm_sets=inp["slopes"], col_override=inp["override"], which=case["which"], which_bg=inp["bg_which"],
                               apply_out_fn=case["apply_out"], want_phi=want_phi)


def _device(case, inp, calls=1):
    """the dicts of ``calls`` calls on one context, and the route of the last"""
    ctx = _context(case, inp)
    try:
        assert ctx.info(capi.INFO_SHAPLEY_ROUTE) == 0
        res = [_call(ctx, case, inp) for _ in range(calls)]
        return res, ctx.info(capi.INFO_SHAPLEY_ROUTE)
    finally:
        ctx.close()


def _check(case, inp, got, want, route, tag=""):
    errs = {k: sh.relative_error(got[k], want[k]) for k in sh.NAMES}
    # the summaries against the device's own phi: the same sums in float64, in another order
    own = sh.outputs(got["phi"], got["fx"], np.zeros((case["sets"], 1, case["n_out"])))
    cons = max(sh.relative_error(got[k], own[k]) for k in ("mean", "sq", "abs"))
    scale = float(np.abs(want["fx"]).max())
    eff = float(max(np.abs(sh.efficiency_gap(got)).max(), np.abs(sh.efficiency_gap(dict(got, phi=None))).max()) / scale)
    print("\nshapley %-30s%-8s route %d players %3d  " % (case["name"], tag, route, len(inp["players"]))
          + " ".join("%s %.2e" % (k, errs[k]) for k in sh.NAMES) + "  consistency %.2e  efficiency %.2e" % (cons, eff))
    for k in sh.NAMES:
        assert got[k].shape == want[k].shape, k
        assert errs[k] <= sh.TOL, (k, errs[k])
    assert cons <= 1e-13, cons
    assert eff <= sh.TOL_EFFICIENCY, eff
    if inp["override"] is not None:
        off = [p for p, cols in enumerate(inp["players"]) if all(not np.isnan(inp["override"][j]) for j in cols)]
        assert off and all(np.all(got[k][:, off] == 0) for k in ("mean", "sq", "abs")) and np.all(got["phi"][:, :, off] == 0)


@pytest.mark.parametrize("name", list(sh.CASES))
def test_case(name, monkeypatch):
    case, inp, want = _case_data(name)
    for k, v in case["env"]:
        monkeypatch.setenv(k, v)
    (a, b), route = _device(case, inp, calls=2)
    assert route == case["route"]
    _check(case, inp, a, want, route)
    for k in sh.NAMES:                              # a second call returns the same bits
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", [n for n, c in sh.CASES.items() if c["reroute"]])
def test_route_1_case_on_route_2(name, monkeypatch):
    case, inp, want = _case_data(name)
    for k, v in case["env"]:
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("NPBNN_SHAPLEY_PLAIN", "1")
    (a, b), route = _device(case, inp, calls=2)
    assert route == 2
    _check(case, inp, a, want, route, tag=" PLAIN")
    for k in sh.NAMES:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", sh.FORCED_WIDE)
def test_route_1_case_on_the_streamed_path(name, monkeypatch):
    case, inp, want = _case_data(name)
    monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    (a,), route = _device(case, inp)
    assert route == 2
    _check(case, inp, a, want, route, tag=" WIDE")


def test_exact_case_against_the_enumeration():
    case, inp, _ = _case_data("exact_4_players")
    want = sh.reference_exact(case, inp)
    (got,), route = _device(case, inp)
    assert route == 1
    _check(case, inp, got, want, route, tag=" exact")


def test_chunks_give_the_values_of_one_chunk(monkeypatch):
    """(other splits of the walks: the same values to the bar, not the same bits)"""
    case, inp, want = _case_data("scratch_in_chunks")
    (whole,), _ = _device(case, inp)
    for k, v in case["env"]:
        monkeypatch.setenv(k, v)
    (chunked,), _ = _device(case, inp)
    for k in sh.NAMES:
        assert sh.relative_error(chunked[k], whole[k]) <= sh.TOL, k


@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("name", ["sets_7_two_a_launch", "sets_7_one_a_launch"])
def test_same_bits_prepared_group_after_group(name, plain, monkeypatch):
    """three sets' blocks prepared at a time (the budget of the case's ``_in_groups`` twin): set order and row order are unchanged"""
    case, inp, _ = _case_data(name)
    if plain:
        monkeypatch.setenv("NPBNN_SHAPLEY_PLAIN", "1")
    (whole,), _ = _device(case, inp)
    for k, v in sh.CASES[name + "_in_groups"]["env"]:
        monkeypatch.setenv(k, v)
    (grouped,), route = _device(case, inp)
    assert route == (2 if plain else 1)
    for k in sh.NAMES:
        assert np.array_equal(whole[k], grouped[k]) and np.abs(whole[k]).max() > 0, k


def test_without_phi_the_summaries_are_the_same_bits():
    case, inp, _ = _case_data("sets_3_two_a_launch")
    ctx = _context(case, inp)
    try:
        a, b = _call(ctx, case, inp), _call(ctx, case, inp, want_phi=False)
        assert b["phi"] is None
        for k in ("mean", "sq", "abs", "fx", "base"):
            assert np.array_equal(a[k], b[k]), k
    finally:
        ctx.close()


def test_refusals_leave_route_0_and_the_outputs_untouched(monkeypatch):
    case, inp, _ = _case_data("sets_3_two_a_launch")
    ctx = _context(case, inp)
    import ctypes as C
    i64, i32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    try:
        n_sets, c, f, e, n_bg = case["sets"], case["n_out"], case["features"], case["n_explain"], case["n_bg"]
        w = capi.as_f64(np.stack([bn.pack_weights(x) for x in inp["weights"]]))
        rows, bg, perms = inp["rows"].copy(), inp["bg_rows"].copy(), np.ascontiguousarray(inp["perms"], dtype=np.int32)
        po = np.arange(f, dtype=np.int32)
        shapes = dict(mean=(e, f, c), sq=(e, f, c), absolute=(n_sets, f, c), fx=(n_sets, e, c), base=(n_sets, c), phi=(n_sets, e, f, c))
        outs = {k: np.full(s, 7.0) for k, s in shapes.items()}

        def call(W=w, n=n_sets, which=capi.TRAIN, rows=rows, n_e=e, which_bg=capi.TRAIN, bg=bg, n_b=n_bg, po=po, n_p=f, perms=perms,
                 n_perm=perms.shape[0], **o):
            o = dict(outs, **o)
            ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)      # noqa: E731
            return ctx._lib.npbnn_predict_shapley(ctx._ctx, capi.dptr(W), None, n, None, which, ptr(rows, i64), n_e, which_bg, ptr(bg, i64), n_b,
                                                  ptr(po, i32), n_p, ptr(perms, i32), n_perm, 1, capi.dptr(o["mean"]), capi.dptr(o["sq"]),
                                                  capi.dptr(o["absolute"]), capi.dptr(o["fx"]), capi.dptr(o["base"]), capi.dptr(o["phi"]))

        def changed(a, at, value):
            a = a.copy()
            a.flat[at] = value
            return a

        doubled = perms.copy()
        doubled[1, 0] = doubled[1, 1]
        two_in_one = po.copy()
        two_in_one[3] = 4                           # (player 3 is left without a column)
        refused = dict(null_weights=dict(W=None), null_rows=dict(rows=None), null_bg=dict(bg=None), null_perms=dict(perms=None),
                       null_mean=dict(mean=None), null_sq=dict(sq=None), null_abs=dict(absolute=None), null_fx=dict(fx=None),
                       null_base=dict(base=None), no_sets=dict(n=0), no_rows=dict(n_e=0), no_bg=dict(n_b=0), no_perm=dict(n_perm=0),
                       no_players=dict(n_p=0), row_below=dict(rows=changed(rows, 2, -1)), row_above=dict(rows=changed(rows, 2, inp["x"].shape[0])),
                       bg_above=dict(bg=changed(bg, 0, inp["x"].shape[0])), bg_below=dict(bg=changed(bg, 1, -1)),
                       which_above=dict(which=2), which_below=dict(which=-1), which_bg_above=dict(which_bg=2), which_bg_below=dict(which_bg=-1), player_above=dict(po=changed(po, 5, f)),
                       player_below=dict(po=changed(po, 5, -1)), player_without_column=dict(po=two_in_one),
                       players_without_map=dict(po=None, n_p=f - 1), not_a_permutation=dict(perms=doubled),
                       permutation_entry_above=dict(perms=changed(perms, 3, f)))
        for tag, kw in refused.items():
            assert call(**kw) == capi.E_ARG, tag
            assert ctx.info(capi.INFO_SHAPLEY_ROUTE) == 0, tag
            assert b"predict_shapley" in ctx._lib.npbnn_last_error(ctx._ctx), tag
            assert all(np.all(a == 7.0) for a in outs.values()), tag
        assert call(which=capi.TEST) == capi.E_STATE and call(which_bg=capi.TEST) == capi.E_STATE      # (no test table)
        assert all(np.all(a == 7.0) for a in outs.values())
        monkeypatch.setenv("NPBNN_SHAPLEY_PHI_BYTES", str(n_sets * f * c * 8 * 10))
        assert call() == capi.E_NOMEM and b"at most 10 explained rows" in ctx._lib.npbnn_last_error(ctx._ctx)
        assert all(np.all(a == 7.0) for a in outs.values()) and ctx.info(capi.INFO_SHAPLEY_ROUTE) == 0
        assert call(phi=None) == 0 and ctx.info(capi.INFO_SHAPLEY_ROUTE) == 1 and np.all(outs["phi"] == 7.0)
        monkeypatch.delenv("NPBNN_SHAPLEY_PHI_BYTES")
        assert call() == 0 and ctx.info(capi.INFO_SHAPLEY_ROUTE) == 1
        assert all(np.abs(a).max() > 0 and not np.any(a == 7.0) for a in outs.values())
        assert call(n=0) == capi.E_ARG and ctx.info(capi.INFO_SHAPLEY_ROUTE) == 0
        fresh = bn.HipContext()
        try:
            fresh.set_data(inp["x"])
            assert fresh._lib.npbnn_predict_shapley(fresh._ctx, capi.dptr(w), None, n_sets, None, capi.TRAIN, rows.ctypes.data_as(i64), e, capi.TRAIN,
                                                    bg.ctypes.data_as(i64), n_bg, None, f, perms.ctypes.data_as(i32), perms.shape[0], 1,
                                                    capi.dptr(outs["mean"]), capi.dptr(outs["sq"]), capi.dptr(outs["absolute"]), capi.dptr(outs["fx"]),
                                                    capi.dptr(outs["base"]), None) == capi.E_STATE      # (no npbnn_set_arch)
        finally:
            fresh.close()
    finally:
        ctx.close()


def test_get_shapley_on_config2_network():
    case, inp, want = _case_data("config2_network")
    res = bn.get_shapley(inp["x"], case["n_out"], bn.ActFun(fun=case["fun"]), bn.SoftMax, inp["weights"],
                         [np.zeros(len(case["nodes"]))] * case["sets"], None, rows=inp["rows"][:40], background=inp["bg_rows"], n_perm=4,
                         return_samples=True)
    # (get_shapley draws its own permutations: the restatement walks those)
    players = sh.players_of(case["features"])
    ref = sh.outputs(*sh.walks(inp["xe"][:40], inp["xb"], inp["weights"], res["permutations"], players))
    assert sh.relative_error(res["samples"]["attributions"], ref["phi"]) <= sh.TOL
    assert sh.relative_error(res["attributions"][..., 0], ref["mean"]) <= sh.TOL
    assert sh.relative_error(res["prediction"], ref["fx"].mean(axis=0)) <= sh.TOL
    assert sh.relative_error(res["base_value"], ref["base"].mean(axis=0)) <= sh.TOL
    assert sh.relative_error(res["importance"][..., 0], ref["abs"].mean(axis=0)) <= sh.TOL
    assert sorted(res["ranking"].tolist()) == list(range(case["features"]))
    assert np.abs(want["phi"]).max() > 0
