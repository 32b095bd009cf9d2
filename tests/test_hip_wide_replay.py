"""The replay of stored weight sets on the weight-streamed path: up to three sets per read of X wherever the first layer's product is
the fused one (at most 64 nodes, one K-slice), one per pass elsewhere.  Whatever shares a pass, a set's predictions are those of its
own single prediction bit for bit (every build of a tiling accumulates alike) and the float64 oracle's within the project's bound;
NPBNN_INFO_REPLAY_PASSES / _MAX_GROUP (HipContext.replay_info) say what was launched.  A set whose scaled layer-0 weights leave the
fp16 range repeats alone on the float32 path, wherever it sits in its group.

Groups of one inside a process: a distinct slope vector per set under tanh, which ignores slopes (the path's environment switches are
read once per process)."""
import numpy as np
import pytest

import cases
import npbnn_amd as bn
import oracle as orc
import pdp_cases
import support_cases
from npbnn_amd import HipContext, _capi as capi

pytestmark = pytest.mark.gpu

TOL = 2e-5      # test_hip_posterior.TOL: float32 forward pass against float64

ACTS = {"tanh": capi.ACT_TANH, "ReLU": capi.ACT_RELU}
OUTS = {"softmax": (capi.OUT_SOFTMAX, orc.out_softmax), "identity": (capi.OUT_IDENTITY, orc.out_identity),
        "softplus_half": (capi.OUT_SOFTPLUS_HALF, orc.out_regress_error)}


def _f32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def _unit_sets(rs, f, nodes, n_out, n_sets):
    """weights N(0, 1 / sqrt(fan_in + 1)): every layer's values of order 1, whatever the widths"""
    shapes = cases.layer_shapes(f, list(nodes), n_out, 2)
    return [[rs.normal(0, 1.0 / np.sqrt(s[1]), s) for s in shapes] for _ in range(n_sets)]


def _distinct_slopes(n_sets, n_hidden):
    return [np.full(n_hidden, 0.001 * (i + 1)) for i in range(n_sets)]


def _fused_info(n_sets):
    """what a replay of n_sets sets that share their slopes launches where the pass is the fused one: groups of three"""
    return ((n_sets + 2) // 3, min(n_sets, 3))


def _three_checks(ctx, x, sets, fun, out, info, slopes=None, which=capi.TRAIN, apply_out_fn=True, oracle_slopes=False):
    """replay_info, every set against its own single prediction (bytes) and against the oracle on the float32-rounded table"""
    y = ctx.predict_sets(sets, act_prm_sets=slopes, which=which, apply_out_fn=apply_out_fn)
    got_info = ctx.replay_info()
    print("replay_info %s, expected %s" % (got_info, info))
    assert got_info == info
    assert y.shape == (len(sets), x.shape[0], sets[0][-1].shape[0])
    out_fn = OUTS[out][1] if apply_out_fn else orc.out_identity
    x32 = _f32(x)
    for i, w in enumerate(sets):
        single = ctx.predict(w, act_prm=None if slopes is None else slopes[i], which=which, apply_out_fn=apply_out_fn)
        ref = orc.forward(x32, w, orc.Act(fun, prm=np.asarray(slopes[i]) if oracle_slopes else None), out_fn)
        print("set %d: max |sets - single| %g, max |sets - oracle| %g" % (i, np.max(np.abs(y[i] - single)), np.max(np.abs(y[i] - ref))))
        np.testing.assert_array_equal(y[i], single, err_msg="set %d" % i)
        np.testing.assert_allclose(y[i], ref, atol=TOL, rtol=0, err_msg="set %d" % i)
    return y


def _context(x, sets, fun="tanh", out="softmax", x_test=None, l0=None, trainable=False, act_kind=None):
    ctx = HipContext(0)
    try:
        ctx.set_data(x)
        if x_test is not None:
            ctx.set_data(x_test, capi.TEST)
        if l0:
            ctx.set_l0_precision(l0)
        if trainable:
            ctx.set_trainable_slopes(True)
        ctx.set_arch_from_weights(sets[0], x.shape[1], ACTS[fun] if act_kind is None else act_kind, OUTS[out][0], capi.LIK_NONE)
    except Exception:
        ctx.close()
        raise
    return ctx


def _seven_sets(seed=11):
    """test_hip_posterior's shape: 999 rows, 6 features, [5, 4], 3 classes - the 128 x 32 tiling, one output tile"""
    rs = np.random.default_rng(seed)
    n, f, c = 999, 6, 3
    x = rs.standard_normal((n, f))
    shapes = cases.layer_shapes(f, [5, 4], c, 2)
    return x, [[rs.normal(0, 0.5, s) for s in shapes] for _ in range(7)]


def test_groups_and_bits(monkeypatch):
    """A. Seven sets go through as three passes of three, three and one; with a slope vector each, as seven of one - the same bytes."""
    monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    x, sets = _seven_sets()
    ctx = _context(x, sets)
    try:
        assert ctx.is_wide()
        y = _three_checks(ctx, x, sets, "tanh", "softmax", (3, 3))
        alone = ctx.predict_sets(sets, act_prm_sets=_distinct_slopes(7, 2))
        assert ctx.replay_info() == (7, 1)
        assert alone.tobytes() == y.tobytes()
        assert ctx.info(capi.INFO_MAX_CANDIDATES) == 1          # (the chains' group pass on this path: untouched)
    finally:
        ctx.close()


_BASE = dict(rows=999, features=6, nodes=(5, 4), n_out=3, fun="tanh", out="softmax", sets=7, apply_out=True, l0=None, test_rows=None)
SHAPES = {
    "default_net_70_features": dict(rows=1000, features=70, nodes=(50, 5), n_out=10, fun="ReLU"),      # 128 x 64, mt = 4, 70 % 32 != 0
    "one_hidden_layer_33_features": dict(features=33, nodes=(20,), n_out=2, out="identity"),           # mt = 2
    "predicted_sigma": dict(features=9, nodes=(12, 7), n_out=4, out="softplus_half"),
    "rows_1": dict(rows=1), "rows_16": dict(rows=16), "rows_130": dict(rows=130), "rows_2048": dict(rows=2048),
    "raw_values": dict(apply_out=False),
    "l0_f32": dict(l0="f32"),
    "test_table": dict(rows=1000, test_rows=300),
    "sets_1": dict(sets=1), "sets_2": dict(sets=2), "sets_3": dict(sets=3), "sets_4": dict(sets=4),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_tilings_and_edges(name, monkeypatch):
    """B. The tilings of the fused end, row counts around a tile and a row block, the float32 builds, the test table, set counts
    around a group: the three checks of A on each, and the groups of one give the same bytes."""
    monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    case = dict(_BASE, **SHAPES[name])
    rs = np.random.default_rng(300 + list(SHAPES).index(name))
    x = rs.standard_normal((case["rows"], case["features"]))
    x_test = rs.standard_normal((case["test_rows"], case["features"])) if case["test_rows"] else None
    sets = _unit_sets(rs, case["features"], case["nodes"], case["n_out"], case["sets"])
    which = capi.TEST if x_test is not None else capi.TRAIN
    ctx = _context(x, sets, case["fun"], case["out"], x_test=x_test, l0=case["l0"])
    try:
        assert ctx.is_wide()
        y = _three_checks(ctx, x_test if x_test is not None else x, sets, case["fun"], case["out"], _fused_info(case["sets"]), which=which,
                          apply_out_fn=case["apply_out"])
        assert ctx.l0_mode() == ("f32" if case["l0"] == "f32" else "f16-split")
        if case["fun"] == "tanh":
            alone = ctx.predict_sets(sets, act_prm_sets=_distinct_slopes(case["sets"], len(case["nodes"])), which=which, apply_out_fn=case["apply_out"])
            assert ctx.replay_info() == (case["sets"], 1)
            assert alone.tobytes() == y.tobytes()
    finally:
        ctx.close()


def test_a_first_layer_the_fused_end_does_not_take(monkeypatch):
    """C. [80, 5]: five output tiles, the 256 x 128 tiling whose waves do not hold whole rows - one set per pass, and the info values say so."""
    monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    rs = np.random.default_rng(41)
    x = rs.standard_normal((500, 24))
    sets = _unit_sets(rs, 24, (80, 5), 4, 5)
    ctx = _context(x, sets)
    try:
        assert ctx.is_wide()
        _three_checks(ctx, x, sets, "tanh", "softmax", (5, 1))
    finally:
        ctx.close()


# D. planted sets -> (passes, layer-0 path the call ends on).  Groups (0 1 2) (3 4 5) (6); a set out of the fp16 range ends its group
# before it (the sets before it are delivered as computed), repeats alone in float32, and a fresh group starts behind it:
#   3     : (0 1 2) (3 4 5)! 3 in f32, (4 5 6)                                   4 passes
#   4     : (0 1 2) (3 4 5)! 3 delivered, 4 in f32, (5 6)                        4
#   5     : (0 1 2) (3 4 5)! 3 4 delivered, 5 in f32, (6)                        4
#   3, 4  : (0 1 2) (3 4 5)! 3 in f32, (4 5 6)! 4 in f32, (5 6)                  6
#   6     : (0 1 2) (3 4 5) (6)! 6 in f32                                        4, and the call ends on the float32 path
PLANTED = {(3,): (4, "f16-split"), (4,): (4, "f16-split"), (5,): (4, "f16-split"), (3, 4): (6, "f16-split"), (6,): (4, "f32")}


@pytest.mark.parametrize("planted", list(PLANTED), ids=lambda p: "set_" + "_".join(map(str, p)))
def test_float32_repeat_inside_a_group(planted, monkeypatch):
    """D. The set that leaves the fp16 range repeats alone, at every position of its group; its neighbours keep their fp16-split bytes."""
    monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    x, sets = _seven_sets()
    for i in planted:
        sets[i][0][0, 3] = 3e5
    passes, ends_on = PLANTED[planted]
    ctx = _context(x, sets)
    try:
        assert ctx.is_wide()
        y = ctx.predict_sets(sets)
        info, mode = ctx.replay_info(), ctx.l0_mode()
        print("planted %s: replay_info %s, ends on %s" % (planted, info, mode))
        assert np.all(np.isfinite(y))
        assert info == (passes, 3)
        assert mode == ends_on
        single = []
        for i, w in enumerate(sets):
            single.append(ctx.predict(w))
            assert ctx.l0_mode() == ("f32" if i in planted else "f16-split")
        ctx.set_l0_precision("f32")
        single_f32 = {i: ctx.predict(sets[i]) for i in planted}
        ctx.set_l0_precision("auto")
        for i in range(7):
            np.testing.assert_array_equal(y[i], single_f32[i] if i in planted else single[i], err_msg="set %d" % i)
    finally:
        ctx.close()


@pytest.mark.parametrize("trainable", [False, True], ids=["slopes_fixed", "slopes_trainable"])
def test_slope_groups(trainable, monkeypatch):
    """E. Slopes a a b b b b a: groups of 2, 3, 1 and 1, with NPBNN_OPT_TRAINABLE_SLOPES off and on (the pass takes its slopes from the
    launch, never from the images: no slope of one set reaches another)."""
    monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    x, sets = _seven_sets(seed=12)
    a, b = np.array([0.05, 0.3]), np.array([0.2, 0.01])
    slopes = [a, a, b, b, b, b, a]
    ctx = _context(x, sets, trainable=trainable, act_kind=bn.ActFun(fun="genReLU", prm=np.zeros(2)).device_kind())
    try:
        assert ctx.is_wide()
        _three_checks(ctx, x, sets, "genReLU", "softmax", (4, 3), slopes=slopes, oracle_slopes=True)
    finally:
        ctx.close()


def _flat_bytes(v):
    if isinstance(v, dict):
        return b"".join(k.encode() + _flat_bytes(v[k]) for k in sorted(v))
    if isinstance(v, (tuple, list)):
        return b"".join(_flat_bytes(e) for e in v)
    return b"none" if v is None else np.asarray(v).tobytes()


def test_the_six_summarising_entries(monkeypatch):
    """F. Twelve sets through every entry that summarises the replay: in groups of three and - a slope vector each - alone, the same bytes."""
    monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    inp = support_cases.inputs("tanh", 10, n_rows=500)
    sets = [s["weights"] for s in inp["samples"]] + [p["weights"] for p in inp["prior"][:2]]
    labels = inp["labels"]
    alone = _distinct_slopes(12, 2)
    entries = {
        "summary": lambda c, ap: c.predict_sets_summary(sets, 1, labels=labels, act_prm_sets=ap),
        "hpd": lambda c, ap: c.predict_sets_hpd(sets, 0.9, act_prm_sets=ap),
        "support": lambda c, ap: c.predict_sets_support(sets, 1, labels, support_cases.GRID, act_prm_sets=ap, want_summary=True),
        "lppd": lambda c, ap: c.predict_sets_lppd(sets, capi.LIK_CATEGORICAL, act_prm_sets=ap),
        "uncertainty": lambda c, ap: c.predict_sets_uncertainty(sets, act_prm_sets=ap),
        "convergence": lambda c, ap: c.predict_sets_convergence(sets, 1, act_prm_sets=ap),
    }
    ctx = HipContext(0)
    try:
        ctx.set_data(inp["x"])
        ctx.set_labels(labels)
        ctx.set_arch_from_weights(sets[0], inp["x"].shape[1], capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
        assert ctx.is_wide()
        for name, call in entries.items():
            together = call(ctx, None)
            info = ctx.replay_info()
            split = call(ctx, alone)
            info_split = ctx.replay_info()
            print("%s: replay_info %s together, %s alone" % (name, info, info_split))
            assert info == (4, 3), name
            assert info_split == (12, 1), name
            assert _flat_bytes(together) == _flat_bytes(split), name
    finally:
        ctx.close()


def test_pdp_route_2(monkeypatch):
    """G. Partial dependence, one pass per (grid point, group of sets): seven sets in groups and alone give the same bytes, within
    test_hip_pdp_envelope's bound of the float64 restatement."""
    from test_hip_pdp import TOL as PDP_TOL, device_means
    monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    case = dict(pdp_cases._DEFAULTS, name="streamed_groups", route=2, seed=4242, sets=7)
    inp = pdp_cases.envelope_inputs(case)
    want = pdp_cases.envelope_oracle(case, inp)
    got, route = device_means(inp["x"], inp["weights"], inp["focal"], inp["grid"], fun="tanh")
    alone, route_alone = device_means(inp["x"], inp["weights"], inp["focal"], inp["grid"], fun="tanh", slopes=_distinct_slopes(7, 2))
    err = float(np.abs(got - want).max())
    print("pdp: max |device - oracle| %.3e (bound %.1e)" % (err, PDP_TOL))
    assert route == 2 and route_alone == 2
    assert got.tobytes() == alone.tobytes()
    assert got.shape == want.shape and err <= PDP_TOL


def test_a_shape_streamed_by_itself():
    """H. The default [50, 5] on 704 features runs streamed unforced; with this many rows its product keeps one K-slice, so the pass
    is the fused one: six sets, two passes of three."""
    probe = HipContext(0)
    n_cu = probe.info(capi.INFO_N_CU)
    probe.close()
    rs = np.random.default_rng(77)
    n, f, c = 128 * (n_cu // 2 + 5) - 7, 704, 10
    x = rs.standard_normal((n, f))
    sets = _unit_sets(rs, f, (50, 5), c, 6)
    ctx = _context(x, sets, fun="ReLU")
    try:
        assert ctx.is_wide()
        _three_checks(ctx, x, sets, "ReLU", "softmax", (2, 3))
    finally:
        ctx.close()
