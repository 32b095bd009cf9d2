"""Accumulated local effects on the GPU (npbnn_predict_ale, bn.get_ale / bn.ale) against the float64 restatement of
tests/ale_cases.py on the table the device holds, over both routes: both edges of a row's bin from one read of X
(NPBNN_INFO_ALE_ROUTE 1) and one pass per edge (2).  The counts must be equal; an effect is the mean of differences of two
predictions, each within test_hip_pdp's TOL of float64, so it is held to 2 TOL, and the curve accumulated over k + 1 edges to
(k + 1) 2 TOL.  tests/test_host_ale.py checks on the host that the references tell a wrong kernel from a right one."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

import ale_cases
import npbnn_amd as bn
from attrib_common import softmax_np
from npbnn_amd import _capi as capi
from test_hip_pdp import TOL

pytestmark = pytest.mark.gpu

BAR = 2 * TOL
OUT_KINDS = {"softmax": capi.OUT_SOFTMAX, "identity": capi.OUT_IDENTITY, "softplus_half": capi.OUT_SOFTPLUS_HALF}
_shared = {}


def _case_data(name):
    """inputs and float64 reference of a case, computed once"""
    if name not in _shared:
        case = ale_cases.CASES[name]
        inp = ale_cases.inputs(case)
        _shared[name] = (case, inp, ale_cases.reference(case, inp))
    return _shared[name]


def _context(case, inp):
    ctx = bn.HipContext()
    ctx.set_data(inp["x"])
    if inp["x_test"] is not None:
        ctx.set_data(inp["x_test"], capi.TEST)
    ctx.set_arch_from_weights(inp["weights"][0], inp["x"].shape[1], bn.ActFun(fun=case["fun"], trainable=case["trainable"]).device_kind(),
                              OUT_KINDS[case["out"]], capi.LIK_NONE)
    return ctx


def _device(case, inp, calls=1):
    """[(counts, effects)] of ``calls`` calls on one context, the route and the layer-0 path of the last"""
    ctx = _context(case, inp)
    try:
        assert ctx.info(capi.INFO_ALE_ROUTE) == 0
        res = [ctx.predict_ale(inp["weights"], inp["column"], inp["edges"], act_prm_sets=inp["slopes"], col_override=inp["override"],
                               which=case["which"], apply_out_fn=case["apply_out"]) for _ in range(calls)]
        return res, ctx.info(capi.INFO_ALE_ROUTE), ctx.l0_mode()
    finally:
        ctx.close()


def _check(case, got, want, route, tag=""):
    counts, effects = got
    err = float(np.abs(effects - want[1]).max())
    print("\nale %-36s%-10s route %d  K %2d  max|device - float64| %.3e (bar %.1e)" % (case["name"], tag, route, len(counts), err, BAR))
    assert counts.dtype == np.int64 and np.array_equal(counts, want[0])
    assert effects.shape == want[1].shape
    assert err <= BAR, (err, BAR)
    if case["pinned"]:
        assert np.all(effects == 0)


@pytest.mark.parametrize("name", list(ale_cases.CASES))
def test_case(name, monkeypatch):
    case, inp, want = _case_data(name)
    for k, v in case["env"]:
        monkeypatch.setenv(k, v)
    (got,), route, l0 = _device(case, inp)
    assert route == case["route"]
    if case["l0"]:
        assert l0 == case["l0"]
    _check(case, got, want, route)


@pytest.mark.parametrize("force", ["NPBNN_ALE_PER_EDGE", "NPBNN_FORCE_WIDE"])
@pytest.mark.parametrize("name", [n for n, c in ale_cases.CASES.items() if c["reroute"]])
def test_route_1_case_on_route_2(name, force, monkeypatch):
    case, inp, want = _case_data(name)
    monkeypatch.setenv(force, "1")
    (got,), route, _ = _device(case, inp)
    assert route == 2
    _check(case, got, want, route, tag=" " + force[6:])


@pytest.mark.parametrize("name,env", [("sets_7_two_a_launch", ()), ("rows_2111", ()), ("rows_9000", ()), ("partials_in_chunks", None),
                                      ("sets_3_two_a_launch", ale_cases._PER_EDGE), ("sets_3_two_a_launch", ale_cases._WIDE)])
def test_same_bits_every_call(name, env, monkeypatch):
    case, inp, _ = _case_data(name)
    for k, v in case["env"] if env is None else env:
        monkeypatch.setenv(k, v)
    (a, b), _, _ = _device(case, inp, calls=2)
    (c,), _, _ = _device(case, inp)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[1], c[1])
    assert np.abs(a[1]).max() > 0


def test_refusals_leave_route_0():
    case, inp, _ = _case_data("bins_7")
    ctx = _context(case, inp)
    try:
        n_sets, n_out, f = len(inp["weights"]), case["n_out"], inp["x"].shape[1]
        w = capi.as_f64(np.stack([bn.pack_weights(x) for x in inp["weights"]]))
        edges = capi.as_f64(inp["edges"])
        k = len(edges) - 1
        counts = np.zeros(1024, dtype=np.int64)
        effects = np.zeros((n_sets, 1024, n_out))
        i64 = ctypes.POINTER(ctypes.c_int64)

        def call(W=w, n=n_sets, focal=3, e=edges, bins=k, cnt=counts, eff=effects):
            return ctx._lib.npbnn_predict_ale(ctx._ctx, capi.dptr(W), None, n, focal, capi.dptr(e), bins, None, capi.TRAIN, 1,
                                              None if cnt is None else cnt.ctypes.data_as(i64), capi.dptr(eff))

        def bad_edges(i, v):
            e = np.linspace(-1.0, 1.0, k + 1)
            e[i] = v
            return e

        refused = dict(null_weights=dict(W=None), null_edges=dict(e=None), null_counts=dict(cnt=None), null_effects=dict(eff=None),
                       no_sets=dict(n=0), no_bins=dict(bins=0), negative_bins=dict(bins=-1),
                       too_many_bins=dict(bins=1025, e=np.linspace(0.0, 1.0, 1026)),
                       focal_below=dict(focal=-1), focal_above=dict(focal=f),
                       edges_equal=dict(e=bad_edges(3, np.linspace(-1.0, 1.0, k + 1)[2])), edges_decreasing=dict(e=bad_edges(3, -0.9)),
                       edge_nan=dict(e=bad_edges(2, np.nan)), edge_inf=dict(e=bad_edges(k, np.inf)))
        for tag, kw in refused.items():
            assert call(**kw) == capi.E_ARG, tag
            assert ctx.info(capi.INFO_ALE_ROUTE) == 0, tag
            assert b"predict_ale" in ctx._lib.npbnn_last_error(ctx._ctx), tag
        assert call() == 0 and ctx.info(capi.INFO_ALE_ROUTE) == 1
        assert call(bins=1024, e=np.linspace(-2.0, 2.0, 1025)) == 0 and counts.sum() == inp["x"].shape[0]
        assert call(focal=f) == capi.E_ARG and ctx.info(capi.INFO_ALE_ROUTE) == 0
    finally:
        ctx.close()


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **k)


@pytest.mark.parametrize("per_edge", [False, True], ids=["route1", "route2"])
def test_get_ale_curve(per_edge, monkeypatch):
    """get_ale on config 2's network: the centred curve of every sample and its summary against the float64 restatement, the
    bar growing with the number of effects summed."""
    case, inp, want = _case_data("config2_network")
    if per_edge:
        monkeypatch.setenv("NPBNN_ALE_PER_EDGE", "1")
    j = inp["column"]
    res = bn.get_ale(inp["x"], [j], "classification", case["n_out"], bn.ActFun(fun=case["fun"]), bn.SoftMax, inp["weights"],
                     [np.zeros(len(case["nodes"]))] * case["sets"], None, n_bins=case["bins"])
    assert np.array_equal(res["feature"], inp["edges"]) and np.array_equal(res["counts"], want[0])
    k = len(inp["edges"]) - 1
    assert res["ale"].shape == (k + 1, case["n_out"], 3) and res["ale_samples"].shape == (case["sets"], k + 1, case["n_out"])
    assert np.abs(res["local_effects"] - want[1]).max() <= BAR
    # the accumulated curve at edge k (get_ale's curve from its value at the first edge) sums k effects: (k + 1) BAR; the centre is
    # a weighted mean of such sums, so the centred curve is within the last edge's bar of that again
    curve_want = ale_cases.curve(*want)
    bars = (np.arange(k + 1) + 1) * BAR
    acc = res["ale_samples"] - res["ale_samples"][:, :1]
    assert np.all(np.abs(acc - (curve_want - curve_want[:, :1])).max(axis=(0, 2)) <= bars)
    assert np.all(np.abs(res["ale_samples"] - curve_want).max(axis=(0, 2)) <= bars + bars[-1])
    assert np.abs(res["ale"][:, :, 0] - curve_want.mean(axis=0)).max() <= 2 * bars[-1]
    tail = np.quantile(curve_want, (0.025, 0.975), axis=0)
    assert np.abs(res["ale"][:, :, 1] - tail[0]).max() <= 2 * bars[-1] and np.abs(res["ale"][:, :, 2] - tail[1]).max() <= 2 * bars[-1]


def test_get_ale_with_a_custom_output_callable():
    """A softmax the package does not know has no device kind: get_ale runs one pass per (edge, sample) for the last layer's values
    and takes the callable, the bins and the means on the host.  The table, samples and quantile edges of ``bins_2`` - the smallest
    case with more than one bin - cut to 257 rows (one past a block), 5 features, one hidden layer of 4 and 3 outputs, genReLU with
    a slope per sample: against the float64 restatement on the table the device holds, and against the same call with bn.SoftMax,
    whose softmax runs on the device."""
    case = dict(ale_cases.CASES["bins_2"], rows=257, features=5, nodes=(4,), n_out=3, sets=2, fun="genReLU", slopes="per_set")
    inp = ale_cases.inputs(case)
    assert inp["x"].shape == (257, 5) and len(inp["edges"]) == 3 and not np.array_equal(*inp["slopes"])

    def call(out_fn):
        return bn.get_ale(inp["x"], [inp["column"]], "classification", 3, bn.ActFun(fun="genReLU"), out_fn, inp["weights"], inp["slopes"],
                          None, n_bins=case["bins"])

    res, same = call(softmax_np), call(bn.SoftMax)
    assert np.array_equal(res["feature"], inp["edges"]) and np.array_equal(same["feature"], inp["edges"])
    held = inp["x"].astype(np.float32).astype(np.float64)
    counts, effects = ale_cases.local_effects(held, inp["column"], inp["edges"], inp["weights"], fun="genReLU", out_fn=softmax_np,
                                              slopes=inp["slopes"])
    curve = ale_cases.curve(counts, effects)
    want = dict(local_effects=effects, ale_samples=curve,
                ale=np.stack([curve.mean(axis=0)] + list(np.quantile(curve, (0.025, 0.975), axis=0)), axis=-1))
    assert np.array_equal(res["counts"], counts) and np.array_equal(same["counts"], counts) and counts.min() > 0
    assert np.abs(effects).max() > 100 * TOL
    for key in ("local_effects", "ale_samples", "ale"):
        print("\nale custom callable, %-13s: max|host branch - float64| %.3e, max|host branch - device softmax| %.3e (bar %.1e)"
              % (key, np.abs(res[key] - want[key]).max(), np.abs(res[key] - same[key]).max(), TOL))
    for key in ("local_effects", "ale_samples", "ale"):
        assert res[key].shape == want[key].shape
        assert np.abs(res[key] - want[key]).max() <= TOL and np.abs(res[key] - same[key]).max() <= TOL, key


def test_ale_of_a_checkpoint(tmp_path):
    """bn.ale on a checkpoint written by postLogger, against the float64 restatement over its stored samples."""
    rs = np.random.default_rng(4)
    n = 300
    x = np.zeros((n, 5))
    x[:, 0] = rs.normal(0, 1, n)
    x[:, 1] = rs.integers(0, 4, n)
    x[:, 2:] = rs.normal(0, 1, (n, 3))
    x[:, 3] = x[:, 0] + 0.1 * x[:, 3]                 # (a near copy of the first focal column)
    labels = (x[:, 0] + 0.5 * x[:, 1] > 1).astype(int) + (x[:, 2] > 0)
    dat = dict(data=x, labels=labels, test_data=np.zeros((0, 5)), test_labels=np.zeros(0))
    np.random.seed(1234)
    bnn = bn.npBNN(dat, n_nodes=[6, 4], actFun=bn.ActFun(fun="tanh"), use_bias_node=2)
    mcmc = bn.MCMC(bnn, n_iteration=200, sampling_f=20, print_f=1000, n_post_samples=10)
    logger = bn.postLogger(bnn, wdir=str(tmp_path), filename="ale", log_all_weights=0)
    quiet(bn.run_mcmc, bnn, mcmc, logger)
    res = bn.ale(logger._pklfile, [[0], 1], n_bins=10)
    _, _, lg = bn.load_obj(logger._pklfile)
    weights = [s["weights"] for s in lg._post_weight_samples]
    assert [len(r["feature"]) for r in res] == [11, 4]
    table = x.astype(np.float32).astype(np.float64)
    for focal, r in zip([0, 1], res):
        counts, effects = ale_cases.local_effects(table, focal, r["feature"], weights)
        assert np.array_equal(r["counts"], counts) and r["ale"].shape == (len(r["feature"]), 3, 3)
        assert np.abs(r["local_effects"] - effects).max() <= BAR
        k = len(counts)
        assert np.abs(r["ale_samples"] - ale_cases.curve(counts, effects)).max() <= 2 * (k + 1) * BAR
