"""Input-gradient saliency on the GPU (npbnn_predict_saliency, bn.get_saliency / bn.saliency) against the float64 restatement of
tests/saliency_cases.py on the table the device holds, over both routes of phase 1: in registers from a weight image in LDS
(NPBNN_INFO_SALIENCY_ROUTE 1) and the plain kernel (2).  The bar is test_hip_pdp's TOL - float32 forward arithmetic against
float64 on these same draws - times max(1, max|reference|), per returned array.  tests/test_host_saliency.py checks on the host
that the references tell a wrong kernel from a right one."""
import contextlib
import io

import numpy as np
import pytest

import npbnn_amd as bn
import saliency_cases as sc
from npbnn_amd import _capi as capi
from test_hip_pdp import TOL

pytestmark = pytest.mark.gpu

OUT_KINDS = {"softmax": capi.OUT_SOFTMAX, "identity": capi.OUT_IDENTITY, "softplus_half": capi.OUT_SOFTPLUS_HALF}
NAMES = ("mean", "abs", "sq")
_shared = {}


def _case_data(name):
    """inputs and float64 reference of a case, computed once"""
    if name not in _shared:
        case = sc.CASES[name]
        inp = sc.inputs(case)
        _shared[name] = (case, inp, sc.reference(case, inp))
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
    """[(mean, abs, sq)] of ``calls`` calls on one context, and the route of the last"""
    ctx = _context(case, inp)
    try:
        assert ctx.info(capi.INFO_SALIENCY_ROUTE) == 0
        res = [ctx.predict_saliency(inp["weights"], act_prm_sets=inp["slopes"], col_override=inp["override"], which=case["which"],
                                    apply_out_fn=case["apply_out"]) for _ in range(calls)]
        return res, ctx.info(capi.INFO_SALIENCY_ROUTE)
    finally:
        ctx.close()


def _check(case, inp, got, want, route, tag=""):
    errs = [float(np.abs(g - w).max()) for g, w in zip(got, want)]
    bars = [TOL * max(1.0, float(np.abs(w).max())) for w in want]
    print("\nsaliency %-32s%-16s route %d  max|device - float64| mean %.3e abs %.3e sq %.3e (bars %.1e %.1e %.1e)"
          % ((case["name"], tag, route) + tuple(errs) + tuple(bars)))
    for name, g, w, err, bar in zip(NAMES, got, want, errs, bars):
        assert g.shape == w.shape, name
        assert err <= bar, (name, err, bar)
    if inp["override"] is not None:
        off = ~np.isnan(inp["override"])
        assert off.any() and all(np.all(g[:, :, off] == 0) for g in got)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_case(name, monkeypatch):
    case, inp, want = _case_data(name)
    for k, v in case["env"]:
        monkeypatch.setenv(k, v)
    (got,), route = _device(case, inp)
    assert route == case["route"]
    _check(case, inp, got, want, route)


@pytest.mark.parametrize("force", ["NPBNN_SALIENCY_PLAIN", "NPBNN_FORCE_WIDE"])
@pytest.mark.parametrize("name", [n for n, c in sc.CASES.items() if c["reroute"]])
def test_route_1_case_on_route_2(name, force, monkeypatch):
    case, inp, want = _case_data(name)
    monkeypatch.setenv(force, "1")
    (got,), route = _device(case, inp)
    assert route == 2
    _check(case, inp, got, want, route, tag=" " + force[6:])


@pytest.mark.parametrize("name,env", [("sets_7_two_a_launch", ()), ("rows_2111", ()), ("scratch_in_chunks", None),
                                      ("sets_3_two_a_launch", (("NPBNN_SALIENCY_PLAIN", "1"),))])
def test_same_bits_every_call(name, env, monkeypatch):
    case, inp, _ = _case_data(name)
    for k, v in case["env"] if env is None else env:
        monkeypatch.setenv(k, v)
    (a, b), _ = _device(case, inp, calls=2)
    (c,), _ = _device(case, inp)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
        assert np.abs(x).max() > 0


@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("name", ["sets_7_two_a_launch", "sets_7_one_a_launch"])
def test_same_bits_prepared_group_after_group(name, plain, monkeypatch):
    """three sets' blocks prepared at a time (the budget of the case's ``_in_groups`` twin): set order and row order are unchanged"""
    case, inp, _ = _case_data(name)
    if plain:
        monkeypatch.setenv("NPBNN_SALIENCY_PLAIN", "1")
    (whole,), _ = _device(case, inp)
    for k, v in sc.CASES[name + "_in_groups"]["env"]:
        monkeypatch.setenv(k, v)
    (grouped,), route = _device(case, inp)
    assert route == (2 if plain else 1)
    for x, y in zip(whole, grouped):
        assert np.array_equal(x, y) and np.abs(x).max() > 0


def test_refusals_leave_route_0():
    case, inp, _ = _case_data("sets_3_two_a_launch")
    ctx = _context(case, inp)
    try:
        n_sets, n_out, f = len(inp["weights"]), case["n_out"], inp["x"].shape[1]
        w = capi.as_f64(np.stack([bn.pack_weights(x) for x in inp["weights"]]))
        outs = [np.zeros((n_sets, n_out, f)) for _ in range(3)]

        def call(W=w, n=n_sets, mean=outs[0], absolute=outs[1], sq=outs[2]):
            return ctx._lib.npbnn_predict_saliency(ctx._ctx, capi.dptr(W), None, n, None, capi.TRAIN, 1, capi.dptr(mean), capi.dptr(absolute),
                                                   capi.dptr(sq))

        refused = dict(null_weights=dict(W=None), null_mean=dict(mean=None), null_abs=dict(absolute=None), null_sq=dict(sq=None),
                       no_sets=dict(n=0))
        for tag, kw in refused.items():
            assert call(**kw) == capi.E_ARG, tag
            assert ctx.info(capi.INFO_SALIENCY_ROUTE) == 0, tag
            assert b"predict_saliency" in ctx._lib.npbnn_last_error(ctx._ctx), tag
        assert call() == 0 and ctx.info(capi.INFO_SALIENCY_ROUTE) == 1
        assert np.abs(outs[1]).max() > 0
        assert call(n=0) == capi.E_ARG and ctx.info(capi.INFO_SALIENCY_ROUTE) == 0
    finally:
        ctx.close()


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **k)


def _against_restatement(res, want, level=0.95):
    """get_saliency's dict against the restatement's (mean, abs, sq): every sample's values within the array's bar (the root of
    the mean square squared again), and the summaries of the two that are linear in the values within the same bars."""
    bars = [TOL * max(1.0, float(np.abs(w).max())) for w in want]
    smp = res["samples"]
    assert np.abs(smp["mean_gradient"] - want[0]).max() <= bars[0] and np.abs(smp["saliency"] - want[1]).max() <= bars[1]
    assert np.abs(smp["rms_gradient"] ** 2 - want[2]).max() <= bars[2]
    tail = 0.5 * (1 - level)
    for key, w, bar in (("mean_gradient", want[0], bars[0]), ("saliency", want[1], bars[1])):
        assert res[key].shape == (w.shape[2], w.shape[1], 3)
        assert np.abs(res[key][:, :, 0] - w.mean(axis=0).T).max() <= bar
        q = np.quantile(w, (tail, 1 - tail), axis=0)
        assert np.abs(res[key][:, :, 1] - q[0].T).max() <= bar and np.abs(res[key][:, :, 2] - q[1].T).max() <= bar


def test_get_saliency_on_config2_network():
    case, inp, want = _case_data("config2_network")
    res = bn.get_saliency(inp["x"], case["n_out"], bn.ActFun(fun=case["fun"]), bn.SoftMax, inp["weights"],
                          [np.zeros(len(case["nodes"]))] * case["sets"], None)
    _against_restatement(res, want)
    total = want[1].mean(axis=0).sum(axis=0)
    order = res["ranking"]
    assert sorted(order.tolist()) == list(range(case["features"]))
    assert np.all(np.diff(total[order]) <= 2 * case["n_out"] * TOL)      # (the order of the restatement's totals, to the bars of a sum over the outputs)


def test_saliency_of_a_checkpoint(tmp_path):
    """bn.saliency on a checkpoint written by postLogger, against the float64 restatement over its stored samples."""
    rs = np.random.default_rng(4)
    n = 300
    x = np.zeros((n, 5))
    x[:, 0] = rs.normal(0, 1, n)
    x[:, 1] = rs.integers(0, 4, n)
    x[:, 2:] = rs.normal(0, 1, (n, 3))
    x[:, 3] = x[:, 0] + 0.1 * x[:, 3]
    labels = (x[:, 0] + 0.5 * x[:, 1] > 1).astype(int) + (x[:, 2] > 0)
    dat = dict(data=x, labels=labels, test_data=np.zeros((0, 5)), test_labels=np.zeros(0))
    np.random.seed(1234)
    bnn = bn.npBNN(dat, n_nodes=[6, 4], actFun=bn.ActFun(fun="tanh"), use_bias_node=2)
    mcmc = bn.MCMC(bnn, n_iteration=200, sampling_f=20, print_f=1000, n_post_samples=10)
    logger = bn.postLogger(bnn, wdir=str(tmp_path), filename="saliency", log_all_weights=0)
    quiet(bn.run_mcmc, bnn, mcmc, logger)
    res = bn.saliency(logger._pklfile)
    _, _, lg = bn.load_obj(logger._pklfile)
    weights = [s["weights"] for s in lg._post_weight_samples]
    want = sc.means(x.astype(np.float32).astype(np.float64), weights)
    assert res["saliency"].shape == (5, 3, 3) and res["samples"]["saliency"].shape == (len(weights), 3, 5)
    _against_restatement(res, want)
