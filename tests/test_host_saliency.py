"""Input-gradient saliency on the host (no GPU): the float64 restatement of tests/saliency_cases.py against central finite
differences of the oracle's forward pass and against closed forms, get_saliency / saliency's bookkeeping with the device seam
replaced by the restatement, the ABI entry, and the guards of tests/test_hip_saliency.py's case table."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import npbnn_amd as bn
import oracle as orc
import pdp_cases
import saliency_cases as sc
from attrib_common import fake_checkpoint
from npbnn_amd import _capi as capi
from test_hip_pdp import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = pdp_cases.load()
SAL_MOD = importlib.import_module("npbnn_amd.saliency")
ACTS = {"relu": dict(fun="ReLU"), "leaky": dict(fun="ReLU", trainable=True), "genrelu": dict(fun="genReLU", slopes=[[0.1, 0.3], [0.45, 0.02]]),
        "swish": dict(fun="swish"), "tanh": dict(fun="tanh")}


def _small(seed=3, rows=40, features=6, nodes=(5, 4), n_out=4, sets=2, bias=1):
    rs = np.random.default_rng(seed)
    x = rs.standard_normal((rows, features))
    dims = [features] + list(nodes) + [n_out]
    weights = [[rs.normal(0, 1.0 / np.sqrt(dims[i] + 1), (dims[i + 1], dims[i] + bias)) for i in range(len(dims) - 1)] for _ in range(sets)]
    return x, weights


def _away_from_kinks(x, weights, kw):
    """the rows on which no hidden pre-activation of any set lies within MARGIN of zero (all of them for a smooth activation)"""
    if kw["fun"] not in sc.PIECEWISE:
        return x
    keep = np.ones(x.shape[0], dtype=bool)
    for s, w in enumerate(weights):
        act = sc._act(kw["fun"], None if kw.get("slopes") is None else kw["slopes"][s], kw.get("trainable", False))
        keep &= np.abs(sc.hidden_preactivations(x, w, act)).min(axis=1) >= sc.MARGIN
    assert keep.sum() >= 0.9 * x.shape[0]
    return x[keep]


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("apply_out", [True, False], ids=["applied", "raw"])
@pytest.mark.parametrize("out", ["softmax", "identity", "softplus_half"])
@pytest.mark.parametrize("act", list(ACTS))
def test_gradients_equal_central_differences(act, out, apply_out):
    """h = 1e-6: rounding contributes about 1e-16 / 1e-6 = 1e-10 and truncation about h^2 = 1e-12, so 1e-7 holds with room; a
    wrong derivative is wrong by a share of the gradient itself, of order 0.1."""
    kw = ACTS[act]
    x, weights = _small()
    x = _away_from_kinks(x, weights, kw)
    got = sc.gradients(x, weights, out=out, apply_out=apply_out, **kw)
    assert got.shape == (2, x.shape[0], 4, 6) and np.abs(got).max() > 0.01
    out_fn = pdp_cases.OUT_FNS[out] if apply_out else orc.out_identity
    h = 1e-6
    for s, w in enumerate(weights):
        a = sc._act(kw["fun"], None if kw.get("slopes") is None else kw["slopes"][s], kw.get("trainable", False))
        for j in range(x.shape[1]):
            hi, lo = np.array(x, copy=True), np.array(x, copy=True)
            hi[:, j] += h
            lo[:, j] -= h
            fd = (orc.forward(hi, w, a, out_fn) - orc.forward(lo, w, a, out_fn)) / (2 * h)
            assert np.abs(got[s, :, :, j] - fd).max() < 1e-7, (s, j)


@pytest.mark.parametrize("bias", [0, 1])
def test_closed_form_of_a_linear_network(bias):
    x, weights = _small(nodes=(), n_out=3, sets=3, bias=bias)
    mean, absolute, sq = sc.means(x, weights, out="identity")
    for s, w in enumerate(weights):
        m = w[0][:, bias:]
        assert np.abs(mean[s] - m).max() < 1e-14 and np.abs(absolute[s] - np.abs(m)).max() < 1e-14 and np.abs(sq[s] - m * m).max() < 1e-14


def test_softmax_gradients_sum_to_zero_over_the_classes():
    x, weights = _small()
    g = sc.gradients(x, weights)
    assert np.abs(g).max() > 0.01 and np.abs(g.sum(axis=2)).max() < 1e-14


def test_overridden_columns_are_exactly_zero():
    x, weights = _small()
    co = np.full(x.shape[1], np.nan)
    co[1], co[4] = 0.7, -1.2
    res = sc.means(x, weights, override=co)
    plain = sc.means(x, weights)
    for a, b in zip(res, plain):
        assert np.all(a[:, :, [1, 4]] == 0) and np.abs(a[:, :, [0, 2, 3, 5]]).min() > 0
        assert np.abs(a[:, :, [0, 2, 3, 5]] - b[:, :, [0, 2, 3, 5]]).max() > 1e-4      # (the other columns see the constants)


# ---- get_saliency / saliency through the stand-in ------------------------------------------------------------------------------------
@pytest.fixture
def oracle_seam(monkeypatch):
    monkeypatch.setattr(SAL_MOD, "_saliency_means", sc.oracle_seam)


def _args(case):
    a = pdp_cases.call_args(bn, case)
    return (a[0], a[3]) + tuple(a[4:])


@pytest.mark.parametrize("name", ["continuous", "genrelu", "regression_onehot"])
def test_get_saliency_shapes_and_summary(name, oracle_seam):
    c = FIXTURE[name]
    args = _args(c)
    res = bn.get_saliency(*args, level=0.8)
    n_sets, n_out, f = len(c["weights"]), int(c["n_out"]), c["x"].shape[1]
    assert set(res) == {"mean_gradient", "saliency", "rms_gradient", "samples", "sign_probability", "ranking"}
    assert set(res["samples"]) == {"mean_gradient", "saliency", "rms_gradient"}
    for key in ("mean_gradient", "saliency", "rms_gradient"):
        smp = res["samples"][key]
        assert smp.shape == (n_sets, n_out, f) and res[key].shape == (f, n_out, 3)
        assert np.abs(res[key][:, :, 0] - smp.mean(axis=0).T).max() < 1e-12
        q = np.quantile(smp, (0.1, 0.9), axis=0)
        assert np.abs(res[key][:, :, 1] - q[0].T).max() < 1e-12 and np.abs(res[key][:, :, 2] - q[1].T).max() < 1e-12
    smp = res["samples"]
    assert np.all(smp["saliency"] >= np.abs(smp["mean_gradient"]) - 1e-15) and np.all(smp["rms_gradient"] >= smp["saliency"] - 1e-15)
    assert np.abs(smp["saliency"]).max() > 1e-3
    assert res["sign_probability"].shape == (f, n_out)
    assert np.array_equal(res["sign_probability"], (smp["mean_gradient"] > 0).mean(axis=0).T)
    assert sorted(res["ranking"].tolist()) == list(range(f))
    total = res["saliency"][:, :, 0].sum(axis=1)
    assert np.all(np.diff(total[res["ranking"]]) <= 0)
    assert np.array_equal(np.asarray(args[2]._prm, dtype=float), c["last_prm"])        # the last sample's slopes stay installed


def test_ranking_and_sign_probability_on_a_known_order(oracle_seam):
    """One matrix, identity output: the saliency of feature j is |W[:, j]| whatever the data, so columns of known size give the
    order, equal ones fall back on the index, and the signs of W give the sign probabilities."""
    rs = np.random.default_rng(5)
    x = rs.standard_normal((30, 5))
    size = np.array([0.5, 3.0, 0.5, 2.0, 1.0])
    base = np.array([[1.0, -1.0, 1.0, 1.0, -1.0], [1.0, 1.0, -1.0, 1.0, -1.0]])
    weights = [[np.concatenate([np.zeros((2, 1)), base * size * (1 + 0.1 * s)], axis=1)] for s in range(4)]
    weights[3][0][0, 1 + 3] *= -1          # one of four samples with a negative weight on (feature 3, output 0)
    res = bn.get_saliency(x, 2, bn.ActFun(fun="tanh"), bn.RegressTransform, weights, [np.zeros(0)] * 4, None)
    assert res["ranking"].tolist() == [1, 3, 4, 0, 2]
    assert np.array_equal(res["sign_probability"], np.array([[1, 1], [0, 1], [1, 0], [0.75, 1], [0, 0]]))


def test_every_sample_runs_with_its_own_slopes(oracle_seam):
    c = FIXTURE["genrelu"]
    args = _args(c)
    res = bn.get_saliency(*args)
    weights, alphas = args[4], args[5]
    assert len({tuple(np.asarray(a).ravel()) for a in alphas}) > 1
    for s in range(len(weights)):
        own = sc.means(c["x"], [weights[s]], fun="genReLU", slopes=[np.asarray(alphas[s], dtype=float)])
        assert np.abs(res["samples"]["saliency"][s] - own[1][0]).max() < 1e-12
    shared = sc.means(c["x"], weights, fun="genReLU", slopes=[np.asarray(alphas[0], dtype=float)] * len(weights))
    assert np.abs(res["samples"]["saliency"] - shared[1]).max() > 1e-6


def test_get_saliency_refusals(oracle_seam):
    args = _args(FIXTURE["continuous"])
    with pytest.raises(ValueError):
        bn.get_saliency(*args[:4], [], [], args[6])
    for level in (0.0, 1.0):
        with pytest.raises(ValueError):
            bn.get_saliency(*args, level=level)
    with pytest.raises(ValueError):
        bn.get_saliency(args[0], args[1] + 1, *args[2:])
    with pytest.raises(ValueError):
        bn.get_saliency(args[0], args[1], args[2], lambda z: z * z, *args[4:])


def test_saliency_reads_checkpoint(oracle_seam, monkeypatch):
    """saliency(pickle_file): the model's matrices, activation and output function, the logger's samples and the model's feature
    indicators go into get_saliency."""
    c = FIXTURE["indicators"]
    args = pdp_cases.call_args(bn, c)
    x, _, mode, n_out, act, out_fn, weights, alphas, transform = args
    x_test = x[::3] + 0.25
    checkpoint = fake_checkpoint(args, c, _test_data=x_test)
    monkeypatch.setattr(SAL_MOD, "load_obj", lambda path: checkpoint)
    off = np.asarray(c["indicators"]) == 0
    assert off.any() and not off.all()
    res = bn.saliency("checkpoint.pkl")
    direct = bn.get_saliency(x, n_out, act, out_fn, weights, alphas, transform)
    for key in ("mean_gradient", "saliency", "rms_gradient"):
        assert np.array_equal(res[key], direct[key])
        assert np.all(res[key][off] == 0) and np.abs(res[key][~off]).max() > 0
    on_test = bn.saliency("checkpoint.pkl", which="test")
    want = bn.get_saliency(x_test, n_out, act, out_fn, weights, alphas, transform)
    assert np.array_equal(on_test["saliency"], want["saliency"]) and not np.array_equal(on_test["saliency"], res["saliency"])
    with pytest.raises(ValueError):
        bn.saliency("checkpoint.pkl", which="validation")


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_entry():
    txt = open(os.path.join(ROOT, "include", "npbnn_hip.h")).read()
    assert "#define NPBNN_ABI_VERSION 1" in txt and re.search(r"NPBNN_INFO_SALIENCY_ROUTE\s*=\s*27\b", txt)
    res, args = capi.SIGNATURES["npbnn_predict_saliency"]
    assert res is ctypes.c_int and len(args) == 10 and capi.INFO_SALIENCY_ROUTE == 27
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "npbnn_predict_saliency") and lib.npbnn_abi_version() == 1
    assert callable(bn.get_saliency) and callable(bn.saliency) and hasattr(bn.HipContext, "predict_saliency")


# ---- the guards of tests/test_hip_saliency.py: its references can tell a wrong kernel from a right one -------------------------------
_shared = {}


def _case_data(name):
    if name not in _shared:
        case = sc.CASES[name]
        inp = sc.inputs(case)
        _shared[name] = (case, inp, sc.reference(case, inp))
    return _shared[name]


@pytest.mark.parametrize("name", list(sc.CASES))
def test_case_references_are_finite_and_tell_sets_apart(name):
    case, inp, want = _case_data(name)
    f = inp["table"].shape[1]
    if case["fun"] in sc.PIECEWISE and case["nodes"]:
        assert inp["min_preactivation"] >= sc.MARGIN and inp["redrawn"] <= sc.MAX_REDRAWN, (inp["min_preactivation"], inp["redrawn"])
    for a in want:
        assert a.shape == (case["sets"], case["n_out"], f) and np.all(np.isfinite(a))
    on = np.ones(f, dtype=bool) if inp["override"] is None else np.isnan(inp["override"])
    assert on.sum() >= f - 2
    # (the mean square through its root: a gradient of 0.03 is 1500 bars, its square 45)
    for a in (want[0], want[1], np.sqrt(want[2])):
        assert np.all(a[:, :, ~on] == 0) and np.abs(a[:, :, on]).max() > 100 * TOL
        for s in range(1, case["sets"]):
            assert np.abs(a[s] - a[s - 1]).max() > 100 * TOL
    if case["which"] == 1:
        assert inp["x_test"].shape[0] != inp["x"].shape[0]


@pytest.mark.parametrize("wrong", ["no_factor", "softmax_diagonal"])
def test_a_wrong_restatement_is_far_from_the_reference(wrong):
    case, inp, want = _case_data("sets_3_two_a_launch")        # (the defaults)
    got = sc.reference(case, inp, wrong=wrong)
    # (the mean square through its root, as above: on these draws it is below 1e-3 itself, 50 bars)
    for a, b in [(got[0], want[0]), (got[1], want[1]), (np.sqrt(got[2]), np.sqrt(want[2]))]:
        assert np.abs(a - b).max() > 100 * TOL * max(1.0, np.abs(b).max())


def test_case_table_covers_what_it_names():
    cases = list(sc.CASES.values())
    assert {c["rows"] for c in cases} >= {1, 255, 256, 257, 2111} and {c["features"] for c in cases} >= {31, 32, 33, 64, 65, 256, 700}
    assert {(c["sets"], c["nodes"][0]) for c in cases if c["nodes"]} >= {(s, h) for s in (1, 2, 3, 7) for h in (20, 40)}
    assert {(c["fun"], c["trainable"], c["slopes"]) for c in cases} >= {("ReLU", False, None), ("ReLU", True, None), ("genReLU", False, "shared"),
                                                                         ("genReLU", False, "per_set"), ("swish", False, None), ("tanh", False, None)}
    assert {(c["out"], c["apply_out"]) for c in cases} == {(o, a) for o in ("softmax", "identity", "softplus_half") for a in (True, False)}
    assert {(c["n_out"], c["route"]) for c in cases} >= {(1, 1), (7, 1), (32, 1), (33, 2)}
    assert {(c["nodes"][0], c["route"]) for c in cases if c["nodes"]} >= {(1, 1), (31, 1), (32, 1), (33, 1), (64, 1), (65, 2), (130, 2)}
    assert {(c["nodes"][1], c["route"]) for c in cases if len(c["nodes"]) > 1} >= {(32, 1), (33, 2)}
    assert {len(c["nodes"]) + 1 for c in cases} >= {1, 5} and {c["bias"] for c in cases} >= {"all", "none", "mixed01", "mixed10"}
    assert all(c["reroute"] == (c["route"] == 1 and not c["env"]) for c in cases)
    assert max(c["rows"] for c in cases) <= 3000
