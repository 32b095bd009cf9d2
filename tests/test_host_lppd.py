"""Log pointwise predictive density and WAIC on the host (no GPU): ``posterior_lppd`` against the reference's values
(tests/golden/lppd.npz), ``get_posterior_lppd`` over a float64 stand-in of the device context, argument checks that raise before any
device call, and the new symbol in the header and the binding."""
import importlib
import os
import pickle
import re
import types

import numpy as np
import pytest

import lppd_cases as lc
import npbnn_amd as bn
import oracle as orc
from npbnn_amd import _capi as capi

posterior = importlib.import_module("npbnn_amd.posterior")
backend = importlib.import_module("npbnn_amd.backend")
lppd = importlib.import_module("npbnn_amd.lppd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11                      # the oracle tests' figure (test_oracle_golden): float64 against float64
ACT_KINDS = {capi.ACT_RELU: "ReLU", capi.ACT_LEAKY: "genReLU", capi.ACT_SWISH: "swish", capi.ACT_TANH: "tanh"}
TOTALS = {"lppd": "lppd_i", "mean_log_lik": "mean_log_lik_i", "p_waic": "p_waic_i"}


class Float64Context:
    """HipContext's posterior interface on float64 numpy arrays (the oracle's forward pass): what the device calls compute, in the
    precision of the reference, with a log of the calls.  (The pattern of test_host_importance.Float64Context.)"""
    log = []

    def __init__(self, device=None):
        self.n_rows = {}

    def set_data(self, X, which=capi.TRAIN):
        Float64Context.log.append("set_data")
        self.x = np.array(X, dtype=np.float64)
        self.n_rows[which] = len(self.x)

    def set_labels(self, labels, which=capi.TRAIN):
        Float64Context.log.append("set_labels")
        self.labels = np.asarray(labels)

    def set_targets(self, targets, which=capi.TRAIN):
        Float64Context.log.append("set_targets")
        self.labels = np.asarray(targets, dtype=np.float64)

    def set_arch_from_weights(self, weights, in_dim, act_kind, out_kind, lik_kind):
        self.shapes = [w.shape for w in weights]
        self.fun = ACT_KINDS[act_kind]
        self.out_kind = out_kind

    def _layers(self, packed):
        out, at = [], 0
        for s in self.shapes:
            out.append(np.asarray(packed[at:at + s[0] * s[1]]).reshape(s))
            at += s[0] * s[1]
        return out

    def predict_sets(self, weight_sets, act_prm_sets=None, which=capi.TRAIN, apply_out_fn=True):
        Float64Context.log.append("predict_sets")
        out = []
        for i, w in enumerate(weight_sets):
            act = orc.Act(self.fun, np.zeros(1) if act_prm_sets is None else act_prm_sets[i])
            z = orc.forward_logits(self.x, self._layers(w), act)
            out.append(orc.out_softmax(z) if (apply_out_fn and self.out_kind == capi.OUT_SOFTMAX) else z)
        return np.array(out)

    def predict_sets_lppd(self, weight_sets, lik_kind, sigma_sets=None, act_prm_sets=None, which=capi.TRAIN, pointwise=True):
        Float64Context.log.append("predict_sets_lppd")
        assert (lik_kind == capi.LIK_CATEGORICAL) == (self.out_kind == capi.OUT_SOFTMAX) and (sigma_sets is None) == (lik_kind == capi.LIK_CATEGORICAL)
        z = self.predict_sets(list(weight_sets), act_prm_sets, apply_out_fn=False)
        del Float64Context.log[-1]
        ll = lc.log_lik_from_values(z, self.labels, "cat" if lik_kind == capi.LIK_CATEGORICAL else "reg", sigma_sets)
        res = lppd.posterior_lppd(ll)
        out = {k: res[k] for k in ("lppd", "mean_log_lik", "p_waic", "log_lik_sample")}
        out.update({k: (res[k] if pointwise else None) for k in ("lppd_i", "mean_log_lik_i", "p_waic_i")})
        return out

    def close(self):
        pass


@pytest.fixture
def float64_seam(monkeypatch):
    Float64Context.log = []
    monkeypatch.setattr(backend, "HipContext", Float64Context)
    return Float64Context


def _assert_golden(res, name, pointwise=True):
    g = lc.load()
    for total, field in TOTALS.items():
        want = g[lc.key(name, field)]
        if pointwise:
            np.testing.assert_allclose(res[field], want, rtol=TOL, atol=TOL, err_msg="%s %s" % (name, field))
        np.testing.assert_allclose(res[total], want.sum(), rtol=TOL, atol=TOL, err_msg="%s %s" % (name, total))
    np.testing.assert_allclose(res["log_lik_sample"], g[lc.key(name, "log_lik_sample")], rtol=TOL, atol=TOL)
    assert res["elpd_waic"] == res["lppd"] - res["p_waic"] and res["waic"] == -2.0 * res["elpd_waic"]
    assert (res["n_samples"], res["n_rows"]) == (lc.CASES[name]["s"], lc.N_ROWS)


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def test_golden_file_is_complete():
    g = lc.load()
    assert sorted(g.files) == sorted(lc.key(n, f) for n in lc.CASES for f in lc.FIELDS)
    assert all(np.all(np.isfinite(g[k])) and g[k].dtype == np.float64 for k in g.files)
    assert {c["s"] for c in lc.CASES.values()} == {1, 2, 3, 4, 7, 64} and {c["n_out"] for c in lc.CASES.values() if c["kind"] == "cat"} == {2, 3, 4, 10}
    assert {c["fun"] for c in lc.CASES.values()} == {"ReLU", "genReLU", "swish", "tanh"} and {len(c["nodes"]) for c in lc.CASES.values()} == {1, 2, 3}
    assert os.path.getsize(lc.GOLDEN) < os.path.getsize(os.path.join(os.path.dirname(lc.GOLDEN), "support.npz")) // 4


@pytest.mark.parametrize("name", lc.CASES)
def test_posterior_lppd_reproduces_the_reference(name):
    _assert_golden(bn.posterior_lppd(lc.oracle_log_lik(lc.inputs(name))), name)


def test_one_sample():
    ll = np.random.default_rng(1).normal(-3, 2, (1, 50))
    res = bn.posterior_lppd(ll)
    np.testing.assert_array_equal(res["lppd_i"], ll[0])
    np.testing.assert_array_equal(res["mean_log_lik_i"], ll[0])
    assert not res["p_waic_i"].any() and res["p_waic"] == 0.0 and res["elpd_waic"] == res["lppd"] and res["n_samples"] == 1


def test_variance_of_large_values_with_a_tiny_spread():
    """|ll| ~ 1e6 with a spread of 1e-3: the variance is that of the spread, not cancellation noise, and lppd stays finite."""
    rs = np.random.default_rng(2)
    base = -1e6 * rs.uniform(1.0, 2.0, 40)
    wobble = 1e-3 * rs.standard_normal((9, 40))
    ll = base[None, :] + wobble
    res = bn.posterior_lppd(ll)
    exact = np.var(ll - base[None, :], axis=0, ddof=1)       # (the subtraction is exact to ~1e-10 here: a power-of-two-scaled offset)
    np.testing.assert_allclose(res["p_waic_i"], exact, rtol=1e-6)
    assert np.all(np.isfinite(res["lppd_i"])) and np.all(np.abs(res["lppd_i"] - base) < 0.01)


def test_underflowing_rows_stay_finite():
    ll = np.array([[-2000.0, -1.0], [-2001.0, -800.0]])
    res = bn.posterior_lppd(ll)
    np.testing.assert_allclose(res["lppd_i"], [-2000.0 + np.log(1 + np.exp(-1.0)) - np.log(2), -1.0 - np.log(2)], rtol=1e-14)


@pytest.mark.parametrize("bad", [np.zeros(5), np.zeros((0, 5)), np.zeros((3, 0)), np.array([[np.nan, 1.0]])], ids=["1d", "no_samples", "no_rows", "nan"])
def test_posterior_lppd_rejects(bad):
    with pytest.raises(ValueError):
        bn.posterior_lppd(bad)


def test_pointwise_log_lik_is_not_offered():
    assert not hasattr(bn, "pointwise_log_lik") and hasattr(bn, "posterior_lppd") and hasattr(bn, "get_posterior_lppd")


# ---- checkpoints over the float64 stand-in ------------------------------------------------------------------------------------------
def _checkpoint(tmp_path, inp, test=True, samples=None, mode=None, out_fn=None):
    reg = inp["kind"] == "reg"
    empty_x, empty_y = np.zeros((0, lc.N_FEATURES)), (np.zeros((0, inp["n_out"])) if reg else np.zeros(0, dtype=int))
    model = types.SimpleNamespace(_data=inp["x"] if not test else inp["x"][::-1].copy(), _labels=inp["labels"] if not test else inp["labels"][::-1].copy(),
                                  _test_data=inp["x"] if test else empty_x, _test_labels=inp["labels"] if test else empty_y,
                                  _act_fun=lc.act_for(bn, inp["fun"], len(inp["nodes"])),
                                  _output_act_fun=out_fn if out_fn is not None else (bn.RegressTransform if reg else bn.SoftMax),
                                  _estimation_mode=mode or ("regression" if reg else "classification"), _size_output=inp["n_out"])
    logger = types.SimpleNamespace(_post_weight_samples=inp["samples"] if samples is None else samples)
    pkl = os.path.join(str(tmp_path), "run.pkl")
    with open(pkl, "wb") as fh:
        pickle.dump([model, None, logger], fh)
    return pkl


@pytest.mark.parametrize("name", lc.CASES)
def test_get_posterior_lppd_reproduces_the_reference(name, float64_seam, tmp_path):
    inp = lc.inputs(name)
    pkl = _checkpoint(tmp_path, inp)
    res = bn.get_posterior_lppd(pkl, pointwise=True)
    _assert_golden(res, name)
    assert float64_seam.log.count("predict_sets_lppd") == 1 and "predict_sets" not in float64_seam.log and float64_seam.log.count("set_data") == 1
    assert sorted(res) == sorted(["lppd", "mean_log_lik", "p_waic", "elpd_waic", "waic", "n_samples", "n_rows", "log_lik_sample",
                                  "lppd_i", "mean_log_lik_i", "p_waic_i"])
    lean = bn.get_posterior_lppd(pkl)
    assert sorted(lean) == sorted(["lppd", "mean_log_lik", "p_waic", "elpd_waic", "waic", "n_samples", "n_rows", "log_lik_sample"])
    _assert_golden(lean, name, pointwise=False)


@pytest.mark.parametrize("name", ["tanh_h2_c4_s7", "swish_h1_reg3_s4"])
def test_training_table_and_a_table_given(name, float64_seam, tmp_path):
    inp = lc.inputs(name)
    pkl = _checkpoint(tmp_path, inp, test=False)
    _assert_golden(bn.get_posterior_lppd(pkl, features="train", pointwise=True), name)
    pkl = _checkpoint(tmp_path, inp, test=True)                 # (its training table is the test table upside down)
    res = bn.get_posterior_lppd(pkl, features="train", pointwise=True)
    g = lc.load()
    np.testing.assert_allclose(res["lppd_i"], g[lc.key(name, "lppd_i")][::-1], rtol=TOL, atol=TOL)
    _assert_golden(bn.get_posterior_lppd(pkl, features=inp["x"], labels=inp["labels"], pointwise=True), name)


def test_custom_output_callable_goes_through_the_stack(float64_seam, tmp_path, monkeypatch):
    inp = lc.inputs("tanh_h2_c4_s7")
    monkeypatch.setattr(lppd, "load_obj", lambda p: [types.SimpleNamespace(
        _test_data=inp["x"], _test_labels=inp["labels"], _act_fun=lc.act_for(bn, "tanh", 2), _output_act_fun=orc.out_softmax,
        _estimation_mode="classification"), None, types.SimpleNamespace(_post_weight_samples=inp["samples"])])
    res = bn.get_posterior_lppd("unused.pkl", pointwise=True)
    assert "predict_sets_lppd" not in float64_seam.log and float64_seam.log.count("predict_sets") == 1
    _assert_golden(res, "tanh_h2_c4_s7")


# ---- argument checks raise before any device call -----------------------------------------------------------------------------------
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError("device call %s" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(backend, "HipContext", lambda *a, **k: _NoDevice())


def test_get_posterior_lppd_argument_checks(no_device, tmp_path):
    inp = lc.inputs("tanh_h2_c4_s7")
    with pytest.raises(ValueError, match="no posterior samples"):
        bn.get_posterior_lppd(_checkpoint(tmp_path, inp, samples=[]))
    with pytest.raises(ValueError, match="empty"):
        bn.get_posterior_lppd(_checkpoint(tmp_path, inp, test=False))
    pkl = _checkpoint(tmp_path, inp)
    for labels in (np.full(lc.N_ROWS, 0.5), np.full(lc.N_ROWS, 4), np.full(lc.N_ROWS, -1), np.zeros((lc.N_ROWS, 1)), np.zeros(lc.N_ROWS - 1)):
        with pytest.raises(ValueError):
            bn.get_posterior_lppd(pkl, features=inp["x"], labels=labels)
    with pytest.raises(ValueError, match="labels"):
        bn.get_posterior_lppd(pkl, features=inp["x"])
    with pytest.raises(ValueError):
        bn.get_posterior_lppd(pkl, features="test")
    with pytest.raises(ValueError, match="out of scope"):
        bn.get_posterior_lppd(_checkpoint(tmp_path, inp, mode="regression-error"))
    reg = lc.inputs("tanh_h2_reg1_s7")
    bare = [{k: v for k, v in s.items() if k != "error_prm"} for s in reg["samples"]]
    with pytest.raises(ValueError, match="error_prm"):
        bn.get_posterior_lppd(_checkpoint(tmp_path, reg, samples=bare))
    with pytest.raises(ValueError, match="targets"):
        bn.get_posterior_lppd(_checkpoint(tmp_path, reg), features=reg["x"], labels=np.zeros((lc.N_ROWS, 2)))
    negative = [dict(s, error_prm=-np.asarray(s["error_prm"])) for s in reg["samples"]]
    with pytest.raises(ValueError, match="positive"):
        bn.get_posterior_lppd(_checkpoint(tmp_path, reg, samples=negative))


def _bare_context(n_rows=10, n_out=3):
    ctx = backend.HipContext.__new__(backend.HipContext)
    ctx._lib = _NoDevice()
    ctx._ctx = None
    ctx.n_rows = {capi.TRAIN: n_rows, capi.TEST: 0}
    ctx.n_out = n_out
    ctx.arch = capi.Arch()
    ctx.arch.n_layers = 2
    return ctx


def test_predict_sets_lppd_argument_checks():
    ctx = _bare_context()
    sets = [np.zeros(5), np.zeros(5)]
    for kind in (capi.LIK_GAUSS_PRED_SIGMA, capi.LIK_POISSON, capi.LIK_NEGBIN, capi.LIK_NONE, 99):
        with pytest.raises(ValueError, match="out of scope"):
            ctx.predict_sets_lppd(sets, kind)
    with pytest.raises(ValueError):
        ctx.predict_sets_lppd(sets, capi.LIK_GAUSS)                                     # no sigma
    with pytest.raises(ValueError):
        ctx.predict_sets_lppd(sets, capi.LIK_CATEGORICAL, sigma_sets=np.ones((2, 3)))    # sigma without the Gaussian likelihood
    with pytest.raises(ValueError):
        ctx.predict_sets_lppd(sets, capi.LIK_GAUSS, sigma_sets=np.ones((3, 3)))          # not one row per set
    with pytest.raises(ValueError):
        ctx.predict_sets_lppd(sets, capi.LIK_GAUSS, sigma_sets=np.ones((2, 2)))          # not one column per output
    for bad in (0.0, -1.0, np.inf, np.nan):
        sig = np.ones((2, 3))
        sig[1, 2] = bad
        with pytest.raises(ValueError, match="positive"):
            ctx.predict_sets_lppd(sets, capi.LIK_GAUSS, sigma_sets=sig)
    with pytest.raises(ValueError):
        ctx.predict_sets_lppd(sets, capi.LIK_CATEGORICAL, act_prm_sets=[np.zeros(1)])    # one slope vector for two sets
    with pytest.raises(ValueError):
        ctx.predict_sets_lppd(sets, capi.LIK_CATEGORICAL, which=capi.TEST)               # no rows
    with pytest.raises(ValueError):
        ctx.predict_sets_lppd(np.zeros((0, 5)), capi.LIK_CATEGORICAL)                    # no sets
    ctx.close = lambda: None


# ---- the boundary --------------------------------------------------------------------------------------------------------------------
def test_symbol_is_in_the_header_and_the_binding():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "npbnn_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+npbnn_predict_sets_lppd\s*\(", txt)
    assert "#define NPBNN_ABI_VERSION 1" in txt
    res, args = capi.SIGNATURES["npbnn_predict_sets_lppd"]
    assert len(args) == 12 and capi.INFO_LPPD_FINAL_NS == 19
    assert "npbnn_lppd.hip" in open(os.path.join(ROOT, "npbnn_amd", "csrc", "Makefile")).read()
