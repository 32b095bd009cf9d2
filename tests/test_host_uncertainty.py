"""Posterior uncertainty decomposition on the host (no GPU): ``posterior_uncertainty`` against the reference's values
(tests/golden/uncertainty.npz), ``get_posterior_uncertainty`` over a float64 stand-in of the device context, argument checks that raise
before any device call, and the new symbol in the header and the binding."""
import importlib
import os
import pickle
import re
import types

import numpy as np
import pytest

import npbnn_amd as bn
import oracle as orc
import uncertainty_cases as uc
from npbnn_amd import _capi as capi

posterior = importlib.import_module("npbnn_amd.posterior")
backend = importlib.import_module("npbnn_amd.backend")
uncertainty = importlib.import_module("npbnn_amd.uncertainty")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11                      # test_host_lppd's figure: float64 against float64
ACT_KINDS = {capi.ACT_RELU: "ReLU", capi.ACT_LEAKY: "genReLU", capi.ACT_SWISH: "swish", capi.ACT_TANH: "tanh"}
OUT_KINDS = {capi.OUT_SOFTMAX: "classification", capi.OUT_IDENTITY: "regression", capi.OUT_SOFTPLUS_HALF: "regression-error"}
OUT_FNS = {"classification": bn.SoftMax, "regression": bn.RegressTransform, "regression-error": bn.RegressTransformError}
CLASS_KEYS = sorted(uc.CLASS_FIELDS + tuple(uc.CLASS_TOTALS) + ("predicted_class", "n_samples", "n_rows"))
REGRESSION_ARRAYS = ("mean", "epistemic_var", "aleatoric_var", "total_var")
REGRESSION_KEYS = sorted(REGRESSION_ARRAYS + tuple(k + "_avg" for k in REGRESSION_ARRAYS) + ("n_samples", "n_rows"))


class Float64Context:
    """HipContext's posterior interface on float64 numpy arrays (the oracle's forward pass): what the device calls compute, in the
    precision of the reference, with a log of the calls.  (The pattern of test_host_lppd.Float64Context.)"""
    log = []

    def __init__(self, device=None):
        self.n_rows = {}

    def set_data(self, X, which=capi.TRAIN):
        Float64Context.log.append("set_data")
        self.x = np.array(X, dtype=np.float64)
        self.n_rows[which] = len(self.x)

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

    def _values(self, weight_sets, act_prm_sets):
        return np.array([orc.forward_logits(self.x, self._layers(w), orc.Act(self.fun, np.zeros(1) if act_prm_sets is None else act_prm_sets[i]))
                         for i, w in enumerate(weight_sets)])

    def predict_sets(self, weight_sets, act_prm_sets=None, which=capi.TRAIN, apply_out_fn=True):
        Float64Context.log.append("predict_sets")
        z = self._values(weight_sets, act_prm_sets)
        return uc.outputs_from_values(z, OUT_KINDS[self.out_kind]) if apply_out_fn else z

    def predict_sets_uncertainty(self, weight_sets, act_prm_sets=None, which=capi.TRAIN, pointwise=True):
        """HipContext.predict_sets_uncertainty's dict from the restatement on the oracle's values (no sigma under OUT_IDENTITY)."""
        Float64Context.log.append("predict_sets_uncertainty")
        kind = OUT_KINDS[self.out_kind]
        z = self._values(list(weight_sets), act_prm_sets)
        res = uc.restatement(z, kind, np.zeros((len(z), z.shape[2])))
        if kind == "classification":
            out = {k: (res[k] if pointwise else None) for k in uc.CLASS_FIELDS}
            out["predicted_class"] = np.argmax(res["mean_prob"], axis=1) if pointwise else None
            out.update({t: float(np.mean(res[f])) for t, f in uc.CLASS_TOTALS.items()})
            return out
        if kind == "regression":
            res["aleatoric_var"] = res["total_var"] = None
        out = {k: (res[k] if pointwise else None) for k in REGRESSION_ARRAYS}
        out.update({k + "_avg": (None if res[k] is None else np.mean(res[k], axis=0)) for k in REGRESSION_ARRAYS})
        return out

    def close(self):
        pass


@pytest.fixture
def float64_seam(monkeypatch):
    Float64Context.log = []
    monkeypatch.setattr(backend, "HipContext", Float64Context)
    return Float64Context


def _want(name):
    g = uc.load()
    want = {f: g[uc.key(name, f)] for f in uc.fields_of(name)}
    if uc.CASES[name]["kind"] != "cat":
        want["total_var"] = want["epistemic_var"] + want["aleatoric_var"]
    return want


def _assert_golden(res, name, pointwise=True, flip=False):
    want = _want(name)
    if flip:
        want = {k: v[::-1] for k, v in want.items()}
    if uc.CASES[name]["kind"] == "cat":
        assert sorted(res) == (CLASS_KEYS if pointwise else sorted(tuple(uc.CLASS_TOTALS) + ("n_samples", "n_rows")))
        for total, field in uc.CLASS_TOTALS.items():
            np.testing.assert_allclose(res[total], want[field].mean(), rtol=TOL, atol=TOL, err_msg="%s %s" % (name, total))
        if pointwise:
            for f in uc.CLASS_FIELDS:
                np.testing.assert_allclose(res[f], want[f], rtol=TOL, atol=TOL, err_msg="%s %s" % (name, f))
            np.testing.assert_array_equal(res["predicted_class"], np.argmax(want["mean_prob"], axis=1))
    else:
        assert sorted(res) == (REGRESSION_KEYS if pointwise else sorted(tuple(k + "_avg" for k in REGRESSION_ARRAYS) + ("n_samples", "n_rows")))
        for f in REGRESSION_ARRAYS:
            np.testing.assert_allclose(res[f + "_avg"], want[f].mean(axis=0), rtol=TOL, atol=TOL, err_msg="%s %s_avg" % (name, f))
            if pointwise:
                np.testing.assert_allclose(res[f], want[f], rtol=TOL, atol=TOL, err_msg="%s %s" % (name, f))
    assert (res["n_samples"], res["n_rows"]) == (uc.CASES[name]["s"], uc.N_ROWS)


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def test_golden_file_is_complete():
    g = uc.load()
    assert sorted(g.files) == sorted(uc.key(n, f) for n in uc.CASES for f in uc.fields_of(n))
    assert all(np.all(np.isfinite(g[k])) and g[k].dtype == np.float64 for k in g.files)
    err = [c for c in uc.CASES.values() if c["kind"] == "err"]
    assert {c["n_out"] for c in err} == {2, 4, 6} and {c["s"] for c in err} == {1, 3, 7} and any(c["fun"] == "genReLU" for c in err)
    for name, c in uc.CASES.items():
        if c["kind"] == "cat" and c["s"] > 1:
            assert g[uc.key(name, "mutual_information_i")].max() > 1e-2, name
    assert os.path.getsize(uc.GOLDEN) < 4 * os.path.getsize(os.path.join(os.path.dirname(uc.GOLDEN), "lppd.npz"))


@pytest.mark.parametrize("name", uc.CASES)
def test_posterior_uncertainty_reproduces_the_reference(name):
    inp, kind = uc.inputs(name), uc.kind_of(name)
    res = bn.posterior_uncertainty(uc.outputs_from_values(uc.oracle_values(inp), kind), kind, uc.sigmas_of(inp))
    _assert_golden(res, name)


@pytest.mark.parametrize("name", uc.CASES)
def test_restatement_reproduces_the_reference(name):
    """The term-by-term restatement from pre-output values (the lse form of the entropy) gives the reference's numbers too."""
    inp, want = uc.inputs(name), _want(name)
    res = uc.restatement(uc.oracle_values(inp), uc.kind_of(name), uc.sigmas_of(inp))
    for f in want:
        np.testing.assert_allclose(res[f], want[f], rtol=TOL, atol=TOL, err_msg="%s %s" % (name, f))


def test_one_sample_gives_exact_zeros():
    rs = np.random.default_rng(1)
    p = rs.dirichlet(np.ones(5), (1, 40))
    res = bn.posterior_uncertainty(p)
    assert not res["mutual_information_i"].any() and res["mutual_information"] == 0.0 and res["n_samples"] == 1
    np.testing.assert_array_equal(res["mean_prob"], p[0])
    np.testing.assert_allclose(res["predictive_entropy_i"], res["expected_entropy_i"], rtol=1e-14)
    y = rs.normal(3.0, 2.0, (1, 40, 4))
    res = bn.posterior_uncertainty(y, "regression", sigma_sets=np.array([[0.5, 1.0, 1.5, 2.0]]))
    assert not res["epistemic_var"].any() and not res["epistemic_var_avg"].any()
    np.testing.assert_array_equal(res["mean"], y[0])
    np.testing.assert_array_equal(res["total_var"], np.tile([0.25, 1.0, 2.25, 4.0], (40, 1)))
    res = bn.posterior_uncertainty(np.abs(y), "regression-error")
    assert not res["epistemic_var"].any() and res["mean"].shape == (40, 2)
    np.testing.assert_array_equal(res["total_var"], np.abs(y[0, :, 2:]) ** 2)


def test_exact_zero_probabilities_stay_finite():
    p = np.array([[[1.0, 0.0, 0.0], [0.5, 0.5, 0.0]], [[0.0, 1.0, 0.0], [0.5, 0.0, 0.5]]])
    res = bn.posterior_uncertainty(p)
    assert all(np.all(np.isfinite(res[k])) for k in uc.CLASS_FIELDS)
    np.testing.assert_allclose(res["predictive_entropy_i"], [np.log(2), 1.5 * np.log(2)], rtol=1e-14)
    np.testing.assert_allclose(res["expected_entropy_i"], [0.0, np.log(2)], atol=1e-16)
    np.testing.assert_allclose(res["mutual_information_i"], [np.log(2), 0.5 * np.log(2)], rtol=1e-14)


def test_variance_of_a_large_mean_with_a_tiny_spread():
    """A mean of 1e6 with a spread of 1e-3: the variance is that of the spread, not cancellation noise."""
    rs = np.random.default_rng(2)
    base = 1e6 * rs.uniform(1.0, 2.0, (40, 2))
    wobble = 1e-3 * rs.standard_normal((9, 40, 2))
    mu = base[None] + wobble
    res = bn.posterior_uncertainty(mu, "regression", sigma_sets=np.ones(9))
    exact = np.var(mu - base[None], axis=0)
    np.testing.assert_allclose(res["epistemic_var"], exact, rtol=1e-6)
    np.testing.assert_allclose(res["mean"], base, rtol=1e-9)


@pytest.mark.parametrize("bad", [
    dict(stack=np.zeros((3, 5))), dict(stack=np.zeros((0, 5, 2))), dict(stack=np.zeros((3, 0, 2))), dict(stack=np.zeros((3, 5, 0))),
    dict(stack=np.full((2, 2, 2), np.nan)), dict(stack=np.ones((2, 3, 2)), kind="counts"), dict(stack=np.ones((2, 3, 2)), kind="regression"),
    dict(stack=np.ones((2, 3, 2)), kind="regression", sigma_sets=np.ones((3, 2))), dict(stack=np.ones((2, 3, 3)), kind="regression-error"),
    dict(stack=np.ones((2, 3, 2)), kind="regression", sigma_sets=np.array([[1.0, np.nan], [1.0, 1.0]]))],
    ids=["2d", "no_samples", "no_rows", "no_outputs", "nan", "unknown_kind", "no_sigma", "sigma_shape", "odd_width", "nan_sigma"])
def test_posterior_uncertainty_rejects(bad):
    with pytest.raises(ValueError):
        bn.posterior_uncertainty(**bad)


def test_the_stack_is_not_offered():
    assert hasattr(bn, "posterior_uncertainty") and hasattr(bn, "get_posterior_uncertainty")
    assert not any(hasattr(bn, n) for n in ("posterior_stack", "get_posterior_stack", "uncertainty_stack"))


# ---- checkpoints over the float64 stand-in ------------------------------------------------------------------------------------------
def _checkpoint(tmp_path, inp, name, test=True, samples=None, mode=None, out_fn=None):
    kind = uc.kind_of(name)
    empty = np.zeros((0, uc.N_FEATURES))
    model = types.SimpleNamespace(_data=inp["x"] if not test else inp["x"][::-1].copy(), _test_data=inp["x"] if test else empty,
                                  _act_fun=uc.act_for(bn, inp["fun"], len(inp["nodes"])), _output_act_fun=out_fn if out_fn is not None else OUT_FNS[kind],
                                  _estimation_mode=mode or kind, _size_output=inp["n_out"])
    logger = types.SimpleNamespace(_post_weight_samples=inp["samples"] if samples is None else samples)
    pkl = os.path.join(str(tmp_path), "run.pkl")
    with open(pkl, "wb") as fh:
        pickle.dump([model, None, logger], fh)
    return pkl


@pytest.mark.parametrize("name", uc.CASES)
def test_get_posterior_uncertainty_reproduces_the_reference(name, float64_seam, tmp_path):
    inp = uc.inputs(name)
    pkl = _checkpoint(tmp_path, inp, name)
    _assert_golden(bn.get_posterior_uncertainty(pkl), name)
    assert float64_seam.log.count("predict_sets_uncertainty") == 1 and "predict_sets" not in float64_seam.log and float64_seam.log.count("set_data") == 1
    _assert_golden(bn.get_posterior_uncertainty(pkl, pointwise=False), name, pointwise=False)


@pytest.mark.parametrize("name", ["tanh_h2_c4_s7", "swish_h1_reg3_s4", "tanh_h2_err2_s7"])
def test_training_table_and_a_table_given(name, float64_seam, tmp_path):
    inp = uc.inputs(name)
    pkl = _checkpoint(tmp_path, inp, name, test=False)
    _assert_golden(bn.get_posterior_uncertainty(pkl, features="train"), name)
    pkl = _checkpoint(tmp_path, inp, name, test=True)                 # (its training table is the test table upside down)
    _assert_golden(bn.get_posterior_uncertainty(pkl, features="train"), name, flip=True)
    _assert_golden(bn.get_posterior_uncertainty(pkl, features=inp["x"]), name)


@pytest.mark.parametrize("name", ["tanh_h2_c4_s7", "swish_h1_reg3_s4"])
def test_custom_output_callable_goes_through_the_stack(name, float64_seam, tmp_path, monkeypatch):
    inp, kind = uc.inputs(name), uc.kind_of(name)
    out_fn = orc.out_softmax if kind == "classification" else orc.out_identity
    monkeypatch.setattr(uncertainty, "load_obj", lambda p: [types.SimpleNamespace(
        _test_data=inp["x"], _act_fun=uc.act_for(bn, inp["fun"], len(inp["nodes"])), _output_act_fun=out_fn, _estimation_mode=kind), None,
        types.SimpleNamespace(_post_weight_samples=inp["samples"])])
    res = bn.get_posterior_uncertainty("unused.pkl")
    assert "predict_sets_uncertainty" not in float64_seam.log and float64_seam.log.count("predict_sets") == 1
    _assert_golden(res, name)


# ---- argument checks raise before any device call -----------------------------------------------------------------------------------
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError("device call %s" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(backend, "HipContext", lambda *a, **k: _NoDevice())


def test_get_posterior_uncertainty_argument_checks(no_device, tmp_path):
    name = "tanh_h2_c4_s7"
    inp = uc.inputs(name)
    with pytest.raises(ValueError, match="no posterior samples"):
        bn.get_posterior_uncertainty(_checkpoint(tmp_path, inp, name, samples=[]))
    with pytest.raises(ValueError, match="empty"):
        bn.get_posterior_uncertainty(_checkpoint(tmp_path, inp, name, test=False))
    with pytest.raises(ValueError):
        bn.get_posterior_uncertainty(_checkpoint(tmp_path, inp, name), features="test")
    with pytest.raises(ValueError, match="empty"):
        bn.get_posterior_uncertainty(_checkpoint(tmp_path, inp, name), features=np.zeros((0, uc.N_FEATURES)))
    for mode in ("custom", "poisson", "negbin", "counts"):
        with pytest.raises(ValueError, match="out of scope"):
            bn.get_posterior_uncertainty(_checkpoint(tmp_path, inp, name, mode=mode))
    reg = uc.inputs("tanh_h2_reg1_s7")
    bare = [{k: v for k, v in s.items() if k != "error_prm"} for s in reg["samples"]]
    with pytest.raises(ValueError, match="error_prm"):
        bn.get_posterior_uncertainty(_checkpoint(tmp_path, reg, "tanh_h2_reg1_s7", samples=bare))
    odd = uc.inputs("swish_h1_reg3_s4")                                 # three outputs cannot be means and sigmas
    with pytest.raises(ValueError, match="odd"):
        bn.get_posterior_uncertainty(_checkpoint(tmp_path, odd, "swish_h1_reg3_s4", mode="regression-error", out_fn=bn.RegressTransformError))


def _bare_context(n_rows=10, n_out=3, out_kind=capi.OUT_SOFTMAX):
    ctx = backend.HipContext.__new__(backend.HipContext)
    ctx._lib = _NoDevice()
    ctx._ctx = None
    ctx.n_rows = {capi.TRAIN: n_rows, capi.TEST: 0}
    ctx.n_out = n_out
    ctx.arch = capi.Arch()
    ctx.arch.n_layers = 2
    ctx.arch.out_kind = out_kind
    return ctx


def test_predict_sets_uncertainty_argument_checks():
    ctx = _bare_context()
    sets = [np.zeros(5), np.zeros(5)]
    with pytest.raises(ValueError):
        ctx.predict_sets_uncertainty(sets, act_prm_sets=[np.zeros(1)])                  # one slope vector for two sets
    with pytest.raises(ValueError):
        ctx.predict_sets_uncertainty(sets, which=capi.TEST)                             # no rows
    with pytest.raises(ValueError):
        ctx.predict_sets_uncertainty(np.zeros((0, 5)))                                  # no sets
    ctx.close = lambda: None
    ctx = _bare_context(out_kind=capi.OUT_SOFTPLUS_HALF)
    with pytest.raises(ValueError, match="odd"):
        ctx.predict_sets_uncertainty(sets)
    ctx.close = lambda: None


def test_predictor_checks_the_kind(no_device):
    inp = uc.inputs("tanh_h2_c4_s7")
    pred = posterior._SamplePredictor(uc.N_FEATURES, inp["samples"], uc.act_for(bn, "tanh", 2), bn.SoftMax)
    with pytest.raises(ValueError):
        pred.uncertainty(inp["x"], "counts")
    with pytest.raises(ValueError, match="output function"):
        pred.uncertainty(inp["x"], "regression", sigma_sets=np.ones((7, 4)))
    reg = uc.inputs("swish_h1_reg3_s4")
    pred = posterior._SamplePredictor(uc.N_FEATURES, reg["samples"], uc.act_for(bn, "swish", 1), bn.RegressTransform)
    with pytest.raises(ValueError, match="sigma_sets"):
        pred.uncertainty(reg["x"], "regression")
    with pytest.raises(ValueError, match="sigma_sets"):
        pred.uncertainty(reg["x"], "regression", sigma_sets=np.ones((3, 3)))              # four samples


# ---- the boundary --------------------------------------------------------------------------------------------------------------------
def test_symbol_is_in_the_header_and_the_binding():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "npbnn_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+npbnn_predict_sets_uncertainty\s*\(", txt)
    assert "#define NPBNN_ABI_VERSION 1" in txt and re.search(r"NPBNN_INFO_UNCERTAINTY_FINAL_NS\s*=\s*20\b", txt)
    res, args = capi.SIGNATURES["npbnn_predict_sets_uncertainty"]
    assert len(args) == 10 and capi.INFO_UNCERTAINTY_FINAL_NS == 20
    assert "npbnn_uncertainty.hip" in open(os.path.join(ROOT, "npbnn_amd", "csrc", "Makefile")).read()
