"""Posterior calibration on the host (no GPU): ``posterior_calibration`` against an independent restatement and against the
reference's values (tests/golden/calibration.npz), hand cases, the conditions on the fixture the GPU tests rely on,
``get_posterior_calibration`` over a float64 stand-in of the device context, argument checks that raise before any device call, and
the new symbol in the header and the binding."""
import importlib
import os
import pickle
import re
import types

import numpy as np
import pytest

import npbnn_amd as bn
import calibration_cases as cc
import oracle as orc
from npbnn_amd import _capi as capi

posterior = importlib.import_module("npbnn_amd.posterior")
backend = importlib.import_module("npbnn_amd.backend")
calibration = importlib.import_module("npbnn_amd.calibration")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12                      # relative, float64 against float64
EDGE_EXACT = 1e-9                # no golden row lies this close to an edge
EDGE_F32 = 1e-4                  # the project's float32 budget
MAX_ROWS_NEAR = 4                # 2 % of 203 rows
ACT_KINDS = {capi.ACT_RELU: "ReLU", capi.ACT_LEAKY: "genReLU", capi.ACT_SWISH: "swish", capi.ACT_TANH: "tanh"}
OUT_KINDS = {capi.OUT_SOFTMAX: "classification", capi.OUT_IDENTITY: "regression", capi.OUT_SOFTPLUS_HALF: "regression-error"}
OUT_FNS = {"classification": bn.SoftMax, "regression": bn.RegressTransform, "regression-error": bn.RegressTransformError}


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1e-300, np.abs(want)))) if got.size else 0.0


def _definition(name, z=None):
    inp, kind = cc.inputs(name), cc.kind_of(name)
    n_bins, levels = cc.params(name)
    z = cc.oracle_values(inp) if z is None else z
    return bn.posterior_calibration(cc.outputs_from_values(z, kind), inp["labels"], kind, n_bins, levels, cc.sigmas_of(inp)), inp, kind, z


def _assert_same(res, want, name, fields, tables):
    for f in fields:
        if f == "predicted_class":
            np.testing.assert_array_equal(res[f], want[f], err_msg="%s %s" % (name, f))
        else:
            assert _rel(res[f], want[f]) <= TOL, (name, f, _rel(res[f], want[f]))
    for f in tables:
        if f == "sum_confidence":
            assert _rel(res[f], want[f]) <= TOL, (name, f)
        else:
            np.testing.assert_array_equal(res[f], want[f], err_msg="%s %s" % (name, f))


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def test_golden_file_is_complete():
    g = cc.load()
    assert sorted(g.files) == sorted(cc.key(n, f) for n in cc.CASES for f in cc.fields_of(n))
    assert all(np.all(np.isfinite(g[k])) for k in g.files)
    assert os.path.getsize(cc.GOLDEN) < 512 * 1024
    assert {cc.params(n)[0] for n in cc.CASES} == {1, 10, 15, 64}
    assert {cc.params(n)[1] for n in cc.CASES if cc.CASES[n]["kind"] != "cat"} == {(), (0.9,), cc.DEFAULT_LEVELS}
    assert all(cc.inputs(n)["labels"].shape == (cc.N_ROWS, cc.CASES[n]["n_out"] // 2) for n in cc.uc.ERROR_CASES)


@pytest.mark.parametrize("name", cc.CASES)
def test_posterior_calibration_equals_the_restatement_and_the_reference(name):
    res, inp, kind, z = _definition(name)
    n_bins, levels = cc.params(name)
    want = cc.restatement(z, inp["labels"], kind, cc.sigmas_of(inp), n_bins, levels)
    tables = cc.CLASS_TABLES if kind == "classification" else cc.REGRESSION_TABLES
    _assert_same(res, want, name, cc.point_fields_of(name), tables)
    for f in cc.score_fields_of(name):
        if want[f] is None:
            assert res[f] is None and not levels
        else:
            assert _rel(res[f], want[f]) <= TOL, (name, f)
    g = cc.load()
    _assert_same(res, {f: g[cc.key(name, f)] for f in cc.fields_of(name)}, name, cc.point_fields_of(name), tables)
    assert (res["n_samples"], res["n_rows"], res["n_bins"]) == (cc.CASES[name]["s"], cc.N_ROWS, n_bins)
    if kind == "classification":
        assert res["count"].sum() == cc.N_ROWS and res["n_correct"].sum() == round(res["accuracy"] * cc.N_ROWS)
        assert "levels" not in res
    else:
        assert np.all(res["pit_hist"].sum(axis=1) == cc.N_ROWS) and res["covered"].shape == (res["pit"].shape[1], len(levels))
        np.testing.assert_array_equal(res["levels"], levels)


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------------
def test_one_sample():
    p = np.array([[[0.7, 0.2, 0.1], [0.1, 0.3, 0.6], [0.25, 0.5, 0.25]]])
    res = bn.posterior_calibration(p, [0, 1, 1], n_bins=4)
    np.testing.assert_array_equal(res["confidence"], [0.7, 0.6, 0.5])
    np.testing.assert_array_equal(res["predicted_class"], [0, 2, 1])
    np.testing.assert_array_equal(res["count"], [0, 0, 3, 0])
    np.testing.assert_array_equal(res["n_correct"], [0, 0, 2, 0])
    np.testing.assert_allclose(res["nll_i"], -np.log([0.7, 0.3, 0.5]), rtol=1e-15)
    np.testing.assert_allclose(res["brier_i"], [0.09 + 0.04 + 0.01, 0.01 + 0.49 + 0.36, 0.0625 + 0.25 + 0.0625], rtol=1e-14)
    assert res["n_samples"] == 1 and abs(res["ece"] - abs(2 / 3 - 1.8 / 3)) < 1e-15 and res["mce"] == res["ece"]
    y = np.array([[[1.0, -2.0], [0.5, 0.0]]])
    res = bn.posterior_calibration(y, [[1.0, 0.0], [0.5, 1.0]], "regression", n_bins=4, levels=(0.5,), sigma_sets=[[1.0, 2.0]])
    np.testing.assert_array_equal(res["mean"], y[0])
    np.testing.assert_array_equal(res["pit"][:, 0], [0.5, 0.5])
    np.testing.assert_allclose(res["pit"][:, 1], [0.8413447460685429, 0.6914624612740131], rtol=1e-15)
    np.testing.assert_array_equal(res["covered"], [[2], [1]])
    np.testing.assert_array_equal(res["pit_hist"], [[0, 0, 2, 0], [0, 0, 1, 1]])
    np.testing.assert_array_equal(res["sq_err"], [[0.0, 4.0], [0.0, 1.0]])


def test_one_bin_compares_accuracy_with_the_mean_confidence():
    rs = np.random.default_rng(3)
    p = rs.dirichlet(np.ones(4), (5, 60))
    lab = rs.integers(0, 4, 60)
    res = bn.posterior_calibration(p, lab, n_bins=1)
    assert res["count"].tolist() == [60]
    assert abs(res["ece"] - abs(res["accuracy"] - res["confidence"].mean())) < 1e-15 and res["mce"] == res["ece"]


def test_a_confidence_of_exactly_one_lands_in_the_last_bin():
    p = np.array([[[1.0, 0.0], [0.0, 1.0]], [[1.0, 0.0], [0.0, 1.0]]])
    for n_bins in (1, 10, 15, 64):
        res = bn.posterior_calibration(p, [0, 0], n_bins=n_bins)
        assert res["count"][-1] == 2 and res["count"].sum() == 2 and res["n_correct"][-1] == 1
        assert res["nll_i"][0] == 0.0 and res["nll_i"][1] == np.inf and res["nll"] == np.inf      # (a value, not an error)
        assert res["sum_confidence"][-1] == 2.0


def test_a_target_a_million_sigmas_away():
    mu = np.zeros((3, 2, 1))
    res = bn.posterior_calibration(mu, [[1e6], [-1e6]], "regression", n_bins=10, levels=cc.DEFAULT_LEVELS + (0.999999,), sigma_sets=np.ones(3))
    np.testing.assert_array_equal(res["pit"], [[1.0], [0.0]])
    np.testing.assert_array_equal(res["pit_hist"], [[1, 0, 0, 0, 0, 0, 0, 0, 0, 1]])
    assert not res["covered"].any() and not res["coverage"].any()
    np.testing.assert_allclose(res["coverage_error"], [np.mean(cc.DEFAULT_LEVELS + (0.999999,))], rtol=1e-15)
    res = bn.posterior_calibration(np.concatenate([mu, np.ones((3, 2, 1))], axis=2), [[1e6], [-1e6]], "regression-error", n_bins=10, levels=(0.95,))
    np.testing.assert_array_equal(res["pit"], [[1.0], [0.0]])
    assert not res["covered"].any()


def test_a_tie_takes_the_first_class():
    p = np.array([[[0.4, 0.4, 0.2], [0.2, 0.4, 0.4]], [[0.4, 0.4, 0.2], [0.2, 0.4, 0.4]]])
    res = bn.posterior_calibration(p, [1, 2], n_bins=5)
    np.testing.assert_array_equal(res["predicted_class"], [0, 1])
    assert res["accuracy"] == 0.0 and res["count"].tolist() == [0, 0, 2, 0, 0]


# ---- conditions on the fixture: the GPU tests cannot hide behind rows that sit on an edge -------------------------------------------------
@pytest.mark.parametrize("name", cc.CASES)
def test_golden_rows_keep_clear_of_the_edges(name):
    g = cc.load()
    cat = cc.CASES[name]["kind"] == "cat"
    values = g[cc.key(name, "confidence" if cat else "pit")]
    assert cc.rows_near_an_edge(name, values, EDGE_EXACT) == 0, name
    near = cc.rows_near_an_edge(name, values, EDGE_F32, g[cc.key(name, "top_two_gap")] if cat else None, 2 * EDGE_F32)
    assert near <= MAX_ROWS_NEAR, (name, near)


# ---- checkpoints over a float64 stand-in -----------------------------------------------------------------------------------------------------
class Float64Context:
    """HipContext's calibration interface on float64 numpy arrays (the oracle's forward pass), with a log of the calls.  (The
    pattern of test_host_uncertainty.Float64Context.)"""
    log = []

    def __init__(self, device=None):
        self.n_rows = {}

    def set_data(self, X, which=capi.TRAIN):
        Float64Context.log.append("set_data")
        self.x = np.array(X, dtype=np.float64)

    def set_labels(self, labels, which=capi.TRAIN):
        Float64Context.log.append("set_labels")
        self.y = np.asarray(labels)

    def set_targets(self, targets, which=capi.TRAIN):
        Float64Context.log.append("set_targets")
        self.y = np.asarray(targets)

    def set_arch_from_weights(self, weights, in_dim, act_kind, out_kind, lik_kind):
        self.shapes = [w.shape for w in weights]
        self.fun = ACT_KINDS[act_kind]
        self.out_kind = out_kind

    def _values(self, weight_sets, act_prm_sets):
        def layers(packed):
            out, at = [], 0
            for s in self.shapes:
                out.append(np.asarray(packed[at:at + s[0] * s[1]]).reshape(s))
                at += s[0] * s[1]
            return out
        return np.array([orc.forward_logits(self.x, layers(w), orc.Act(self.fun, np.zeros(1) if act_prm_sets is None else act_prm_sets[i]))
                         for i, w in enumerate(weight_sets)])

    def predict_sets(self, weight_sets, act_prm_sets=None, which=capi.TRAIN, apply_out_fn=True):
        Float64Context.log.append("predict_sets")
        z = self._values(weight_sets, act_prm_sets)
        return cc.outputs_from_values(z, OUT_KINDS[self.out_kind]) if apply_out_fn else z

    def predict_sets_calibration(self, weight_sets, n_bins=15, levels=cc.DEFAULT_LEVELS, sigma_sets=None, act_prm_sets=None, which=capi.TRAIN,
                                 pointwise=True):
        Float64Context.log.append("predict_sets_calibration")
        kind = OUT_KINDS[self.out_kind]
        z = self._values(list(weight_sets), act_prm_sets)
        res = cc.restatement(z, self.y, kind, sigma_sets, n_bins, levels)
        res.update(n_samples=len(z), n_rows=len(self.x), n_bins=n_bins)
        if kind != "classification":
            res["levels"] = np.asarray(levels, dtype=np.float64)
        return res if pointwise else {k: (None if k in cc.CLASS_POINT + cc.REGRESSION_POINT else v) for k, v in res.items()}

    def close(self):
        pass


@pytest.fixture
def float64_seam(monkeypatch):
    Float64Context.log = []
    monkeypatch.setattr(backend, "HipContext", Float64Context)
    return Float64Context


def _checkpoint(tmp_path, inp, name, test=True, samples=None, mode=None, out_fn=None, labels=None):
    kind = cc.kind_of(name)
    labels = inp["labels"] if labels is None else labels
    empty = np.zeros((0, cc.N_FEATURES))
    model = types.SimpleNamespace(_data=inp["x"] if not test else inp["x"][::-1].copy(), _labels=labels if not test else labels[::-1].copy(),
                                  _test_data=inp["x"] if test else empty, _test_labels=labels if test else labels[:0],
                                  _act_fun=cc.act_for(bn, inp["fun"], len(inp["nodes"])), _output_act_fun=out_fn if out_fn is not None else OUT_FNS[kind],
                                  _estimation_mode=mode or kind, _size_output=inp["n_out"])
    logger = types.SimpleNamespace(_post_weight_samples=inp["samples"] if samples is None else samples)
    pkl = os.path.join(str(tmp_path), "run.pkl")
    with open(pkl, "wb") as fh:
        pickle.dump([model, None, logger], fh)
    return pkl


def _assert_golden(res, name, pointwise=True, flip=False):
    g = cc.load()
    kind = cc.kind_of(name)
    tables = cc.CLASS_TABLES if kind == "classification" else cc.REGRESSION_TABLES
    want = {f: g[cc.key(name, f)] for f in cc.point_fields_of(name) + tables}
    if flip:
        want.update({f: want[f][::-1] for f in cc.point_fields_of(name)})
    _assert_same(res, want, name, cc.point_fields_of(name) if pointwise else (), tables)
    assert all((f in res) == pointwise for f in cc.point_fields_of(name))
    assert all(f in res for f in cc.score_fields_of(name))
    assert (res["n_samples"], res["n_rows"]) == (cc.CASES[name]["s"], cc.N_ROWS)


@pytest.mark.parametrize("name", ["tanh_h2_c4_s7", "genrelu_h2_c10_s64", "swish_h1_reg3_s4", "relu_h2_reg4_s64", "tanh_h2_err2_s7", "genrelu_h2_err1_s3"])
def test_get_posterior_calibration_reproduces_the_reference(name, float64_seam, tmp_path):
    inp = cc.inputs(name)
    n_bins, levels = cc.params(name)
    pkl = _checkpoint(tmp_path, inp, name)
    _assert_golden(bn.get_posterior_calibration(pkl, n_bins=n_bins, levels=levels), name)
    assert float64_seam.log.count("predict_sets_calibration") == 1 and "predict_sets" not in float64_seam.log
    assert float64_seam.log.count("set_labels" if cc.kind_of(name) == "classification" else "set_targets") == 1
    _assert_golden(bn.get_posterior_calibration(pkl, n_bins=n_bins, levels=levels, pointwise=False), name, pointwise=False)
    _assert_golden(bn.get_posterior_calibration(pkl, features="train", n_bins=n_bins, levels=levels), name, flip=True)
    _assert_golden(bn.get_posterior_calibration(pkl, features=inp["x"], labels=inp["labels"], n_bins=n_bins, levels=levels), name)


@pytest.mark.parametrize("name", ["tanh_h2_c4_s7", "swish_h1_reg3_s4"])
def test_custom_output_callable_goes_through_the_stack(name, float64_seam, tmp_path, monkeypatch):
    inp, kind = cc.inputs(name), cc.kind_of(name)
    n_bins, levels = cc.params(name)
    out_fn = orc.out_softmax if kind == "classification" else orc.out_identity
    monkeypatch.setattr(calibration, "load_obj", lambda p: [types.SimpleNamespace(
        _test_data=inp["x"], _test_labels=inp["labels"], _act_fun=cc.act_for(bn, inp["fun"], len(inp["nodes"])), _output_act_fun=out_fn,
        _estimation_mode=kind), None, types.SimpleNamespace(_post_weight_samples=inp["samples"])])
    res = bn.get_posterior_calibration("unused.pkl", n_bins=n_bins, levels=levels)
    assert "predict_sets_calibration" not in float64_seam.log and float64_seam.log.count("predict_sets") == 1
    _assert_golden(res, name)


# ---- argument checks raise before any device call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [
    dict(stack=np.zeros((3, 5)), labels=np.zeros(5, dtype=int)), dict(stack=np.zeros((0, 5, 2)), labels=np.zeros(5, dtype=int)),
    dict(stack=np.full((2, 2, 2), np.nan), labels=[0, 1]), dict(stack=np.ones((2, 3, 2)), labels=[0, 1, 0], kind="counts"),
    dict(stack=np.ones((2, 3, 2)), labels=[0, 1, 2]), dict(stack=np.ones((2, 3, 2)), labels=[0, -1, 1]), dict(stack=np.ones((2, 3, 2)), labels=[0, 1]),
    dict(stack=np.ones((2, 3, 2)), labels=[0.5, 1, 1]), dict(stack=np.ones((2, 3, 2)), labels=[0, 1, 1], n_bins=0),
    dict(stack=np.ones((2, 3, 2)), labels=[0, 1, 1], n_bins=65), dict(stack=np.ones((2, 3, 2)), labels=[0, 1, 1], n_bins=2.5),
    dict(stack=np.ones((2, 3, 2)), labels=[0, 1, 1], sigma_sets=np.ones(2)),
    dict(stack=np.ones((2, 3, 2)), labels=np.ones((3, 2)), kind="regression"),
    dict(stack=np.ones((2, 3, 2)), labels=np.ones((3, 2)), kind="regression", sigma_sets=np.ones((3, 2))),
    dict(stack=np.ones((2, 3, 2)), labels=np.ones((3, 2)), kind="regression", sigma_sets=np.array([[1.0, 0.0], [1.0, 1.0]])),
    dict(stack=np.ones((2, 3, 2)), labels=np.ones((3, 2)), kind="regression", sigma_sets=np.array([[1.0, np.inf], [1.0, 1.0]])),
    dict(stack=np.ones((2, 3, 2)), labels=np.ones((3, 1)), kind="regression", sigma_sets=np.ones((2, 2))),
    dict(stack=np.ones((2, 3, 2)), labels=np.full((3, 2), np.nan), kind="regression", sigma_sets=np.ones((2, 2))),
    dict(stack=np.ones((2, 3, 2)), labels=np.ones((3, 2)), kind="regression", sigma_sets=np.ones((2, 2)), levels=(0.5, 1.0)),
    dict(stack=np.ones((2, 3, 2)), labels=np.ones((3, 2)), kind="regression", sigma_sets=np.ones((2, 2)), levels=(0.0,)),
    dict(stack=np.ones((2, 3, 2)), labels=np.ones((3, 2)), kind="regression", sigma_sets=np.ones((2, 2)), levels=np.linspace(0.1, 0.9, 17)),
    dict(stack=np.ones((2, 3, 3)), labels=np.ones((3, 1)), kind="regression-error"),
    dict(stack=np.ones((2, 3, 2)), labels=np.ones((3, 1)), kind="regression-error", sigma_sets=np.ones((2, 1)))],
    ids=["2d", "no_samples", "nan", "unknown_kind", "label_too_large", "label_negative", "label_count", "label_fraction", "no_bins", "too_many_bins",
         "fractional_bins", "sigma_with_classes", "no_sigma", "sigma_shape", "zero_sigma", "infinite_sigma", "target_width", "nan_target", "level_one",
         "level_zero", "too_many_levels", "odd_width", "sigma_with_predicted_sigma"])
def test_posterior_calibration_rejects(bad):
    with pytest.raises(ValueError):
        bn.posterior_calibration(**bad)


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError("device call %s" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(backend, "HipContext", lambda *a, **k: _NoDevice())


def test_get_posterior_calibration_argument_checks(no_device, tmp_path):
    name = "tanh_h2_c4_s7"
    inp = cc.inputs(name)
    with pytest.raises(ValueError, match="no posterior samples"):
        bn.get_posterior_calibration(_checkpoint(tmp_path, inp, name, samples=[]))
    with pytest.raises(ValueError, match="empty"):
        bn.get_posterior_calibration(_checkpoint(tmp_path, inp, name, test=False))
    with pytest.raises(ValueError):
        bn.get_posterior_calibration(_checkpoint(tmp_path, inp, name), features="test")
    with pytest.raises(ValueError, match="needs its labels"):
        bn.get_posterior_calibration(_checkpoint(tmp_path, inp, name), features=inp["x"])
    with pytest.raises(ValueError, match="class indices"):
        bn.get_posterior_calibration(_checkpoint(tmp_path, inp, name), features=inp["x"], labels=inp["labels"] + 1)
    with pytest.raises(ValueError, match="labels for"):
        bn.get_posterior_calibration(_checkpoint(tmp_path, inp, name), features=inp["x"], labels=inp["labels"][:-1])
    with pytest.raises(ValueError, match="n_bins"):
        bn.get_posterior_calibration(_checkpoint(tmp_path, inp, name), n_bins=65)
    with pytest.raises(ValueError, match="level"):
        bn.get_posterior_calibration(_checkpoint(tmp_path, inp, name), levels=(1.5,))
    for mode in ("custom", "poisson", "negbin", "counts"):
        with pytest.raises(ValueError, match="out of scope.*custom.*count likelihoods"):
            bn.get_posterior_calibration(_checkpoint(tmp_path, inp, name, mode=mode))
    reg = cc.inputs("tanh_h2_reg1_s7")
    bare = [{k: v for k, v in s.items() if k != "error_prm"} for s in reg["samples"]]
    with pytest.raises(ValueError, match="error_prm"):
        bn.get_posterior_calibration(_checkpoint(tmp_path, reg, "tanh_h2_reg1_s7", samples=bare))
    with pytest.raises(ValueError, match="targets are"):
        bn.get_posterior_calibration(_checkpoint(tmp_path, reg, "tanh_h2_reg1_s7", labels=np.ones((cc.N_ROWS, 2))))
    odd = cc.inputs("swish_h1_reg3_s4")                                 # three outputs cannot be means and sigmas
    with pytest.raises(ValueError, match="odd"):
        bn.get_posterior_calibration(_checkpoint(tmp_path, odd, "swish_h1_reg3_s4", mode="regression-error", out_fn=bn.RegressTransformError))


def _bare_context(n_rows=10, n_out=3, out_kind=capi.OUT_SOFTMAX):
    ctx = backend.HipContext.__new__(backend.HipContext)
    ctx._lib = _NoDevice()
    ctx._ctx = None
    ctx.n_rows = {capi.TRAIN: n_rows, capi.TEST: 0}
    ctx.n_out = n_out
    ctx.arch = capi.Arch()
    ctx.arch.n_layers = 2
    ctx.arch.out_kind = out_kind
    ctx.close = lambda: None
    return ctx


def test_predict_sets_calibration_argument_checks():
    ctx = _bare_context()
    sets = [np.zeros(5), np.zeros(5)]
    for kw in (dict(act_prm_sets=[np.zeros(1)]), dict(which=capi.TEST), dict(n_bins=0), dict(n_bins=65), dict(levels=(0.0,)), dict(sigma_sets=np.ones(2))):
        with pytest.raises(ValueError):
            ctx.predict_sets_calibration(sets, **kw)
    with pytest.raises(ValueError):
        ctx.predict_sets_calibration(np.zeros((0, 5)))
    ctx = _bare_context(out_kind=capi.OUT_SOFTPLUS_HALF)
    with pytest.raises(ValueError, match="odd"):
        ctx.predict_sets_calibration(sets)
    ctx = _bare_context(out_kind=capi.OUT_IDENTITY)
    for sig in (None, np.ones((3, 3)), np.zeros((2, 3)), np.full((2, 3), np.nan)):
        with pytest.raises(ValueError):
            ctx.predict_sets_calibration(sets, sigma_sets=sig)


def test_predictor_checks_the_kind(no_device):
    inp = cc.inputs("tanh_h2_c4_s7")
    pred = posterior._SamplePredictor(cc.N_FEATURES, inp["samples"], cc.act_for(bn, "tanh", 2), bn.SoftMax)
    with pytest.raises(ValueError):
        pred.calibration(inp["x"], inp["labels"], "counts")
    with pytest.raises(ValueError, match="output function"):
        pred.calibration(inp["x"], inp["labels"], "regression", sigma_sets=np.ones((7, 4)))
    reg = cc.inputs("swish_h1_reg3_s4")
    pred = posterior._SamplePredictor(cc.N_FEATURES, reg["samples"], cc.act_for(bn, "swish", 1), bn.RegressTransform)
    with pytest.raises(ValueError, match="sigma_sets"):
        pred.calibration(reg["x"], reg["labels"], "regression")


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_in_the_header_and_the_binding():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "npbnn_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+npbnn_predict_sets_calibration\s*\(", txt)
    assert "#define NPBNN_ABI_VERSION 1" in txt and re.search(r"NPBNN_INFO_CALIBRATION_FINAL_NS\s*=\s*25\b", txt)
    res, args = capi.SIGNATURES["npbnn_predict_sets_calibration"]
    assert len(args) == 16 and capi.INFO_CALIBRATION_FINAL_NS == 25
    assert "npbnn_calibration.hip" in open(os.path.join(ROOT, "npbnn_amd", "csrc", "Makefile")).read()
    assert hasattr(bn, "posterior_calibration") and hasattr(bn, "get_posterior_calibration")
