"""The posterior predictive distribution on the host: ``posterior_predictive`` (the definition in plain numpy) against the independent
restatement of tests/predictive_cases.py under its acceptance rules, the closed forms of a single component, and every refusal of
``posterior_predictive`` and ``get_posterior_predictive`` - the latter's before any device context is built (the context is replaced
by one that fails when built, or by a float64 stand-in)."""
import importlib
import math
import os
import pickle
import types

import numpy as np
import pytest

import npbnn_amd as bn
import oracle as orc
import predictive_cases as pc
from npbnn_amd import _capi as capi

backend = importlib.import_module("npbnn_amd.backend")

KEYS = sorted(("n_samples", "n_rows", "probs", "quantiles", "mean", "crps_i", "crps"))


def _as_stack(mu, sg, sigma_cols):
    """(stack, kind, sigma_sets): per-cell sigmas as the second half of the outputs, per-sample ones beside the stack"""
    n = len(mu)
    if sigma_cols == 0:
        return np.concatenate([mu.reshape(n, 1, -1), sg.reshape(n, 1, -1)], axis=2), "regression-error", None
    return mu.reshape(n, -1, sigma_cols), "regression", sg


# ---- the definition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n_cols,sigma_cols", [(1, 3, 0), (2, 6, 3), (3, 5, 1), (64, 2, 0), (65, 3, 3), (257, 3, 0)])
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_posterior_predictive_equals_the_restatement(family, S, n_cols, sigma_cols):
    mu, sg, y = pc.make(family, S, n_cols, sigma_cols)
    stack, kind, sigma = _as_stack(mu, sg, sigma_cols)
    res = bn.posterior_predictive(stack, kind, sigma_sets=sigma, probs=pc.PROBS, targets=y.reshape(stack.shape[1], -1))
    n_t = stack.shape[2] // 2 if sigma is None else stack.shape[2]
    assert sorted(res) == KEYS and (res["n_samples"], res["n_rows"]) == (S, stack.shape[1]) and np.array_equal(res["probs"], pc.PROBS)
    assert res["quantiles"].shape == (5, stack.shape[1], n_t) and res["mean"].shape == res["crps_i"].shape == (stack.shape[1], n_t)
    label = "%s S=%d cols=%d sigma_cols=%d" % (family, S, n_cols, sigma_cols)
    worst, by_root = pc.check_quantiles(res["quantiles"].reshape(5, -1), mu, sg, pc.PROBS, sigma_cols > 0, label)
    worst_crps = pc.check_crps(res["crps_i"].ravel(), mu, sg, y, sigma_cols > 0, label)
    print("host %s: largest residual / bound %.3f, %d cells by the root, largest CRPS difference / bound %.4f" % (label, worst, by_root, worst_crps))
    assert np.array_equal(res["mean"].ravel(), pc.mean_of(mu))
    assert np.array_equal(res["crps"], np.sum(res["crps_i"], axis=0) / stack.shape[1])
    assert np.all(np.diff(res["quantiles"], axis=0) >= 0)                        # non-decreasing in p


def test_closed_forms_of_a_single_component():
    rs = np.random.default_rng(4)
    mu, sg, y = rs.normal(0, 3, (1, 7, 2)), np.exp(rs.normal(0, 1, (1, 2))), rs.normal(0, 4, (7, 2))
    res = bn.posterior_predictive(mu, "regression", sigma_sets=sg, probs=pc.PROBS, targets=y)
    for j, p in enumerate(pc.PROBS):
        np.testing.assert_allclose(res["quantiles"][j], mu[0] + sg * pc.normal_quantile(p), rtol=1e-13, atol=0)
    u = (y - mu[0]) / sg
    phi = np.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
    big_phi = np.array([[0.5 * math.erfc(-v / math.sqrt(2)) for v in row] for row in u])
    np.testing.assert_allclose(res["crps_i"], sg * (u * (2 * big_phi - 1) + 2 * phi - 1 / math.sqrt(math.pi)), rtol=1e-12, atol=1e-14)
    assert np.array_equal(res["mean"], mu[0])
    bare = bn.posterior_predictive(mu, "regression", sigma_sets=sg[:, 0], probs=())
    assert sorted(bare) == sorted(k for k in KEYS if not k.startswith("crps")) and bare["quantiles"].shape == (0, 7, 2)


def test_quantiles_do_not_decrease_in_p():
    mu, sg, _ = pc.make("wide", 9, 4)
    stack, kind, _ = _as_stack(mu, sg, 0)
    probs = np.sort(np.concatenate([np.linspace(0.01, 0.99, 12), [1e-12, 1e-6, 1 - 1e-6, 1 - 2e-12]]))
    res = bn.posterior_predictive(stack, kind, probs=probs)
    assert np.all(np.diff(res["quantiles"], axis=0) > 0)
    shuffled = bn.posterior_predictive(stack, kind, probs=probs[::-1])             # (no ordering is required)
    assert np.array_equal(shuffled["quantiles"][::-1], res["quantiles"])


def test_posterior_predictive_refusals():
    ok, sig, t = np.random.default_rng(0).standard_normal((6, 4, 2)), np.ones((6, 2)), np.zeros((4, 2))
    pos = np.concatenate([ok, np.exp(ok)], axis=2)
    for bad in (dict(stack=ok[:, :, 0], sigma_sets=sig), dict(stack=ok[:, :0], sigma_sets=sig), dict(stack=np.zeros((0, 4, 2)), sigma_sets=sig),
                dict(stack=ok, sigma_sets=sig, kind="classification"), dict(stack=ok, sigma_sets=sig, kind="counts"), dict(stack=ok),
                dict(stack=ok, sigma_sets=sig[:5]), dict(stack=ok, sigma_sets=np.ones((6, 3))), dict(stack=ok, sigma_sets=sig * 0), dict(stack=ok, sigma_sets=-sig),
                dict(stack=ok, sigma_sets=sig * np.inf), dict(stack=ok, sigma_sets=sig, targets=t[:3]), dict(stack=ok, sigma_sets=sig, targets=t[:, :1]),
                dict(stack=ok, sigma_sets=sig, targets=t + np.nan), dict(stack=ok, sigma_sets=sig, targets=t + np.inf),
                dict(stack=ok, sigma_sets=sig, probs=(0.0,)), dict(stack=ok, sigma_sets=sig, probs=(1.0,)), dict(stack=ok, sigma_sets=sig, probs=(0.5, 1e-13)),
                dict(stack=ok, sigma_sets=sig, probs=(0.5, 1 - 1e-13)), dict(stack=ok, sigma_sets=sig, probs=(float("nan"),)),
                dict(stack=ok, sigma_sets=sig, probs=np.linspace(0.1, 0.9, 17)), dict(stack=np.zeros((16385, 1, 1)), sigma_sets=np.ones(16385)),
                dict(stack=pos[:, :, :3], kind="regression-error"), dict(stack=pos, kind="regression-error", sigma_sets=sig),
                dict(stack=np.concatenate([ok, np.abs(ok) * 0], axis=2), kind="regression-error"), dict(stack=np.concatenate([ok, -np.exp(ok)], axis=2), kind="regression-error")):
        with pytest.raises(ValueError, match="posterior_predictive"):
            bn.posterior_predictive(**bad)
    for v in (np.nan, np.inf, -np.inf):
        bad = ok.copy()
        bad[5, 1, 1] = v
        with pytest.raises(ValueError, match="NaN or infinite"):
            bn.posterior_predictive(bad, sigma_sets=sig)
    assert bn.posterior_predictive(ok, sigma_sets=sig, probs=(1e-12, 1 - 2e-12, 0.5) * 5 + (0.3,))["quantiles"].shape == (16, 4, 2)    # (the caps pass)
    assert bn.posterior_predictive(pos, "regression-error", targets=t)["crps"].shape == (2,)


# ---- checkpoints --------------------------------------------------------------------------------------------------------------------
N_FEATURES = 5


def _samples(n, n_out=2, seed=0, error_prm=True, genrelu=False):
    rs = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = dict(weights=[rs.normal(0, 0.3, (4, N_FEATURES + 1)), rs.normal(0, 0.3, (n_out, 5))], alphas=rs.uniform(0, 0.3, 1) if genrelu else np.zeros(1), mcmc_it=i)
        if error_prm:
            s["error_prm"] = np.exp(rs.normal(-0.5, 0.3, n_out))
        out.append(s)
    return out


def _checkpoint(tmp_path, name, samples, mode="regression", out_fn=bn.RegressTransform, fun="tanh", n_targets=2, test_rows=7):
    rs = np.random.default_rng(99)
    x, y = rs.standard_normal((11, N_FEATURES)), rs.standard_normal((11, n_targets))
    act = bn.ActFun(fun=fun, prm=np.zeros(1)) if fun == "genReLU" else bn.ActFun(fun=fun)
    model = types.SimpleNamespace(_data=x, _labels=y, _test_data=x[:test_rows], _test_labels=y[:test_rows], _act_fun=act, _output_act_fun=out_fn,
                                  _estimation_mode=mode)
    pkl = os.path.join(str(tmp_path), name + ".pkl")
    with open(pkl, "wb") as fh:
        pickle.dump([model, None, types.SimpleNamespace(_post_weight_samples=samples)], fh)
    return pkl, x, y


class NoDevice:
    def __init__(self, *a, **k):
        raise AssertionError("a device context was built")


def test_get_posterior_predictive_refuses_before_any_device_call(tmp_path, monkeypatch):
    monkeypatch.setattr(backend, "HipContext", NoDevice)
    who = "get_posterior_predictive"
    good, x, y = _checkpoint(tmp_path, "good", _samples(6))
    with pytest.raises(ValueError, match=who + ".*no posterior samples"):
        bn.get_posterior_predictive(_checkpoint(tmp_path, "none", [])[0])
    for mode in ("classification", "custom", "count"):
        with pytest.raises(ValueError, match=who + ".*%r is out of scope" % mode):
            bn.get_posterior_predictive(_checkpoint(tmp_path, mode, _samples(6), mode=mode, out_fn=bn.SoftMax)[0])
    with pytest.raises(ValueError, match=who + ".*error_prm"):
        bn.get_posterior_predictive(_checkpoint(tmp_path, "bare", _samples(6, error_prm=False))[0])
    with pytest.raises(ValueError, match=who + ".*odd"):
        bn.get_posterior_predictive(_checkpoint(tmp_path, "odd", _samples(6, n_out=3), mode="regression-error", out_fn=bn.RegressTransformError)[0])
    with pytest.raises(ValueError, match=who + ".*targets are"):
        bn.get_posterior_predictive(good, features=x, labels=y[:5])
    with pytest.raises(ValueError, match=who + ".*targets are"):
        bn.get_posterior_predictive(_checkpoint(tmp_path, "narrow", _samples(6), n_targets=1)[0])
    for v in (np.nan, np.inf):
        with pytest.raises(ValueError, match=who + ".*NaN or infinite"):
            bn.get_posterior_predictive(good, features=x, labels=np.where(np.arange(22).reshape(11, 2) == 7, v, y))
    for probs in ((0.0,), (1.0,), (0.5, 1e-13), (float("nan"),), (-0.1,)):
        with pytest.raises(ValueError, match=who + ".*min\\(p, 1 - p\\)"):
            bn.get_posterior_predictive(good, probs=probs)
    with pytest.raises(ValueError, match=who + ".*at most 16 probabilities"):
        bn.get_posterior_predictive(good, probs=np.linspace(0.1, 0.9, 17))
    with pytest.raises(ValueError, match=who + ".*empty"):
        bn.get_posterior_predictive(_checkpoint(tmp_path, "empty", _samples(6), test_rows=0)[0])
    with pytest.raises(ValueError, match=who + ".*features"):
        bn.get_posterior_predictive(good, features="test")


class Float64Context:
    """The calls of HipContext that get_posterior_predictive makes, on the float64 oracle's forward pass and the host definition."""
    log = []

    def __init__(self, device=None):
        self.x = {}

    def set_data(self, X, which=capi.TRAIN):
        Float64Context.log.append(("set_data", which, len(X)))
        self.x[which] = np.array(X, dtype=np.float64)

    def set_arch_from_weights(self, weights, in_dim, act_kind, out_kind, lik_kind):
        self.shapes = [w.shape for w in weights]
        self.fun = {capi.ACT_TANH: "tanh", capi.ACT_LEAKY: "genReLU"}[act_kind]
        self.out_kind = out_kind

    def predict_sets_predictive(self, weight_sets, probs=(0.025, 0.5, 0.975), sigma_sets=None, targets=None, act_prm_sets=None, which=capi.TRAIN,
                                want_mean=True, want_crps_i=True):
        Float64Context.log.append(("predict_sets_predictive", which, targets is not None))
        out = []
        for i, packed in enumerate(weight_sets):
            layers, at = [], 0
            for s in self.shapes:
                layers.append(np.asarray(packed[at:at + s[0] * s[1]]).reshape(s))
                at += s[0] * s[1]
            z = orc.forward_logits(self.x[which], layers, orc.Act(self.fun, np.zeros(1) if act_prm_sets is None else act_prm_sets[i]))
            if self.out_kind == capi.OUT_SOFTPLUS_HALF:
                t = z.shape[1] // 2
                z = np.concatenate([z[:, :t], np.logaddexp(0.0, z[:, t:])], axis=1)
            out.append(z)
        kind = "regression-error" if self.out_kind == capi.OUT_SOFTPLUS_HALF else "regression"
        res = bn.posterior_predictive(np.array(out), kind, sigma_sets=sigma_sets, probs=probs, targets=targets)
        return dict(quantiles=res["quantiles"] if len(res["probs"]) else None, mean=res["mean"], crps_i=res.get("crps_i"),
                    crps_total=None if targets is None else np.sum(res["crps_i"], axis=0))

    def close(self):
        pass


@pytest.mark.parametrize("mode", ["regression", "regression-error"])
def test_get_posterior_predictive_assembles_its_result(mode, tmp_path, monkeypatch):
    monkeypatch.setattr(backend, "HipContext", Float64Context)
    error = mode == "regression-error"
    samples = _samples(6, n_out=4 if error else 2, seed=3, error_prm=not error, genrelu=True)
    pkl, x, y = _checkpoint(tmp_path, "run", samples, mode=mode, out_fn=bn.RegressTransformError if error else bn.RegressTransform, fun="genReLU")
    z = np.array([orc.forward_logits(x, s["weights"], orc.Act("genReLU", s["alphas"])) for s in samples])
    stack = np.concatenate([z[:, :, :2], np.logaddexp(0.0, z[:, :, 2:])], axis=2) if error else z
    sigma = None if error else np.array([s["error_prm"] for s in samples])
    Float64Context.log = []
    res = bn.get_posterior_predictive(pkl)                                         # the test table: the first 7 rows
    assert Float64Context.log == [("set_data", capi.TRAIN, 7), ("predict_sets_predictive", capi.TRAIN, True)]
    want = bn.posterior_predictive(stack[:, :7], mode, sigma_sets=sigma, targets=y[:7])
    assert sorted(res) == KEYS and (res["n_samples"], res["n_rows"]) == (6, 7)
    for k in ("quantiles", "mean", "crps_i", "crps"):
        np.testing.assert_allclose(res[k], want[k], rtol=1e-12, atol=1e-14, err_msg=k)
    # without the CRPS the targets are never sent; a feature matrix without labels has none
    for kw in (dict(crps=False), dict(features=x[:7])):
        Float64Context.log = []
        lean = bn.get_posterior_predictive(pkl, probs=(0.5, 0.1), **kw)
        assert Float64Context.log[-1] == ("predict_sets_predictive", capi.TRAIN, False)
        assert sorted(lean) == sorted(k for k in KEYS if not k.startswith("crps")) and np.array_equal(lean["probs"], (0.5, 0.1))
        np.testing.assert_allclose(lean["quantiles"][0], want["quantiles"][1], rtol=1e-12, atol=1e-14)
    # the training table under a budget of four rows a block: the whole table goes up once, then block after block as the second table
    monkeypatch.setenv("NPBNN_HPD_STACK_BYTES", str(6 * stack.shape[2] * 4 * 4))
    Float64Context.log = []
    blocked = bn.get_posterior_predictive(pkl, features="train")
    assert Float64Context.log == [("set_data", capi.TRAIN, 11)] + [e for n in (4, 4, 3) for e in (("set_data", capi.TEST, n), ("predict_sets_predictive", capi.TEST, True))]
    want = bn.posterior_predictive(stack, mode, sigma_sets=sigma, targets=y)
    for k in ("quantiles", "mean", "crps_i", "crps"):
        np.testing.assert_allclose(blocked[k], want[k], rtol=1e-12, atol=1e-14, err_msg=k)


def test_a_custom_output_callable_is_refused_in_the_callers_name(tmp_path, monkeypatch):
    monkeypatch.setattr(backend, "HipContext", Float64Context)
    Float64Context.log = []
    rs = np.random.default_rng(5)
    x, y = rs.standard_normal((7, N_FEATURES)), rs.standard_normal((7, 2))
    loaded = [types.SimpleNamespace(_test_data=x, _test_labels=y, _act_fun=bn.ActFun(fun="tanh"), _output_act_fun=lambda z: 0.5 * z,
                                    _estimation_mode="regression"), None, types.SimpleNamespace(_post_weight_samples=_samples(6))]
    monkeypatch.setattr(importlib.import_module("npbnn_amd.predictive"), "load_obj", lambda path: loaded)
    with pytest.raises(ValueError, match="get_posterior_predictive.*custom callable"):
        bn.get_posterior_predictive("unused.pkl")
    assert Float64Context.log == []                                                # (no table went up, no stack was built)
