"""PSIS-LOO on the host: ``posterior_loo`` (the definition in plain numpy) against the independent restatement of tests/loo_cases.py
under its bar, the consequences of the definition, ``loo_compare``, and every refusal of ``posterior_loo``, ``loo_compare`` and
``get_posterior_loo`` - the latter's before any device context is built (the context is replaced by one that fails when built, or
by a float64 stand-in, through which a blocked run is held against the whole one)."""
import importlib
import os
import pickle
import re
import types

import numpy as np
import pytest

import loo_cases as lc
import lppd_cases
import npbnn_amd as bn
import oracle as orc
from npbnn_amd import _capi as capi

backend = importlib.import_module("npbnn_amd.backend")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOTALS = ("elpd_loo", "se_elpd_loo", "p_loo", "looic", "lppd", "k_threshold", "n_bad_k", "n_samples", "n_rows")
POINT = ("elpd_loo_i", "lppd_i", "p_loo_i", "pareto_k")


def _within_the_bar(got, ll, label):
    want, bars = lc.reference(ll)
    for f in lc.FIELDS:
        dev = lc.deviation(got, want, f)
        print("host %s %s: deviation %.3e, bar %.3e" % (label, f, dev, bars[f]))
        assert dev <= bars[f], (label, f, dev, bars[f])
    return want


# ---- the definition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n_cols", [(2, 3), (20, 5), (21, 7), (26, 7), (64, 33), (100, 9), (257, 5), (1025, 3)])
def test_posterior_loo_equals_the_restatement(S, n_cols):
    ll = lc.matrix(S, n_cols)
    res = bn.posterior_loo(ll)
    assert sorted(res) == sorted(TOTALS + POINT) and (res["n_samples"], res["n_rows"]) == (S, n_cols)
    _within_the_bar(res, ll, "S=%d cols=%d" % (S, n_cols))
    el = res["elpd_loo_i"]
    assert res["elpd_loo"] == float(np.sum(el)) and res["looic"] == -2.0 * res["elpd_loo"] and res["lppd"] == float(np.sum(res["lppd_i"]))
    assert res["se_elpd_loo"] == float(np.sqrt(n_cols * np.var(el, ddof=1)))
    assert np.array_equal(res["p_loo_i"], res["lppd_i"] - el) and res["p_loo"] == float(np.sum(res["p_loo_i"]))
    assert res["k_threshold"] == min(1.0 - 1.0 / np.log10(S), 0.7) and res["n_bad_k"] == int(np.sum(res["pareto_k"] > res["k_threshold"]))
    assert np.all(res["p_loo_i"] >= -1e-12)                                        # (leaving a row out never helps its own prediction)
    assert bn.posterior_loo(ll[:, :1])["se_elpd_loo"] == 0.0


def test_the_special_columns():
    ll = lc.special_matrix()
    res = bn.posterior_loo(ll)
    _within_the_bar(res, ll, "special")
    assert res["pareto_k"][0] == np.inf and res["elpd_loo_i"][0] == -1.25 and res["lppd_i"][0] == -1.25       # a column of equal values
    assert res["pareto_k"][1] == np.inf                                            # two values, half the column each: nothing above the cut
    for f in lc.FIELDS:
        assert res[f][2] == res[f][3]
    # (1e6 + ll keeps ll to half an ulp of 1e6, 5.8e-11: the shifted column is the plain one to a small multiple of that, not to the bit)
    assert abs(res["pareto_k"][4] - res["pareto_k"][2]) <= 1e-8 and abs(res["elpd_loo_i"][4] - 1e6 - res["elpd_loo_i"][2]) <= 1e-8
    assert np.isfinite(res["elpd_loo_i"][5]) and res["elpd_loo_i"][5] < -700.0


@pytest.mark.parametrize("S", [2, 5, 20])
def test_twenty_samples_or_fewer_are_plain_importance_sampling(S):
    ll = lc.matrix(S, 6)
    res = bn.posterior_loo(ll)
    assert np.all(res["pareto_k"] == np.inf) and res["n_bad_k"] == 6
    np.testing.assert_allclose(res["elpd_loo_i"], -np.log(np.mean(np.exp(-ll), axis=0)), rtol=0, atol=1e-13)


def test_a_shift_moves_elpd_and_leaves_k():
    ll = np.round(lc.matrix(64, 9) * 2.0 ** 20) / 2.0 ** 20                          # (multiples of 2^-20: the shift below is exact)
    a, b = bn.posterior_loo(ll), bn.posterior_loo(ll + 2.5)
    assert np.array_equal(a["pareto_k"], b["pareto_k"]) and np.all(np.isfinite(a["pareto_k"]))
    np.testing.assert_allclose(b["elpd_loo_i"], a["elpd_loo_i"] + 2.5, rtol=0, atol=1e-13)
    c = bn.posterior_loo(ll + 1e6)                                                   # (not exact: k within its bar)
    _, bars = lc.reference(ll)
    assert np.max(np.abs(c["pareto_k"] - a["pareto_k"])) <= max(bars["pareto_k"], 1e-8)      # x carries the rounding of 1e6 + ll: 2^-33 of it


def test_ties_at_the_cut_shorten_the_tail():
    """S = 100: M = 20.  Where `tied` of the M largest ratios take the value of the 21st, the values strictly above the cut are
    20 - tied; four of them or fewer and the column is not fitted."""
    rs = np.random.default_rng(3)
    base = -np.sort(rs.gamma(1.5, 1.0, 100))                                         # ll descending: the largest ratio is the last entry
    cols, tails = [], (0, 5, 15, 16, 18)
    for tied in tails:
        c = base.copy()
        c[80:80 + tied] = c[79]                                                      # c[79] is the 21st largest ratio
        cols.append(rs.permutation(c))
    ll = np.stack(cols, axis=1)
    res = bn.posterior_loo(ll)
    _within_the_bar(res, ll, "ties")
    assert np.array_equal(np.isfinite(res["pareto_k"]), [20 - t > 4 for t in tails])


def test_the_order_of_the_samples_does_not_matter():
    ll = lc.matrix(257, 6)
    want, bars = lc.reference(ll)
    a, b = bn.posterior_loo(ll), bn.posterior_loo(ll[np.random.default_rng(0).permutation(257)])
    for f in lc.FIELDS:
        assert lc.deviation(b, a, f) <= bars[f], f


def test_loo_compare():
    la, lb = lc.matrix(64, 40), lc.matrix(64, 40, seed=1)
    a, b = bn.posterior_loo(la), bn.posterior_loo(lb)
    cmp_ = bn.loo_compare(a, b)
    d = a["elpd_loo_i"] - b["elpd_loo_i"]
    assert cmp_ == dict(elpd_diff=float(np.sum(d)), se_diff=float(np.sqrt(40 * np.var(d, ddof=1))), n_rows=40)
    assert bn.loo_compare(b, a)["elpd_diff"] == -cmp_["elpd_diff"] and bn.loo_compare(a, a) == dict(elpd_diff=0.0, se_diff=0.0, n_rows=40)
    lean = {k: v for k, v in a.items() if k not in POINT}
    for bad in ((lean, b), (a, lean), (a, dict(b, elpd_loo_i=None)), (a, bn.posterior_loo(lb[:, :39])), (a, None)):
        with pytest.raises(ValueError, match="loo_compare"):
            bn.loo_compare(*bad)


def test_posterior_loo_refusals():
    ok = lc.matrix(8, 4)
    for bad in (ok[:, 0], ok[:, :0], ok[:1], np.zeros((16385, 1)), ok[None]):
        with pytest.raises(ValueError, match="posterior_loo"):
            bn.posterior_loo(bad)
    for v in (np.nan, np.inf, -np.inf):
        bad = ok.copy()
        bad[5, 1] = v
        with pytest.raises(ValueError, match="NaN or infinite"):
            bn.posterior_loo(bad)


def test_public_names_and_header():
    for name in ("posterior_loo", "get_posterior_loo", "loo_compare"):
        assert callable(getattr(bn, name))
    txt = open(os.path.join(ROOT, "include", "npbnn_hip.h")).read()
    for sym in ("npbnn_op_psis", "npbnn_predict_sets_loo"):
        assert re.search(r"\bint %s\(" % sym, txt) and sym in capi.SIGNATURES


# ---- checkpoints --------------------------------------------------------------------------------------------------------------------
N_FEATURES = 5


def _samples(n, n_out=3, seed=0, error_prm=False, genrelu=False):
    rs = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = dict(weights=[rs.normal(0, 0.5, (4, N_FEATURES + 1)), rs.normal(0, 0.5, (n_out, 5))], alphas=rs.uniform(0, 0.3, 1) if genrelu else np.zeros(1),
                 mcmc_it=i)
        if error_prm:
            s["error_prm"] = np.exp(rs.normal(-0.5, 0.3, n_out))
        out.append(s)
    return out


def _checkpoint(tmp_path, name, samples, mode="classification", out_fn=bn.SoftMax, fun="tanh", n_out=3, test_rows=7):
    rs = np.random.default_rng(99)
    x = rs.standard_normal((11, N_FEATURES))
    y = rs.integers(0, n_out, 11) if mode != "regression" else rs.standard_normal((11, n_out))
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


def test_get_posterior_loo_refuses_before_any_device_call(tmp_path, monkeypatch):
    monkeypatch.setattr(backend, "HipContext", NoDevice)
    who = "get_posterior_loo"
    good, x, y = _checkpoint(tmp_path, "good", _samples(6))
    with pytest.raises(ValueError, match=who + ".*no posterior samples"):
        bn.get_posterior_loo(_checkpoint(tmp_path, "none", [])[0])
    with pytest.raises(ValueError, match=who + ".*at least 2"):
        bn.get_posterior_loo(_checkpoint(tmp_path, "one", _samples(1))[0])
    for mode in ("regression-error", "custom", "count"):
        with pytest.raises(ValueError, match=who + ".*%r is out of scope.*predicted-sigma regression and the count likelihoods are not" % mode):
            bn.get_posterior_loo(_checkpoint(tmp_path, mode, _samples(6), mode=mode)[0])
    with pytest.raises(ValueError, match=who + ".*error_prm"):
        bn.get_posterior_loo(_checkpoint(tmp_path, "bare", _samples(6), mode="regression", out_fn=bn.RegressTransform)[0])
    with pytest.raises(ValueError, match=who + ".*class indices"):
        bn.get_posterior_loo(good, features=x, labels=np.where(np.arange(11) == 4, 3, y))
    with pytest.raises(ValueError, match=who + ".*labels for"):
        bn.get_posterior_loo(good, features=x, labels=y[:5])
    with pytest.raises(ValueError, match=who + ".*needs its labels"):
        bn.get_posterior_loo(good, features=x)
    with pytest.raises(ValueError, match=who + ".*targets are"):
        bn.get_posterior_loo(_checkpoint(tmp_path, "reg", _samples(6, error_prm=True), mode="regression", out_fn=bn.RegressTransform)[0],
                             features=x, labels=np.zeros((11, 2)))
    with pytest.raises(ValueError, match=who + ".*empty"):
        bn.get_posterior_loo(_checkpoint(tmp_path, "empty", _samples(6), test_rows=0)[0])
    with pytest.raises(ValueError, match=who + ".*features"):
        bn.get_posterior_loo(good, features="test")


class Float64Context:
    """The calls of HipContext that get_posterior_loo makes, on the float64 oracle's forward pass and the host definition."""
    log = []

    def __init__(self, device=None):
        self.x, self.y = {}, {}

    def set_data(self, X, which=capi.TRAIN):
        Float64Context.log.append(("set_data", which, len(X)))
        self.x[which] = np.array(X, dtype=np.float64)

    def set_labels(self, labels, which=capi.TRAIN):
        Float64Context.log.append(("set_labels", which, len(labels)))
        self.y[which] = np.asarray(labels)

    set_targets = set_labels

    def set_arch_from_weights(self, weights, in_dim, act_kind, out_kind, lik_kind):
        self.shapes = [w.shape for w in weights]
        self.fun = {capi.ACT_TANH: "tanh", capi.ACT_LEAKY: "genReLU"}[act_kind]

    def predict_sets_loo(self, weight_sets, lik_kind, sigma_sets=None, act_prm_sets=None, which=capi.TRAIN, log_lik=False):
        Float64Context.log.append(("predict_sets_loo", which, log_lik))
        out = []
        for i, packed in enumerate(weight_sets):
            layers, at = [], 0
            for s in self.shapes:
                layers.append(np.asarray(packed[at:at + s[0] * s[1]]).reshape(s))
                at += s[0] * s[1]
            out.append(orc.forward_logits(self.x[which], layers, orc.Act(self.fun, np.zeros(1) if act_prm_sets is None else act_prm_sets[i])))
        ll = lppd_cases.log_lik_from_values(np.array(out), self.y[which], "reg" if lik_kind == capi.LIK_GAUSS else "cat", sigma_sets)
        res = bn.posterior_loo(ll)
        return dict(elpd_loo_i=res["elpd_loo_i"], lppd_i=res["lppd_i"], pareto_k=res["pareto_k"], log_lik_sample=np.sum(ll, axis=1),
                    log_lik=ll if log_lik else None)

    def close(self):
        pass


@pytest.mark.parametrize("mode", ["classification", "regression"])
def test_get_posterior_loo_assembles_its_result_whole_and_in_blocks(mode, tmp_path, monkeypatch):
    monkeypatch.setattr(backend, "HipContext", Float64Context)
    reg = mode == "regression"
    samples = _samples(30, seed=3, error_prm=reg, genrelu=True)
    pkl, x, y = _checkpoint(tmp_path, "run", samples, mode=mode, out_fn=bn.RegressTransform if reg else bn.SoftMax, fun="genReLU")
    z = np.array([orc.forward_logits(x, s["weights"], orc.Act("genReLU", s["alphas"])) for s in samples])
    sigma = np.array([s["error_prm"] for s in samples]) if reg else None
    ll = lppd_cases.log_lik_from_values(z, y, "reg" if reg else "cat", sigma)
    Float64Context.log = []
    res = bn.get_posterior_loo(pkl, pointwise=True, log_lik=True)                   # the test table: the first 7 rows
    assert Float64Context.log == [("set_data", capi.TRAIN, 7), ("set_labels", capi.TRAIN, 7), ("predict_sets_loo", capi.TRAIN, True)]
    want = bn.posterior_loo(ll[:, :7])
    assert sorted(res) == sorted(TOTALS + POINT + ("log_lik_sample", "log_lik"))
    for k in TOTALS + POINT:
        np.testing.assert_allclose(res[k], want[k], rtol=1e-12, atol=1e-13, err_msg=k)
    np.testing.assert_allclose(res["log_lik"], ll[:, :7], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(res["log_lik_sample"], ll[:, :7].sum(axis=1), rtol=1e-12)
    lean = bn.get_posterior_loo(pkl)
    assert sorted(lean) == sorted(TOTALS + ("log_lik_sample",)) and lean["elpd_loo"] == res["elpd_loo"]
    # the training table under a budget of four rows a block: the whole table goes up once, then block after block as the second table
    whole = bn.get_posterior_loo(pkl, features="train", pointwise=True, log_lik=True)
    monkeypatch.setenv("NPBNN_HPD_STACK_BYTES", str(30 * 8 * 4))
    Float64Context.log = []
    blocked = bn.get_posterior_loo(pkl, features="train", pointwise=True, log_lik=True)
    assert Float64Context.log == [("set_data", capi.TRAIN, 11)] + [e for n in (4, 4, 3) for e in
                                                                   (("set_data", capi.TEST, n), ("set_labels", capi.TEST, n), ("predict_sets_loo", capi.TEST, True))]
    for k in TOTALS + POINT + ("log_lik",):
        assert np.array_equal(blocked[k], whole[k]), k                              # (a row's results depend on its own column alone)
    np.testing.assert_allclose(blocked["log_lik_sample"], whole["log_lik_sample"], rtol=1e-13)
    want = bn.posterior_loo(ll)
    for k in TOTALS + POINT:
        np.testing.assert_allclose(blocked[k], want[k], rtol=1e-12, atol=1e-13, err_msg=k)


def test_a_custom_output_callable_goes_through_the_host(tmp_path, monkeypatch):
    """No device kind: the stack is built from ``predict_sets`` and the callable, then ``log_lik_of_stack`` and ``posterior_loo``."""
    calls = []

    class StackContext(Float64Context):
        def predict_sets(self, weight_sets, act_prm_sets=None, apply_out_fn=True):
            calls.append(apply_out_fn)
            return np.array([orc.forward_logits(self.x[capi.TRAIN], [np.asarray(p[:24]).reshape(4, 6), np.asarray(p[24:]).reshape(3, 5)], orc.Act("tanh"))
                             for p in weight_sets])

    monkeypatch.setattr(backend, "HipContext", StackContext)

    def my_softmax(z):
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    samples = _samples(25, seed=5)
    Float64Context.log = []
    rs = np.random.default_rng(99)
    x = rs.standard_normal((11, N_FEATURES))
    y = rs.integers(0, 3, 11)
    from npbnn_amd.posterior import _SamplePredictor
    with _SamplePredictor(N_FEATURES, samples, bn.ActFun(fun="tanh"), my_softmax) as pred:
        assert pred.custom_output
        res = pred.loo(x, y, capi.LIK_CATEGORICAL, log_lik=True)
    z = np.array([orc.forward_logits(x, s["weights"], orc.Act("tanh")) for s in samples])
    want = bn.posterior_loo(lppd_cases.log_lik_from_values(z, y, "cat"))
    assert calls and "predict_sets_loo" not in [e[0] for e in Float64Context.log]
    for k in POINT:
        np.testing.assert_allclose(res[k], want[k], rtol=1e-10, atol=1e-12, err_msg=k)
