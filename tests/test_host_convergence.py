"""Convergence diagnostics on the host: ``posterior_convergence`` (the definition in plain numpy) against the independent restatement
of tests/convergence_cases.py, its behaviour on series whose answer is known, and every refusal of ``posterior_convergence`` and
``get_posterior_convergence`` - the latter's before any device call (the device context is replaced by one that fails when built, or
by a float64 stand-in).

``posterior_convergence`` sums whole arrays at once, the restatement column by column: measured deviation between the two over every
case, 1.1e-11 (rhat) and 4.4e-11 (ess), no column within 1e-6 of a stop or monotone decision (the smallest margin is 8.9e-06)."""
import importlib
import os
import pickle
import types

import numpy as np
import pytest

import npbnn_amd as bn
import convergence_cases as cc
import oracle as orc
from npbnn_amd import _capi as capi

backend = importlib.import_module("npbnn_amd.backend")

KEYS = sorted(("rhat", "ess", "max_rhat", "min_ess", "frac_rhat_above", "n_constant", "per_output", "n_chains", "n_draws"))


# ---- the definition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_posterior_convergence_equals_the_restatement(shape, dtype):
    ref = cc.reference(shape[0], shape[1], dtype)
    v = ref["values"]
    res = bn.posterior_convergence(v.reshape(v.shape[0], 1, v.shape[1]), n_chains=shape[0])
    assert sorted(res) == KEYS and res["rhat"].shape == (1, v.shape[1]) and (res["n_chains"], res["n_draws"]) == shape
    dr, de, left = cc.compare(res["rhat"][0], res["ess"][0], ref, use_ld=False)
    dr_ld, de_ld, _ = cc.compare(res["rhat"][0], res["ess"][0], ref, use_ld=True)
    print("host deviation %s %s: rhat %.3e ess %.3e (longdouble: %.3e %.3e), %d columns left out" % (shape, dtype, dr, de, dr_ld, de_ld, left))
    assert left == 0                                        # (the seeds keep every column clear of a decision)
    assert dr <= cc.RHAT_RTOL and de <= cc.ESS_RTOL and dr_ld <= cc.RHAT_RTOL and de_ld <= cc.ESS_RTOL
    # the rows x outputs layout is the columns' order, whatever the split between the two axes
    again = bn.posterior_convergence(v.reshape(v.shape[0], v.shape[1], 1), n_chains=shape[0])
    np.testing.assert_array_equal(again["rhat"][:, 0], res["rhat"][0])
    np.testing.assert_array_equal(again["ess"][:, 0], res["ess"][0])


def test_restatements_agree_and_no_column_sits_on_a_decision():
    """The float64 restatement against the longdouble one: the basis of the device test's bounds (three orders below them)."""
    worst_r = worst_e = 0.0
    margin = np.inf
    for dtype in cc.DTYPES:
        for shape in cc.SHAPES:
            ref = cc.reference(shape[0], shape[1], dtype)
            live = ~np.isnan(ref["rhat"])
            assert np.count_nonzero(~live) == 1
            worst_r = max(worst_r, float(np.max(np.abs(ref["rhat"][live] - ref["rhat_ld"][live]) / ref["rhat_ld"][live])))
            worst_e = max(worst_e, float(np.max(np.abs(ref["ess"][live] - ref["ess_ld"][live]) / ref["ess_ld"][live])))
            margin = min(margin, float(ref["margin"].min()), float(ref["margin_ld"].min()))
    print("float64 against longdouble restatement: rhat %.3e, ess %.3e; smallest decision margin %.3e" % (worst_r, worst_e, margin))
    assert worst_r <= 1e-10 and worst_e <= 1e-9 and margin >= cc.MARGIN


# ---- series whose answer is known -------------------------------------------------------------------------------------------------
def _series(phi, n_cols, n_chains=4, n_draws=250, seed=5):
    rs = np.random.default_rng([seed, int(1000 * phi) % 1000])
    return np.stack([cc.ar1(rs, phi, n_chains, n_draws) for _ in range(n_cols)], axis=1)


def test_iid_columns_have_rhat_one_and_full_ess():
    x = _series(0.0, 200)
    res = bn.posterior_convergence(x[:, :, None], n_chains=4)
    rhat, ratio = float(np.median(res["rhat"])), float(np.median(res["ess"])) / len(x)
    print("iid (4, 250): median rhat %.4f, median ess / S %.3f" % (rhat, ratio))
    assert abs(rhat - 1.0) <= 0.01 and 0.8 <= ratio <= 1.2
    assert res["n_constant"] == 0 and res["max_rhat"] == res["rhat"].max() and res["min_ess"] == res["ess"].min()
    assert res["frac_rhat_above"] == np.count_nonzero(res["rhat"] > 1.01) / res["rhat"].size


def test_autocorrelated_columns_lose_ess_as_theory_says():
    """AR(1) with phi = 0.9: ess / S -> (1 - phi) / (1 + phi) = 0.0526."""
    x = _series(0.9, 200)
    res = bn.posterior_convergence(x[:, :, None], n_chains=4)
    ratio = float(np.median(res["ess"])) / len(x)
    print("phi 0.9 (4, 250): median ess / S %.4f" % ratio)
    assert 0.03 <= ratio <= 0.09


def test_a_shifted_chain_is_found():
    rs = np.random.default_rng(17)
    x = rs.standard_normal((2, 250, 6))
    x[1] += 5.0
    res = bn.posterior_convergence(x.reshape(500, 2, 3), n_chains=2)
    assert res["rhat"].min() > 2.0 and res["frac_rhat_above"] == 1.0
    alone = bn.posterior_convergence(x[0].reshape(250, 2, 3), n_chains=1)      # (each chain by itself is fine)
    assert alone["rhat"].max() < 1.1


def test_constant_columns_are_nan_and_counted():
    rs = np.random.default_rng(3)
    x = rs.standard_normal((40, 5, 2))
    x[:, 1, 0] = 0.25
    x[:, 3, 1] = -7.0
    x[:, 4, 1] = 1024.0
    res = bn.posterior_convergence(x, n_chains=2, rhat_threshold=0.0)
    assert np.array_equal(np.isnan(res["rhat"]), np.isnan(res["ess"]))
    assert np.argwhere(np.isnan(res["rhat"])).tolist() == [[1, 0], [3, 1], [4, 1]] and res["n_constant"] == 3
    np.testing.assert_array_equal(res["per_output"][:, 3], [1, 2])
    np.testing.assert_array_equal(res["per_output"][:, 2], [4, 3])            # (threshold 0: every live column is above)
    assert res["frac_rhat_above"] == 7 / 10 and res["max_rhat"] == np.nanmax(res["rhat"]) and res["min_ess"] == np.nanmin(res["ess"])
    # a chain that is constant in one half only is not a constant column
    y = rs.standard_normal((16, 1, 1))
    y[:4] = 2.0
    assert np.isfinite(bn.posterior_convergence(y)["rhat"][0, 0])
    everything = bn.posterior_convergence(np.ones((16, 2, 2)))
    assert everything["n_constant"] == 4 and np.isnan(everything["max_rhat"]) and np.isnan(everything["min_ess"])
    assert everything["frac_rhat_above"] == 0.0


def test_the_middle_draw_of_an_odd_chain_is_dropped():
    rs = np.random.default_rng(8)
    x = rs.standard_normal((2, 9, 3))
    y = x.copy()
    y[:, 4] = 1e3                                                             # the middle draw of either chain
    a = bn.posterior_convergence(x.reshape(18, 1, 3), n_chains=2)
    b = bn.posterior_convergence(y.reshape(18, 1, 3), n_chains=2)
    np.testing.assert_array_equal(a["rhat"], b["rhat"])
    np.testing.assert_array_equal(a["ess"], b["ess"])
    c = bn.posterior_convergence(np.delete(x, 4, axis=1).reshape(16, 1, 3), n_chains=2)
    np.testing.assert_array_equal(a["rhat"], c["rhat"])


def test_posterior_convergence_refusals():
    ok = np.random.default_rng(0).standard_normal((16, 3, 2))
    for bad, kw in ((ok[:, :, 0], {}), (ok[:, :0], {}), (np.zeros((0, 3, 2)), {}), (ok[:7], {}), (ok, dict(n_chains=3)), (ok, dict(n_chains=4)),
                    (ok, dict(n_chains=0)), (np.zeros((65 * 8, 1, 1)), dict(n_chains=65)), (np.zeros((16385, 1, 1)), {}),
                    (ok, dict(rhat_threshold=float("nan")))):
        with pytest.raises(ValueError):
            bn.posterior_convergence(bad, **kw)
    for v in (np.nan, np.inf, -np.inf):
        bad = ok.copy()
        bad[5, 1, 1] = v
        with pytest.raises(ValueError, match="NaN or infinite"):
            bn.posterior_convergence(bad)
    assert bn.posterior_convergence(np.zeros((64 * 8, 1, 1)), n_chains=64)["n_constant"] == 1       # (the caps themselves pass)
    assert bn.posterior_convergence(np.zeros((16384, 1, 1)))["n_draws"] == 16384


# ---- checkpoints --------------------------------------------------------------------------------------------------------------------
N_FEATURES = 5


def _samples(n, seed=0, shapes=((4, N_FEATURES + 1), (3, 5)), genrelu=False):
    rs = np.random.default_rng(seed)
    return [dict(weights=[rs.normal(0, 0.3, s) for s in shapes], alphas=rs.uniform(0, 0.3, 1) if genrelu else np.zeros(1), mcmc_it=i) for i in range(n)]


def _checkpoint(tmp_path, name, samples, fun="tanh", out_fn=bn.SoftMax, test_rows=7):
    x = np.random.default_rng(99).standard_normal((11, N_FEATURES))
    act = bn.ActFun(fun=fun, prm=np.zeros(1)) if fun == "genReLU" else bn.ActFun(fun=fun)
    model = types.SimpleNamespace(_data=x, _test_data=x[:test_rows], _act_fun=act, _output_act_fun=out_fn, _estimation_mode="classification")
    pkl = os.path.join(str(tmp_path), name + ".pkl")
    with open(pkl, "wb") as fh:
        pickle.dump([model, None, types.SimpleNamespace(_post_weight_samples=samples)], fh)
    return pkl


class NoDevice:
    def __init__(self, *a, **k):
        raise AssertionError("a device context was built")


def test_get_posterior_convergence_refuses_before_any_device_call(tmp_path, monkeypatch):
    monkeypatch.setattr(backend, "HipContext", NoDevice)
    good = _checkpoint(tmp_path, "good", _samples(12))
    with pytest.raises(ValueError, match="no posterior samples"):
        bn.get_posterior_convergence(_checkpoint(tmp_path, "none", []))
    with pytest.raises(ValueError, match="no checkpoints"):
        bn.get_posterior_convergence([])
    with pytest.raises(ValueError, match="at least 8"):
        bn.get_posterior_convergence([good, _checkpoint(tmp_path, "short", _samples(7))])
    with pytest.raises(ValueError, match="at most 64"):
        bn.get_posterior_convergence([good] * 65)
    with pytest.raises(ValueError, match="at most 16384"):
        bn.get_posterior_convergence([_checkpoint(tmp_path, "long", _samples(8193, shapes=((1, N_FEATURES + 1), (2, 2))))] * 2)
    with pytest.raises(ValueError, match="empty"):
        bn.get_posterior_convergence(_checkpoint(tmp_path, "empty", _samples(12), test_rows=0))
    with pytest.raises(ValueError, match="empty"):
        bn.get_posterior_convergence(good, features=np.zeros((0, N_FEATURES)))
    with pytest.raises(ValueError, match="features"):
        bn.get_posterior_convergence(good, features="test")
    with pytest.raises(ValueError, match="NaN"):
        bn.get_posterior_convergence(good, rhat_threshold=float("nan"))
    for other in (_checkpoint(tmp_path, "wider", _samples(12, shapes=((5, N_FEATURES + 1), (3, 6)))),
                  _checkpoint(tmp_path, "deeper", _samples(12, shapes=((4, N_FEATURES + 1), (4, 5), (3, 5)))),
                  _checkpoint(tmp_path, "swish", _samples(12), fun="swish"),
                  _checkpoint(tmp_path, "regress", _samples(12), out_fn=bn.RegressTransform)):
        with pytest.raises(ValueError, match="share architecture and activation"):
            bn.get_posterior_convergence([good, other])


def _halved(z):
    return 0.5 * z


class Float64Context:
    """The two calls of HipContext that get_posterior_convergence's routes make, on the float64 oracle's forward pass."""
    log = []

    def __init__(self, device=None):
        self.n_rows = {}

    def set_data(self, X, which=capi.TRAIN):
        self.x = np.array(X, dtype=np.float64)

    def set_arch_from_weights(self, weights, in_dim, act_kind, out_kind, lik_kind):
        self.shapes = [w.shape for w in weights]
        self.fun = {capi.ACT_TANH: "tanh", capi.ACT_LEAKY: "genReLU"}[act_kind]
        self.softmax = out_kind == capi.OUT_SOFTMAX

    def predict_sets(self, weight_sets, act_prm_sets=None, which=capi.TRAIN, apply_out_fn=True):
        Float64Context.log.append("predict_sets")
        out = []
        for i, packed in enumerate(weight_sets):
            layers, at = [], 0
            for s in self.shapes:
                layers.append(np.asarray(packed[at:at + s[0] * s[1]]).reshape(s))
                at += s[0] * s[1]
            z = orc.forward_logits(self.x, layers, orc.Act(self.fun, np.zeros(1) if act_prm_sets is None else act_prm_sets[i]))
            out.append(orc.out_softmax(z) if apply_out_fn and self.softmax else z)
        return np.array(out)

    def predict_sets_convergence(self, weight_sets, n_chains=1, rhat_threshold=1.01, act_prm_sets=None, which=capi.TRAIN, apply_out_fn=True,
                                 pointwise=True):
        Float64Context.log.append("predict_sets_convergence")
        y = self.predict_sets(list(weight_sets), act_prm_sets, which, apply_out_fn)
        Float64Context.log.pop()
        res = bn.posterior_convergence(y, n_chains, rhat_threshold)
        return res if pointwise else dict(res, rhat=None, ess=None)

    def close(self):
        pass


def test_get_posterior_convergence_assembles_the_chains(tmp_path, monkeypatch):
    """Three chains of 12, 9 and 10 draws: each keeps its last 9, chain-major; a custom output callable goes through the host stack."""
    monkeypatch.setattr(backend, "HipContext", Float64Context)
    Float64Context.log = []
    chains = [_samples(12, 1, genrelu=True), _samples(9, 2, genrelu=True), _samples(10, 3, genrelu=True)]
    files = [_checkpoint(tmp_path, "c%d" % i, c, fun="genReLU") for i, c in enumerate(chains)]
    res = bn.get_posterior_convergence(files, rhat_threshold=1.2)
    assert sorted(res) == KEYS and (res["n_chains"], res["n_draws"]) == (3, 9) and res["rhat"].shape == (7, 3)
    assert Float64Context.log == ["predict_sets_convergence"]
    kept = chains[0][3:] + chains[1] + chains[2][1:]
    x = np.random.default_rng(99).standard_normal((11, N_FEATURES))
    y = np.array([orc.out_softmax(orc.forward_logits(x[:7], s["weights"], orc.Act("genReLU", s["alphas"]))) for s in kept])
    want = bn.posterior_convergence(y, 3, 1.2)
    for k in ("rhat", "ess", "per_output"):
        np.testing.assert_allclose(res[k], want[k], rtol=1e-12)
    assert res["frac_rhat_above"] == want["frac_rhat_above"]
    train = bn.get_posterior_convergence(files[0], features="train", pointwise=False)
    assert sorted(train) == sorted(k for k in KEYS if k not in ("rhat", "ess")) and (train["n_chains"], train["n_draws"]) == (1, 12)
    # a custom output callable: the host stack
    Float64Context.log = []
    custom = [_checkpoint(tmp_path, "h%d" % i, c, fun="genReLU", out_fn=_halved) for i, c in enumerate(chains)]
    res = bn.get_posterior_convergence(custom, features=x)
    assert Float64Context.log == ["predict_sets"] and res["rhat"].shape == (11, 3)
    z = np.array([0.5 * orc.forward_logits(x, s["weights"], orc.Act("genReLU", s["alphas"])) for s in kept])
    np.testing.assert_allclose(res["rhat"], bn.posterior_convergence(z, 3)["rhat"], rtol=1e-12)
