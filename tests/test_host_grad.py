"""CPU checks of the weight gradient (npbnn_amd/gradient.py) and of the references tests/test_hip_grad.py holds the device to.

The restatement of tests/grad_cases.py against central differences of the oracle's likelihoods; bn.loglik_grad, the package's host
definition, against the restatement; every deliberately wrong variant beyond the device's bar; the prior's closed forms against
differences of calc_prior; the ridge identity; and map_estimate through a float64 stand-in for the device seam."""
import contextlib
import io

import numpy as np
import pytest

import grad_cases as gc
import npbnn_amd as bn
import oracle as orc
import saliency_cases as sc
from attrib_common import _act, _apply_override
from npbnn_amd import gradient
from oracle_backend import serve_from_oracle

LIKS = {"cat": bn.calc_likelihood, "gauss": bn.calc_likelihood_regression, "pred": bn.calc_likelihood_regression_error}


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **k)


def _oracle_loglik(case, inp, w):
    """the case's log-likelihood at the weights ``w`` through the oracle's forward pass and likelihood functions"""
    x = _apply_override(inp["table"].astype(np.float32).astype(np.float64), inp["override"])
    act = _act(case["fun"], inp["slopes1"], case["trainable"])
    z = orc.forward_logits(x, w, act)
    if case["lik"] == "cat":
        rw = gc.row_weight(case, inp)
        return orc.lik_categorical(orc.out_softmax(z), inp["labels"], np.arange(len(x)), instance_weight=rw, lik_temp=case["lik_temp"])
    t = inp["labels"].astype(np.float32).astype(np.float64)
    if case["lik"] == "gauss":
        return orc.lik_gaussian(z, t, lik_temp=case["lik_temp"], sig2=inp["sigma"])
    return orc.lik_gaussian_error(orc.out_regress_error(z), t, lik_temp=case["lik_temp"])


@pytest.mark.parametrize("name", gc.FD_CASES)
def test_restatement_against_central_differences(name):
    case, inp, want, _ = gc.case_data(name)
    assert case["fun"] in ("tanh", "swish")
    assert abs(_oracle_loglik(case, inp, inp["w"]) - want["loglik"]) <= 1e-10 * abs(want["loglik"])
    rs = np.random.default_rng(5)
    for l, g in enumerate(want["grads"]):
        # "Relative 1e-6" is taken relative to the layer's largest entry, with an absolute floor of 1e-6, not entry by entry: the
        # difference quotient's rounding noise, about eps |log-likelihood| / step, is absolute - the same for a small entry as for
        # a large one - so a per-entry relative bound would measure the noise, not the restatement.
        tol = 1e-6 * max(1.0, float(np.abs(g).max()))
        picks = {(0, 0), (g.shape[0] - 1, g.shape[1] - 1)} | {(int(rs.integers(g.shape[0])), int(rs.integers(g.shape[1]))) for _ in range(4)}
        if l == 0 and inp["override"] is not None:
            hb = g.shape[1] - inp["table"].shape[1]
            picks |= {(0, hb + int(c)) for c in np.flatnonzero(~np.isnan(inp["override"]))}
        for i, j in sorted(picks):
            step = 1e-5 * max(1.0, abs(inp["w"][l][i, j]))
            up, down = [np.array(m, copy=True) for m in inp["w"]], [np.array(m, copy=True) for m in inp["w"]]
            up[l][i, j] += step
            down[l][i, j] -= step
            fd = (_oracle_loglik(case, inp, up) - _oracle_loglik(case, inp, down)) / (2 * step)
            assert abs(fd - g[i, j]) <= tol, (l, i, j, fd, g[i, j])


@pytest.mark.parametrize("name", list(gc.CASES))
def test_host_definition_against_restatement(name):
    case, inp, want, want32 = gc.case_data(name)
    assert inp["redrawn"] <= sc.MAX_REDRAWN
    act = bn.ActFun(fun=case["fun"], trainable=case["trainable"])
    if inp["slopes1"] is not None:
        act.reset_prm(inp["slopes1"])
    table = inp["table"].astype(np.float32).astype(np.float64)
    lab = inp["labels"] if case["lik"] == "cat" else inp["labels"].astype(np.float32).astype(np.float64)
    train = case["which"] == 0
    r, grads = bn.loglik_grad(table, lab, inp["w"], act, LIKS[case["lik"]], sigma=inp["sigma"], lik_temp=case["lik_temp"],
                              class_weight=inp["class_w"] if train else None,
                              instance_weight=None if inp["inst_w"] is None or not train else inp["inst_w"].astype(np.float32).astype(np.float64),
                              col_override=inp["override"])
    assert abs(r["loglik"] - want["loglik"]) <= 1e-12 * abs(want["loglik"])
    assert len(grads) == len(want["grads"])
    for g, w, big in zip(grads, want["grads"], want["A"]):
        assert g.shape == w.shape and np.abs(g - w).max() <= 1e-12 * big
    if case["lik"] == "gauss":
        assert np.allclose(r["sum_r2"], want["sum_r2"], rtol=1e-12) and np.allclose(r["sum_r"], want["sum_r"], rtol=1e-9, atol=1e-9)
    if case["lik"] == "pred":
        z = orc.forward_logits(table, inp["w"], _act(case["fun"], None, False))
        assert orc.softplus(z[:, case["k"]:]).min() > 1e-3              # (no predicted sigma near underflow)
    # the float32 restatement is a rounding distance away, not a different function
    bar, a, b = gc.bars(want, want32)
    assert all(x <= 64 * y for x, y in zip(a, b)), (a, b)


@pytest.mark.parametrize("wrong,name", [("no_factor", "rows_257"), ("no_factor", "act_relu_33x9"), ("bias_as_feature", "rows_257"),
                                        ("bias_as_feature", "gauss_k3"), ("drop_last_row", "rows_2111"), ("drop_last_row", "scratch_in_chunks"),
                                        ("softmax_no_p", "outputs_7"), ("softmax_no_p", "cat_class_weights"), ("no_lik_temp", "cat_lik_temp_037")])
def test_wrong_variants_lie_beyond_the_device_bar(wrong, name):
    case, inp, want, want32 = gc.case_data(name)
    bar, _, _ = gc.bars(want, want32)
    bad = gc.reference(case, inp, wrong=wrong)
    over = [float(np.abs(g - w).max()) / b for g, w, b in zip(bad["grads"], want["grads"], bar)]
    assert max(over) > 10.0, (wrong, name, over)
    assert set(gc.WRONG) == {"no_factor", "bias_as_feature", "drop_last_row", "softmax_no_p", "no_lik_temp"}


# ---- the model side ---------------------------------------------------------------------------------------------------------------

def _model(mode="classification", n=300, f=7, nodes=(5, 4), seed=3, fun="tanh", **kw):
    rs = np.random.default_rng(seed)
    x = rs.standard_normal((n, f))
    teacher = [rs.normal(0, 1.0, (4, f + 1)), rs.normal(0, 1.0, (3, 5))]
    z = orc.forward_logits(x, teacher, orc.Act("tanh"))
    if mode == "classification":
        labels = np.digitize(z[:, 0], np.quantile(z[:, 0], [1 / 3, 2 / 3]))       # (three classes of equal size)
    else:
        labels = z[:, :2] + 0.3 * rs.standard_normal((n, 2))
    dat = dict(data=x, labels=labels, test_data=np.zeros((0, f)), test_labels=np.zeros(0))
    np.random.seed(1234)
    return quiet(bn.npBNN, dat, n_nodes=list(nodes), actFun=bn.ActFun(fun=fun), estimation_mode=mode, **kw)


@pytest.mark.parametrize("prior_f,hyper", [(1, 0), (2, 0), (3, 0), (0, 0), (1, 3)])
def test_prior_gradient_against_differences_of_calc_prior(prior_f, hyper):
    bnn = _model(prior_f=prior_f, p_scale=0.8)
    rs = np.random.default_rng(2)
    if hyper:
        bnn._prior_scale = [rs.uniform(0.5, 2.0, w.shape) for w in bnn._w_layers]
    w = [rs.normal(0, 0.7, m.shape) for m in bnn._w_layers]
    g = gradient.prior_grad(bnn, w)
    for l, m in enumerate(w):
        assert g[l].shape == m.shape
        for _ in range(5):
            i, j = int(rs.integers(m.shape[0])), int(rs.integers(m.shape[1]))
            up, down = [np.array(a, copy=True) for a in w], [np.array(a, copy=True) for a in w]
            up[l][i, j] += 1e-6
            down[l][i, j] -= 1e-6
            fd = (bnn.calc_prior(w=up) - bnn.calc_prior(w=down)) / 2e-6
            assert abs(fd - g[l][i, j]) <= 1e-6 * max(1.0, abs(g[l][i, j]))


def test_ridge_identity():
    """One matrix, identity output, normal prior with scale s and sigma 1: the MAP is the ridge solution
    W = Y^T X1 (X1^T X1 + I / s^2)^-1 with X1 = [1, X], and log_posterior_grad vanishes there."""
    rs = np.random.default_rng(8)
    n, f, k, s = 300, 7, 2, 1.7
    x = rs.standard_normal((n, f))
    y = x @ rs.standard_normal((f, k)) + 0.5 + 0.3 * rs.standard_normal((n, k))
    dat = dict(data=x, labels=y, test_data=np.zeros((0, f)), test_labels=np.zeros(0))
    bnn = quiet(bn.npBNN, dat, n_nodes=[], estimation_mode="regression", p_scale=s, prior_f=1, init_weights=[np.zeros((k, f + 1))])
    serve_from_oracle(lambda m: gc.GradOracleBackend(m, out_kind=1))
    x1 = np.concatenate([np.ones((n, 1)), x], axis=1)
    w = np.linalg.solve(x1.T @ x1 + np.eye(f + 1) / s ** 2, x1.T @ y).T
    ll, lp, grad, sigma = bn.log_posterior_grad(bnn, [w])
    big = gc.restate(x, y, [w], orc.Act("ReLU"), "gauss", sigma=np.ones(k))["A"][0]
    assert grad[0].shape == (k, f + 1) and np.abs(grad[0]).max() <= 1e-9 * big
    assert np.array_equal(sigma, np.ones(k))
    assert abs(ll - orc.lik_gaussian(orc.dense(x, w), y, sig2=np.ones(k))) <= 1e-9 * abs(ll) and lp == bnn.calc_prior(w=[w])
    moved = [w + 1e-3]
    assert np.abs(bn.log_posterior_grad(bnn, moved)[2][0]).max() > 1e-6 * big


def _served(dtype=np.float64):
    cls = gc.GradOracleBackend if dtype == np.float64 else gc.GradOracleBackend32
    serve_from_oracle(lambda m: cls(m, out_kind=0 if m._estimation_mode == "classification" else 1))


def test_map_estimate_classification():
    bnn = _model()
    _served()
    start = [np.array(w, copy=True) for w in bnn._w_layers]
    res = bn.map_estimate(bnn, n_iter=40, lr=0.05)
    assert res["n_iter"] == 40 and len(res["log_posterior"]) == 41 == len(res["log_lik"]) == len(res["grad_norm"])
    assert res["log_posterior"].max() > res["log_posterior"][0] + 10.0
    best = int(np.argmax(res["log_posterior"]))
    assert all(np.array_equal(a, b) for a, b in zip(bnn._w_layers, res["weights"]))            # (apply: the model is where the dict says)
    ll, lp, _, _ = bn.log_posterior_grad(bnn)
    assert ll + lp == res["log_posterior"][best] and ll == res["log_lik"][best]
    mcmc = quiet(bn.MCMC, bnn, n_iteration=10)
    assert abs(mcmc._logLik - res["log_lik"][best]) <= 1e-9 * abs(mcmc._logLik)
    # deterministic: the same run from the same start gives the same bits, and draws no random numbers
    bnn2 = _model()
    _served()
    assert all(np.array_equal(a, b) for a, b in zip(bnn2._w_layers, start))
    state = np.random.get_state()[1].copy()
    res2 = bn.map_estimate(bnn2, n_iter=40, lr=0.05, apply=False)
    assert np.array_equal(np.random.get_state()[1], state)
    assert np.array_equal(res2["log_posterior"], res["log_posterior"])
    assert all(np.array_equal(a, b) for a, b in zip(bnn2._w_layers, start))                  # (apply=False: untouched)


def test_map_estimate_float32_seam_stays_close():
    """the float32 restatement through the same seam, on the very model, seed and steps tests/test_hip_grad.py runs on the device
    (grad_cases.teacher_model): what the device's trace may differ by"""
    a, b = gc.teacher_model(), gc.teacher_model()
    _served()
    ra = bn.map_estimate(a, n_iter=gc.TEACHER_STEPS)
    _served(np.float32)
    rb = bn.map_estimate(b, n_iter=gc.TEACHER_STEPS)
    assert len(ra["log_posterior"]) == gc.TEACHER_STEPS + 1 == len(rb["log_posterior"])
    assert np.abs(rb["log_posterior"] / ra["log_posterior"] - 1).max() <= 1e-5


def test_map_estimate_mask_bound_and_early_stop():
    bnn = _model(w_bound=0.3)
    _served()
    rs = np.random.default_rng(4)
    mask = [(rs.random(w.shape) < 0.6).astype(float) for w in bnn._w_layers]
    quiet(bnn.apply_mask, mask)
    res = bn.map_estimate(bnn, n_iter=30, lr=0.05)
    for w, m in zip(res["weights"], mask):
        assert np.all(w[m == 0] == 0) and np.abs(w).max() <= 0.3
    assert np.abs(np.concatenate([w.ravel() for w in res["weights"]])).max() == 0.3            # (the walls were reached)
    _, _, grad, _ = bn.log_posterior_grad(bnn)
    assert all(np.all(g[m == 0] == 0) for g, m in zip(grad, mask))
    stopped = bn.map_estimate(_model(), n_iter=30, lr=0.05, tol=1.0)
    assert stopped["n_iter"] == 1 and len(stopped["log_posterior"]) == 2


def test_map_estimate_regression_sets_sigma():
    bnn = _model(mode="regression")
    _served()
    res = bn.map_estimate(bnn, n_iter=30, lr=0.05)
    assert res["log_posterior"].max() > res["log_posterior"][0]
    assert np.array_equal(bnn._error_prm, res["error_prm"]) and res["error_prm"].shape == (2,)
    z = orc.forward_logits(bnn._data, res["weights"], orc.Act("tanh"))
    assert np.allclose(res["error_prm"], np.sqrt(((bnn._labels - z) ** 2).mean(axis=0)), rtol=1e-12)
    fixed = _model(mode="regression")
    _served()
    kept = bn.map_estimate(fixed, n_iter=5, update_error_prm=False)
    assert np.array_equal(kept["error_prm"], np.ones(2)) and np.array_equal(fixed._error_prm, np.ones(2))


def test_indicators_and_feature_switches_reach_the_gradient():
    bnn = _model(feature_indicators=True)
    _served()
    bnn._feature_indicators[2] = 0
    ind = np.ones(bnn._w_layers[0].shape)
    ind[1, :] = 0
    bnn.reset_indicators(ind)
    ll, lp, grad, _ = bn.log_posterior_grad(bnn)
    x = bnn._data.copy()
    x[:, 2] = bnn._feature_means[2]
    fw = [bnn._w_layers[0] * ind] + list(bnn._w_layers[1:])
    want = gc.restate(x, bnn._labels, fw, orc.Act("tanh"), "cat")
    prior = gradient.prior_grad(bnn, bnn._w_layers)
    assert abs(ll - want["loglik"]) <= 1e-12 * abs(ll)
    assert np.abs(grad[0] - (want["grads"][0] * ind + prior[0])).max() <= 1e-12 * want["A"][0]
    assert np.array_equal(grad[0][1], prior[0][1])                                      # (a switched-off row: the prior alone)


def test_refusals():
    _served()
    with pytest.raises(ValueError, match="custom"):
        bn.map_estimate(_model(mode="custom", size_output=3))
    with pytest.raises(ValueError, match="poi_likelihood"):
        bn.map_estimate(_model(mode="regression"), likelihood_f=bn.poi_likelihood)
    with pytest.raises(ValueError, match="negbin_likelihood"):
        bn.log_posterior_grad(_model(mode="regression"), likelihood_f=bn.negbin_likelihood)
    with pytest.raises(ValueError, match="custom output callable"):
        bn.map_estimate(_model(mode="regression", output_act_fun=lambda z: z))
    with pytest.raises(ValueError, match="poi_likelihood"):
        bn.loglik_grad(np.zeros((3, 2)), np.zeros((3, 1)), [np.zeros((1, 3))], bn.ActFun(), bn.poi_likelihood)
    with pytest.raises(ValueError, match="sigma"):
        bn.loglik_grad(np.zeros((3, 2)), np.zeros((3, 1)), [np.zeros((1, 3))], bn.ActFun(), bn.calc_likelihood_regression)

    class Broken(gc.GradOracleBackend):
        def loglik_grad(self, weights, **kw):
            r, g = super().loglik_grad(weights, **kw)
            self.n_eval += 1
            if self.n_eval > 3:
                g[0][0, 0] = np.nan
            return r, g

    serve_from_oracle(lambda m: Broken(m, out_kind=0))
    with pytest.raises(FloatingPointError, match="step 3"):
        bn.map_estimate(_model(), n_iter=10)
