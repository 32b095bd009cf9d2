"""GPU tests of the reference's helper call surface (activation / output / likelihood / accuracy callables and the
free forward functions) served by the stand-alone device operators, against the golden vectors of the reference."""
import os

import numpy as np
import pytest

import cases
import npbnn_amd as bn
import oracle as orc

pytestmark = pytest.mark.gpu


def test_helper_callables_against_reference_golden(golden_dir):
    grid = np.load(os.path.join(golden_dir, "grid.npz"))
    case = [c for c in cases.grid_cases() if c["name"] == "f64_h32x8_c5_tanh_b2"][0]
    inp = cases.grid_inputs(case)
    k = case["name"]
    act = bn.ActFun(fun="tanh")
    x, w, lab = inp["x"], inp["weights"], inp["labels"]
    sid = np.arange(len(x))
    y = bn.RunPredict(x, w, act, bn.SoftMax)
    np.testing.assert_allclose(y[:16], grid[k + "/y_head"], atol=2e-5)
    z = bn.RunPredict(x, w, act, bn.RegressTransform)
    np.testing.assert_allclose(z[:16], grid[k + "/z_head"], rtol=2e-5, atol=2e-5)
    h0 = bn.RunHiddenLayer(x + 0, w[0], act, 0)
    np.testing.assert_allclose(h0[:16], grid[k + "/h0_head"], atol=2e-5)
    # likelihood / accuracy helpers on the float64 prediction matrix of the oracle: float64 device kernels
    y64 = orc.forward(x, w, orc.Act("tanh"), orc.out_softmax)
    lik = grid[k + "/lik"]
    np.testing.assert_allclose(bn.calc_likelihood(y64, lab, sid), lik[0], rtol=1e-12)
    np.testing.assert_allclose(bn.calc_likelihood(y64, lab, sid, instance_weight=inp["inst_w"]), lik[1], rtol=1e-12)
    np.testing.assert_allclose(bn.calc_likelihood(y64, lab, sid, class_weight=inp["class_w"]), lik[2], rtol=1e-12)
    np.testing.assert_allclose(bn.calc_likelihood(y64, lab, sid, lik_temp=0.5), lik[3], rtol=1e-12)
    with pytest.raises(Exception):
        bn.calc_likelihood(y64, lab, sid, class_weight=inp["class_w"], instance_weight=inp["inst_w"])
    assert bn.CalcAccuracy(y64, lab) == grid[k + "/acc"]
    np.testing.assert_array_equal(bn.CalcLabelAccuracy(y64, lab), grid[k + "/label_acc"])
    np.testing.assert_array_equal(bn.CalcLabelFreq(y64), grid[k + "/label_freq"])
    np.testing.assert_array_equal(bn.CalcAccuracy(np.stack([y64, y64]), lab), [grid[k + "/acc"]] * 2)
    # elementwise helpers
    zz = np.random.default_rng(0).normal(0, 2, (37, 9))
    np.testing.assert_allclose(bn.SoftMax(zz), orc.out_softmax(zz), rtol=1e-13)
    np.testing.assert_allclose(bn.SoftPlus(zz), orc.softplus(zz), rtol=1e-13)
    np.testing.assert_allclose(bn.tanh_f(zz + 0, 0), orc.activate(zz + 0, orc.Act("tanh"), 0), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(bn.swish_f(zz + 0, 0), orc.activate(zz + 0, orc.Act("swish"), 0), rtol=1e-13)
    a = zz + 0
    assert bn.relu_f(a, 0) is a and a.min() == 0.0                       # in place, like the reference
    np.testing.assert_allclose(bn.ActFun("genReLU", prm=np.array([0.1, 0.2])).eval(zz + 0, 1),
                               orc.activate(zz + 0, orc.Act("genReLU", prm=np.array([0.1, 0.2])), 1), rtol=1e-13)
    np.testing.assert_allclose(bn.MatrixMultiplicationD(x, w[0]), orc.dense(x, w[0]), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(bn.MatrixMultiplication(x, w[0]), orc.dense(x, w[0]), rtol=2e-5, atol=2e-5)
    ind = (np.random.default_rng(1).random(w[0].shape) < 0.7).astype(float)
    np.testing.assert_allclose(bn.RunPredictInd(x, w, ind, act, bn.SoftMax),
                               orc.forward(x, w, orc.Act("tanh"), orc.out_softmax, indicators=ind), atol=2e-5)


def test_regression_and_count_helpers(golden_dir):
    g = np.load(os.path.join(golden_dir, "regression.npz"))
    inp = cases.regression_inputs()
    y, t = g["y"], inp["targets"]
    np.testing.assert_allclose(bn.calc_likelihood_regression(y, t, None, sig2=1), g["lik_sig1"], rtol=1e-12)
    np.testing.assert_allclose(bn.calc_likelihood_regression(y, t, None, sig2=inp["sig_vec"]), g["lik_sigvec"], rtol=1e-12)
    np.testing.assert_allclose(bn.calc_likelihood_regression(y, t, None, sig2=g["emp_sigma"], lik_temp=0.7), g["lik_emp_temp"], rtol=1e-12)
    np.testing.assert_allclose(bn.CalcAccuracyRegression(y, t), g["mse"], rtol=1e-12)
    np.testing.assert_allclose(bn.CalcLabelAccuracyRegression(y, t), g["mse_col"], rtol=1e-12)
    inp2 = cases.regression_inputs(seed=12, double_out=True)
    np.testing.assert_allclose(bn.calc_likelihood_regression_error(g["y_err"], inp2["targets"], None), g["lik_err"], rtol=1e-12)
    z = orc.forward_logits(inp2["x"], inp2["weights"], orc.Act("tanh"))
    np.testing.assert_allclose(bn.RegressTransformError(z + 0), g["y_err"], rtol=1e-12, atol=1e-14)
    c = np.load(os.path.join(golden_dir, "counts.npz"))
    a = cases.count_inputs(seed=23, n_out=1, k=1)
    np.testing.assert_allclose(bn.poi_likelihood(c["poi_z"], a["counts"]), c["poi"], rtol=1e-11)
    np.testing.assert_allclose(bn.poi_acc(c["poi_z"], a["counts"]), c["poi_acc"], rtol=1e-12)
    b = cases.count_inputs(seed=24, n_out=2, k=1)
    np.testing.assert_allclose(bn.negbin_likelihood(c["nb_z"], b["counts"]), c["nb"], rtol=1e-9)
    np.testing.assert_allclose(bn.negbin_likelihood_base10(c["nb_z"], b["counts"]), c["nb10"], rtol=1e-9)
    np.testing.assert_allclose(bn.negbin_acc(c["nb_z"], b["counts"]), c["nb_acc"], rtol=1e-12)
    np.testing.assert_allclose(bn.negbin_acc_base10(c["nb_z"], b["counts"]), c["nb10_acc"], rtol=1e-12)
    d = cases.count_inputs(seed=25, n_out=4, k=2)
    np.testing.assert_allclose(bn.negbin_likelihood2d(c["nb2d_z"], d["counts"]), c["nb2d"], rtol=1e-9)
    np.testing.assert_allclose(bn.negbin2d_acc(c["nb2d_z"], d["counts"]), c["nb2d_acc"], rtol=1e-12)


def test_custom_callables_take_the_slow_path():
    """User output function + likelihood + accuracy callables (estimation_mode='custom', as in the reference's
    test_BNNexpectation.py): the device returns the last layer's values, the callables run on the host."""
    import contextlib, io
    rs = np.random.default_rng(3)
    n, f = 400, 12
    x = rs.standard_normal((n, f))
    counts = rs.poisson(4.0, (n, 1)).astype(float)
    dat = dict(data=x, labels=counts, test_data=np.zeros((0, f)), test_labels=np.zeros(0))

    def my_out(z):
        return np.clip(z, -5, 5)

    def my_lik(prediction, true_values, sample_id=None, class_weight=None, instance_weight=None, lik_temp=1, sig2=0):
        return float(np.sum(true_values[:, 0] * prediction[:, 0] - np.exp(prediction[:, 0])))

    np.random.seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        bnn = bn.npBNN(dat, n_nodes=[6, 3], estimation_mode="custom", size_output=1, output_act_fun=my_out,
                       actFun=bn.ActFun(fun="swish"), use_bias_node=2)
    mcmc = bn.MCMC(bnn, likelihood_f=my_lik, n_iteration=100)
    y64 = my_out(orc.forward_logits(x, bnn._w_layers, orc.Act("swish")))
    np.testing.assert_allclose(mcmc._logLik, my_lik(y64, counts), rtol=1e-5)
    for _ in range(30):
        mcmc.mh_step(bnn)
    mcmc.run_steps(bnn, 20)                       # falls back to mh_step: custom likelihood
    assert mcmc._current_iteration == 50 and mcmc._accuracy == 1.0
    y64 = my_out(orc.forward_logits(x, bnn._w_layers, orc.Act("swish")))
    np.testing.assert_allclose(mcmc._logLik, my_lik(y64, counts), rtol=1e-5)
    # the fused plug-in likelihood gives the same chain law: check its value on the same weights
    with contextlib.redirect_stdout(io.StringIO()):
        bnn2 = bn.npBNN(dat, n_nodes=[6, 3], estimation_mode="custom", size_output=1, actFun=bn.ActFun(fun="swish"),
                        use_bias_node=2, init_weights=[w + 0 for w in bnn._w_layers])
    m2 = bn.MCMC(bnn2, likelihood_f=bn.poi_likelihood, accuracy_f=bn.poi_acc, n_iteration=100)
    z64 = orc.forward_logits(x, bnn2._w_layers, orc.Act("swish"))
    np.testing.assert_allclose(m2._logLik, orc.lik_poisson(z64, counts), rtol=2e-6)
    m2.run_steps(bnn2, 40)                        # device-resident chain with the fused Poisson likelihood
    z64 = orc.forward_logits(x, bnn2._w_layers, orc.Act("swish"))
    np.testing.assert_allclose(m2._logLik, orc.lik_poisson(z64, counts), rtol=2e-6)
    np.testing.assert_allclose(m2._accuracy, np.mean((np.exp(z64[:, 0]) - counts[:, 0]) ** 2), rtol=1e-4)


# ---- every operator at every size, against float64 ----------------------------------------------------------------------------
# grid_for caps a launch at 1 024 blocks of 256 threads: 300 001 rows take the grid-stride loops of lik_kernel / sse_kernel /
# confusion_kernel round a second time.  The likelihood bar is relative to S, the sum of the absolute values of the addends
# (the count likelihoods cancel: terms of 1e6 summing to a few units per row).
OP_ROWS = [1, 255, 256, 257, 300_001]
OP_RTOL = 1e-12


def _count_addends(kind, z, y):
    from scipy.special import gammaln as g
    k = y.shape[1]
    if kind == "poi":
        return np.sum(np.abs(y[:, 0] * z[:, 0]) + np.exp(z[:, 0]) + np.abs(g(y[:, 0] + 1)))
    kk = k if kind == "nb2d" else 1
    off = k if kind == "nb2d" else 1
    b = np.log(10.0) if kind == "nb10" else 1.0
    mean, p = np.exp(b * z[:, :kk]), 1 / (1 + np.exp(-b * z[:, off:off + kk]))
    n = p * mean / (1 - p)
    c = y[:, :kk]
    return np.sum(np.abs(g(c + n)) + np.abs(g(c + 1)) + np.abs(g(n)) + np.abs(n * np.log(p)) + np.abs(c * np.log1p(-p)))


def _op_inputs(kind, n, rs, edge=False):
    """A prediction matrix and targets for one likelihood kind; ``edge``: eta to +-80, NegBin logits to +-30, large counts."""
    if kind == "err":
        k = 3
        y = rs.standard_normal((n, 2 * k))
        y[:, k:] = orc.softplus(y[:, k:] * (20 if edge else 1) - (30 if edge else 0))
        return y, rs.standard_normal((n, k)), k
    if kind == "poi":
        z = rs.uniform(-80, 80, (n, 2)) if edge else rs.normal(1, 1, (n, 2))
        t = rs.poisson(np.exp(np.clip(z[:, :1], -20, 25))).astype(float)
        return z, t, 1
    k = 3 if kind == "nb2d" else 1
    z = rs.normal(0.5, 1.0, (n, 2 * k + (kind == "nb")))
    off = k if kind == "nb2d" else 1
    if edge:
        z[:, off:off + k] = rs.uniform(-30, 30, (n, k)) if kind != "nb10" else rs.uniform(-6, 6, (n, k))
        z[:, :k] *= 4
    t = rs.poisson(np.exp(np.clip(z[:, :k] * (np.log(10.0) if kind == "nb10" else 1), -20, 12))).astype(float)
    return z, t, k


COUNT_OPS = {"poi": (bn.poi_likelihood, orc.lik_poisson), "nb": (bn.negbin_likelihood, orc.lik_negbin),
             "nb10": (bn.negbin_likelihood_base10, orc.lik_negbin_base10), "nb2d": (bn.negbin_likelihood2d, orc.lik_negbin2d)}


@pytest.mark.parametrize("n", OP_ROWS)
def test_likelihood_operators_at_every_size(n):
    rs = np.random.default_rng(n)
    # categorical: plain, instance / class weights, tempered, and a subset of rows through sample_id
    c = 7
    y = rs.random((n, c)) + 1e-3
    y /= y.sum(axis=1, keepdims=True)
    lab = rs.integers(0, c, n)
    sid = np.arange(n)
    s = np.sum(np.abs(np.log(y[sid, lab])))
    iw, cw = rs.uniform(0.5, 2, n), rs.uniform(0.5, 2, c)
    for kw in ({}, dict(instance_weight=iw), dict(class_weight=cw), dict(lik_temp=0.3)):
        got = bn.calc_likelihood(y, lab, sid, **kw)
        want = orc.lik_categorical(y, lab, sid, **kw)
        assert abs(got - want) <= OP_RTOL * 2 * s, (kw, got, want)
    sub = rs.permutation(n)[: max(1, n // 3)]
    got = bn.calc_likelihood(y, lab[sub], sub)
    assert abs(got - orc.lik_categorical(y, lab[sub], sub)) <= OP_RTOL * s
    # Gaussian with a sigma per column, and with predicted sigma
    t = rs.standard_normal((n, 2))
    sig = np.array([0.7, 1.9])
    got = bn.calc_likelihood_regression(y[:, :2], t, None, sig2=sig, lik_temp=0.8)
    want = orc.lik_gaussian(y[:, :2], t, None, sig2=sig, lik_temp=0.8)
    assert abs(got - want) <= OP_RTOL * abs(want)               # (every addend is negative here: |want| is S)
    for edge in (False, True):
        p, tt, k = _op_inputs("err", n, rs, edge)
        r = (tt - p[:, :k]) / p[:, k:]
        s = np.sum(0.9189385332046727 + np.abs(np.log(p[:, k:])) + 0.5 * r * r)
        got = bn.calc_likelihood_regression_error(p, tt, None, lik_temp=0.6)
        want = orc.lik_gaussian_error(p, tt, None, lik_temp=0.6)
        assert abs(got - want) <= OP_RTOL * 0.6 * s, (edge, got, want)


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("kind", ["poi", "nb", "nb10", "nb2d"])
@pytest.mark.parametrize("n", OP_ROWS)
def test_count_likelihood_operators_at_every_size(n, kind, edge):
    rs = np.random.default_rng(n + 17)
    z, t, k = _op_inputs(kind, n, rs, edge)
    f, ref = COUNT_OPS[kind]
    got = f(z, t, None)
    with np.errstate(all="ignore"):
        want = ref(z, t)
        s = _count_addends(kind, z, t)
    assert np.isfinite(want) and np.isfinite(s)
    assert abs(got - want) <= OP_RTOL * s, (got, want, abs(got - want) / s)
    assert f(z, t, None, lik_temp=0.25) == got                  # ignored, as upstream does


def test_count_likelihood_operator_gives_the_references_non_finite_class():
    """Base-10 NegBin logits of 30: p = 1 / (1 + 10^-30) rounds to 1 and n to inf, float64's result is NaN - the device's too;
    a row with exp(eta) = inf gives -inf on both."""
    z = np.array([[1.0, 0.5], [0.2, 30.0], [0.3, -0.2]])
    t = np.array([[2.0], [3.0], [0.0]])
    with np.errstate(all="ignore"):
        assert np.isnan(orc.lik_negbin_base10(z, t))
    assert np.isnan(bn.negbin_likelihood_base10(z, t, None))
    zp = np.array([[1.0], [800.0]])
    tp = np.array([[0.0], [0.0]])
    with np.errstate(all="ignore"):
        assert orc.lik_poisson(zp, tp) == -np.inf
    assert bn.poi_likelihood(zp, tp, None) == -np.inf


def _argmax_matrix(n, rs, c=6):
    """Random rows, with ties (first maximum wins) and NaN rows (the first NaN wins, as np.argmax) sprinkled in."""
    y = rs.random((n, c))
    y[::7] = np.round(y[::7] * 2) / 2                 # many exact ties
    y[3::11, 2] = np.nan
    y[5::13, :] = 0.25                                # a row of equal values
    y[8::17, 4] = np.nan
    y[8::17, 1] = np.nan
    return y


@pytest.mark.parametrize("n", OP_ROWS)
def test_accuracy_operators_at_every_size_with_ties_and_nan(n):
    rs = np.random.default_rng(n + 3)
    y = _argmax_matrix(n, rs)
    lab = rs.integers(0, y.shape[1], n)
    assert bn.CalcAccuracy(y, lab) == orc.acc_classification(y, lab)
    np.testing.assert_array_equal(bn.CalcLabelAccuracy(y, lab), orc.label_acc_classification(y, lab))
    np.testing.assert_array_equal(bn.CalcLabelFreq(y), orc.label_freq(y))
    np.testing.assert_array_equal(np.stack([bn.CalcLabelFreq(y)] * 2), [orc.label_freq(y)] * 2)


def test_argmax_of_a_nan_row_is_the_first_nan():
    y = np.array([[0.1, np.nan, 0.9, np.nan], [np.nan, 0.5, 0.2, 0.1], [0.3, 0.3, 0.1, 0.3], [0.1, 0.2, 0.9, 0.9]])
    want = np.bincount(np.argmax(y, axis=1), minlength=4) / 4          # the rows pick 1, 0, 0, 2
    np.testing.assert_array_equal(bn.CalcLabelFreq(y), want)
    np.testing.assert_array_equal(want, [0.5, 0.25, 0.25, 0.0])


@pytest.mark.parametrize("n", OP_ROWS)
def test_mse_operators_at_every_size(n):
    rs = np.random.default_rng(n + 5)
    y = rs.normal(0.5, 1.0, (n, 5))
    lab = rs.normal(1.0, 2.0, (n, 3))
    np.testing.assert_allclose(bn.CalcAccuracyRegression(y, lab), orc.mse_all(y, lab), rtol=OP_RTOL)
    np.testing.assert_allclose(bn.CalcLabelAccuracyRegression(y, lab), orc.mse_per_column(y, lab), rtol=OP_RTOL)
    cnt = rs.poisson(3.0, (n, 3)).astype(float)
    np.testing.assert_allclose(bn.poi_acc(y, cnt), np.mean((np.exp(y[:, 0]) - cnt[:, 0]) ** 2), rtol=OP_RTOL)
    np.testing.assert_allclose(bn.negbin_acc(y, cnt), np.mean((np.exp(y[:, 0]) - cnt[:, 0]) ** 2), rtol=OP_RTOL)
    np.testing.assert_allclose(bn.negbin_acc_base10(y, cnt), np.mean((10 ** y[:, 0] - cnt[:, 0]) ** 2), rtol=OP_RTOL)
    np.testing.assert_allclose(bn.negbin2d_acc(y, cnt), np.mean((np.exp(y[:, :3]) - cnt) ** 2), rtol=OP_RTOL)
