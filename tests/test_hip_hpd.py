"""HPD intervals on the GPU: npbnn_op_hpd (calcHPD, posterior_hpd) against the reference's outputs (tests/golden/hpd.npz), and
npbnn_predict_sets_hpd / get_posterior_hpd against npbnn_predict_sets / get_posterior_est followed by the numpy restatement of
calcHPD (tests/hpd_cases.py) on both evaluation paths."""
import os

import numpy as np
import pytest

import cases
import hpd_cases
import npbnn_amd as bn
from npbnn_amd import _capi as capi, device_ops

pytestmark = pytest.mark.gpu

CASES = hpd_cases.load()


@pytest.mark.parametrize("name", sorted(CASES))
def test_posterior_hpd_matches_reference(name):
    c = CASES[name]
    lo, hi = bn.posterior_hpd(c["x"], c["level"])
    assert lo.dtype == np.dtype(c["dtype"]) and lo.shape == (hpd_cases.N_COLS,)
    assert np.array_equal(lo.astype(np.float64), c["lo"]) and np.array_equal(hi.astype(np.float64), c["hi"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_calchpd_matches_reference(name):
    c = CASES[name]
    for col in (0, 1, 5):
        lo, hi = bn.calcHPD(c["x"][:, col], c["level"])
        assert type(lo) is np.dtype(c["dtype"]).type
        assert float(lo) == c["lo"][col] and float(hi) == c["hi"][col]


def test_calchpd_of_a_list():
    x = [0.3, -1.0, 2.5, 0.1, 0.2, 0.25, 9.0, 0.15, 0.05, 0.22]
    lo, hi = bn.calcHPD(x, 0.5)
    want = hpd_cases.hpd_columns(np.array(x), 0.5)
    assert (lo, hi) == (want[0], want[1])


@pytest.mark.parametrize("dtype,S,n_cols", [("float32", 1000, 100_000), ("float64", 257, 30_000), ("float32", 16384, 37),
                                            ("float64", 16384, 3)])
def test_posterior_hpd_large_shapes(dtype, S, n_cols):
    rs = np.random.default_rng(S + n_cols)
    x = rs.standard_normal((S, n_cols)).astype(dtype)
    x[:, ::7] = np.round(x[:, ::7] * 4)            # ties
    for level in (0.95, 0.05):
        lo, hi = bn.posterior_hpd(x, level)
        want = hpd_cases.hpd_columns(x, level)
        assert np.array_equal(lo, want[0]) and np.array_equal(hi, want[1])


def test_posterior_hpd_keeps_trailing_shape():
    x = np.random.default_rng(1).standard_normal((50, 4, 3))
    lo, hi = bn.posterior_hpd(x, 0.9)
    want = hpd_cases.hpd_columns(x, 0.9)
    assert lo.shape == (4, 3) and np.array_equal(lo, want[0]) and np.array_equal(hi, want[1])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("S,n_cols", [(17, 1), (17, 65), (257, 130)])
def test_op_hpd_strided_equals_packed_and_a_column_does_not_depend_on_its_tile(S, n_cols, dtype):
    """The columns sit in a wider array (col_stride = n_cols + 3): bounds byte for byte those of the packed call.  The columns are five
    distinct ones over and over, ties included, so a copy lands in another tile and at another place in it (65 columns of 17: a
    tile of 64 and one of 1; 130 of 257: tiles of 32 in float32 and of 16 in float64, the last of 2) and gives the bytes of the first."""
    rs = np.random.default_rng(1000 * S + n_cols)
    base = rs.standard_normal((S, 5)).astype(dtype)
    base[:, 3] = np.round(base[:, 3] * 4)
    idx = np.arange(n_cols) % 5
    v = np.ascontiguousarray(base[:, idx])
    lo, hi = bn.posterior_hpd(v, 0.9)
    want = hpd_cases.hpd_columns(v, 0.9)
    assert np.array_equal(lo, want[0]) and np.array_equal(hi, want[1])
    for j in range(n_cols):
        assert lo[j].tobytes() == lo[idx[j]].tobytes() and hi[j].tobytes() == hi[idx[j]].tobytes(), j
    lib, dev = device_ops._lib()
    wide = np.full((S, n_cols + 3), 7.0, dtype=dtype)
    wide[:, :n_cols] = v
    lo2, hi2 = np.empty(n_cols), np.empty(n_cols)
    rc = lib.npbnn_op_hpd(dev, wide.ctypes.data, capi.VALUE_F32 if dtype == "float32" else capi.VALUE_F64, S, n_cols, n_cols + 3, 0.9,
                          capi.dptr(lo2), capi.dptr(hi2))
    assert rc == 0 and lo2.tobytes() == lo.astype(np.float64).tobytes() and hi2.tobytes() == hi.astype(np.float64).tobytes()


# ---- the fused entry: replay into a device stack, one HPD launch

def _net(seed, n_features, n_nodes, n_out, n_sets, fun):
    rs = np.random.default_rng(seed)
    dims = [n_features] + list(n_nodes) + [n_out]
    weights = [[rs.normal(0, 0.6, (dims[i + 1], dims[i] + 1)) for i in range(len(dims) - 1)] for _ in range(n_sets)]
    slopes = None
    if fun == "genReLU":
        slopes = [rs.uniform(0.01, 0.4, len(n_nodes)) for _ in range(n_sets)]
        slopes[1] = slopes[0]                            # two neighbours that share their slopes, the rest do not
    return weights, slopes


FUSED = [
    dict(name="softmax", fun="tanh", out=capi.OUT_SOFTMAX, n_out=4, n_sets=10, level=0.95),
    dict(name="genrelu_slopes", fun="genReLU", out=capi.OUT_SOFTMAX, n_out=3, n_sets=11, level=0.8),
    dict(name="regression_3_targets", fun="swish", out=capi.OUT_IDENTITY, n_out=3, n_sets=7, level=0.5),
    dict(name="regress_error", fun="tanh", out=capi.OUT_SOFTPLUS_HALF, n_out=4, n_sets=32, level=0.9),
]


def _fused(c, wide, monkeypatch, n_rows=700):
    if wide:
        monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    rs = np.random.default_rng(5)
    x = rs.standard_normal((n_rows, 12))
    weights, slopes = _net(7, 12, (9, 5), c["n_out"], c["n_sets"], c["fun"])
    ctx = bn.HipContext()
    try:
        ctx.set_data(x)
        ctx.set_arch_from_weights(weights[0], 12, bn.ActFun(fun=c["fun"]).device_kind(), c["out"], capi.LIK_NONE)
        assert ctx.is_wide() == wide
        stack = ctx.predict_sets(weights, act_prm_sets=slopes)
        got = ctx.predict_sets_hpd(weights, c["level"], act_prm_sets=slopes)
    finally:
        ctx.close()
    return stack, got


@pytest.mark.parametrize("wide", [False, True], ids=["resident", "streamed"])
@pytest.mark.parametrize("c", FUSED, ids=lambda c: c["name"])
def test_predict_sets_hpd_equals_restatement_of_predict_sets(c, wide, monkeypatch):
    stack, (mean, lo, hi) = _fused(c, wide, monkeypatch)
    want_lo, want_hi = hpd_cases.hpd_columns(stack, c["level"])
    assert lo.shape == stack.shape[1:]
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)
    np.testing.assert_allclose(mean, np.mean(stack, axis=0), rtol=1e-12, atol=0)


def test_predict_sets_hpd_errors(monkeypatch):
    x = np.random.default_rng(2).standard_normal((500, 6))
    weights, _ = _net(3, 6, (5,), 2, 8, "tanh")
    ctx = bn.HipContext()
    try:
        ctx.set_data(x)
        ctx.set_arch_from_weights(weights[0], 6, bn.ActFun(fun="tanh").device_kind(), capi.OUT_SOFTMAX, capi.LIK_NONE)
        monkeypatch.setenv("NPBNN_HPD_STACK_BYTES", str(8 * 2 * 4 * 499))
        with pytest.raises(capi.NpbnnError) as e:
            ctx.predict_sets_hpd(weights, 0.9)
        assert e.value.code == capi.E_NOMEM and "499 rows" in str(e.value)
        monkeypatch.setenv("NPBNN_HPD_STACK_BYTES", str(8 * 2 * 4 * 500))
        mean, lo, hi = ctx.predict_sets_hpd(weights, 0.9)
        assert lo.shape == (500, 2)
        with pytest.raises(capi.NpbnnError) as e:
            ctx.predict_sets_hpd([weights[0]] * 16385, 0.9)
        assert e.value.code == capi.E_ARG
        for level in (0.0, 1.0, 0.1):              # (0.1 * 8 rounds to 1: too little data)
            with pytest.raises(capi.NpbnnError) as e:
                ctx.predict_sets_hpd(weights, level)
            assert e.value.code == capi.E_ARG
    finally:
        ctx.close()


# ---- from a checkpoint

def _regression_checkpoint(tmp_path, n_samples=7):
    dat = cases.regression_data(seed=5, n_rows=150, n_features=6, k=2, n_test=30)
    np.random.seed(1234)
    bnn = bn.npBNN(dat, n_nodes=[5, 4], actFun=bn.ActFun(fun="tanh"), use_bias_node=2, estimation_mode="regression")
    mcmc = bn.MCMC(bnn, n_iteration=50, sampling_f=10, print_f=1000, n_post_samples=n_samples)
    logger = bn.postLogger(bnn, wdir=str(tmp_path), filename="reg", log_all_weights=0)
    rs = np.random.default_rng(3)
    logger._post_weight_samples = [dict(weights=[w + rs.normal(0, 0.1, w.shape) for w in bnn._w_layers], alphas=np.zeros(3),
                                        mcmc_it=i, error_prm=np.array([1.0 + 0.1 * i, 0.9])) for i in range(n_samples)]
    pkl = os.path.join(str(tmp_path), "reg.pkl")
    bn.SaveObject([bnn, mcmc, logger], pkl)
    return pkl, dat


def _check_against_est(res, est, level, keys=("", "_test")):
    for sfx in keys:
        lo, hi = hpd_cases.hpd_columns(est['post_est' + sfx], level)
        assert np.array_equal(res['lower' + sfx], lo) and np.array_equal(res['upper' + sfx], hi)
        np.testing.assert_allclose(res['prm_mean' + sfx], est['prm_mean' + sfx], rtol=1e-12, atol=0)


@pytest.mark.parametrize("wide", [False, True], ids=["resident", "streamed"])
def test_get_posterior_hpd_of_a_checkpoint(tmp_path, wide, monkeypatch):
    if wide:
        monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    pkl, dat = _regression_checkpoint(tmp_path)
    est = bn.get_posterior_est(pkl)
    res = bn.get_posterior_hpd(pkl, level=0.8)
    assert sorted(res) == ['error_prm', 'lower', 'lower_test', 'prm_mean', 'prm_mean_test', 'upper', 'upper_test']
    _check_against_est(res, est, 0.8)
    np.testing.assert_array_equal(np.array(res['error_prm']), np.array(est['error_prm']))
    # a small stack budget: row blocks of 16 rows, the same result to float32 rounding (the row count of a launch picks the
    # evaluation kernel's build, whose sums round differently)
    monkeypatch.setenv("NPBNN_HPD_STACK_BYTES", str(7 * 2 * 4 * 16))
    blocked = bn.get_posterior_hpd(pkl, level=0.8)
    for k in res:
        if k != 'error_prm':
            np.testing.assert_allclose(blocked[k], res[k], rtol=1e-5, atol=1e-6, err_msg=k)


def test_get_posterior_hpd_with_features(tmp_path):
    pkl, dat = _regression_checkpoint(tmp_path)
    x = np.random.default_rng(8).standard_normal((90, 6))
    res = bn.get_posterior_hpd(pkl, level=0.95, features=x)
    assert sorted(res) == ['error_prm', 'lower', 'prm_mean', 'upper']
    model, _, logger = bn.load_obj(pkl)
    per_sample, _ = bn.get_posterior_cat_prob(x, logger._post_weight_samples, actFun=model._act_fun,
                                              output_act_fun=model._output_act_fun)
    lo, hi = hpd_cases.hpd_columns(per_sample, 0.95)
    assert np.array_equal(res['lower'], lo) and np.array_equal(res['upper'], hi)
    np.testing.assert_allclose(res['prm_mean'], per_sample.mean(axis=0), rtol=1e-12, atol=0)


def test_get_posterior_hpd_custom_output_callable(tmp_path, monkeypatch):
    """An output callable with no device kind: the host stack goes through posterior_hpd."""
    import importlib
    pkl, dat = _regression_checkpoint(tmp_path)
    model, mcmc, logger = bn.load_obj(pkl)
    model._output_act_fun = lambda z: np.tanh(z) * 2.0
    for mod in ("npbnn_amd.hpd", "npbnn_amd.posterior"):
        monkeypatch.setattr(importlib.import_module(mod), "load_obj", lambda path: [model, mcmc, logger])
    est = bn.get_posterior_est(pkl)
    res = bn.get_posterior_hpd(pkl, level=0.7)
    _check_against_est(res, est, 0.7)
