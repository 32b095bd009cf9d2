"""HPD intervals on the host (no GPU): the numpy restatement of calcHPD against the reference's outputs (tests/golden/hpd.npz), the
argument checks that run before any device call, and get_posterior_hpd's bookkeeping with the device seam replaced by the oracle's
float64 forward pass and the restatement."""
import importlib
import os
import re

import numpy as np
import pytest

import hpd_cases
import npbnn_amd as bn
import oracle as orc
from attrib_common import _Holder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = hpd_cases.load()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_reference(name):
    c = CASES[name]
    lo, hi = hpd_cases.hpd_columns(c["x"], c["level"])
    assert lo.dtype == np.dtype(c["dtype"])
    assert np.array_equal(lo.astype(np.float64), c["lo"]) and np.array_equal(hi.astype(np.float64), c["hi"])


def test_fixture_covers_the_issue_grid():
    names = set(CASES)
    for s in hpd_cases.SIZES:
        assert "S%d_L0.95_float32" % s in names or hpd_cases.n_in(s, 0.95) < 2
    assert {"half_S10_L0.95_float64", "half_S30_L0.95_float32", "half_S5_L0.5_float64"} <= names
    assert hpd_cases.n_in(10, 0.95) == 10 and hpd_cases.n_in(30, 0.95) == 28 and hpd_cases.n_in(5, 0.5) == 2


@pytest.fixture
def no_device(monkeypatch):
    """Any device call fails the test."""
    hpd = importlib.import_module("npbnn_amd.hpd")

    def boom(*a, **k):
        raise AssertionError("device called")
    monkeypatch.setattr(hpd, "_op_hpd", boom)
    monkeypatch.setattr(hpd, "_hpd_row_blocks", boom)


@pytest.mark.parametrize("level", [0, 1, -0.5, 1.5])
def test_level_outside_0_1_asserts(level, no_device):
    with pytest.raises(AssertionError, match="^$"):
        bn.calcHPD(np.arange(10.0), level)
    with pytest.raises(AssertionError, match="^$"):
        bn.posterior_hpd(np.zeros((10, 3)), level)


@pytest.mark.parametrize("n,level", [(1, 0.95), (3, 0.3), (2, 0.7), (0, 0.5)])
def test_too_little_data_exits_like_upstream(n, level, no_device):
    with pytest.raises(SystemExit) as e:
        bn.calcHPD(np.arange(float(n)), level)
    assert e.value.code == '\n\nToo little data to calculate marginal parameters.'


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_raises_value_error(bad, no_device):
    x = np.arange(20.0)
    x[7] = bad
    with pytest.raises(ValueError):
        bn.calcHPD(x, 0.9)
    with pytest.raises(ValueError):
        bn.posterior_hpd(x.astype(np.float32).reshape(20, 1), 0.9)


def test_more_than_16384_samples_raises_value_error(no_device):
    with pytest.raises(ValueError):
        bn.calcHPD(np.zeros(16385), 0.95)
    with pytest.raises(ValueError):
        bn.posterior_hpd(np.zeros((16385, 2), dtype=np.float32))


def test_public_names_and_header():
    for name in ("calcHPD", "posterior_hpd", "get_posterior_hpd"):
        assert callable(getattr(bn, name))
    txt = open(os.path.join(ROOT, "include", "npbnn_hip.h")).read()
    for sym in ("npbnn_op_hpd", "npbnn_predict_sets_hpd"):
        assert re.search(r"\bint %s\(" % sym, txt)
    from npbnn_amd import _capi
    assert "npbnn_op_hpd" in _capi.SIGNATURES and "npbnn_predict_sets_hpd" in _capi.SIGNATURES


# ---- get_posterior_hpd on a checkpoint, the device seam replaced

def _checkpoint(fun="tanh", n_samples=9, n_out=3, classification=True, seed=0, n_rows=37, n_test=11):
    rs = np.random.default_rng(seed)
    n_features = 5
    dims = [n_features, 6, 4, n_out]
    samples = []
    for i in range(n_samples):
        w = [rs.normal(0, 0.7, (dims[l + 1], dims[l] + 1)) for l in range(3)]
        alphas = rs.uniform(0.01, 0.4, 2) if fun == "genReLU" else np.zeros(2)
        samples.append(dict(weights=w, alphas=alphas, error_prm=np.array([0.5 + i])))
    model = _Holder(_data=rs.standard_normal((n_rows, n_features)), _test_data=rs.standard_normal((n_test, n_features)),
                    _act_fun=bn.ActFun(fun=fun, prm=np.zeros(2)),
                    _output_act_fun=bn.SoftMax if classification else bn.RegressTransform, _size_output=n_out)
    return model, _Holder(_post_weight_samples=samples)


def _oracle_blocks(calls):
    def seam(blocks, post_samples, actFun, output_act_fun, level):
        out_fn = orc.out_softmax if output_act_fun is bn.SoftMax else orc.out_identity
        res = []
        for x in blocks:
            calls.append(x.shape)
            stack = np.array([out_fn(orc.forward_logits(x, s["weights"], orc.Act(actFun._function, prm=np.asarray(s["alphas"]))))
                              for s in post_samples])
            lo, hi = hpd_cases.hpd_columns(stack, level)
            res.append((stack.mean(axis=0), lo, hi))
        return res
    return seam


def _want(model, logger, matrix, level):
    act = model._act_fun
    out_fn = orc.out_softmax if model._output_act_fun is bn.SoftMax else orc.out_identity
    stack = np.array([out_fn(orc.forward_logits(np.asarray(matrix, dtype=float), s["weights"],
                                                orc.Act(act._function, prm=np.asarray(s["alphas"]))))
                      for s in logger._post_weight_samples])
    lo, hi = hpd_cases.hpd_columns(stack, level)
    return stack.mean(axis=0), lo, hi


@pytest.fixture
def seam(monkeypatch):
    hpd = importlib.import_module("npbnn_amd.hpd")
    calls = []
    monkeypatch.setattr(hpd, "_hpd_row_blocks", _oracle_blocks(calls))

    def use(model, logger):
        monkeypatch.setattr(hpd, "load_obj", lambda path: [model, None, logger])
        return calls
    return use


@pytest.mark.parametrize("fun,classification", [("tanh", True), ("genReLU", False)])
def test_get_posterior_hpd_keys_and_values(fun, classification, seam):
    model, logger = _checkpoint(fun=fun, n_out=3 if classification else 2, classification=classification)
    calls = seam(model, logger)
    res = bn.get_posterior_hpd("checkpoint.pkl", level=0.8)
    assert sorted(res) == ['error_prm', 'lower', 'lower_test', 'prm_mean', 'prm_mean_test', 'upper', 'upper_test']
    for sfx, matrix in (("", model._data), ("_test", model._test_data)):
        mean, lo, hi = _want(model, logger, matrix, 0.8)
        np.testing.assert_allclose(res['prm_mean' + sfx], mean, rtol=1e-14)
        assert np.array_equal(res['lower' + sfx], lo) and np.array_equal(res['upper' + sfx], hi)
    assert calls == [(37, 5), (11, 5)]
    np.testing.assert_array_equal(np.array(res['error_prm']), np.array([s['error_prm'] for s in logger._post_weight_samples]))
    # the last sample's slopes stay installed, as upstream's loop leaves them
    assert np.array_equal(np.asarray(model._act_fun._prm), logger._post_weight_samples[-1]['alphas'])


def test_get_posterior_hpd_with_features(seam):
    model, logger = _checkpoint()
    seam(model, logger)
    x = np.random.default_rng(9).standard_normal((23, 5))
    res = bn.get_posterior_hpd("checkpoint.pkl", level=0.95, features=x)
    assert sorted(res) == ['error_prm', 'lower', 'prm_mean', 'upper']
    mean, lo, hi = _want(model, logger, x, 0.95)
    assert np.array_equal(res['lower'], lo) and np.array_equal(res['upper'], hi)
    np.testing.assert_allclose(res['prm_mean'], mean, rtol=1e-14)


def test_get_posterior_hpd_row_blocks(seam, monkeypatch):
    """A stack over NPBNN_HPD_STACK_BYTES is served in row blocks whose stack fits; the result is the one of a single block (to
    the rounding of the oracle's matrix products, which differ with the block's shape)."""
    model, logger = _checkpoint(n_samples=9, n_out=3, n_rows=37, n_test=11)
    calls = seam(model, logger)
    whole = bn.get_posterior_hpd("checkpoint.pkl", level=0.9)
    del calls[:]
    monkeypatch.setenv("NPBNN_HPD_STACK_BYTES", str(9 * 3 * 4 * 10))        # ten rows per block
    blocked = bn.get_posterior_hpd("checkpoint.pkl", level=0.9)
    assert calls == [(10, 5), (10, 5), (10, 5), (7, 5), (10, 5), (1, 5)]
    for k in whole:
        if k != 'error_prm':
            np.testing.assert_allclose(blocked[k], whole[k], rtol=1e-13, atol=1e-15, err_msg=k)


def test_get_posterior_hpd_checks_before_the_device(monkeypatch, no_device):
    model, logger = _checkpoint(n_samples=3)
    monkeypatch.setattr(importlib.import_module("npbnn_amd.hpd"), "load_obj", lambda path: [model, None, logger])
    with pytest.raises(SystemExit):
        bn.get_posterior_hpd("checkpoint.pkl", level=0.3)
    with pytest.raises(AssertionError):
        bn.get_posterior_hpd("checkpoint.pkl", level=1.0)
