"""CPU: the stand-alone operators (npbnn_amd.device_ops) check their per-row arguments before the device is touched.

npbnn_op_likelihood / _confusion / _sse read ``rows`` entries of every per-row host array, in their label checks and in their
copies to the device; a shorter array was read past its end.  The wrapper now refuses it with a ValueError (the reference fails
on such arguments with a numpy error) - and does so before it loads the library, which these tests make impossible."""
import numpy as np
import pytest

import npbnn_amd as bn
from npbnn_amd import _capi as capi
from npbnn_amd import device_ops


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def refuse():
        raise AssertionError("the operator touched the device before checking its arguments")
    monkeypatch.setattr(device_ops, "_lib", refuse)


def _probs(n, c, seed=0):
    p = np.random.default_rng(seed).random((n, c))
    return p / p.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("n_lab", [9, 11, 0])
def test_categorical_labels_must_match_the_rows(n_lab):
    with pytest.raises(ValueError, match="labels"):
        bn.calc_likelihood(_probs(10, 3), np.zeros(n_lab, dtype=int), np.arange(10))


def test_categorical_instance_weight_must_match_the_rows():
    with pytest.raises(ValueError, match="instance_weight"):
        bn.calc_likelihood(_probs(10, 3), np.zeros(10, dtype=int), np.arange(10), instance_weight=np.ones(7))


def test_sample_id_selects_the_rows_and_the_labels_follow_it():
    """prediction[sample_id, labels]: 4 rows used, so 4 labels (and 4 instance weights) - not the prediction's 10."""
    p = _probs(10, 3)
    sid = np.array([1, 4, 5, 9])
    with pytest.raises(ValueError, match="labels has 10 rows, the prediction rows used are 4"):
        bn.calc_likelihood(p, np.zeros(10, dtype=int), sid)
    with pytest.raises(ValueError, match="instance_weight"):
        bn.calc_likelihood(p, np.zeros(4, dtype=int), sid, instance_weight=np.ones(10))
    with pytest.raises(IndexError):
        bn.calc_likelihood(p, np.zeros(4, dtype=int), np.array([1, 4, 5, 10]))     # a row the prediction does not have


@pytest.mark.parametrize("f", [bn.poi_likelihood, bn.negbin_likelihood, bn.negbin_likelihood_base10, bn.negbin_likelihood2d,
                               bn.calc_likelihood_regression, bn.calc_likelihood_regression_error])
def test_targets_must_match_the_rows(f):
    z = np.zeros((10, 4))
    for n_t in (9, 11):
        with pytest.raises(ValueError, match="targets"):
            f(z, np.ones((n_t, 2)), None)


def test_the_count_kinds_ignore_sample_id_and_instance_weight_like_upstream(monkeypatch):
    """BNN_lik.py: sample_id and instance_weight are accepted and unused - a short one is no error, and reaches no copy."""
    seen = {}

    class Lib:
        def npbnn_op_likelihood(self, dev, kind, pred, rows, cols, lab, tg, k, iw, cw, n_cw, temp, sg, out):
            seen.update(rows=rows, k=k, iw=iw)
            return 0
    monkeypatch.setattr(device_ops, "_lib", lambda: (Lib(), 0))
    bn.poi_likelihood(np.zeros((10, 1)), np.ones((10, 1)), np.arange(3), instance_weight=np.ones(2))
    assert seen["rows"] == 10 and seen["k"] == 1 and not seen["iw"]


def test_sample_id_rows_reach_the_operator(monkeypatch):
    """Only the selected rows are handed to the C operator, in sample_id's order."""
    seen = {}

    class Lib:
        def npbnn_op_likelihood(self, dev, kind, pred, rows, cols, lab, tg, k, iw, cw, n_cw, temp, sg, out):
            seen["pred"] = np.ctypeslib.as_array(pred, (rows, cols)).copy()
            seen["lab"] = np.ctypeslib.as_array(lab, (rows,)).copy()
            return 0
    monkeypatch.setattr(device_ops, "_lib", lambda: (Lib(), 0))
    p = _probs(10, 3)
    sid = np.array([9, 0, 4])
    bn.calc_likelihood(p, np.array([2, 1, 0]), sid)
    np.testing.assert_array_equal(seen["pred"], p[sid])
    np.testing.assert_array_equal(seen["lab"], [2, 1, 0])


@pytest.mark.parametrize("stat", [bn.CalcAccuracy, bn.CalcLabelAccuracy])
def test_accuracy_labels_must_match_the_rows(stat):
    with pytest.raises(ValueError, match="labels"):
        stat(_probs(10, 3), np.zeros(8, dtype=int))


@pytest.mark.parametrize("stat", [bn.CalcAccuracyRegression, bn.CalcLabelAccuracyRegression, bn.poi_acc, bn.negbin_acc,
                                  bn.negbin_acc_base10, bn.negbin2d_acc])
def test_mse_targets_must_match_the_rows(stat):
    with pytest.raises(ValueError, match="targets"):
        stat(np.zeros((10, 4)), np.ones((12, 2)))


def test_mse_targets_wider_than_the_prediction_are_refused():
    with pytest.raises(ValueError, match="target columns"):
        bn.CalcAccuracyRegression(np.zeros((10, 2)), np.ones((10, 3)))


def test_the_operators_take_matrices():
    with pytest.raises(ValueError, match="matrix"):
        device_ops.likelihood(capi.LIK_POISSON, np.zeros(10), np.ones(10))
    with pytest.raises(ValueError, match="matrix"):
        bn.CalcLabelFreq(np.zeros(10))
