"""Partial dependence on the host (no GPU): the grid, the feature summary and get_pdp / pdp's bookkeeping against the reference's
outputs (tests/golden/pdp.npz).  The device seam is replaced by the oracle's float64 forward pass (tests/pdp_cases.py)."""
import importlib

import numpy as np
import pytest

import npbnn_amd as bn
import pdp_cases

CASES = pdp_cases.load()


@pytest.mark.parametrize("name", sorted(CASES))
def test_grid_and_summary_match_reference(name):
    c = CASES[name]
    assert np.array_equal(bn.get_feature_summary(c["x"], c["focal"]), c["summary"])
    grid = bn.make_pdp_features(c["x"], c["focal"])
    assert grid.shape == c["grid"].shape and np.array_equal(grid, c["grid"])


def test_grid_quirks():
    c = CASES["ordinal_min1"]
    assert not np.all(c["grid"] == np.round(c["grid"]))            # min 1: linspace(1, 4, 5) has non-integer steps
    assert np.array_equal(bn.make_pdp_features(CASES["two_continuous"]["x"], [0, 3]), np.eye(2))
    assert bn.make_pdp_features(CASES["continuous"]["x"], [0]).shape == (100, 1)


@pytest.fixture
def oracle_seam(monkeypatch):
    pdp_mod = importlib.import_module("npbnn_amd.pdp")
    monkeypatch.setattr(pdp_mod, "_pdp_row_means", pdp_cases.oracle_row_means)


@pytest.mark.parametrize("name", sorted(CASES))
def test_get_pdp_matches_reference(name, oracle_seam):
    c = CASES[name]
    args = pdp_cases.call_args(bn, c)
    res = bn.get_pdp(*args)
    assert np.array_equal(res["feature"], c["feature"])
    assert res["pdp"].shape == c["pdp"].shape
    np.testing.assert_allclose(res["pdp"], c["pdp"], rtol=0, atol=1e-12)
    assert np.array_equal(np.asarray(args[4]._prm, dtype=float), c["last_prm"])      # the last sample's slopes stay installed


def test_switched_off_focal_column_is_flat(oracle_seam):
    res = bn.get_pdp(*pdp_cases.call_args(bn, CASES["indicators"]))
    assert np.ptp(res["pdp"][:, :, 0], axis=0).max() < 1e-12


class _Holder:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_pdp_reads_checkpoint(oracle_seam, monkeypatch):
    """pdp(pickle_file, lists): the model's training matrix, mode, outputs, activation and output function, the logger's samples and
    the model's feature indicators go into get_pdp, one result per list."""
    pdp_mod = importlib.import_module("npbnn_amd.pdp")
    c = CASES["indicators"]
    x, focal, mode, n_out, act, out_fn, weights, alphas, _ = pdp_cases.call_args(bn, c)
    model = _Holder(_data=x, _estimation_mode=mode, _size_output=n_out, _act_fun=act, _output_act_fun=out_fn,
                    _feature_indicators=c["indicators"], _feature_means=c["means"])
    logger = _Holder(_post_weight_samples=[{"weights": w, "alphas": a} for w, a in zip(weights, alphas)])
    monkeypatch.setattr(pdp_mod, "load_obj", lambda path: [model, None, logger])
    other = CASES["onehot"]
    res = bn.pdp("checkpoint.pkl", [focal, [4, 5, 6]])
    assert len(res) == 2
    np.testing.assert_allclose(res[0]["pdp"], c["pdp"], rtol=0, atol=1e-12)
    assert res[1]["feature"].shape == (3, 3) and res[1]["pdp"].shape == (3, n_out, 3)
    assert other["feature"].shape == (3, 3)
