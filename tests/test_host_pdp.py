"""Partial dependence on the host (no GPU): the grid, the feature summary and get_pdp / pdp's bookkeeping against the reference's
outputs (tests/golden/pdp.npz).  The device seam is replaced by the oracle's float64 forward pass (tests/pdp_cases.py)."""
import importlib

import numpy as np
import pytest

import npbnn_amd as bn
import pdp_cases
from attrib_common import fake_checkpoint

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


def test_pdp_reads_checkpoint(oracle_seam, monkeypatch):
    """pdp(pickle_file, lists): the model's training matrix, mode, outputs, activation and output function, the logger's samples and
    the model's feature indicators go into get_pdp, one result per list."""
    pdp_mod = importlib.import_module("npbnn_amd.pdp")
    c = CASES["indicators"]
    args = pdp_cases.call_args(bn, c)
    focal, n_out = args[1], args[3]
    checkpoint = fake_checkpoint(args, c)
    monkeypatch.setattr(pdp_mod, "load_obj", lambda path: checkpoint)
    other = CASES["onehot"]
    res = bn.pdp("checkpoint.pkl", [focal, [4, 5, 6]])
    assert len(res) == 2
    np.testing.assert_allclose(res[0]["pdp"], c["pdp"], rtol=0, atol=1e-12)
    assert res[1]["feature"].shape == (3, 3) and res[1]["pdp"].shape == (3, n_out, 3)
    assert other["feature"].shape == (3, 3)


# ---- the guard of tests/test_hip_pdp_envelope.py: its references can tell a wrong kernel from a right one ------------------------------
MOVES = 1e-3


@pytest.mark.parametrize("name", list(pdp_cases.ENVELOPE))
def test_envelope_references_depend_on_grid_sets_and_overrides(name):
    """Every envelope case's float64 means are finite, move across the grid points and differ from set to set by more than 1e-3 (50
    times the GPU test's bar): a kernel that ignored the grid, an override or the table asked for, or that repeated one set, could
    not pass.  Only where col_override pins every focal column (or there is none) must the means NOT move.  A case of one grid point
    moves against the table left as it is; a case of one set has no second set to differ from."""
    case = pdp_cases.ENVELOPE[name]
    inp = pdp_cases.envelope_inputs(case)
    per_set = pdp_cases.envelope_oracle(case, inp, per_set=True)            # [grid, set, row, output]
    means = per_set.mean(axis=1)
    assert np.array_equal(means, pdp_cases.envelope_oracle(case, inp))
    assert means.shape == (len(inp["grid"]), inp["table"].shape[0], case["n_out"]) and np.all(np.isfinite(per_set))
    if case["pinned"]:
        assert np.ptp(means, axis=0).max() == 0
    elif len(inp["grid"]) > 1:
        assert np.abs(np.diff(means, axis=0)).max(axis=(1, 2)).min() > MOVES          # (every grid point against the next)
    else:
        assert np.abs(means - pdp_cases.envelope_oracle(case, inp, grid=False)).max() > MOVES
    for s in range(1, case["sets"]):
        assert np.abs(per_set[:, s] - per_set[:, s - 1]).max() > MOVES
    if inp["override"] is not None:
        assert np.abs(means - pdp_cases.envelope_oracle(case, inp, override=False)).max() > MOVES
    if case["which"] == 1:
        assert inp["x_test"].shape[0] != inp["x"].shape[0]
    if not case["apply_out"] and case["out"] != "identity":
        applied = pdp_cases.envelope_oracle(dict(case, apply_out=True), inp)
        assert np.abs(means - applied).max() > MOVES


def test_envelope_covers_what_it_names():
    """The table's spread, counted: depths, bias patterns, widths at route 1's edges, both routes, every activation and output kind."""
    cases = list(pdp_cases.ENVELOPE.values())
    assert {len(c["nodes"]) + 1 for c in cases} >= {1, 2, 3, 5}
    assert {c["bias"] for c in cases} == {"all", "none", "mixed01", "mixed10"}
    assert {c["nodes"][0] for c in cases if c["nodes"]} >= {1, 31, 32, 33, 63, 64, 65}
    assert {c["nodes"][1] for c in cases if len(c["nodes"]) > 1} >= {1, 3, 5, 9, 31, 32, 33}
    assert {c["n_out"] for c in cases} >= {1, 2, 3, 7, 32, 33}
    assert {c["rows"] for c in cases} >= {1, 255, 256, 257, 2111} and max(c["rows"] for c in cases) <= 2111
    assert max(c["features"] for c in cases) <= 528
    assert {c["route"] for c in cases} == {1, 2}
    assert {(c["fun"], c["trainable"]) for c in cases} == {("ReLU", False), ("ReLU", True), ("genReLU", False), ("swish", False), ("tanh", False)}
    assert {(c["out"], c["apply_out"]) for c in cases} == {(o, a) for o in ("softmax", "identity", "softplus_half") for a in (True, False)}
    assert sum(c["pinned"] for c in cases) <= 4
