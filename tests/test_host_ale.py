"""Accumulated local effects on the host (no GPU): the float64 restatements of tests/ale_cases.py against each other and against
a closed form, the edges, get_ale / ale's bookkeeping with the device seam replaced by the oracle's forward pass, the ABI
entry, and the guard of tests/test_hip_ale.py's case table."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import ale_cases
import npbnn_amd as bn
import oracle as orc
import pdp_cases
from attrib_common import fake_checkpoint
from npbnn_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = pdp_cases.load()
ALE_MOD = importlib.import_module("npbnn_amd.ale")


def _small(seed=3, rows=70, features=6, nodes=(5,), n_out=3, sets=3):
    rs = np.random.default_rng(seed)
    x = rs.standard_normal((rows, features))
    dims = [features] + list(nodes) + [n_out]
    weights = [[rs.normal(0, 1.0 / np.sqrt(dims[i] + 1), (dims[i + 1], dims[i] + 1)) for i in range(len(dims) - 1)] for _ in range(sets)]
    return x, weights


# ---- the two restatements ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(out_fn=orc.out_identity, fun="swish"), dict(fun="genReLU", slopes=[[0.1], [0.3], [0.45]]),
                                dict(override={4: 0.7}), dict(override={2: 0.7})],
                         ids=["softmax_tanh", "identity_swish", "own_slopes", "override_beside", "override_on_focal"])
def test_vectorised_form_equals_the_row_loop(kw):
    x, weights = _small()
    kw = dict(kw)
    if "override" in kw:
        co = np.full(x.shape[1], np.nan)
        for col, v in kw["override"].items():
            co[col] = v
        kw["override"] = co
    edges = bn.make_ale_edges(x, 2, n_bins=6)
    edges[0] += 0.3          # rows below the first edge ...
    edges[-1] -= 0.3         # ... and above the last
    counts, effects = ale_cases.local_effects(x, 2, edges, weights, **kw)
    counts_loop, effects_loop = ale_cases.loop_local_effects(x, 2, edges, weights, **kw)
    assert np.array_equal(counts, counts_loop) and counts.sum() == x.shape[0]
    assert np.abs(effects - effects_loop).max() < 1e-12
    if kw.get("override") is not None and not np.isnan(kw["override"][2]):
        assert np.all(effects == 0)
    else:
        assert np.abs(effects).min(axis=(1, 2)).max() > 0
    assert np.abs(ALE_MOD.accumulate_and_centre(counts, effects) - ale_cases.curve(counts, effects)).max() < 1e-12


def test_bins_follow_the_definition_at_ties_and_ends():
    edges = np.array([0.0, 1.0, 2.0, 3.0])
    col = np.array([-5.0, 0.0, 0.5, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), 2.0, 3.0, 3.5])
    assert ale_cases.bins_of(col, edges).tolist() == [0, 0, 0, 0, 1, 1, 2, 2]
    # a tie in float64 stays a tie after both sides are rounded to float32
    z = 0.1
    assert ale_cases.bins_of(np.array([z]), np.array([0.0, z, 1.0])).tolist() == [0]


@pytest.mark.parametrize("near_copy", [False, True])
@pytest.mark.parametrize("bias", [0, 1])
def test_closed_form_of_a_linear_network(near_copy, bias):
    """One matrix, identity output: f(x) = b + W x, so moving column j from z_(k-1) to z_k changes output c by W[c, j] (z_k - z_(k-1))
    whatever the other columns hold - also when one of them is nearly column j itself, where partial dependence and ALE part ways."""
    rs = np.random.default_rng(11)
    n, f, c, j = 200, 5, 4, 1
    x = rs.standard_normal((n, f))
    if near_copy:
        x[:, 3] = x[:, j] + 1e-3 * rs.standard_normal(n)
    weights = [[rs.normal(0, 1, (c, f + bias))] for _ in range(3)]
    edges = bn.make_ale_edges(x, j, n_bins=8)
    counts, effects = ale_cases.local_effects(x, j, edges, weights, out_fn=orc.out_identity)
    assert counts.min() > 0
    for s, w in enumerate(weights):
        want = np.outer(np.diff(edges), w[0][:, bias + j])
        assert np.abs(effects[s] - want).max() < 1e-12
    centred = ale_cases.curve(counts, effects)
    mid = 0.5 * (centred[:, :-1] + centred[:, 1:])
    assert np.abs(np.einsum("k,skc->sc", counts, mid)).max() / n < 1e-12
    # the centred curve is the line through the count-weighted mean of the bin midpoints
    z_mean = np.sum(counts * 0.5 * (edges[:-1] + edges[1:])) / n
    for s, w in enumerate(weights):
        assert np.abs(centred[s] - np.outer(edges - z_mean, w[0][:, bias + j])).max() < 1e-12


# ---- the edges -----------------------------------------------------------------------------------------------------------------------
def test_edges_of_a_continuous_column():
    x = np.random.default_rng(0).standard_normal((500, 3))
    edges = bn.make_ale_edges(x, [1], n_bins=10)
    assert edges.shape == (11,) and np.all(np.diff(edges) > 0)
    assert edges[0] == x[:, 1].min() and edges[-1] == x[:, 1].max()
    assert np.array_equal(edges, np.quantile(x[:, 1], np.linspace(0, 1, 11)))
    counts = np.bincount(ale_cases.bins_of(x[:, 1], edges), minlength=10)
    assert counts.sum() == 500 and counts.min() >= 49 and counts.max() <= 51
    assert bn.make_ale_edges(x, 1).shape == (41,)


def test_edges_of_an_ordinal_column_are_its_values():
    rs = np.random.default_rng(1)
    x = rs.standard_normal((300, 3))
    x[:, 2] = rs.integers(1, 5, 300)
    assert np.array_equal(bn.make_ale_edges(x, 2, n_bins=40), [1.0, 2.0, 3.0, 4.0])
    x[:, 0] = rs.integers(0, 2, 300)
    assert np.array_equal(bn.make_ale_edges(x, 0), [0.0, 1.0])


def test_edges_refuse_a_constant_column_and_two_columns():
    x = np.random.default_rng(2).standard_normal((50, 3))
    x[:, 1] = 2.5
    with pytest.raises(ValueError):
        bn.make_ale_edges(x, 1)
    with pytest.raises(ValueError):
        bn.make_ale_edges(x, [0, 2])


def test_repeated_quantiles_collapse():
    rs = np.random.default_rng(3)
    col = np.concatenate([np.zeros(750), rs.uniform(0.5, 1.5, 250)])      # (0.5 apart and not integers: not ordinal)
    x = np.stack([col, rs.standard_normal(1000)], axis=1)
    edges = bn.make_ale_edges(x, 0, n_bins=10)
    assert len(edges) == 4 and edges[0] == 0.0 and np.all(np.diff(edges) > 0)      # quantiles 0 .. 0.7 are all 0
    counts = np.bincount(ale_cases.bins_of(col, edges), minlength=3)
    assert counts[0] >= 750 and counts.sum() == 1000


# ---- get_ale / ale through the stand-in ----------------------------------------------------------------------------------------------
@pytest.fixture
def oracle_seam(monkeypatch):
    monkeypatch.setattr(ALE_MOD, "_ale_local_effects", ale_cases.oracle_seam)


def _one_focal(case):
    args = list(pdp_cases.call_args(bn, case))
    args[1] = [case["focal"][0]]
    return args


@pytest.mark.parametrize("name", ["continuous", "genrelu", "regression_onehot"])
def test_get_ale_shapes_and_summary(name, oracle_seam):
    c = FIXTURE[name]
    args = _one_focal(c)
    res = bn.get_ale(*args, n_bins=12, level=0.8)
    n_sets, n_out = len(c["weights"]), int(c["n_out"])
    edges = bn.make_ale_edges(c["x"], args[1], n_bins=12)
    k = len(edges) - 1
    assert np.array_equal(res["feature"], edges)
    assert res["counts"].shape == (k,) and res["counts"].sum() == c["x"].shape[0]
    assert res["ale"].shape == (k + 1, n_out, 3)
    assert res["ale_samples"].shape == (n_sets, k + 1, n_out) and res["local_effects"].shape == (n_sets, k, n_out)
    assert np.abs(res["ale_samples"] - ale_cases.curve(res["counts"], res["local_effects"])).max() < 1e-12
    assert np.abs(res["ale"][:, :, 0] - res["ale_samples"].mean(axis=0)).max() < 1e-12
    q = np.quantile(res["ale_samples"], (0.1, 0.9), axis=0)
    assert np.abs(res["ale"][:, :, 1] - q[0]).max() < 1e-12 and np.abs(res["ale"][:, :, 2] - q[1]).max() < 1e-12
    assert np.all(res["ale"][:, :, 1] <= res["ale"][:, :, 2])
    assert np.abs(res["local_effects"]).max() > 1e-3
    if c["mode"] == "classification":
        # probabilities, not cumulative ones: at every edge a sample's curves sum to the same value over the classes, as the
        # probabilities sum to 1 at both ends of every move
        assert np.abs(res["local_effects"].sum(axis=2)).max() < 1e-12
    assert np.array_equal(np.asarray(args[4]._prm, dtype=float), c["last_prm"])        # the last sample's slopes stay installed


def test_every_sample_runs_with_its_own_slopes(oracle_seam):
    c = FIXTURE["genrelu"]
    args = _one_focal(c)
    res = bn.get_ale(*args, n_bins=6)
    weights, alphas = args[6], args[7]
    assert len({tuple(np.asarray(a).ravel()) for a in alphas}) > 1
    for s in range(len(weights)):
        _, own = ale_cases.local_effects(c["x"], args[1][0], res["feature"], [weights[s]], fun="genReLU", slopes=[np.asarray(alphas[s], dtype=float)])
        assert np.abs(res["local_effects"][s] - own[0]).max() < 1e-12
    _, shared = ale_cases.local_effects(c["x"], args[1][0], res["feature"], weights, fun="genReLU",
                                        slopes=[np.asarray(alphas[0], dtype=float)] * len(weights))
    assert np.abs(res["local_effects"] - shared).max() > 1e-6


def test_switched_off_focal_column_is_flat_zero(oracle_seam):
    c = FIXTURE["indicators"]
    args = _one_focal(c)
    assert np.asarray(c["indicators"])[args[1][0]] == 0
    res = bn.get_ale(*args)
    assert np.all(res["ale"] == 0) and np.all(res["local_effects"] == 0) and res["counts"].sum() == c["x"].shape[0]


def test_get_ale_refuses_two_columns_and_bad_levels(oracle_seam):
    args = _one_focal(FIXTURE["continuous"])
    with pytest.raises(ValueError):
        bn.get_ale(args[0], [0, 1], *args[2:])
    with pytest.raises(ValueError):
        bn.get_ale(*args, level=1.0)


def test_ale_reads_checkpoint(oracle_seam, monkeypatch):
    """ale(pickle_file, columns): the model's training matrix, activation and output function, the logger's samples and the model's
    feature indicators go into get_ale, one result per column."""
    c = FIXTURE["indicators"]
    args = pdp_cases.call_args(bn, c)
    x, focal, mode, n_out, act, out_fn, weights, alphas, transform = args
    checkpoint = fake_checkpoint(args, c)
    monkeypatch.setattr(ALE_MOD, "load_obj", lambda path: checkpoint)
    on = int(np.flatnonzero(np.asarray(c["indicators"]) != 0)[0])
    res = bn.ale("checkpoint.pkl", [[focal[0]], on], n_bins=9)
    assert len(res) == 2
    assert np.all(res[0]["ale"] == 0)
    direct = bn.get_ale(x, on, mode, n_out, act, out_fn, weights, alphas, transform, n_bins=9)
    assert np.array_equal(res[1]["ale"], direct["ale"]) and np.abs(res[1]["ale"]).max() > 0
    assert len(res[1]["feature"]) <= 10


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_entry():
    txt = open(os.path.join(ROOT, "include", "npbnn_hip.h")).read()
    assert "#define NPBNN_ABI_VERSION 1" in txt and re.search(r"NPBNN_INFO_ALE_ROUTE\s*=\s*26\b", txt)
    res, args = capi.SIGNATURES["npbnn_predict_ale"]
    assert res is ctypes.c_int and len(args) == 12 and capi.INFO_ALE_ROUTE == 26
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "npbnn_predict_ale") and lib.npbnn_abi_version() == 1
    assert callable(bn.get_ale) and callable(bn.ale) and callable(bn.make_ale_edges) and hasattr(bn.HipContext, "predict_ale")


# ---- the guard of tests/test_hip_ale.py: its references can tell a wrong kernel from a right one -------------------------------------
MOVES = 1e-3      # 25 times the GPU test's bar


@pytest.mark.parametrize("name", list(ale_cases.CASES))
def test_case_references_are_finite_and_tell_sets_apart(name):
    case = ale_cases.CASES[name]
    inp = ale_cases.inputs(case)
    counts, effects = ale_cases.reference(case, inp)
    k = len(inp["edges"]) - 1
    assert counts.shape == (k,) and counts.sum() == inp["table"].shape[0]
    assert effects.shape == (case["sets"], k, case["n_out"]) and np.all(np.isfinite(effects))
    if case["pinned"]:
        assert np.all(effects == 0)
        return
    assert np.abs(effects).max() > MOVES
    for s in range(1, case["sets"]):
        assert np.abs(effects[s] - effects[s - 1]).max() > MOVES
    if inp["override"] is not None:
        assert np.abs(effects - ale_cases.reference(case, inp, override=False)[1]).max() > MOVES
    if not case["apply_out"] and case["out"] != "identity":
        assert np.abs(effects - ale_cases.reference(dict(case, apply_out=True), inp)[1]).max() > MOVES
    if case["which"] == 1:
        assert inp["x_test"].shape[0] != inp["x"].shape[0]


def test_case_table_covers_what_it_names():
    cases = list(ale_cases.CASES.values())
    inputs = {c["name"]: ale_cases.inputs(c) for c in cases}
    assert {c["rows"] for c in cases} >= {1, 255, 256, 257, 2111}
    assert {len(inputs[c["name"]]["edges"]) - 1 for c in cases} >= {1, 2, 7, 40}
    assert {(c["sets"], c["nodes"][0]) for c in cases if c["nodes"]} >= {(s, h) for s in (1, 2, 3, 7) for h in (20, 40)}
    assert {c["fun"] for c in cases} == {"ReLU", "genReLU", "swish", "tanh"}
    assert {(c["out"], c["apply_out"]) for c in cases} == {(o, a) for o in ("softmax", "identity", "softplus_half") for a in (True, False)}
    assert {(c["n_out"], c["route"]) for c in cases} >= {(1, 1), (7, 1), (32, 1), (33, 2)}
    assert {(c["nodes"][0], c["route"]) for c in cases if c["nodes"]} >= {(32, 1), (33, 1), (64, 1), (65, 2)}
    assert {(c["nodes"][1], c["route"]) for c in cases if len(c["nodes"]) > 1} >= {(32, 1), (33, 2)}
    assert {len(c["nodes"]) + 1 for c in cases} >= {1, 5} and {c["bias"] for c in cases} >= {"all", "none", "mixed01", "mixed10"}
    # rows exactly on the edges, values beyond both end edges, an empty bin
    inp = inputs["ordinal_rows_on_edges"]
    assert np.isin(inp["table"][:, inp["column"]], inp["edges"]).all()
    inp = inputs["test_table_beyond_the_edges"]
    col = inp["table"][:, inp["column"]]
    assert (col < inp["edges"][0]).sum() > 5 and (col > inp["edges"][-1]).sum() > 5
    counts, _ = ale_cases.reference(ale_cases.CASES["test_table_empty_bin"], inputs["test_table_empty_bin"])
    assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0
    assert max(c["rows"] for c in cases) <= 9000
