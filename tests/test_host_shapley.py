"""Shapley attributions on the host (no GPU): the float64 restatement of tests/shapley_cases.py against the properties of the
definition - efficiency, exactness under all permutations, the closed form of a linear network, exact zeros on overridden players -
get_shapley / shapley's bookkeeping with the device seam replaced by the restatement, the ABI entry, and the guards of
tests/test_hip_shapley.py's case table."""
import ctypes
import importlib
import itertools
import os
import re

import numpy as np
import pytest

import npbnn_amd as bn
import pdp_cases
import shapley_cases as sh
from attrib_common import fake_checkpoint
from npbnn_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = pdp_cases.load()
SHAP_MOD = importlib.import_module("npbnn_amd.shapley")
ACTS = {"relu": dict(fun="ReLU"), "leaky": dict(fun="ReLU", trainable=True), "genrelu": dict(fun="genReLU", slopes=[[0.1, 0.3], [0.45, 0.02]]),
        "swish": dict(fun="swish"), "tanh": dict(fun="tanh")}


def _small(seed=3, rows=12, n_bg=3, features=6, nodes=(5, 4), n_out=4, sets=2, bias=1):
    rs = np.random.default_rng(seed)
    xe, xb = rs.standard_normal((rows, features)), rs.standard_normal((n_bg, features))
    dims = [features] + list(nodes) + [n_out]
    weights = [[rs.normal(0, 1.0 / np.sqrt(dims[i] + 1), (dims[i + 1], dims[i] + bias)) for i in range(len(dims) - 1)] for _ in range(sets)]
    return xe, xb, weights, rs


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("apply_out", [True, False], ids=["applied", "raw"])
@pytest.mark.parametrize("out", ["softmax", "identity", "softplus_half"])
@pytest.mark.parametrize("act", list(ACTS))
def test_efficiency(act, out, apply_out):
    """the sum over the players telescopes to f(x_e) - mean_b f(b), whatever the permutations: rounding of a few sums of order 1"""
    xe, xb, weights, rs = _small()
    players = [[0, 3], [1], [2, 4, 5]]
    perms = np.array([rs.permutation(3) for _ in range(5)])
    res = sh.outputs(*sh.walks(xe, xb, weights, perms, players, out=out, apply_out=apply_out, **ACTS[act]))
    assert res["phi"].shape == (2, 12, 3, 4) and np.abs(res["phi"]).max() > 0.01
    assert np.abs(sh.efficiency_gap(res)).max() < 1e-12
    assert np.abs(sh.efficiency_gap(dict(res, phi=None))).max() < 1e-12


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_all_permutations_give_the_exact_value(act):
    xe, xb, weights, _ = _small(features=7)
    players = [[0, 6], [1, 2], [3], [4, 5]]
    perms = np.array(list(itertools.permutations(range(4))))
    assert perms.shape == (24, 4)
    got = sh.walks(xe, xb, weights, perms, players, **ACTS[act])[0]
    want = sh.exact(xe, xb, weights, players, **ACTS[act])[0]
    assert np.abs(want).max() > 0.01 and np.abs(got - want).max() < 1e-12
    # (four sampled permutations are an estimate, not the value)
    few = sh.walks(xe, xb, weights, perms[[1, 8, 14, 21]], players, **ACTS[act])[0]
    assert np.abs(few - want).max() > 1e-4


@pytest.mark.parametrize("bias", [0, 1])
def test_closed_form_of_a_linear_network(bias):
    xe, xb, weights, rs = _small(nodes=(), n_out=3, sets=3, bias=bias)
    players = [[0], [1, 4], [2], [3, 5]]
    for perms in (np.array([[0, 1, 2, 3]]), np.array([rs.permutation(4) for _ in range(3)])):
        phi = sh.walks(xe, xb, weights, perms, players, out="identity")[0]
        for s, w in enumerate(weights):
            m = w[0][:, bias:]
            want = np.stack([(xe[:, cols] - xb[:, cols].mean(axis=0)) @ m[:, cols].T for cols in players], axis=1)
            assert np.abs(phi[s] - want).max() < 1e-13


def test_a_player_of_overridden_columns_is_exactly_zero():
    xe, xb, weights, rs = _small()
    co = np.full(6, np.nan)
    co[1], co[4] = 0.7, -1.2
    players = [[1, 4], [0], [2, 3], [5]]
    perms = np.array([rs.permutation(4) for _ in range(4)])
    res = sh.outputs(*sh.walks(xe, xb, weights, perms, players, override=co))
    plain = sh.outputs(*sh.walks(xe, xb, weights, perms, players))
    assert np.all(res["phi"][:, :, 0] == 0) and np.abs(plain["phi"][:, :, 0]).max() > 0.01
    assert np.all(res["mean"][:, 0] == 0) and np.all(res["sq"][:, 0] == 0) and np.all(res["abs"][:, 0] == 0)
    assert np.abs(res["phi"][:, :, 1:] - plain["phi"][:, :, 1:]).max() > 1e-4      # (the other players see the constants)
    assert np.abs(sh.efficiency_gap(res)).max() < 1e-12


# ---- get_shapley / shapley through the stand-in ----------------------------------------------------------------------------------------
@pytest.fixture
def oracle_seam(monkeypatch):
    monkeypatch.setattr(SHAP_MOD, "_shapley_device", sh.oracle_seam)


def _args(case):
    a = pdp_cases.call_args(bn, case)
    return (a[0], a[3]) + tuple(a[4:])


@pytest.mark.parametrize("name", ["continuous", "genrelu", "regression_onehot"])
def test_get_shapley_shapes_and_summary(name, oracle_seam):
    c = FIXTURE[name]
    args = _args(c)
    rows = np.arange(0, c["x"].shape[0], 3)[:9]
    res = bn.get_shapley(*args, rows=rows, background=5, n_perm=4, level=0.8, return_samples=True)
    n_sets, n_out, f, e = len(c["weights"]), int(c["n_out"]), c["x"].shape[1], len(rows)
    assert set(res) == {"attributions", "prediction", "base_value", "importance", "ranking", "players", "permutations", "background_rows",
                        "samples"}
    smp = res["samples"]
    assert smp["attributions"].shape == (n_sets, e, f, n_out) and res["attributions"].shape == (e, f, n_out, 3)
    assert res["prediction"].shape == (e, n_out) and res["base_value"].shape == (n_out,) and res["importance"].shape == (f, n_out, 3)
    assert res["permutations"].shape == (4, f) and len(res["background_rows"]) == 5 and res["players"] == [[j] for j in range(f)]
    assert np.abs(res["attributions"][..., 0] - smp["attributions"].mean(axis=0)).max() < 1e-12
    q = np.quantile(smp["attributions"], (0.1, 0.9), axis=0)
    assert np.abs(res["attributions"][..., 1] - q[0]).max() < 1e-12 and np.abs(res["attributions"][..., 2] - q[1]).max() < 1e-12
    assert np.abs(res["importance"][..., 0] - np.abs(smp["attributions"]).mean(axis=(0, 1))).max() < 1e-12
    qi = np.quantile(smp["importance"], (0.1, 0.9), axis=0)
    assert np.abs(res["importance"][..., 1] - qi[0]).max() < 1e-12 and np.abs(res["importance"][..., 2] - qi[1]).max() < 1e-12
    # additivity, per sample and of the posterior means
    assert np.abs(smp["attributions"].sum(axis=2) - (smp["prediction"] - smp["base_value"][:, None, :])).max() < 1e-12
    assert np.abs(res["attributions"][..., 0].sum(axis=1) - (res["prediction"] - res["base_value"])).max() < 1e-12
    assert np.abs(smp["attributions"]).max() > 1e-3
    assert sorted(res["ranking"].tolist()) == list(range(f))
    assert np.all(np.diff(res["importance"][:, :, 0].sum(axis=1)[res["ranking"]]) <= 0)
    assert np.array_equal(np.asarray(args[2]._prm, dtype=float), c["last_prm"])        # the last sample's slopes stay installed
    # without the samples: the same means, the band from the mean of phi^2
    plain = bn.get_shapley(*_args(c), rows=rows, background=5, n_perm=4, level=0.8)
    assert "samples" not in plain and np.abs(plain["attributions"][..., 0] - res["attributions"][..., 0]).max() < 1e-12
    sd = smp["attributions"].std(axis=0)
    z = 1.2815515655446004
    assert np.abs(plain["attributions"][..., 1] - (res["attributions"][..., 0] - z * sd)).max() < 1e-9
    assert np.abs(plain["attributions"][..., 2] - (res["attributions"][..., 0] + z * sd)).max() < 1e-9


def test_ranking_on_a_known_order(oracle_seam):
    """One matrix, identity output: phi of feature j is w_cj (x_ej - mean_b b_j), so columns of known size give the order and
    equal ones fall back on the index."""
    rs = np.random.default_rng(5)
    x = np.abs(rs.standard_normal((30, 5))) + 1.0
    x[:3] = 0.0                                     # the background rows
    size = np.array([0.5, 3.0, 0.5, 2.0, 1.0])
    weights = [[np.concatenate([np.zeros((2, 1)), np.ones((2, 5)) * size * (1 + 0.1 * s)], axis=1)] for s in range(4)]
    x[3:] = 1.0 + np.arange(27)[:, None] / 27.0     # (every column the same: the importance is the weight's size times the mean row)
    res = bn.get_shapley(x, 2, bn.ActFun(fun="tanh"), bn.RegressTransform, weights, [np.zeros(0)] * 4, None, rows=np.arange(3, 30),
                         background=np.arange(3), n_perm=2)
    assert res["ranking"].tolist() == [1, 3, 4, 0, 2]
    assert np.array_equal(res["background_rows"], np.arange(3))


def test_antithetic_pairs_and_seed(oracle_seam):
    c = FIXTURE["continuous"]
    kw = dict(rows=[0, 4], background=3, n_perm=6)
    a = bn.get_shapley(*_args(c), **kw)
    perms = a["permutations"]
    assert perms.shape[0] == 6 and all(sorted(p.tolist()) == list(range(perms.shape[1])) for p in perms)
    for k in range(3):
        assert np.array_equal(perms[2 * k + 1], perms[2 * k][::-1])
    assert not np.array_equal(perms[0], perms[2])
    b = bn.get_shapley(*_args(c), **kw)
    assert np.array_equal(a["attributions"], b["attributions"]) and np.array_equal(a["background_rows"], b["background_rows"])
    d = bn.get_shapley(*_args(c), seed=99, **kw)
    assert not np.array_equal(a["permutations"], d["permutations"]) and not np.array_equal(a["attributions"], d["attributions"])
    free = bn.get_shapley(*_args(c), antithetic=False, rows=[0, 4], background=3, n_perm=5)
    assert free["permutations"].shape[0] == 5
    assert len(np.unique(a["background_rows"])) == 3 and a["background_rows"].max() < c["x"].shape[0]
    everything = bn.get_shapley(*_args(c), rows=[0], background=10 ** 6, n_perm=2)
    assert np.array_equal(everything["background_rows"], np.arange(c["x"].shape[0]))


def test_grouping(oracle_seam):
    c = FIXTURE["continuous"]
    f = c["x"].shape[1]
    res = bn.get_shapley(*_args(c), rows=[1, 2, 3], background=4, n_perm=4, feature_indx_list=[[2, 0], [f - 1]], return_samples=True)
    rest = [j for j in range(f) if j not in (0, 2, f - 1)]
    assert res["players"] == [[2, 0], [f - 1]] + [[j] for j in rest]
    p = len(res["players"])
    assert res["attributions"].shape[1] == p and res["permutations"].shape == (4, p)
    smp = res["samples"]
    assert np.abs(smp["attributions"].sum(axis=2) - (smp["prediction"] - smp["base_value"][:, None, :])).max() < 1e-12
    # a background drawn from another table
    other = c["x"][::2] + 0.5
    res2 = bn.get_shapley(*_args(c), rows=[1, 2, 3], background=4, background_data=other, n_perm=4, return_samples=True)
    assert res2["background_rows"].max() < other.shape[0]
    assert np.abs(res2["base_value"] - res["base_value"]).max() > 1e-6


def test_every_sample_runs_with_its_own_slopes(oracle_seam):
    c = FIXTURE["genrelu"]
    args = _args(c)
    res = bn.get_shapley(*args, rows=[0, 1, 2], background=[3, 4], n_perm=2, return_samples=True)
    weights, alphas = args[4], args[5]
    assert len({tuple(np.asarray(a).ravel()) for a in alphas}) > 1
    players = [[j] for j in range(c["x"].shape[1])]
    for s in range(len(weights)):
        own = sh.walks(c["x"][:3], c["x"][3:5], [weights[s]], res["permutations"], players, fun="genReLU",
                       slopes=[np.asarray(alphas[s], dtype=float)])[0]
        assert np.abs(res["samples"]["attributions"][s] - own[0]).max() < 1e-12


def test_get_shapley_refusals(oracle_seam):
    args = _args(FIXTURE["continuous"])
    kw = dict(rows=[0, 1], background=3, n_perm=2)
    with pytest.raises(ValueError):
        bn.get_shapley(*args[:4], [], [], args[6], **kw)
    for level in (0.0, 1.0):
        with pytest.raises(ValueError):
            bn.get_shapley(*args, level=level, **kw)
    with pytest.raises(ValueError):
        bn.get_shapley(args[0], args[1] + 1, *args[2:], **kw)
    with pytest.raises(ValueError):
        bn.get_shapley(args[0], args[1], args[2], lambda z: z * z, *args[4:], **kw)
    with pytest.raises(ValueError):
        bn.get_shapley(*args, rows=[0, 1], background=3, n_perm=3)
    assert bn.get_shapley(*args, rows=[0, 1], background=3, n_perm=3, antithetic=False)["permutations"].shape[0] == 3
    with pytest.raises(ValueError):
        bn.get_shapley(*args, feature_indx_list=[[0, 1], [1, 2]], **kw)
    with pytest.raises(ValueError):
        bn.get_shapley(*args, rows=[args[0].shape[0]], background=3, n_perm=2)
    with pytest.raises(ValueError):
        bn.get_shapley(*args, rows=[0], background=[args[0].shape[0]], n_perm=2)


def test_shapley_reads_checkpoint(oracle_seam, monkeypatch):
    """shapley(pickle_file): the model's matrices, activation and output function, the logger's samples and the model's feature
    indicators go into get_shapley; the test matrix is explained against the training matrix."""
    c = FIXTURE["indicators"]
    args = pdp_cases.call_args(bn, c)
    x, _, mode, n_out, act, out_fn, weights, alphas, transform = args
    x_test = x[::3] + 0.25
    checkpoint = fake_checkpoint(args, c, _test_data=x_test)
    monkeypatch.setattr(SHAP_MOD, "load_obj", lambda path: checkpoint)
    off = np.asarray(c["indicators"]) == 0
    assert off.any() and not off.all()
    kw = dict(rows=[0, 1, 2, 5], background=6, n_perm=4)
    res = bn.shapley("checkpoint.pkl", **kw)
    direct = bn.get_shapley(x_test, n_out, act, out_fn, weights, alphas, transform, background_data=x, **kw)
    assert np.array_equal(res["attributions"], direct["attributions"]) and np.array_equal(res["base_value"], direct["base_value"])
    assert np.all(res["attributions"][:, off] == 0) and np.abs(res["attributions"][:, ~off]).max() > 0
    on_train = bn.shapley("checkpoint.pkl", which="train", **kw)
    want = bn.get_shapley(x, n_out, act, out_fn, weights, alphas, transform, **kw)
    assert np.array_equal(on_train["attributions"], want["attributions"]) and not np.array_equal(on_train["attributions"], res["attributions"])
    with pytest.raises(ValueError):
        bn.shapley("checkpoint.pkl", which="validation")


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_entry():
    txt = open(os.path.join(ROOT, "include", "npbnn_hip.h")).read()
    assert "#define NPBNN_ABI_VERSION 1" in txt and re.search(r"NPBNN_INFO_SHAPLEY_ROUTE\s*=\s*29\b", txt)
    assert re.search(r"NPBNN_INFO_SHAPLEY_WALK_NS\s*=\s*30\b", txt)
    res, args = capi.SIGNATURES["npbnn_predict_shapley"]
    assert res is ctypes.c_int and len(args) == 22 and capi.INFO_SHAPLEY_ROUTE == 29 and capi.INFO_SHAPLEY_WALK_NS == 30
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "npbnn_predict_shapley") and lib.npbnn_abi_version() == 1
    assert callable(bn.get_shapley) and callable(bn.shapley) and hasattr(bn.HipContext, "predict_shapley")


# ---- the guards of tests/test_hip_shapley.py: its references can tell a wrong kernel from a right one --------------------------------
_shared = {}


def _case_data(name):
    if name not in _shared:
        case = sh.CASES[name]
        inp = sh.inputs(case)
        _shared[name] = (case, inp, sh.reference(case, inp))
    return _shared[name]


def _applies(wrong, case, inp):
    """inverse_perm: more than one player's step depends on the order - not for a linear network, and not where the permutations
    as a set are their own inverses; no_reset: a second walk; bias_column: a bias column on layer 0."""
    if wrong == "inverse_perm":
        linear = not case["nodes"] and (not case["apply_out"] or case["out"] == "identity")
        own = sorted(map(tuple, inp["perms"])) == sorted(tuple(np.argsort(p)) for p in inp["perms"])
        return not linear and not own
    if wrong == "no_reset":
        return len(inp["perms"]) * len(inp["xb"]) > 1
    return inp["weights"][0][0].shape[1] == case["features"] + 1


@pytest.mark.parametrize("name", list(sh.CASES))
def test_case_references_hold_the_definition_and_tell_wrong_kernels_apart(name):
    case, inp, want = _case_data(name)
    n_sets, e, p, c = case["sets"], case["n_explain"], len(inp["players"]), case["n_out"]
    shapes = dict(mean=(e, p, c), sq=(e, p, c), abs=(n_sets, p, c), fx=(n_sets, e, c), base=(n_sets, c), phi=(n_sets, e, p, c))
    for key in sh.NAMES:
        assert want[key].shape == shapes[key] and np.all(np.isfinite(want[key])), key
    assert np.abs(sh.efficiency_gap(want)).max() < 1e-12
    assert np.abs(want["phi"]).max() > 100 * sh.TOL
    for s in range(1, n_sets):
        assert np.abs(want["phi"][s] - want["phi"][s - 1]).max() > 100 * sh.TOL
    if inp["override"] is not None:
        off = [k for k, cols in enumerate(inp["players"]) if all(not np.isnan(inp["override"][j]) for j in cols)]
        assert off and np.all(want["phi"][:, :, off] == 0)
    applied = 0
    for wrong in ("inverse_perm", "no_reset", "bias_column"):
        if _applies(wrong, case, inp):
            got = sh.reference(case, inp, wrong=wrong)
            assert sh.relative_error(got["phi"], want["phi"]) > 100 * sh.TOL, wrong
            assert sh.relative_error(got["mean"], want["mean"]) > 100 * sh.TOL, wrong
            applied += 1
    assert applied >= (1 if name in ("players_1", "one_matrix_no_bias") else 2), applied
    if case["bg_table"] is not None:
        assert inp["bg_which"] != case["which"] and inp["x_test"].shape[0] != inp["x"].shape[0]


def test_exact_case_is_the_exact_value():
    case, inp, want = _case_data("exact_4_players")
    assert inp["perms"].shape == (24, 4) and case["features"] == 40
    ex = sh.reference_exact(case, inp)
    for key in sh.NAMES:
        assert np.abs(ex[key] - want[key]).max() < 1e-12, key


def test_case_table_covers_what_it_names():
    cases = list(sh.CASES.values())
    assert {c["n_explain"] for c in cases} >= {1, 63, 64, 65, 255, 256, 257, 300} and any(c["repeats"] for c in cases)
    assert {c["n_bg"] for c in cases} >= {1, 2, 3, 5} and {c["n_perm"] for c in cases} >= {1, 2, 4, 7}
    assert {c["n_groups"] for c in cases} >= {None, 1, 2, 4, 31, 32, 33} and {c["features"] for c in cases} >= {31, 32, 33, 40, 64, 65, 256, 700}
    assert {(c["sets"], c["nodes"][0]) for c in cases if c["nodes"]} >= {(s, h) for s in (1, 2, 3, 7) for h in (20, 40)}
    assert {(c["fun"], c["trainable"], c["slopes"]) for c in cases} >= {("ReLU", False, None), ("ReLU", True, None), ("genReLU", False, "shared"),
                                                                         ("genReLU", False, "per_set"), ("swish", False, None), ("tanh", False, None)}
    assert {(c["out"], c["apply_out"]) for c in cases} == {(o, a) for o in ("softmax", "identity", "softplus_half") for a in (True, False)}
    assert {(c["n_out"], c["route"]) for c in cases} >= {(32, 1), (33, 2)}
    assert {(c["nodes"][0], c["route"]) for c in cases if c["nodes"]} >= {(64, 1), (65, 2), (130, 2)}
    assert {(c["nodes"][1], c["route"]) for c in cases if len(c["nodes"]) > 1} >= {(32, 1), (33, 2)}
    assert {len(c["nodes"]) + 1 for c in cases} >= {1, 5} and {c["bias"] for c in cases} >= {"all", "none", "mixed01", "mixed10"}
    assert all(c["reroute"] == (c["route"] == 1) for c in cases) and sh.CASES["scratch_in_chunks"]["reroute"]
    grouped = sh.inputs(sh.CASES["override_grouped"])
    assert grouped["players"][0] == [5, 17] and len(grouped["players"]) > 3 and all(5 not in g and 17 not in g for g in grouped["players"][1:])
    assert all(n in sh.CASES and sh.CASES[n]["reroute"] for n in sh.FORCED_WIDE)
    uneven = sh.inputs(sh.CASES["players_31"])["players"]
    assert len(uneven) == 31 and len({len(g) for g in uneven}) > 1 and sorted(j for g in uneven for j in g) == list(range(40))
    assert 1e-6 <= sh.TOL <= 1e-4 and 1e-6 <= sh.TOL_EFFICIENCY <= 1e-4
