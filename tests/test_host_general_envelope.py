"""tests/general_cases.py without a GPU: the whole table rehearsed on the float64 stand-in.  Every size, list length and setting
the table has to contain is computed from the cases and their draws (dropping one from the table fails here); the planted
patterns are the stand-in's decisions; both walls reflect where a case says so; and a chain that divided by a wrong sum - left to
right, or eight accumulators without numpy's halving - would not return the stand-in's weights."""
import numpy as np
import pytest

import general_cases as gc
import range_cases as rc

NAMES = list(gc.CASES)
TREES = [n for n in NAMES if gc.CASES[n]["kind"] == gc.PROP_NORMAL_NORMALIZED]


@pytest.mark.parametrize("name", NAMES)
def test_planted_pattern_is_the_standins(name):
    sc = gc.scenario(name)
    assert 1 <= len(sc["batches"]) <= 2
    for b in sc["batches"]:
        K = b["K"]
        assert 12 <= K <= 30
        assert np.array_equal(b["want"]["acc"].astype(bool), b["pattern"]), (name, "the stand-in left the planted pattern")
        assert 3 * b["pattern"].sum() >= K and 3 * (~b["pattern"]).sum() >= K
        # every decision is MARGIN_FACTOR bars away from its threshold
        assert np.all(np.abs(b["log_u"] - b["stat"]) >= 0.999 * gc.MARGIN_FACTOR * gc.LL_BAR)
        assert np.all(np.isfinite(b["want"]["llp"])) and np.all(np.isfinite(b["want"]["lpp"])) and np.all(np.isfinite(b["log_u"]))
    # a second batch starts where the first ended
    if len(sc["batches"]) == 2:
        assert rc.pack(sc["batches"][1]["start"]["w"]).tobytes() == sc["batches"][0]["want"]["w"].tobytes()


def _tree_sizes():
    """size of a summed layer -> the cases that sum a layer of that size."""
    out = {}
    for n in TREES:
        for s in gc.summed_sizes(gc.scenario(n)):
            out.setdefault(s, []).append(n)
    return out


def test_tree_sizes_are_in_the_table():
    sizes = _tree_sizes()
    have = set(sizes)
    assert 1 in have and len([s for s in have if s < 8]) >= 3, sorted(have)
    for s in (8, 9, 15, 16, 17, 128, 129, 136, 256, 264):
        assert s in have, (s, sorted(have))
    assert 137 in have or 130 in have
    assert any(120 <= s <= 127 for s in have)
    assert any(257 <= s <= 263 for s in have)
    assert any(1025 <= s <= 2048 and s % 8 for s in have)
    assert any(s >= 4104 for s in have)
    assert max(have) <= 5000
    # the name of a tree case lists its layers' sizes
    for n in TREES:
        named = [int(x) for x in n.split("_") if x.isdigit()]
        if named:
            assert named == gc.layer_sizes(gc.CASES[n]), n
    every, none, masked = False, False, False
    for n in TREES:
        sc = gc.scenario(n)
        L = len(sc["p"]["shapes"])
        for b in sc["batches"]:
            lm, cnt = b["draws"]["layer_mask"], b["draws"]["cnt"]
            every |= bool(np.any(lm == (1 << L) - 1))
            none |= bool(np.any((lm == 0) & (cnt == 0)))
        if sc["p"]["mask"] is not None:
            zeros = sc["p"]["mask"][0] == 0
            masked |= bool(zeros.any()) and any((m & 1) for b in sc["batches"] for m in b["draws"]["layer_mask"])
        assert sc["case"]["w_bound"] == np.inf
        assert all(np.all(w >= 0) for w in sc["p"]["w"])
    assert every and none and masked


@pytest.mark.parametrize("name", TREES)
def test_numpy_sum_restated(name):
    """The plain restatement of numpy's pairwise tree equals np.sum on every layer of the case's start and accepted weights, 1-D
    and 2-D."""
    sc = gc.scenario(name)
    for b in sc["batches"]:
        for w in rc.unpack(b["want"]["w"], sc["p"]["shapes"]) + list(b["start"]["w"]):
            assert gc.numpy_tree_sum(w) == np.sum(w) == np.sum(w.ravel()), (name, w.shape)


def _weights_with(sc, layer_sum):
    be = gc.standin(sc["p"], layer_sum)
    return [rc.run_standin_general(sc["p"], b, be)["w"].tobytes() for b in sc["batches"]]


@pytest.mark.parametrize("name", TREES)
def test_a_wrong_sum_cannot_pass(name):
    """Dividing by a left-to-right sum changes the accepted weights' bytes in every case that sums a layer of 16 elements or
    more; dividing by an eight-accumulator sum without the halving does in every case that sums a layer of more than 128 (up to
    128 elements that sum IS numpy's).  The right restatement reproduces the stand-in's bytes."""
    sc = gc.scenario(name)
    want = [b["want"]["w"].tobytes() for b in sc["batches"]]
    assert _weights_with(sc, gc.numpy_tree_sum) == want
    largest = max(gc.summed_sizes(sc))
    if largest >= 16:
        assert _weights_with(sc, gc.sum_left_to_right) != want, (name, "left to right")
    if largest > 128:
        assert _weights_with(sc, gc.sum_eight_accumulators) != want, (name, "eight accumulators, no halving")
    assert any(b["want"]["acc"].any() for b in sc["batches"])


def test_entry_lists_are_in_the_table():
    C = gc.CASES
    ms = sorted(c["M"] for c in C.values())
    assert 1025 in ms and any(2400 <= m <= 2600 for m in ms)
    long_rows = padded = empty = full = False
    for n in NAMES:
        if C[n]["M"] <= 1024:
            continue
        sc = gc.scenario(n)
        assert sum(gc.layer_sizes(C[n])) >= C[n]["M"]
        for b in sc["batches"]:
            g = b["draws"]
            long_rows |= bool(np.any(g["cnt"] > 1024))
            empty |= bool(np.any(g["cnt"] == 0))
            full |= bool(np.any(g["cnt"] == C[n]["M"]))
            for t in range(b["K"]):
                assert np.all(g["idx"][t, :g["cnt"][t]] >= 0) and np.all(g["idx"][t, g["cnt"][t]:] == -1)
                padded |= g["cnt"][t] < C[n]["M"]
    assert long_rows and padded and empty and full
    # the fixed-normal Hastings list: longer than the proposal's (positions drawn more than once), and longer than the block
    dup = long_h = False
    for n in NAMES:
        if C[n]["kind"] != gc.PROP_FIXED_NORMAL:
            continue
        for b in gc.scenario(n)["batches"]:
            g = b["draws"]
            dup |= bool(np.any(g["h_cnt"] > g["cnt"]))
            long_h |= bool(np.any(g["h_cnt"] > 1024))
            for t in range(b["K"]):          # the last draw of a position is the one in idx
                pos, v = g["h_idx"][t, :g["h_cnt"][t]], g["h_val"][t, :g["h_cnt"][t]]
                last = {int(q): x for q, x in zip(pos, v)}
                assert sorted(last) == sorted(int(q) for q in g["idx"][t, :g["cnt"][t]])
                assert all(last[int(q)] == x for q, x in zip(g["idx"][t, :g["cnt"][t]], g["val"][t, :g["cnt"][t]]))
    assert dup and long_h
    # flips of weight indicators and of feature indicators: 0, 1 and more than 1024 positions in one batch
    for key, cases_ in (("ind_ptr", [n for n in NAMES if C[n]["wind"]]), ("find_ptr", [n for n in NAMES if C[n]["find"]])):
        ok = False
        for n in cases_:
            for b in gc.scenario(n)["batches"]:
                lens = set(np.diff(b["draws"][key]).tolist())
                ok |= {0, 1} <= lens and max(lens) > 1024
        assert ok, key


def test_walls_reflect_in_every_batch():
    walled = [n for n in NAMES if np.isfinite(gc.CASES[n]["w_bound"])]
    kinds = set()
    for n in walled:
        sc = gc.scenario(n)
        wb = sc["case"]["w_bound"]
        assert all(np.all(np.abs(w) <= wb) for w in sc["p"]["w"]), (n, "a start weight lies outside the walls")
        for b in sc["batches"]:
            assert b["reflected"][0] > 0 and b["reflected"][1] > 0, (n, b["reflected"])
            assert np.all(np.abs(b["want"]["w"]) <= wb)
        kinds.add(sc["case"]["kind"])
    assert kinds == {gc.PROP_NORMAL, gc.PROP_FIXED_NORMAL}
    assert {"walls_normal", "walls_fixed"} <= set(walled)


def test_priors_tempering_and_likelihoods_are_in_the_table():
    C = list(gc.CASES.values())
    assert {c["prior"] for c in C} == {0, 1, 2, 3}
    assert {"layers", "per_weight"} <= {c["scales"] for c in C if isinstance(c["scales"], str)}
    assert {(c["temperature"], c["lik_temp"]) for c in C} >= {(0.7, 1.0), (1.0, 0.6), (0.7, 0.6), (1.0, 1.0)}
    assert any(c["wind"] and c["prior_ind1"] != 0.5 for c in C)
    assert any(c["class_w"] for c in C) and any(c["inst_w"] and not c["class_w"] for c in C)
    assert {c["sigma"] for c in C if c["lik"] == "gauss"} == {"empirical", "given", "mult"}
    for lik in ("err", "pois", "nb"):      # later layers <= 16: the MTI = 1 generic build; 40 nodes: MTI = 8
        assert {max(c["widths"][1:]) <= 16 for c in C if c["lik"] == lik} == {True, False}, lik
    sc = gc.scenario("cat_class_weights")
    assert len(sc["p"]["bnn"]._class_w) == 3 and np.ptp(sc["p"]["bnn"]._class_w) > 0.05
    assert gc.scenario("prior_normal_per_weight")["p"]["prior_scale"][0].shape == gc.scenario("prior_normal_per_weight")["p"]["shapes"][0]


def test_feature_indicator_cases_are_in_the_table():
    finds = [n for n in NAMES if gc.CASES[n]["find"]]
    C = gc.CASES
    assert {1, 15, 17, 40} <= {C[n]["F"] for n in finds}
    assert {C[n]["bias"] >= 1 for n in finds} == {True, False}
    assert {C[n]["F"] % 16 != 0 for n in finds} >= {True}
    assert any(C[n]["wind"] and len(C[n]["widths"]) == 3 for n in finds)
    assert any(C[n]["path"] == "streamed" and C[n]["bias"] < 1 for n in finds) and any(C[n]["path"] == "streamed" and C[n]["bias"] >= 1 for n in finds)
    assert any(C[n]["l0"] == "f32" for n in finds)
    for n in finds:
        sc = gc.scenario(n)
        b = sc["batches"][0]
        g = b["draws"]
        use = g["find_use"]
        assert use[0] == 0 and use[-1] == 1 and np.all(np.diff(use) >= 0), (n, "find_use switches from 0 to 1 inside the batch")
        # while find_use is 0 the chain holds feature indicators that are 0: the override must not apply to them
        assert any(use[t] == 0 and not b["find_seen"][t].all() for t in range(b["K"])), n
        every = none = False
        for t in range(b["K"]):
            prop = b["find_seen"][t].copy()
            fl = g["find_pos"][g["find_ptr"][t]:g["find_ptr"][t + 1]]
            prop[fl] = np.abs(prop[fl] - 1)
            every |= bool(use[t]) and not prop.any()
            none |= bool(use[t]) and bool(prop.all())
        assert every and none, (n, every, none)
        # the chain's feature indicators move
        assert any(not np.array_equal(bb["want"]["find"], bb["start"]["find"]) for bb in sc["batches"]), n


def test_shapes_and_paths_are_in_the_table():
    C = gc.CASES
    assert {c["rows"] for c in C.values()} >= {1, 15, 17, "wg-1", "wg+1"}
    assert any(len(c["widths"]) == 7 for c in C.values())
    assert any(sum(gc.layer_sizes(c)) < 64 for c in C.values())
    assert any(sum(gc.layer_sizes(c)) % 1024 and sum(gc.layer_sizes(c)) > 1024 for c in C.values())
    assert {c["bias"] for c in C.values()} == {0, 1, 2, 3, -1}
    assert {c["act"] for c in C.values()} == {"ReLU", "swish", "tanh", "genReLU"}
    assert all(c["slopes"] is not None and all(s != 0 for s in c["slopes"]) for c in C.values() if c["act"] == "genReLU")
    streamed = [c for c in C.values() if c["path"] == "streamed"]
    assert {c["kind"] for c in streamed} == {gc.PROP_NORMAL, gc.PROP_FIXED_NORMAL, gc.PROP_NORMAL_NORMALIZED}
    assert any(c["wind"] for c in streamed) and any(c["find"] for c in streamed)
    assert any(c["mask_blocks"] for c in C.values())
