"""CPU guards of tests/importance_envelope_cases.py (no GPU): bit equality on the device says something only if a wrong gather would
give another matrix, and a case checks an edge only if its draw has that edge.

  * every wrong variant of the gather that can differ on a case's calls does differ from the right matrix in a shuffled entry, the ones
    that cannot are the right matrix, and every variant is told apart by many cases;
  * column lists lie inside the matrix, name no column twice and hold the boundary columns their case is about;
  * the conditions on the draws: largest entries kept, the planted entry dropped and above the scale's 1 once restored, moved and
    unmoved columns shuffled, labels covering the classes, one class winning every row, item counts past the grid cap;
  * case (b)'s reference by itself: a numpy float32 forward pass of the restored table within half of test_hip_posterior.TOL of the
    float64 oracle."""
import importlib

import numpy as np
import pytest

import importance_envelope_cases as iec
import scale_cases as sc
import split_model as sm
from test_hip_importance import _host_shuffle, _table
from test_hip_posterior import TOL

posterior = importlib.import_module("npbnn_amd.posterior")

VARIANTS = ("block_permutation", "next_column", "from_the_shuffled", "no_restore")


@pytest.mark.parametrize("name", list(iec.GATHER))
def test_wrong_gathers_are_other_matrices(name):
    inp = iec.gather_inputs(name)
    differing, same = iec.wrong_variants(inp), iec.not_applicable(inp)
    assert len(differing) + len(same) == 2 * len(inp["calls"]) + 2 * (len(inp["calls"]) - 1)
    for (variant, k), (wrong, right, touched) in same.items():
        np.testing.assert_array_equal(wrong, right, err_msg="%s, call %d" % (variant, k))
    if inp["degenerate"]:                                 # one row: the only index is 0, every gather is the identity
        assert inp["table"].shape[0] == 1
        for wrong, right, _ in differing.values():
            np.testing.assert_array_equal(wrong, right)
        return
    assert len(differing) >= 1                            # (one feature: no other column, no second permutation - the second call's source)
    assert inp["table"].shape[1] == 1 or any(v == "next_column" for v, _ in differing)
    for (variant, k), (wrong, right, touched) in differing.items():
        assert np.any(wrong[:, touched] != right[:, touched]), "%s, call %d: the same matrix" % (variant, k)
        others = [c for c in range(right.shape[1]) if c not in touched]
        np.testing.assert_array_equal(wrong[:, others], right[:, others])
    for k, right in enumerate(iec.right_matrices(inp)):   # the right matrix itself: shuffled columns moved, every other one in place
        cols = inp["calls"][k][0]
        others = [c for c in range(right.shape[1]) if c not in cols]
        np.testing.assert_array_equal(right[:, others], inp["table"][:, others])
        assert all(np.any(right[:, c] != inp["table"][:, c]) for c in cols)


def test_every_variant_is_told_apart_by_many_cases():
    count = dict.fromkeys(VARIANTS, 0)
    for name in iec.GATHER:
        inp = iec.gather_inputs(name)
        if not inp["degenerate"]:
            for variant in {v for v, _ in iec.wrong_variants(inp)}:
                count[variant] += 1
    print(count)
    assert min(count.values()) >= 20, count


@pytest.mark.parametrize("name", list(iec.GATHER))
def test_column_lists(name):
    inp = iec.gather_inputs(name)
    case, f = inp["case"], inp["table"].shape[1]
    assert 1 <= len(inp["calls"]) <= 2 and inp["table"].shape == ((inp["x_test"] if inp["which"] else inp["x"]).shape)
    assert inp["x"].shape[1] == f and set(case["paths"]) <= set(iec.PATHS)
    for cols, idx in inp["calls"]:
        assert len(cols) >= 1 and len(set(cols)) == len(cols) and all(0 <= c < f for c in cols)
        assert idx.shape in ((1, inp["table"].shape[0]), (len(cols), inp["table"].shape[0]))
        assert idx.min() >= 0 and idx.max() < inp["table"].shape[0]
        if case["kind"] not in ("largest_kept", "planted"):
            for p in idx:
                np.testing.assert_array_equal(np.sort(p), np.arange(len(p)))
    first = inp["calls"][0][0]
    if name.startswith("features_"):
        assert f == case["features"]
        want = {0, f - 1}
        if f >= 8:
            want.add(8 * (f // 8) - 1)                    # the last column of a full group
        if f % 8:
            want.add(f - f % 8)                           # the first column of the last, partial, group
        assert set(first) == want == set(iec.boundary_columns(f))
    if name == "two_columns_of_one_group":
        assert len(first) == 2 and first[0] // 8 == first[1] // 8
    if name in ("eight_columns_in_eight_groups", "rows_past_the_grid_cap_8_groups"):
        assert len(first) == 8 and sorted(c // 8 for c in first) == list(range(8))
    if name.startswith("all_columns"):
        assert sorted(first) == list(range(f))
    if name == "one_column_one_permutation":
        assert len(first) == 1 and inp["calls"][0][1].shape[0] == 1
    if name == "second_call_overlaps_the_first":
        second = inp["calls"][1][0]
        assert set(first) & set(second) and set(first) - set(second) and set(second) - set(first)
    if case["kind"] == "blocked":                         # two columns of one block of 16 features and one of another
        blocks = [c // 16 for c in first]
        assert len(first) == 3 and len(set(blocks)) == 2
        w0 = inp["sets"][0][0]
        assert w0.shape == (48, 161) and not np.any(w0[:, 1:][inp["mask"][0][:, 1:] == 0]) and np.all(w0[:, 0] != 0)
        assert 0.05 < inp["mask"][0][:, 1:].mean() < 0.2  # 10 blocks: a tenth of the first layer is wired
    if inp["which"] == 1:
        cols, idx = inp["train_call"]
        assert len(set(cols)) == len(cols) and max(cols) < f and idx.shape == (len(cols), inp["x"].shape[0])


def test_item_counts_pass_the_grid_cap():
    a, b = iec.gather_inputs("rows_past_the_grid_cap"), iec.gather_inputs("rows_past_the_grid_cap_8_groups")
    for inp in (a, b):
        n = inp["table"].shape[0]
        cols, idx = inp["calls"][0]
        assert idx.size > iec.FI_GRID_CAP                 # perm_check
        assert n * len(cols) > iec.FI_GRID_CAP            # perm_save and perm_gather; perm_restore in the second call
    groups = {c // 8 for c in b["calls"][0][0]}
    assert b["table"].shape[0] * len(groups) > iec.FI_GRID_CAP                 # perm_patch_split: rows x groups
    assert a["table"].shape[0] * 1 <= iec.FI_GRID_CAP
    for name in ("rows_past_the_grid_cap_3_classes", "rows_past_the_grid_cap_4_classes"):
        case = iec.SUMMARY[name]
        per_set = case["rows"] * case["n_out"]
        assert case["rows"] > iec.FI_GRID_CAP
        if case["n_out"] == 3:
            assert per_set % 4 != 0                       # the scalar kernels
        else:
            assert per_set % 4 == 0 and per_set // 4 > iec.FI_GRID_CAP         # the vector kernels' n4


def test_heavy_tails_shuffle_moved_and_unmoved_columns():
    inp = iec.gather_inputs("heavy_tails")
    x = inp["table"]
    assert x is sc.train_table("lognormal3")
    shift = sm.ensure_scales(x)[2]
    assert 0 < (shift > 0).sum() < x.shape[1]
    for cols, _ in inp["calls"]:
        assert any(shift[c] > 0 for c in cols) and any(shift[c] == 0 for c in cols)
    # the table stays on the pair under its own scales and so do the weights: the default path reports f16-split
    xs, ws = sm.ensure_scales(x)[:2]
    assert sm.table_state(x, xs, True)[0] == sm.USABLE
    assert all(np.abs(w[0][:, 1:] * ws).max() <= sm.F16_SAFE for w in inp["sets"])
    # a shuffle leaves what the scales are taken from alone: the same shifts for every matrix a fresh context is given
    for m in iec.right_matrices(inp):
        np.testing.assert_array_equal(sm.ensure_scales(m)[2], shift)
    # layer 0 normalised as scale_cases.weight_sets does it: its sums are of order 1
    z0 = x.astype(np.float64) @ inp["sets"][0][0][:, 1:].T
    assert 0.3 < np.median(np.abs(z0)) < 30


@pytest.mark.parametrize("name,pair,l0", [("test_table_under_moved_scales", "moved_train_normal", "f32"),
                                          ("lognormal_test_table_under_moved_scales", "moved_train_lognormal", "f16-split")])
def test_moved_training_scales_cases_are_scale_cases(name, pair, l0):
    inp = iec.gather_inputs(name)
    assert inp["x"] is sc.tables(pair)[0] and inp["table"] is sc.tables(pair)[1] and inp["l0"] == l0
    for m in iec.right_matrices(inp):                     # (a shuffle does not change what ensure_x16 decides for the table)
        assert sm.states(inp["x"], m)[1] == sm.states(inp["x"], inp["table"])[1]
    xs, ws, shift, _ = sm.ensure_scales(inp["x"])
    assert (shift > 0).any()
    # the training table's own launches stay on the pair: the table is usable and the normalised weights fit fp16 under its scales
    assert sm.table_state(inp["x"], xs, True)[0] == sm.USABLE
    assert all(np.abs(w[0][:, 1:] * ws).max() <= sm.F16_SAFE for w in inp["sets"])


def test_largest_entries_are_kept():
    inp = iec.gather_inputs("with_replacement_largest_kept")
    x = inp["table"]
    for (cols, idx), m in zip(inp["calls"], iec.right_matrices(inp)):
        assert any(len(np.unique(p)) < len(p) for p in idx)                    # drawn with replacement: no permutation
        for c in cols:
            assert np.abs(m[:, c]).max() == np.abs(x[:, c]).max()
        np.testing.assert_array_equal(sm.ensure_scales(m.astype(np.float32))[0], sm.ensure_scales(x.astype(np.float32))[0])
        assert not sm.ensure_scales(m.astype(np.float32))[2].any()


def test_planted_entry_is_dropped_and_lies_above_the_scale():
    inp = iec.gather_inputs("with_replacement_planted_entry_dropped")
    x = inp["table"]
    (cols, idx), = inp["calls"]
    assert x[iec.PLANTED_ROW, iec.PLANTED_COL] == iec.PLANTED_VALUE and iec.PLANTED_COL in cols
    assert iec.PLANTED_ROW not in idx and len(np.unique(idx)) < idx.size
    shuffled = _host_shuffle(x, cols, idx)
    assert np.abs(shuffled).max() < 10 and np.count_nonzero(x == iec.PLANTED_VALUE) == 1
    # the scales a first launch after the shuffle takes do not know the entry: restored, it is 2^4 or more above the column's 1
    scale = sm.ensure_scales(shuffled.astype(np.float32))[0]
    assert iec.PLANTED_VALUE * scale[iec.PLANTED_COL] >= 16
    assert scale[iec.PLANTED_COL] > sm.ensure_scales(x.astype(np.float32))[0][iec.PLANTED_COL]
    # ... and inside the rules a table has to keep to stay on the pair (it is not asked again after a restore)
    assert iec.PLANTED_VALUE * scale[iec.PLANTED_COL] <= sm.F16_SAFE
    assert sm.weight_floor_sum(x.astype(np.float32), scale) <= sm.FLOOR_S


def test_float32_model_of_the_restored_table_is_inside_half_the_bound():
    inp = iec.gather_inputs("with_replacement_planted_entry_dropped")
    want = iec.oracle_sets(inp["table"], inp["sets"])
    got = iec.float32_model_sets(inp["table"], inp["sets"])
    err = max(float(np.abs(g - w).max()) for g, w in zip(got, want))
    print("float32 model against float64 on the restored table: %.3e (half the bound: %.1e)" % (err, TOL / 2))
    assert err <= TOL / 2
    # the planted entry matters: without it the predictions of its row are other ones by far more than the bound
    without = np.array(inp["table"])
    without[iec.PLANTED_ROW, iec.PLANTED_COL] = 0.0
    other = iec.oracle_sets(without, inp["sets"])
    assert max(float(np.abs(a[iec.PLANTED_ROW] - b[iec.PLANTED_ROW]).max()) for a, b in zip(other, want)) > 100 * TOL


@pytest.mark.parametrize("name", list(iec.SUMMARY))
def test_summary_draws(name):
    inp = iec.summary_inputs(name)
    case, labels = inp["case"], inp["labels"]
    c, n = case["n_out"], inp["table"].shape[0]
    assert labels.shape == (n,) and labels.min() >= 0 and labels.max() < c
    assert inp["sets"][0][-1].shape[0] == c and len(inp["sets"]) == case["sets"]
    if case["kind"] == "one_cell":
        label = c - iec.ONE_CELL_LABEL_FROM_END
        assert np.all(labels == label) and label != iec.ONE_CELL_WINNER
        stack = np.array(iec.oracle_sets(inp["table"], inp["sets"]))
        assert np.all(np.argmax(stack, axis=2) == iec.ONE_CELL_WINNER) and stack[:, :, iec.ONE_CELL_WINNER].min() > 0.99
        for mode in (0, 1):
            table = _table(posterior._summarise(stack, mode), labels)
            assert table[label, iec.ONE_CELL_WINNER] == n and np.count_nonzero(table) == 1
    else:
        assert set(labels) == set(range(c)) if n >= c else len(set(labels)) == n
    assert (c > iec.CONF_LDS_CLASSES) == (name in ("classes_65", "classes_100", "one_cell_65_classes"))
    if name == "test_table":
        assert inp["which"] == 1 and n == 173 and inp["x"].shape[0] == 1000


def test_case_counts():
    print("GATHER: %d cases, %d (case, path) runs; SUMMARY: %d cases" % (
        len(iec.GATHER), sum(len(c["paths"]) for c in iec.GATHER.values()), len(iec.SUMMARY)))
    assert sum(c["eval"] for c in iec.GATHER.values()) == 1 and all(
        c["paths"] == iec.PATHS for c in iec.GATHER.values() if c["eval"])     # eval with a confusion table: one case, every path
    assert sum(c["before"] for c in iec.GATHER.values()) >= 6
