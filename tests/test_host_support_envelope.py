"""The guards of tests/test_hip_support_envelope.py, on the CPU: a numpy model of support_final_kernel (npbnn_amd/csrc/npbnn_support.hip)
AS LAID OUT - one dynamic LDS block per workgroup, [thresholds | bf thresholds | cube cells | bf cells] at the kernel's offsets, filled
with a pattern before the kernel zeroes what it counts in; the three LDS-or-global switches; the grid of grid_for with the cap of three
workgroups per compute unit and the stride over the rows; the bisection, reading whichever copy of the thresholds the switches choose;
32-bit LDS counters flushed into 64-bit global ones workgroup by workgroup - and the same model with one deliberate mistake.

The right model gives the restatement of support_envelope_cases byte for byte on every case and mode.  For every mistake ``applies`` says
from first principles whether it can show on a case (True), cannot (False: the wrong model then IS the right one, which is asserted
too, so nothing is left out by choice) or may (None: rounding decides; nothing asserted); and CAUGHT_BY names cases on which each mistake
must show.  So a device kernel with one of these mistakes cannot pass test_hip_support_envelope.py, and an edit of the table cannot
silently lose the case that catches it.  The values summarised are the float64 oracle's predictions rounded to float32.

The mistakes:
  search_le           ``t <= p`` in the bisection: a row whose p is a threshold, or whose factor is a Bayes-factor threshold;
  last_of_ties        the last of tied classes is the call: a row with two classes at its largest value;
  label_call_swapped  cell (b * C + call) * C + label: a bin whose table is not symmetric;
  first_stride_only   rows past the first pass of the grid are dropped: more rows than grid x 256;
  last_flush_dropped  the last workgroup does not flush its LDS counters: anything counted in LDS;
  bf_offset_0         the Bayes-factor thresholds are read from offset 0 of the threshold buffer: a prior, thresholds of both kinds;
  bf_formula          the factor as p * (1e-10 + 1 - r) / (r * (1e-10 + 1 - p)): a row whose factor IS a threshold, rounding decides;
  train_labels        the training slot's labels are read on the test table;
  train_row_count     the training slot's row count is used on the test table: 300 of the 513 rows are counted;
  keep_ge             ``p >= cutoff`` keeps: a row whose p is the cutoff;
  f32_quotient        mode 0's votes / n_sets in float32: a kept row with a quotient float32 does not hold;
  flush_short         cells - 1 LDS counters are flushed: a count in the last cell (every threshold passed, last class, rightly called)."""
import numpy as np
import pytest

import support_envelope_cases as sec

MISTAKES = ("search_le", "last_of_ties", "label_call_swapped", "first_stride_only", "last_flush_dropped", "bf_offset_0", "bf_formula", "train_labels",
            "train_row_count", "keep_ge", "f32_quotient", "flush_short")
# (case, mode): where each mistake MUST show
CAUGHT_BY = {
    "search_le": [("thresholds_are_the_votes", 0), ("thresholds_outside_0_1", 0), ("prior_built", 0), ("prior_built", 1), ("cutoff_attained", 0)],
    "last_of_ties": [("sets_2", 0), ("sets_4", 0), ("sets_64", 0), ("cutoff_attained", 0)],
    "label_call_swapped": [("default", 0), ("default", 1), ("classes_2", 0), ("classes_100", 1), ("edge_32_classes_lds", 1)],
    "first_stride_only": [("grid_capped", 0), ("grid_capped", 1), ("grid_max_blocks_global", 0), ("grid_max_blocks_global", 1)],
    "last_flush_dropped": [("rows_1", 0), ("rows_257", 1), ("rows_769", 0), ("grid_capped", 1), ("classes_11_bf_4", 0), ("near_full_lds", 1)],
    "bf_offset_0": [("bf_1", 0), ("bf_4", 1), ("bf_513", 0), ("near_full_lds", 1), ("prior_built", 0), ("classes_11_thr_513_bf_512", 1)],
    "bf_formula": [("prior_built", 0), ("prior_built", 1)],
    "train_labels": [("test_table", 0), ("test_table", 1), ("test_table_classes_32_thr_9", 0), ("test_table_classes_32_thr_9", 1)],
    "train_row_count": [("test_table", 0), ("test_table", 1), ("test_table_classes_32_thr_9", 0), ("test_table_classes_32_thr_9", 1)],
    "keep_ge": [("cutoff_attained", 0), ("cutoff_1", 0)],
    "f32_quotient": [("default", 0), ("sets_3", 0), ("sets_7", 0), ("rows_257_classes_11_thr_513_bf_513_cutoff", 0)],
    "flush_short": [("default", 0), ("thresholds_0", 0), ("thresholds_0", 1), ("classes_1", 0), ("classes_1", 1), ("bf_4", 0)],
}
LDS_FILL = 0xA5A5A5A5                           # what a workgroup's LDS holds before the kernel writes to it


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def accumulate(stack, mode):
    """launch_summary_accumulate's accumulator: uint32 votes for the first class holding a set's largest value, or float64 sums in set
    order."""
    n_sets, n, c = stack.shape
    if mode == 0:
        votes = np.zeros((n, c), dtype=np.uint32)
        for s in range(n_sets):
            best, bk = stack[s][:, 0].copy(), np.zeros(n, dtype=np.int64)
            for k in range(1, c):
                up = stack[s][:, k] > best
                best, bk = np.where(up, stack[s][:, k], best), np.where(up, k, bk)
            votes[np.arange(n), bk] += 1
        return votes
    acc = np.zeros((n, c))
    for s in range(n_sets):
        acc += stack[s]
    return acc


def _count_below(read, n, v, le):
    """count_below: the bisection, every row at its own step; ``read(mid)`` the threshold a row's thread loads."""
    lo, hi = np.zeros(len(v), dtype=np.int64), np.full(len(v), n, dtype=np.int64)
    while True:
        active = lo < hi
        if not active.any():
            return lo
        mid = np.where(active, (lo + hi) >> 1, 0)
        t = read(mid)
        with np.errstate(invalid="ignore"):
            below = (t <= v) if le else (t < v)
        lo = np.where(active & below, mid + 1, lo)
        hi = np.where(active & ~below, mid, hi)


def model(name, mode, acc, n_sets, prior, bf_thresholds, bug=None, n_cu=sec.ASSUMED_N_CU):
    """What npbnn_predict_sets_support returns for a case, from the accumulator: dict(cube, bf, keep, summary)."""
    inp = sec.inputs(name, n_cu)
    case, labels, thr = inp["case"], inp["labels"], inp["thresholds"]
    n_rows, c = acc.shape
    n_all = n_rows
    if not case["train_rows"] and bug in ("train_labels", "train_row_count"):       # (no other slot to read from)
        bug = None
    if bug == "train_labels":
        labels = inp["train_labels"][np.arange(n_rows) % case["train_rows"]]      # (rows past the training slot's: whatever lies there)
    if bug == "train_row_count":
        n_rows = case["train_rows"]
    n_thr, n_bf = len(thr), None if prior is None else len(bf_thresholds)
    cells, bf_cells = (n_thr + 1) * c * c, 0 if prior is None else (n_bf + 1) * 2
    # the host side: switches, dynamic LDS, grid; the threshold buffer [thresholds | bf thresholds | one spare]
    lds_cube, lds_thr, lds_bf = cells <= sec.LDS_CELLS, n_thr <= sec.LDS_THRESHOLDS, prior is not None and n_bf <= sec.LDS_THRESHOLDS
    lay = sec.lds_layout(c, n_thr, n_bf, lds_cube, lds_thr, lds_bf)
    grid = min(max(1, -(-n_rows // sec.WORKGROUP)), sec.FI_MAX_BLOCKS)
    if lds_cube:
        grid = min(grid, sec.WG_PER_CU * n_cu)
    d_thr = np.concatenate([thr, bf_thresholds if prior is not None else np.zeros(0), [0.0]])
    bft_at = 0 if bug == "bf_offset_0" else n_thr
    g_cube, g_bf = np.zeros(cells, dtype=np.uint64), np.zeros(bf_cells, dtype=np.uint64)
    # the kernel's prologue: every workgroup stages and zeroes its own LDS, as 32-bit words
    assert lay["total"] % 4 == 0 and lay["total"] < 64 * 1024
    lds = np.full((grid, lay["total"] // 4), LDS_FILL, dtype=np.uint32)
    w_thr, w_bft, w_cube, w_bf = lay["thr"] // 4, lay["bft"] // 4, lay["cube"] // 4, lay["bf"] // 4
    if lds_thr:
        lds[:, w_thr:w_thr + 2 * n_thr] = d_thr[:n_thr].view(np.uint32)[None]
    if lds_bf:
        lds[:, w_bft:w_bft + 2 * n_bf] = d_thr[bft_at:bft_at + n_bf].view(np.uint32)[None]
        lds[:, w_bf:w_bf + bf_cells] = 0
    if lds_cube:
        lds[:, w_cube:w_cube + cells] = 0
    s_thr = np.ascontiguousarray(lds[:, w_thr:w_thr + 2 * n_thr]).view(np.float64) if lds_thr else None
    s_bft = np.ascontiguousarray(lds[:, w_bft:w_bft + 2 * n_bf]).view(np.float64) if lds_bf else None
    # the rows a thread reaches: r = (blockIdx.x * 256 + threadIdx.x) + pass * gridDim.x * 256
    r = np.arange(n_rows)
    if bug == "first_stride_only":
        r = r[r < grid * sec.WORKGROUP]
    wg = (r // sec.WORKGROUP) % grid
    a = acc[r]
    if mode == 0 and bug == "f32_quotient":
        q = (a.astype(np.float32) / np.float32(n_sets)).astype(np.float64)
    else:
        q = a.astype(np.float64) / np.float64(n_sets)
    best, bk = q[:, 0].copy(), np.zeros(len(r), dtype=np.int64)
    for k in range(1, c):
        up = (q[:, k] >= best) if bug == "last_of_ties" else (q[:, k] > best)
        best, bk = np.where(up, q[:, k], best), np.where(up, k, bk)
    cutoff = inp["cutoff"]
    kept = np.ones(len(r), dtype=bool) if cutoff is None else ((best >= cutoff) if bug == "keep_ge" else (best > cutoff))
    keep, summary = np.zeros(n_all, dtype=bool), np.zeros((n_all, c))
    keep[r] = kept
    summary[r] = np.where(kept[:, None], q, np.nan)
    lab = labels[r]
    assert np.all((lab >= 0) & (lab < c))
    b = _count_below((lambda mid: s_thr[wg, mid]) if lds_thr else (lambda mid: d_thr[mid]), n_thr, best, bug == "search_le")
    cell = (b * c + bk) * c + lab if bug == "label_call_swapped" else (b * c + lab) * c + bk
    if lds_cube:
        np.add.at(lds, (wg, w_cube + cell), 1)
    else:
        np.add.at(g_cube, cell, 1)
    if prior is not None:
        pr = prior[r, bk]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if bug == "bf_formula":
                factor = best * (1e-10 + 1 - pr) / (pr * (1e-10 + 1 - best))
            else:
                factor = (best / (1e-10 + 1 - best)) / (pr / (1e-10 + 1 - pr))
        bb = _count_below((lambda mid: s_bft[wg, mid]) if lds_bf else (lambda mid: d_thr[bft_at + mid]), n_bf, factor, bug == "search_le")
        bcell = bb * 2 + (bk == lab)
        if lds_bf:
            np.add.at(lds, (wg, w_bf + bcell), 1)
        else:
            np.add.at(g_bf, bcell, 1)
    # the epilogue: every workgroup adds its non-zero 32-bit counters to the 64-bit tables
    flushing = range(grid - 1 if bug == "last_flush_dropped" else grid)
    short = 1 if bug == "flush_short" else 0
    for w in flushing:
        if lds_cube:
            g_cube[:cells - short] += lds[w, w_cube:w_cube + cells - short]
        if lds_bf:
            g_bf[:bf_cells - short] += lds[w, w_bf:w_bf + bf_cells - short]
    return dict(cube=g_cube.astype(np.int64).reshape(n_thr + 1, c, c), bf=g_bf.astype(np.int64).reshape(-1, 2) if prior is not None else None, keep=keep,
                summary=summary)


# ---- where a mistake can show -----------------------------------------------------------------------------------------------------------
def applies(bug, case, mode, acc, n_sets, want, thr, prior, bft, n_cu=sec.ASSUMED_N_CU):
    """True: the mistake changes an output of this case; False: it cannot; None: rounding decides."""
    c = case["n_out"]
    n_thr, n_bf = len(thr), None if prior is None else len(bft)
    cells = (n_thr + 1) * c * c
    lds_cube, lds_bf = cells <= sec.LDS_CELLS, prior is not None and n_bf <= sec.LDS_THRESHOLDS
    plan = sec.launch_plan(case, n_cu)
    assert (plan["cells"], plan["lds_cube"]) == (cells, lds_cube)
    if bug == "search_le":
        return sec.rows_on_a_threshold(want["p"], thr) > 0 or (prior is not None and sec.rows_on_a_threshold(want["factor"], bft) > 0)
    if bug == "last_of_ties":
        return sec.tied_rows(acc / n_sets) > 0
    if bug == "label_call_swapped":
        return any(not np.array_equal(t, t.T) for t in want["cube"])
    if bug == "first_stride_only":
        return plan["strides"] > 1
    if bug == "last_flush_dropped":
        return lds_cube or lds_bf
    if bug == "bf_offset_0":                                    # (a single row may fall in the same bin of either array)
        return prior is not None and n_bf > 0 and n_thr > 0 and (True if plan["n_rows"] > 1 else None)
    if bug == "bf_formula":
        return None if prior is not None else False
    if bug in ("train_labels", "train_row_count"):
        return bool(case["train_rows"])
    if bug == "keep_ge":
        return case["cutoff"] is not None and bool(np.any(want["p"] == case["cutoff"]))
    if bug == "f32_quotient":
        if mode != 0:
            return False
        moved = np.any((acc.astype(np.float32) / np.float32(n_sets)).astype(np.float64) != acc / n_sets, axis=1)
        return True if np.any(moved & want["keep"]) else (None if moved.any() else False)
    assert bug == "flush_short"
    return bool((lds_cube and want["cube"][-1, -1, -1] > 0) or (lds_bf and want["bf"][-1, 1] > 0))


@pytest.fixture(scope="module")
def seen():
    """{(mistake, case, mode): True | False | None} as test_model_and_every_mistake found them."""
    return {}


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sec.CASES))
def test_model_and_every_mistake(name, seen):
    inp = sec.inputs(name)
    case, labels, thr = inp["case"], inp["labels"], inp["thresholds"]
    stack = sec.oracle_stack(name)
    n_sets = stack.shape[0]
    for mode in sec.MODES:
        summary = sec.summarise(stack, mode)
        prior, bft = inp["prior"], inp["bf_thresholds"]
        if case["prior"] == "built":
            prior, bft = sec.built_prior(name, summary)
        want = sec.restatement(summary, labels, thr, prior, bft, inp["cutoff"])
        acc = accumulate(stack, mode)
        right = model(name, mode, acc, n_sets, prior, bft)
        assert sec.differing_fields(right, want) == [], (name, mode)
        assert want["cube"].sum() == len(labels) and (want["bf"] is None or want["bf"].sum() == len(labels))
        edge = sec.edge_count(case, mode, want, summary, thr, bft, inp["cutoff"])
        assert edge is None or edge > 0, (name, mode, case["edge"])
        assert not sec.must_tie(case, mode) or sec.tied_rows(summary) > 0, (name, mode)
        for bug in MISTAKES:
            can = applies(bug, case, mode, acc, n_sets, want, thr, prior, bft)
            shows = sec.differing_fields(model(name, mode, acc, n_sets, prior, bft, bug), want)
            seen[(bug, name, mode)] = bool(shows)
            if can is not None:
                assert bool(shows) == can, (name, mode, bug, shows)


@pytest.mark.parametrize("bug", MISTAKES)
def test_every_mistake_is_caught_on_its_named_cases(bug, seen):
    assert CAUGHT_BY[bug]
    for name, mode in CAUGHT_BY[bug]:
        if (bug, name, mode) not in seen:                       # (this test run on its own)
            test_model_and_every_mistake(name, seen)
        assert seen[(bug, name, mode)], (bug, name, mode)


def test_table_sanity():
    assert all(c["name"] == n for n, c in sec.CASES.items())
    assert len(sec.CASES) == 65
    plans = {n: sec.launch_plan(c) for n, c in sec.CASES.items()}
    # every combination of the switches the entry can reach: cube and thresholds in LDS or global, the Bayes-factor side absent, in LDS
    # or global.  (The built prior's thresholds are 44: LDS.)
    reached = {(p["lds_cube"], p["lds_thr"], sec.bf_side(44 if p["n_bf"] == -1 else p["n_bf"])) for p in plans.values()}
    assert reached == {(a, b, s) for a in (True, False) for b in (True, False) for s in ("none", "lds", "global")}
    # the two 10240-cell cases are exactly at the edge, their neighbours the first counts above it
    for lds, glob in (("edge_32_classes_lds", "edge_32_classes_global"), ("edge_8_classes_lds", "edge_8_classes_global")):
        assert plans[lds]["cells"] == sec.LDS_CELLS and plans[lds]["lds_cube"]
        c = sec.CASES[glob]["n_out"]
        assert plans[glob]["cells"] == sec.LDS_CELLS + c * c and not plans[glob]["lds_cube"]
    assert (plans["classes_10"]["cells"], plans["classes_10"]["lds_cube"]) == (10000, True)
    assert (plans["classes_11"]["cells"], plans["classes_11"]["lds_cube"]) == (12100, False)
    # 513 thresholds with 4 classes: searched in global memory, counted in LDS
    assert plans["thresholds_513"]["lds_cube"] and not plans["thresholds_513"]["lds_thr"] and plans["thresholds_512"]["lds_thr"]
    # the largest dynamic LDS of the table is the near-full case's, under the 64 KiB a workgroup can have and three to a 160 KiB unit
    sizes = {}
    for n, c in sec.CASES.items():
        p = plans[n]
        n_bf = 44 if p["n_bf"] == -1 else p["n_bf"]
        sizes[n] = sec.lds_layout(c["n_out"], len(sec.thresholds_of(c)), n_bf, p["lds_cube"], p["lds_thr"], sec.bf_side(n_bf) == "lds")["total"]
    assert max(sizes, key=sizes.get) == "near_full_lds" and sizes["near_full_lds"] == 159 * 8 + 512 * 8 + 10240 * 4 + 513 * 2 * 4 == 50432
    assert sizes["near_full_lds"] < 64 * 1024 and 3 * sizes["near_full_lds"] <= 160 * 1024
    # the grid: the cap binds and a second stride is taken on the capped case; grid_for's own cap and a second stride on the other
    cap = plans["grid_capped"]
    assert cap["lds_cube"] and cap["grid"] == sec.WG_PER_CU * sec.ASSUMED_N_CU and cap["strides"] == 2
    assert cap["n_rows"] - cap["grid"] * sec.WORKGROUP == 300
    big = plans["grid_max_blocks_global"]
    assert not big["lds_cube"] and not big["lds_thr"] and big["grid"] == sec.FI_MAX_BLOCKS and big["strides"] == 2 and big["cells"] == 10244
    assert all(p["strides"] == 1 for n, p in plans.items() if not n.startswith("grid_"))
    assert max(p["n_rows"] for n, p in plans.items() if not n.startswith("grid_")) == 769                  # (no workload sizes)
    assert {p["grid"] for n, p in plans.items() if not n.startswith("grid_")} == {1, 2, 3, 4}
    # the test table: its own row count, labels of its own draw
    for name in ("test_table", "test_table_classes_32_thr_9"):
        inp = sec.inputs(name)
        assert (len(inp["x"]), len(inp["train_x"])) == (513, 300) and not np.array_equal(inp["labels"][:300], inp["train_labels"])
    # the slope pattern travels as passes of 2, 3 and 1; five tanh sets as 3 and 2
    assert [g for _, g in sec.inputs("slopes_aabbba")["groups"]] == [2, 3, 1] and [g for _, g in sec.inputs("default")["groups"]] == [3, 2]
    # every class occurs among the labels wherever the rows allow
    for name, c in sec.CASES.items():
        if not name.startswith("grid_") and c["rows"] >= c["n_out"]:
            assert len(np.unique(sec.inputs(name)["labels"])) == c["n_out"], name
    assert set(sec.ROUTED) <= set(sec.CASES) and set(sec.SAME_BYTES) <= set(sec.CASES) and len(sec.CROSSED) >= 4


def test_bf_thresholds_of_the_table():
    for n_bf in (0, 1, 4, 512, 513):
        t = sec.drawn_bf_thresholds(n_bf)
        assert len(t) == n_bf and np.all(t[1:] >= t[:-1])
        if n_bf >= 4:
            assert 1.0 in t and np.inf in t and np.any(t[1:] == t[:-1])
    for name, c in sec.CASES.items():
        t = sec.thresholds_of(c)
        assert not np.any(np.isnan(t)) and np.all(t[1:] >= t[:-1]), name
