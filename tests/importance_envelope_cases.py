"""The envelope of npbnn_permute_columns and npbnn_predict_sets_summary (npbnn_amd/csrc/npbnn_importance.hip): the case tables GATHER and
SUMMARY, their seeded inputs and the host references.  tests/test_hip_importance_envelope.py runs them on the device,
tests/test_host_importance_envelope.py checks on the CPU that the references tell a wrong gather from a right one and that every
condition a case rests on holds for its draw.  Nothing here needs a GPU.

GATHER.  The claim of every case is test_hip_importance.test_gather_is_exact's: after a sequence of permute_columns calls a context
gives the bytes of a fresh context that was handed the host-shuffled matrix.  A case is one or two axes away from the default (1000 rows
x 40 standard-normal features, network [12, 7], tanh, 6 classes, 4 weight sets) and names its calls as (columns, "one" permutation for
the block | one for "each" column).  The second call comes without a restore in between and, wherever the columns allow, shares some
of the first call's columns and drops others: the library's restore and save then touch the same column in one call.

SUMMARY.  The reference is the host's own: posterior._summarise on the array predict_sets returns from the same context, and
test_hip_importance._table of that summary against the labels."""
import functools

import numpy as np

import cases
import oracle as orc
import pdp_cases
import scale_cases as sc
import split_model as sm
from test_hip_importance import _host_shuffle

PATHS = ("default", "f32", "streamed")          # test_hip_importance.PATHS' names
FI_GRID_CAP = 2048 * 256                        # kFiMaxBlocks * kFiThreads: items past it take a grid-stride loop a second time
CONF_LDS_CLASSES = 64                           # kConfLdsClasses: more classes count in the global table
PLANTED_VALUE, PLANTED_ROW, PLANTED_COL = 100.0, 123, 21

_G_DEFAULTS = dict(rows=1000, features=40, nodes=(12, 7), n_out=6, sets=4, kind="plain", calls=None, paths=PATHS, before=False, eval=False)
GATHER = {}


def _gather(name, **kw):
    unknown = set(kw) - set(_G_DEFAULTS)
    assert not unknown and name not in GATHER, (name, unknown)
    GATHER[name] = dict(_G_DEFAULTS, name=name, **kw)


def boundary_columns(f):
    """Column 0, column F - 1, the last column of a full 8-feature group and the first column of the last, partial, group."""
    cols = [0, f - 1]
    if f >= 8:
        cols.append(8 * (f // 8) - 1)
    if f % 8:
        cols.append(8 * (f // 8))
    return list(dict.fromkeys(cols))


def _second_call(first, f):
    """All but the first of ``first``'s columns and the lowest column it does not name: a partial overlap where the matrix allows."""
    other = [c for c in range(f) if c not in first][:1]
    return (first[1:] + other) or list(first)


_FOUR = ([3, 4, 21, 39], [5, 4, 21, 30])        # test_hip_importance.SHUFFLES' linked block and the call that follows it

# rows: a 16-row tile of X16w, a workgroup of 256 and the padding rows of both; one row: the only index is 0 and every gather is the identity
for _n in (1, 15, 16, 17, 255, 256, 257, 2111):
    _gather("rows_%d" % _n, rows=_n, calls=[(_FOUR[0], "one"), (_FOUR[1], "each")], before=_n in (1, 17), eval=_n == 2111)
# rows x columns past the grid cap: 70 001 x 8 = 560 008 items in perm_check (8 permutations), perm_save, perm_gather and, in the second
# call, perm_restore.  The patch kernel counts rows x 8-feature GROUPS, 70 001 here; the 64-feature case below gives it 8 groups
_gather("rows_past_the_grid_cap", rows=70001, features=8, nodes=(4,), calls=[(list(range(8)), "each"), ([7, 0, 3], "one")])
_gather("rows_past_the_grid_cap_8_groups", rows=70001, features=64, nodes=(4,),
        calls=[([8 * g + (3 * g) % 8 for g in range(8)], "each"), ([8 * g + (5 * g + 1) % 8 for g in range(8)], "one")])
# features: Fp and Fp16 padding, n_units = ceil(F / 32), groups at and past a K-unit
for _f in (1, 7, 8, 9, 31, 32, 33, 40, 63, 64, 65, 130):
    _b = boundary_columns(_f)
    _gather("features_%d" % _f, features=_f, calls=[(_b, "each" if len(_b) > 1 else "one"), (_second_call(_b, _f), "one")],
            before=_f in (1, 33, 130))
# column sets
_gather("one_column", calls=[([17], "one"), ([5], "one")])
_gather("one_column_one_permutation", calls=[([0], "one"), ([39, 0], "each")], before=True)        # n_cols == n_perm == 1
_gather("all_columns_one_permutation", calls=[(list(range(40)), "one"), ([39, 0, 8], "each")])
_gather("all_columns_each_its_own", calls=[(list(range(40)), "each"), (list(range(39, -1, -1)), "one")])
_gather("two_columns_of_one_group", calls=[([9, 14], "each"), ([14, 10], "one")])
_gather("eight_columns_in_eight_groups", features=64, calls=[([8 * g + (3 * g) % 8 for g in range(8)], "each"),
                                                             ([8 * g + (3 * g) % 8 for g in range(4, 8)] + [1, 10, 19, 28], "each")])
_gather("second_call_overlaps_the_first", calls=[([3, 4, 21, 39], "each"), ([4, 39, 7, 22], "each")], before=True)
# heavy tails: scale_cases.train_table("lognormal3"), layer 0 normalised as scale_cases.weight_sets does it; the columns come from the CPU
# model of ensure_scales (gather_inputs): moved and unmoved ones.  That project's own draw (seed 101) gives both, no seed was picked
_gather("heavy_tails", kind="heavy_tails", before=True)
# the test table (173 rows under 1000 training rows), and scale_cases.tables("moved_train_normal"): 300 rows under moved training scales
_gather("test_table", kind="test_table", calls=[(_FOUR[0], "one"), (_FOUR[1], "each")])
_gather("test_table_under_moved_scales", kind="test_table_moved", calls=[(_FOUR[0], "each"), (_FOUR[1], "one")])
# (the model of ensure_x16 sends that N(0, 1) table to the float32 layer 0: its split copy is dropped and only X and X16w are patched.
# scale_cases.tables("moved_train_lognormal")'s test table stays on the pair under the moved scales: its X16 is patched)
_gather("lognormal_test_table_under_moved_scales", kind="test_table_moved_lognormal", calls=[(_FOUR[0], "one"), (_FOUR[1], "each")])
# test_hip_parity.test_layer0_block_structure_is_the_dense_result_bit_for_bit's first layer: 160 features, 48 nodes, 10 groups of 16
# features; two columns of block 1 and one of block 9, then one of block 1, one of block 0 and one of block 5
_gather("block_structure", kind="blocked", rows=257, features=160, nodes=(48, 8), paths=("default", "f32"),
        calls=[([17, 30, 159], "each"), ([30, 2, 80], "one")])
# indices that are no permutation: rows drawn with replacement
_gather("with_replacement_largest_kept", kind="largest_kept", calls=[(_FOUR[0], "each"), (_FOUR[1], "one")])
_gather("with_replacement_planted_entry_dropped", kind="planted", calls=[([PLANTED_COL, 5], "one")])
# a reader of the float32 table: predict_pdp on both routes, on pdp_cases' plain default (300 x 40, [20, 6], 5 outputs, 3 sets)
_gather("pdp_reads_the_shuffled_table", kind="pdp", rows=300, nodes=(20, 6), n_out=5, sets=3, paths=("default",), calls=[([5, 17, 39], "each")])


def _seed(name):
    return cases.hash_name("importance_envelope/" + name) % (2 ** 31)


def _unit_sets(rs, f, nodes, n_out, n_sets, bias=2):
    """N(0, 1 / sqrt(fan_in + 1)) weights: every layer's sums of order 1 whatever the widths, so a moved entry moves the predictions"""
    shapes = cases.layer_shapes(f, list(nodes), n_out, bias)
    return [[rs.normal(0, 1.0 / np.sqrt(s[1]), s) for s in shapes] for _ in range(n_sets)]


def _normalised_sets(rs, x, nodes, n_out, n_sets):
    """scale_cases.weight_sets' draw for a heavy-tailed table: N(0, 0.5), layer 0 divided by the columns' mean |value|"""
    shapes = cases.layer_shapes(x.shape[1], list(nodes), n_out, 2)
    sets = [[rs.normal(0, 0.5, s) for s in shapes] for _ in range(n_sets)]
    for w in sets:
        w[0][:, 1:] /= np.abs(x.astype(np.float64)).mean(axis=0)
    return sets


def _perms(rs, n_rows, n_cols, how):
    return np.stack([rs.permutation(n_rows) for _ in range(1 if how == "one" else n_cols)])


def _keeping_the_largest(rs, x, cols, how):
    """Row indices drawn with replacement that still name, for every column, the row of its largest |entry|."""
    n = x.shape[0]
    idx = rs.integers(0, n, (1 if how == "one" else len(cols), n))
    at = rs.permutation(n)[:len(cols)]                    # (one position per column: a shared index keeps them all)
    for j, c in enumerate(cols):
        idx[j if how == "each" else 0, at[j]] = int(np.argmax(np.abs(x[:, c])))
    return idx


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=4)
def gather_inputs(name):
    """The arrays of a GATHER case.  ``table``: the matrix the calls shuffle (``which`` says which one it is); ``calls``: [(columns,
    indices [1 | len(columns), rows])]; ``x`` / ``x_test``: what set_data gets; ``l0``: the layer-0 path ``which``'s launches report
    where the case's path leaves the choice to the library."""
    case = GATHER[name]
    rs = np.random.default_rng(_seed(name))
    kind, f, n = case["kind"], case["features"], case["rows"]
    out = dict(case=case, x_test=None, which=0, labels=None, mask=None, l0="f16-split", train_call=None, moved=None)
    if kind == "heavy_tails":
        x = sc.train_table("lognormal3")
        shift = sm.ensure_scales(x)[2]
        moved, unmoved = np.nonzero(shift > 0)[0], np.nonzero(shift == 0)[0]
        out["moved"] = moved
        first = [int(moved[0]), int(unmoved[0]), int(moved[-1]), int(unmoved[-1])]
        second = [int(unmoved[0]), int(moved[-1]), int(moved[len(moved) // 2]), int(unmoved[len(unmoved) // 2])]
        case_calls = [(list(dict.fromkeys(first)), "each"), (list(dict.fromkeys(second)), "one")]
        sets = _normalised_sets(rs, x, case["nodes"], case["n_out"], case["sets"])
    elif kind in ("test_table_moved", "test_table_moved_lognormal"):
        x, x_test = sc.tables("moved_train_normal" if kind == "test_table_moved" else "moved_train_lognormal")
        out.update(x_test=x_test, which=1, l0="f16-split" if sm.states(x, x_test)[1] == sm.USABLE else "f32")
        sets = _normalised_sets(rs, x, case["nodes"], case["n_out"], case["sets"])
        case_calls = case["calls"]
    elif kind == "pdp":
        pc = pdp_cases.ENVELOPE["depth3_bias_all"]
        assert {k: pc[k] for k in pdp_cases._DEFAULTS} == pdp_cases._DEFAULTS
        inp = pdp_cases.envelope_inputs(pc)
        x, sets, case_calls = inp["x"], inp["weights"], case["calls"]
        out.update(focal=inp["focal"], grid=inp["grid"])
    else:
        x = rs.standard_normal((n, f))
        if kind == "test_table":
            out.update(x_test=rs.standard_normal((173, f)), which=1)
        if kind == "blocked":
            x = x.astype(np.float32)
        if kind == "planted":
            x[PLANTED_ROW, PLANTED_COL] = PLANTED_VALUE
        sets = _unit_sets(rs, f, case["nodes"], case["n_out"], case["sets"])
        case_calls = case["calls"]
    if kind == "blocked":
        groups = np.repeat(np.arange(10), 16)
        per_group = [4, 5, 5, 5, 5, 5, 5, 5, 5, 4]
        mask = [np.ones(w.shape) for w in sets[0]]
        mask[0][:, 1:] = orc.block_mask([sets[0][0][:, 1:]], [groups], [per_group])[0]      # (column 0 is the bias: it stays)
        sets = [[w * m for w, m in zip(ws, mask)] for ws in sets]
        out["mask"] = mask
    if case["eval"]:
        out["labels"] = rs.integers(0, case["n_out"], x.shape[0])
    table = out["x_test"] if out["which"] == 1 else x
    calls = []
    for cols, how in case_calls:
        if kind == "largest_kept":
            idx = _keeping_the_largest(rs, table, cols, how)
        elif kind == "planted":
            idx = rs.integers(0, table.shape[0], (1, table.shape[0]))
            idx[idx == PLANTED_ROW] = PLANTED_ROW + 1
        else:
            idx = _perms(rs, table.shape[0], len(cols), how)
        calls.append((list(cols), _frozen(idx)))
    if out["which"] == 1:                                 # the step that shuffles both tables: these training columns
        out["train_call"] = ([2, 11, 39], _frozen(_perms(rs, x.shape[0], 3, "each")))
    out.update(x=x, table=table, sets=sets, calls=calls, degenerate=table.shape[0] == 1)
    return out


def right_matrices(inp):
    """The table after the first call and after the second (no restore in between: each a shuffle of the pristine table)."""
    return [_host_shuffle(inp["table"], cols, idx) for cols, idx in inp["calls"]]


def wrong_variants(inp):
    """{(variant, call): (wrong matrix, right matrix, columns either touches)} for every wrong gather that CAN differ from the right one
    on this case's calls.
      block_permutation   per-column permutations read as one for the block: needs a call with one permutation per column;
      next_column         column c + 1 shuffled instead of c: needs other columns, or other permutations, than the shift leaves in place;
      from_the_shuffled   the second call gathers from the matrix as the first call left it: needs a column both calls name;
      no_restore          the second call forgets to put the first call's columns back: needs a column only the first call names.
    ``not_applicable(inp)`` lists the rest; the host test shows that those ARE the right matrix, so nothing is left out by choice."""
    return _variants(inp, True)


def not_applicable(inp):
    return _variants(inp, False)


def _variants(inp, differing):
    x, f = inp["table"], inp["table"].shape[1]
    right = right_matrices(inp)
    out = {}
    for k in range(len(inp["calls"])):
        for variant, (wrong, touched) in _variants_of_call(x, f, k, inp["calls"], right).items():
            if _can_differ(variant, k, inp["calls"], f) == differing:
                out[(variant, k)] = (wrong, right[k], sorted(touched))
    return out


def _can_differ(variant, k, calls, f):
    cols, idx = calls[k]
    if variant == "block_permutation":
        return len(idx) > 1
    if variant == "next_column":
        return not (len(idx) == 1 and {(c + 1) % f for c in cols} == set(cols))
    first = set(calls[0][0])
    return bool(first & set(cols)) if variant == "from_the_shuffled" else bool(first - set(cols))


def _variants_of_call(x, f, k, calls, right):
    cols, idx = calls[k]
    shifted = [(c + 1) % f for c in cols]
    out = {"block_permutation": (_host_shuffle(x, cols, idx[:1]), set(cols)),
           "next_column": (_host_shuffle(x, shifted, idx), set(cols) | set(shifted))}
    if k == 1:
        before = right[0]
        from_shuffled = x.copy()
        no_restore = before.copy()
        for j, c in enumerate(cols):
            p = idx[j if len(idx) > 1 else 0]
            from_shuffled[:, c] = before[p, c]
            no_restore[:, c] = x[p, c]
        out["from_the_shuffled"] = (from_shuffled, set(cols))
        out["no_restore"] = (no_restore, set(cols) | set(calls[0][0]))
    return out


# ---- case (b): the float32 model of the restored table ------------------------------------------------------------------------------
def f32_table(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def oracle_sets(x, sets):
    """Every set's float64 predictions on the float32-rounded table (test_hip_wide_replay._three_checks' reference)."""
    x32 = f32_table(x)
    return [orc.forward(x32, w, orc.Act("tanh"), orc.out_softmax) for w in sets]


def float32_model_sets(x, sets):
    """A numpy float32 forward pass: float32 weights, layer 0 accumulated in float32 one feature after the other, values rounded to
    float32 between the layers (split_model.l0_f32 / finish), softmax of the last layer's values."""
    x32 = np.asarray(x).astype(np.float32)
    return [sm.softmax(sm.finish(sm.l0_f32(x32, w[0][:, 1:], accumulate=True), w, x32.shape[1])) for w in sets]


# ---- the summary ------------------------------------------------------------------------------------------------------------------------
_S_DEFAULTS = dict(rows=500, features=24, nodes=(12, 7), n_out=6, sets=3, kind="plain", test_rows=None, bias=2)
SUMMARY = {}


def _summary(name, **kw):
    unknown = set(kw) - set(_S_DEFAULTS)
    assert not unknown and name not in SUMMARY, (name, unknown)
    SUMMARY[name] = dict(_S_DEFAULTS, name=name, **kw)


# classes: 64 is the last LDS table, 65 and 100 count with global atomics; one class: every vote goes to class 0
for _c in (1, 2, 3, 63, 64, 65, 100):
    _summary("classes_%d" % _c, n_out=_c)
# rows past the grid cap, one thread per row.  3 classes: rows x classes is no multiple of 4, the scalar kernels; 4: the vector kernels,
# whose n4 = rows x classes / 4 passes the cap too
for _c in (3, 4):
    _summary("rows_past_the_grid_cap_%d_classes" % _c, rows=FI_GRID_CAP + 257, features=4, nodes=(3,), n_out=_c, sets=2)
_summary("test_table", rows=1000, test_rows=173)
# all labels equal and a last-layer bias that makes one class win: a single cell receives every count (LDS histogram / global table)
for _c in (5, 65):
    _summary("one_cell_%d_classes" % _c, n_out=_c, kind="one_cell", bias=3)

ONE_CELL_LABEL_FROM_END, ONE_CELL_WINNER = 2, 1          # the label is class C - 2, the winner class 1


@functools.lru_cache(maxsize=2)
def summary_inputs(name):
    case = SUMMARY[name]
    rs = np.random.default_rng(_seed("summary/" + name))
    n, f, c = case["rows"], case["features"], case["n_out"]
    x = rs.standard_normal((n, f))
    x_test = rs.standard_normal((case["test_rows"], f)) if case["test_rows"] else None
    sets = _unit_sets(rs, f, case["nodes"], c, case["sets"], bias=case["bias"])
    n_lab = case["test_rows"] or n
    if case["kind"] == "one_cell":
        labels = np.full(n_lab, c - ONE_CELL_LABEL_FROM_END)
        for w in sets:
            w[-1][ONE_CELL_WINNER, 0] += 50.0             # (bias = 3: the last layer has a bias column)
    else:
        labels = rs.integers(0, c, n_lab)
        labels[:min(c, n_lab)] = np.arange(min(c, n_lab))          # every class at least once
    return dict(case=case, x=x, x_test=x_test, which=1 if x_test is not None else 0, table=x if x_test is None else x_test, sets=sets,
                labels=labels)
