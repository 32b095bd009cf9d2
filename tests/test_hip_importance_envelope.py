"""GPU: npbnn_permute_columns and npbnn_predict_sets_summary over their whole envelope (tests/importance_envelope_cases.py; the CPU
guards of the case tables are tests/test_host_importance_envelope.py).

The gather: after launch, permute, permute other columns without a restore, restore - and, where the case says so, a permutation
before the first launch - a context gives the bytes of a fresh context that was handed the host-shuffled matrix: ``predict_sets`` of
the case's weight sets, and ``eval`` with its confusion table where the case has labels.  Every run asserts the path it names
(``is_wide``, ``l0_mode``) and prints it.  One case has no fresh context to compare with (the restored entry lies above scales that
were taken without it) and is held to the float64 oracle instead, to test_hip_posterior.TOL and no other tolerance.

The summary: the host's own ``_summarise`` and table on the array ``predict_sets`` returns from the same context, as bytes."""
import importlib

import numpy as np
import pytest

import importance_envelope_cases as iec
from npbnn_amd import HipContext, _capi as capi
from test_hip_importance import PATHS, _context, _host_shuffle, _table
from test_hip_posterior import TOL

pytestmark = pytest.mark.gpu

posterior = importlib.import_module("npbnn_amd.posterior")

TRAIN, TEST = capi.TRAIN, capi.TEST
RUNS = [(name, path) for name, case in iec.GATHER.items() for path in case["paths"]]
assert set(iec.PATHS) == set(PATHS)


@pytest.fixture
def opened():
    """contexts a test opened: closed whatever the test's end"""
    held = []
    yield held
    for ctx in held:
        ctx.close()


def _open(opened, inp, x, x_test=None, mask=None):
    if inp["labels"] is None and x_test is None:
        ctx = _context(x, inp["sets"])
        opened.append(ctx)
    else:
        ctx = HipContext(0)
        opened.append(ctx)
        ctx.set_data(x)
        if x_test is not None:
            ctx.set_data(x_test, TEST)
        if inp["labels"] is not None:
            ctx.set_labels(inp["labels"])
        ctx.set_arch_from_weights(inp["sets"][0], x.shape[1], capi.ACT_TANH, capi.OUT_SOFTMAX,
                                  capi.LIK_NONE if inp["labels"] is None else capi.LIK_CATEGORICAL)
    if mask is not None:
        ctx.set_layer_mask(mask)
    return ctx


def _results(ctx, inp, path, which=TRAIN, l0="f16-split"):
    """What the case compares, as bytes; the launch ran on the path the run names."""
    out = [ctx.predict_sets(inp["sets"], which=which).tobytes()]
    assert ctx.is_wide() == (path == "streamed")
    mode = ctx.l0_mode()
    if path == "f32":
        assert mode == "f32"
    elif l0 is not None:
        assert mode == l0
    if inp["labels"] is not None:
        r = ctx.eval(inp["sets"][0], which=which, want_confusion=True)
        assert r["confusion"].sum() == ctx.n_rows[which]
        out += [np.float64(r["loglik"]).tobytes(), r["confusion"].tobytes()]
    return out, mode


def _fresh(opened, inp, path, matrix, mask=None):
    ctx = _open(opened, inp, matrix, mask=mask)
    res = _results(ctx, inp, path)[0]
    moved = ctx.f16_moved_columns()
    ctx.close()
    return res, moved


def _set_path(path, monkeypatch):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)


def _plain(inp, path, opened, masks=(None,)):
    """launch, permute, permute other columns without a restore, restore: back to the base bytes.  ``masks``: the layer masks the
    sequence runs under, every one against a fresh context of its own and (block structure) the first one's bytes."""
    x, (call1, call2) = inp["x"], inp["calls"]
    heavy = inp["moved"] is not None
    first = None
    for mask in masks:
        ctx = _open(opened, inp, x, mask=mask)
        base = _results(ctx, inp, path)[0]               # (builds the split copies the gather then has to patch)
        scales = ctx.f16_moved_columns()
        if heavy and path != "f32":                      # (the float32 layer 0 never takes scales: nothing to move there)
            assert scales[0] == len(inp["moved"]) > 0, scales
        else:
            assert scales[0] == 0
        steps = [base]
        for cols, idx in (call1, call2):
            ctx.permute_columns(cols, idx)
            got = _results(ctx, inp, path)[0]
            want, want_scales = _fresh(opened, inp, path, _host_shuffle(x, cols, idx), mask)
            assert got == want, "columns %s" % (cols,)
            assert got != base or inp["degenerate"]
            assert ctx.f16_moved_columns() == scales == want_scales
            steps.append(got)
        if call1[1].size > iec.FI_GRID_CAP:              # a row index outside the matrix past the cap: perm_check finds it, nothing is written
            bad = np.array(call1[1])
            bad[-1, -1] = x.shape[0]
            with pytest.raises(capi.NpbnnError) as e:
                ctx.permute_columns(call1[0], bad)
            assert e.value.code == capi.E_ARG and "row index" in str(e.value)
            assert _results(ctx, inp, path)[0] == steps[2]
        ctx.permute_columns([], None)
        assert _results(ctx, inp, path)[0] == base
        assert _fresh(opened, inp, path, x, mask) == (base, scales)
        ctx.close()
        if inp["case"]["before"]:                        # nothing built the split copies yet: they are split from the permuted matrix
            ctx = _open(opened, inp, x, mask=mask)
            ctx.permute_columns(*call1)
            assert _results(ctx, inp, path)[0] == steps[1]
            assert ctx.f16_moved_columns() == scales
            ctx.permute_columns(*call2)
            assert _results(ctx, inp, path)[0] == steps[2]
            ctx.permute_columns([], None)
            assert _results(ctx, inp, path)[0] == base
            ctx.close()
        if first is None:
            first = steps
        assert steps == first, "the blocked first layer is not the dense one"


def _test_table(inp, path, opened):
    x, x_test, (call1, call2), l0 = inp["x"], inp["x_test"], inp["calls"], inp["l0"]
    train_l0 = "f16-split"

    def fresh(test_matrix):
        c = _open(opened, inp, x, x_test=test_matrix)
        res = _results(c, inp, path, TEST, l0)
        c.close()
        return res

    ctx = _open(opened, inp, x, x_test=x_test)
    base_train = _results(ctx, inp, path, TRAIN, train_l0)[0]
    base_test, mode = _results(ctx, inp, path, TEST, l0)
    print("    test-table launches report %s" % mode)
    scales = ctx.f16_moved_columns()
    assert (scales[0] > 0) == (inp["case"]["kind"] != "test_table" and path != "f32")
    assert (base_test, mode) == fresh(x_test)
    # test columns shuffled: the fresh context's bytes, and the training table's results are the base bytes
    ctx.permute_columns(*call1, which=TEST)
    shuffled = _results(ctx, inp, path, TEST, l0)
    assert shuffled == fresh(_host_shuffle(x_test, *call1)) and shuffled[0] != base_test
    assert _results(ctx, inp, path, TRAIN, train_l0)[0] == base_train
    # both tables shuffled, then the training table alone restored: the test table is still shuffled
    ctx.permute_columns(*inp["train_call"], which=TRAIN)
    assert _results(ctx, inp, path, TRAIN, train_l0)[0] != base_train
    assert _results(ctx, inp, path, TEST, l0) == shuffled
    ctx.permute_columns([], None, which=TRAIN)
    assert _results(ctx, inp, path, TRAIN, train_l0)[0] == base_train
    assert _results(ctx, inp, path, TEST, l0) == shuffled
    # other test columns without a restore, then the restore
    ctx.permute_columns(*call2, which=TEST)
    assert _results(ctx, inp, path, TEST, l0) == fresh(_host_shuffle(x_test, *call2))
    assert _results(ctx, inp, path, TRAIN, train_l0)[0] == base_train
    ctx.permute_columns([], None, which=TEST)
    assert _results(ctx, inp, path, TEST, l0) == (base_test, mode)
    assert ctx.f16_moved_columns() == scales


def _planted(inp, path, opened):
    """Case (b).  The draw comes before the first launch and drops the row of the planted 100.0: the scales are taken from a matrix
    without it.  Restored, the entry lies 2^4 or more above its column's 1 and no fresh context has these scales; every set's
    predictions on the restored table are held to the float64 oracle on the float32-rounded table instead."""
    x, sets = inp["x"], inp["sets"]
    (cols, idx), = inp["calls"]
    ctx = _open(opened, inp, x)
    ctx.permute_columns(cols, idx)
    shuffled = _results(ctx, inp, path)[0]
    assert (shuffled, (0, 0)) == _fresh(opened, inp, path, _host_shuffle(x, cols, idx))
    ctx.permute_columns([], None)
    y = ctx.predict_sets(sets)
    assert ctx.is_wide() == (path == "streamed") and ctx.l0_mode() == ("f32" if path == "f32" else "f16-split")
    want = iec.oracle_sets(x, sets)
    errs = []
    for i, w in enumerate(sets):                         # (test_hip_wide_replay._three_checks' reading of the bound)
        np.testing.assert_array_equal(y[i], ctx.predict(w), err_msg="set %d is not its own predict" % i)
        errs.append(float(np.max(np.abs(y[i] - want[i]))))
    print("    planted entry restored: max |device - float64| = %.3e (row of the entry: %.3e), bound %.1e" % (
        max(errs), float(np.max(np.abs(y[:, iec.PLANTED_ROW] - np.array(want)[:, iec.PLANTED_ROW]))), TOL))
    for i in range(len(sets)):
        np.testing.assert_allclose(y[i], want[i], atol=TOL, rtol=0, err_msg="set %d" % i)
    assert y.tobytes() != shuffled[0]


def _pdp(inp, path, opened, monkeypatch):
    """predict_pdp reads the float32 table: after a shuffle both of its routes give the fresh context's bytes."""
    x, sets = inp["x"], inp["sets"]
    (cols, idx), = inp["calls"]
    for route, env in ((1, None), (2, "1")):
        if env:
            monkeypatch.setenv("NPBNN_PDP_PER_GRID", env)
        ctx, ref = _open(opened, inp, x), _open(opened, inp, _host_shuffle(x, cols, idx))
        base = ctx.predict_pdp(sets, inp["focal"], inp["grid"])
        assert ctx.info(capi.INFO_PDP_ROUTE) == route
        ctx.predict_sets(sets)                           # (the split copies exist, as in an importance run)
        ctx.permute_columns(cols, idx)
        got, want = ctx.predict_pdp(sets, inp["focal"], inp["grid"]), ref.predict_pdp(sets, inp["focal"], inp["grid"])
        assert ctx.info(capi.INFO_PDP_ROUTE) == ref.info(capi.INFO_PDP_ROUTE) == route
        assert got.tobytes() == want.tobytes() and got.tobytes() != base.tobytes()
        ctx.permute_columns([], None)
        assert ctx.predict_pdp(sets, inp["focal"], inp["grid"]).tobytes() == base.tobytes()
        print("    predict_pdp route %d" % route)
        ctx.close()
        ref.close()


@pytest.mark.parametrize("name,path", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_gather_is_a_fresh_upload(name, path, monkeypatch, opened):
    _set_path(path, monkeypatch)
    inp = iec.gather_inputs(name)
    kind = inp["case"]["kind"]
    print("\n  gather %s on the %s path (%d rows x %d features)" % (name, path, inp["table"].shape[0], inp["table"].shape[1]))
    if inp["which"] == TEST:
        _test_table(inp, path, opened)
    elif kind == "planted":
        _planted(inp, path, opened)
    elif kind == "pdp":
        _pdp(inp, path, opened, monkeypatch)
    elif kind == "blocked":
        _plain(inp, path, opened, masks=(None, inp["mask"]))
    else:
        _plain(inp, path, opened)


@pytest.mark.parametrize("name", list(iec.SUMMARY))
def test_summary_is_the_hosts_everywhere(name, opened):
    inp = iec.summary_inputs(name)
    case, sets, labels, which = inp["case"], inp["sets"], inp["labels"], inp["which"]
    n, c = inp["table"].shape[0], case["n_out"]
    ctx = _open(opened, dict(inp, labels=None), inp["x"], x_test=inp["x_test"])
    stack = ctx.predict_sets(sets, which=which)
    print("\n  summary %s on the default path (streamed %s, layer 0 %s): %d rows, %d classes, %s confusion table" % (
        name, ctx.is_wide(), ctx.l0_mode(), n, c, "LDS" if c <= iec.CONF_LDS_CLASSES else "global"))
    assert stack.shape == (case["sets"], n, c) and not ctx.is_wide() and ctx.l0_mode() == "f16-split"
    for mode in (0, 1):
        want = posterior._summarise(stack, mode)
        summary, table = ctx.predict_sets_summary(sets, mode, labels=labels, which=which)
        only_table = ctx.predict_sets_summary(sets, mode, labels=labels, which=which, want_summary=False)
        only_summary = ctx.predict_sets_summary(sets, mode, which=which)
        assert only_table[0] is None and only_summary[1] is None
        assert summary.shape == want.shape and summary.dtype == want.dtype == np.float64
        assert summary.tobytes() == want.tobytes(), "mode %d: max |device - host| = %g" % (mode, np.max(np.abs(summary - want)))
        assert table.dtype == np.int64 and table.shape == (c, c) and table.sum() == n
        assert table.tobytes() == _table(want, labels).tobytes()
        assert only_table[1].tobytes() == table.tobytes() and only_summary[0].tobytes() == summary.tobytes()
        if case["kind"] == "one_cell":
            assert table[c - iec.ONE_CELL_LABEL_FROM_END, iec.ONE_CELL_WINNER] == n
