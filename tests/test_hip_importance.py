"""Permutation importance on the GPU: npbnn_permute_columns (a column gather inside the resident matrix and its fp16-split
copies), npbnn_predict_sets_summary (votes / mean over the stored samples and the confusion table, accumulated on the device) and
feature_importance's device route against the reference's tables (tests/golden/importance.npz)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import cases
import importance_cases as ic
import npbnn_amd as bn
from npbnn_amd import HipContext, _capi as capi
from npbnn_amd.backend import pack_weights

pytestmark = pytest.mark.gpu

posterior = importlib.import_module("npbnn_amd.posterior")

N, F = 1000, 40


def _x():
    return np.random.default_rng(11).standard_normal((N, F))


def _sets(n_sets, c=6, f=F, seed=5, tie=None):
    rs = np.random.default_rng(seed)
    shapes = cases.layer_shapes(f, [12, 7], c, 2)
    sets = [[rs.normal(0, 0.5, s) for s in shapes] for _ in range(n_sets)]
    if tie is not None:                          # two classes with the same weights: equal probabilities in every row
        for w in sets:
            w[-1][tie[1]] = w[-1][tie[0]]
    return sets


def _context(x, sets, act=capi.ACT_TANH):
    ctx = HipContext(0)
    ctx.set_data(x)
    ctx.set_arch_from_weights(sets[0], x.shape[1], act, capi.OUT_SOFTMAX, capi.LIK_NONE)
    return ctx


def _host_shuffle(x, cols, perms):
    out = x.copy()
    for j, c in enumerate(cols):
        out[:, c] = x[perms[j if len(perms) > 1 else 0], c]
    return out


PATHS = {"default": {}, "f32": {"NPBNN_L0": "f32"}, "streamed": {"NPBNN_FORCE_WIDE": "1"}}
SHUFFLES = {"one_column": ([17], 1), "linked_block": ([3, 4, 21, 39], 1), "unlinked_block": ([8, 0, 33], 3)}


@pytest.mark.parametrize("shuffle", sorted(SHUFFLES))
@pytest.mark.parametrize("path", sorted(PATHS))
def test_gather_is_exact(path, shuffle, monkeypatch):
    """After permute_columns the predictions are, bit for bit, those of a fresh context given the host-shuffled matrix: X and every
    split copy a launch reads hold what an upload would have put there.  No column's fp16 scale was moved, so the scales of both
    contexts are the plain ones and equality is the claim."""
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    x, sets = _x(), _sets(4)
    cols, n_perm = SHUFFLES[shuffle]
    rs = np.random.default_rng(3)
    perms = np.stack([rs.permutation(N) for _ in range(n_perm)])
    perms2 = np.stack([rs.permutation(N) for _ in range(n_perm)])

    def fresh(matrix):
        c = _context(matrix, sets)
        try:
            y = c.predict_sets(sets)
            assert c.is_wide() == (path == "streamed") and c.l0_mode() == ("f32" if path == "f32" else "f16-split")
            assert c.f16_moved_columns()[0] == 0
            return y
        finally:
            c.close()

    ctx = _context(x, sets)
    try:
        base = ctx.predict_sets(sets)                    # (builds the split copies the gather then has to patch)
        assert ctx.f16_moved_columns()[0] == 0
        ctx.permute_columns(cols, perms)
        moved = ctx.predict_sets(sets)
        np.testing.assert_array_equal(moved, fresh(_host_shuffle(x, cols, perms)))
        assert not np.array_equal(moved, base)
        ctx.permute_columns([], None)                    # restore
        np.testing.assert_array_equal(ctx.predict_sets(sets), base)
        ctx.permute_columns(cols, perms)
        other = {"one_column": [5], "linked_block": [5, 4, 21, 30], "unlinked_block": [33, 2, 8]}[shuffle]
        ctx.permute_columns(other, perms2)               # no restore in between: a permutation of the pristine matrix
        np.testing.assert_array_equal(ctx.predict_sets(sets), fresh(_host_shuffle(x, other, perms2)))
        assert ctx.f16_moved_columns()[0] == 0
    finally:
        ctx.close()
    np.testing.assert_array_equal(base, fresh(x))


def test_gather_before_the_first_launch(monkeypatch):
    """A permutation before anything built the split copies: they are then split from the permuted matrix."""
    x, sets = _x(), _sets(2)
    perms = np.random.default_rng(8).permutation(N).reshape(1, -1)
    ctx, ref = _context(x, sets), _context(_host_shuffle(x, [2, 30], perms), sets)
    try:
        ctx.permute_columns([2, 30], perms)
        np.testing.assert_array_equal(ctx.predict_sets(sets), ref.predict_sets(sets))
    finally:
        ctx.close()
        ref.close()


def _table(summary, labels):
    t = np.zeros((summary.shape[1], summary.shape[1]), dtype=np.int64)
    np.add.at(t, (labels, np.argmax(summary, axis=1)), 1)
    return t


@pytest.mark.parametrize("shape", [(1000, 6), (1000, 4), (999, 5)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fun", ["tanh", "genReLU"])
@pytest.mark.parametrize("n_sets", [1, 2, 3, 4, 7, 64])
def test_summary_is_the_hosts(n_sets, fun, shape):
    """predict_sets_summary against _summarise on the array predict_sets returns from the same context: groups of three with a
    tail of one, two or none (tanh), groups of one (genReLU sets with their own slopes); classes a multiple of four (16-byte
    reads of a row), rows x classes a multiple of four, and neither."""
    n, c = shape
    rs = np.random.default_rng(n_sets)
    x = rs.standard_normal((n, 24))
    sets = _sets(n_sets, c=c, f=24, seed=n_sets + 1)
    slopes = [rs.uniform(0.01, 0.4, 2) for _ in range(n_sets)] if fun == "genReLU" else None
    labels = rs.integers(0, c, n)
    ctx = _context(x, sets, bn.ActFun(fun=fun, prm=np.zeros(2)).device_kind() if fun == "genReLU" else capi.ACT_TANH)
    try:
        stack = ctx.predict_sets(sets, act_prm_sets=slopes)
        for mode in (0, 1):
            want = posterior._summarise(stack, mode)
            summary, table = ctx.predict_sets_summary(sets, mode, labels=labels, act_prm_sets=slopes)
            only_table = ctx.predict_sets_summary(sets, mode, labels=labels, act_prm_sets=slopes, want_summary=False)
            only_summary = ctx.predict_sets_summary(sets, mode, act_prm_sets=slopes)
            assert only_table[0] is None and only_summary[1] is None
            np.testing.assert_array_equal(only_table[1], table)
            np.testing.assert_array_equal(only_summary[0], summary)
            assert table.dtype == np.int64 and table.sum() == n
            err = np.max(np.abs(summary - want))
            print("S=%d %s %dx%d mode %d: max |device - host| = %g" % (n_sets, fun, n, c, mode, err))
            if mode == 0:
                np.testing.assert_array_equal(summary, want)
                np.testing.assert_array_equal(table, _table(want, labels))
            else:
                # any order of float64 addition of S values in [0, 1] stays within S * 2^-53 (derived, not measured); the device
                # adds in the host's order (set after set), so equality is what is expected - and it holds on every case here
                assert err <= n_sets * 2.0 ** -53
                np.testing.assert_array_equal(summary, want)
                np.testing.assert_array_equal(table, _table(summary, labels))
    finally:
        ctx.close()


@pytest.mark.parametrize("n_sets", [1, 4])
def test_ties_go_to_the_first_class(n_sets):
    """Classes 1 and 3 share their last-layer weights: equal probabilities in every row and set.  Neither the votes nor the argmax of
    the summary may ever name class 3."""
    n, c = 1000, 5
    rs = np.random.default_rng(21)
    x = rs.standard_normal((n, 24))
    sets = _sets(n_sets, c=c, f=24, seed=9, tie=(1, 3))
    labels = rs.integers(0, c, n)
    ctx = _context(x, sets)
    try:
        stack = ctx.predict_sets(sets)
        np.testing.assert_array_equal(stack[:, :, 1], stack[:, :, 3])
        for mode in (0, 1):
            summary, table = ctx.predict_sets_summary(sets, mode, labels=labels)
            np.testing.assert_array_equal(summary, posterior._summarise(stack, mode))
            assert table[:, 3].sum() == 0 and table[:, 1].sum() > 0
            if mode == 0:
                assert not summary[:, 3].any()
            else:
                np.testing.assert_array_equal(summary[:, 1], summary[:, 3])
            np.testing.assert_array_equal(table, _table(summary, labels))
    finally:
        ctx.close()


def _same_by_existing_rule(order, values, want_order, want_values, n_rows):
    """test_hip_posterior.test_feature_importance_matches_reference's rule: values within 1.5 / N, or two neighbours of the ranking
    swapped by a one-instance near-tie."""
    if np.array_equal(order, want_order):
        np.testing.assert_allclose(values, want_values, atol=1.5 / n_rows, rtol=0)
    else:
        np.testing.assert_allclose(np.sort(values[:, 0]), np.sort(want_values[:, 0]), atol=1.5 / n_rows, rtol=0)


@pytest.mark.parametrize("name", ic.CASES)
def test_feature_importance_matches_reference_on_both_routes(name, monkeypatch):
    g = ic.load()
    monkeypatch.delenv("NPBNN_FI_HOST", raising=False)
    for mode, unlink, tag in ic.combinations():
        k = ic.key(name, mode, unlink, tag)
        order, values, df = ic.run(bn, name, mode, unlink, tag)
        _same_by_existing_rule(order, values, g[k + "/index"], g[k + "/values"], ic.N_ROWS)
        monkeypatch.setenv("NPBNN_FI_HOST", "1")
        _, _, df_host = ic.run(bn, name, mode, unlink, tag)
        monkeypatch.delenv("NPBNN_FI_HOST")
        assert df.equals(df_host), k                     # both routes rest on the same float32 predictions


def test_feature_importance_uploads_the_matrix_once(monkeypatch):
    calls = {"set_data": 0, "permute_columns": 0, "predict_sets": 0}
    for name in calls:
        def wrapped(self, *a, _f=getattr(HipContext, name), _n=name, **kw):
            calls[_n] += 1
            return _f(self, *a, **kw)
        monkeypatch.setattr(HipContext, name, wrapped)
    monkeypatch.delenv("NPBNN_FI_HOST", raising=False)
    ic.run(bn, "tanh", 1, True, "dict")
    assert calls == {"set_data": 1, "permute_columns": 1 + 3 * ic.N_PERMUTATIONS + 1, "predict_sets": 0}
    calls.update(set_data=0, permute_columns=0, predict_sets=0)
    monkeypatch.setenv("NPBNN_FI_HOST", "1")
    ic.run(bn, "tanh", 1, True, "dict")
    assert calls == {"set_data": 1 + 3 * ic.N_PERMUTATIONS, "permute_columns": 0, "predict_sets": 1 + 3 * ic.N_PERMUTATIONS}


def _raises(code, f, *a, **kw):
    with pytest.raises(capi.NpbnnError) as e:
        f(*a, **kw)
    assert e.value.code == code, e.value
    return str(e.value)


def test_errors():
    x, sets = _x(), _sets(3)
    rs = np.random.default_rng(1)
    perm = rs.permutation(N).reshape(1, -1)
    ctx, other = _context(x, sets), HipContext(0)
    try:
        base = ctx.predict_sets(sets)
        # a row index outside the matrix: found by the device-side check before anything is written
        for bad_value in (N, -1, 2 ** 40):
            bad = perm.copy()
            bad[0, 123] = bad_value
            assert "row index" in _raises(capi.E_ARG, ctx.permute_columns, [4, 9], bad)
            np.testing.assert_array_equal(ctx.predict_sets(sets), base)
        # ... also with a permutation in place: it stays
        ctx.permute_columns([4, 9], perm)
        moved = ctx.predict_sets(sets)
        bad = perm.copy()
        bad[0, 0] = N
        _raises(capi.E_ARG, ctx.permute_columns, [7], bad)
        np.testing.assert_array_equal(ctx.predict_sets(sets), moved)
        ctx.permute_columns([], None)
        np.testing.assert_array_equal(ctx.predict_sets(sets), base)
        # columns outside the matrix or named twice; a number of permutations that is neither one nor one per column
        _raises(capi.E_ARG, ctx.permute_columns, [F], perm)
        _raises(capi.E_ARG, ctx.permute_columns, [-1], perm)
        _raises(capi.E_ARG, ctx.permute_columns, [3, 3], perm)
        cols3 = np.array([1, 2, 3], dtype=np.int32)
        perm2 = np.ascontiguousarray(np.stack([perm[0], perm[0]]), dtype=np.int64)
        rc = ctx._lib.npbnn_permute_columns(ctx._ctx, capi.TRAIN, cols3.ctypes.data_as(C.POINTER(C.c_int32)), 3,
                                            perm2.ctypes.data_as(C.POINTER(C.c_int64)), 2)
        assert rc == capi.E_ARG
        np.testing.assert_array_equal(ctx.predict_sets(sets), base)
        # labels outside the classes, both outputs missing
        labels = rs.integers(0, 6, N)
        for bad_label in (6, -1):
            lab = labels.copy()
            lab[77] = bad_label
            assert "label" in _raises(capi.E_ARG, ctx.predict_sets_summary, sets, 0, labels=lab)
        packed = np.stack([pack_weights(w) for w in sets])
        rc = ctx._lib.npbnn_predict_sets_summary(ctx._ctx, capi.dptr(packed), None, 3, capi.TRAIN, 1, 0, None, None, None)
        assert rc == capi.E_ARG
        # set_data drops the saved columns: a restoring call afterwards has nothing to put back
        ctx.permute_columns([4, 9], perm)
        x2 = rs.standard_normal((N, F))
        ctx.set_data(x2)
        after_upload = ctx.predict_sets(sets)
        ctx.permute_columns([], None)
        np.testing.assert_array_equal(ctx.predict_sets(sets), after_upload)
        ref = _context(x2, sets)
        try:
            np.testing.assert_array_equal(after_upload, ref.predict_sets(sets))
        finally:
            ref.close()
        # a borrowed matrix, and an owner with borrowers
        other.share_data(ctx)
        _raises(capi.E_STATE, other.permute_columns, [1], perm)
        _raises(capi.E_STATE, ctx.permute_columns, [1], perm)
    finally:
        other.close()
        ctx.close()
