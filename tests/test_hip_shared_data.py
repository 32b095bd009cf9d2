"""Feature matrices shared between contexts on the GPU (npbnn_share_data): the matrices, their fp16-split copies and the scales are
one store that every context using them holds, and that goes with the last of them - whichever context uploaded it, whichever built
a copy in it, and in whatever order they are closed.  Every result is compared bit for bit with a context that uploaded a private
copy of the same arrays with the same options, and every case checks (npbnn_get_info) that it ran on the path it means to test."""
import numpy as np
import pytest

import cases
from npbnn_amd import HipContext, _capi as capi

pytestmark = pytest.mark.gpu

N_TRAIN, N_TEST, F, HIDDEN, CLASSES = 300, 130, 40, 8, 3      # ragged last row tile in both tables; 40 features pad to 48 / 64
TABLES = (capi.TRAIN, capi.TEST)

_rs = np.random.default_rng(20)
X = {capi.TRAIN: _rs.standard_normal((N_TRAIN, F)), capi.TEST: _rs.standard_normal((N_TEST, F))}
LABELS = {capi.TRAIN: _rs.integers(0, CLASSES, N_TRAIN), capi.TEST: _rs.integers(0, CLASSES, N_TEST)}
X_OTHER = _rs.standard_normal((N_TRAIN + 21, F))
LABELS_OTHER = _rs.integers(0, CLASSES, N_TRAIN + 21)
W = [_rs.normal(0, 0.5, s) for s in cases.layer_shapes(F, [HIDDEN], CLASSES, 1)]


def _context(wide, source=None, train=None):
    """A context on the fp16-split layer 0, resident or weight-streamed: with the matrices of `source`, or with an upload of its own
    (`train`: (matrix, labels) in place of the module's training table, and no test table)."""
    ctx = HipContext(0)
    ctx.set_l0_precision("f16")
    ctx.set_wide(wide)
    if source is not None:
        ctx.share_data(source)
        tables = TABLES
    elif train is not None:
        ctx.set_data(train[0])
        tables = ()
        ctx.set_labels(train[1])
    else:
        for t in TABLES:
            ctx.set_data(X[t], t)
        tables = TABLES
    for t in tables:
        ctx.set_labels(LABELS[t], t)
    ctx.set_arch_from_weights(W, F, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_CATEGORICAL)
    return ctx


def _results(ctx, wide, tables=TABLES):
    """Likelihood, confusion table and predictions on every table, and the path they ran on."""
    out = []
    for t in tables:
        r = ctx.eval(W, which=t, want_confusion=True)
        assert ctx.info(capi.INFO_L0_F16) == 1 and ctx.info(capi.INFO_WIDE) == (1 if wide else 0)
        y = ctx.predict(W, which=t)
        assert ctx.info(capi.INFO_L0_F16) == 1 and ctx.info(capi.INFO_WIDE) == (1 if wide else 0)
        out.append((np.float64(r["loglik"]), r["confusion"], y))
    return out


def _assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            np.testing.assert_array_equal(a, b)


def _assert_finite(want):
    for res in want.values():
        for loglik, conf, y in res:
            assert np.isfinite(loglik) and np.isfinite(y).all() and conf.sum() in (N_TRAIN, N_TEST)


@pytest.fixture(scope="module")
def private():
    """What contexts with private copies give: {wide: results on both tables}."""
    want = {}
    for wide in (False, True):
        ctx = _context(wide)
        try:
            want[wide] = _results(ctx, wide)
        finally:
            ctx.close()
    _assert_finite(want)
    return want


def _raises(code, f, *a, **kw):
    with pytest.raises(capi.NpbnnError) as e:
        f(*a, **kw)
    assert e.value.code == code, e.value
    return str(e.value)


def test_lifetime_on_the_resident_path(private):
    owner = _context(False)
    b1, b2 = _context(False, owner), _context(False, owner)
    try:
        for ctx in (owner, b1, b2):
            _assert_same(_results(ctx, False), private[False])
        owner.close()
        for ctx in (b1, b2):
            _assert_same(_results(ctx, False), private[False])
        b1.close()
        _assert_same(_results(b2, False), private[False])
        # the last one is given a matrix of its own: it lets go of both tables and is a context like any other
        b2.set_data(X_OTHER)
        b2.set_labels(LABELS_OTHER)
        b2.set_arch_from_weights(W, F, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_CATEGORICAL)
        fresh = _context(False, train=(X_OTHER, LABELS_OTHER))
        try:
            _assert_same(_results(b2, False, (capi.TRAIN,)), _results(fresh, False, (capi.TRAIN,)))
        finally:
            fresh.close()
        assert "no data matrix" in _raises(capi.E_STATE, b2.eval, W, which=capi.TEST)      # (the test table went back too)
    finally:
        for ctx in (owner, b1, b2):
            ctx.close()


def test_lifetime_on_the_weight_streamed_path(private):
    owner = _context(False)          # resident: it never builds the piece-ordered split copy
    b1, b2 = _context(True, owner), _context(True, owner)
    try:
        _assert_same(_results(owner, False), private[False])
        _assert_same(_results(b1, True), private[True])          # builds the piece-ordered copy into the shared store
        owner.close()
        _assert_same(_results(b2, True), private[True])
        b1.close()                                                 # the context that built the copy
        _assert_same(_results(b2, True), private[True])
    finally:
        for ctx in (owner, b1, b2):
            ctx.close()


def test_borrower_of_a_borrower(private):
    a = _context(False)
    b = _context(False, a)
    c = _context(False, b)
    try:
        a.close()
        b.close()
        _assert_same(_results(c, False), private[False])
    finally:
        for ctx in (a, b, c):
            ctx.close()


def test_refusals():
    perm = np.random.default_rng(4).permutation(N_TRAIN)
    owner = _context(False)
    b1, b2 = _context(False, owner), _context(False, owner)
    spare = _context(False)
    try:
        msg = _raises(capi.E_STATE, owner.set_data, X[capi.TRAIN])
        assert "2 other context(s) use this one's matrices (npbnn_share_data)" in msg
        assert "2 other context(s) use this one's matrices" in _raises(capi.E_STATE, owner.share_data, spare)
        assert "borrow from each other" in _raises(capi.E_ARG, owner.share_data, b1)
        assert "bad arguments" in _raises(capi.E_ARG, owner.share_data, owner)
        assert "bad arguments" in _raises(capi.E_ARG, b1.share_data, b1)
        assert "use this one's matrices" in _raises(capi.E_STATE, owner.permute_columns, [1], perm)
        assert "belong to another one" in _raises(capi.E_STATE, b1.permute_columns, [1], perm)
        empty = HipContext(0)
        try:
            assert "no training matrix" in _raises(capi.E_STATE, b1.share_data, empty)
        finally:
            empty.close()
        b2.close()
        assert "1 other context(s)" in _raises(capi.E_STATE, owner.set_data, X[capi.TRAIN])
        # the borrowers gone, the owner is a context like any other again
        b1.share_data(spare)
        owner.permute_columns([1], perm)
        owner.permute_columns([], None)
        owner.set_data(X_OTHER)
        # a borrower stays one after the uploader is closed
        spare.close()
        assert "belong to another one" in _raises(capi.E_STATE, b1.permute_columns, [1], perm)
    finally:
        for ctx in (owner, b1, b2, spare):
            ctx.close()
