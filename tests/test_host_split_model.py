"""CPU: the numpy model of the fp16-split first layer (tests/split_model.py) on every table pair of tests/scale_cases.py.

Two things are pinned for the device test (tests/test_hip_test_table_scales.py), which runs the same tables:

  * the inputs are fair: on every kind, variant and network the FLOAT32 model of layer 0 stays inside half of the prediction bar
    (2e-5 * max(1, |value|)) and half of the log-likelihood bar (2e-6 relative) - so a device result outside the bars is the pair's
    doing, not the table's;
  * the state ensure_x16's rules give the test table of each kind, and with it the layer-0 mode the device test asserts.

The model of the pair path shows what the rule for a table that did not give the scales is for: with small weights on a column whose
scaled entries are large, a weight's absolute floor of 2^-25 times the entry leaves the bar (col_x1e3, col_x1e4, one_entry_2e5), while
every table the rule keeps on the pair stays inside it."""
import numpy as np
import pytest

import oracle as orc
import scale_cases as sc
import split_model as sm

LL_RTOL = 2e-6
TANH = orc.Act("tanh")


def _oracle(net, x32, w):
    x64 = x32.astype(np.float64)
    if net == "linear":
        return orc.forward(x64, w, TANH, orc.out_identity), None
    return orc.forward(x64, w, TANH, orc.out_softmax), orc.forward_logits(x64, w, TANH)


def _model(net, x32, w, path, scales=None):
    z0 = sm.l0_f32(x32, w[0][:, 1:], accumulate=True) if path == "f32" else sm.l0_pair(x32, w[0][:, 1:], *scales)
    return sm.finish(z0, w, sc.F)


def _errors(net, x32, lab, w, path, scales=None):
    """(prediction error / bar, log-likelihood error / bar) of a model path against the float64 oracle."""
    y64, z64 = _oracle(net, x32, w)
    z = _model(net, x32, w, path, scales)
    if net == "linear":
        return sm.scaled_error(z, y64) / sm.Z_BAR, 0.0
    pred = max(sm.scaled_error(z, z64), sm.scaled_error(sm.softmax(z), y64)) / sm.Z_BAR
    want = orc.lik_categorical(y64, lab, np.arange(len(lab)))
    return pred, abs(sm.loglik_categorical(z, lab) - want) / abs(want) / LL_RTOL


def test_a_wide_table_drawn_like_its_training_table_stays_on_the_pair():
    """1024 N(0, 1) columns, 11 200 training and 6 400 test rows (test_hip_wide_tables' shapes): a fifth of the test columns exceed the
    training column's power of two, by a few per cent each.  The rule counts the excess over 1, not those maxima themselves - as a sum
    they pass the bound that one column of 168 times the training range meets."""
    x = np.random.default_rng(7).standard_normal((11200 + 6400, 1024)).astype(np.float32)
    xs = sm.ensure_scales(x[:11200])[0]
    m = sm.col_absmax(x[11200:]).astype(np.float64) * xs
    assert m[m > 1.0].sum() > sm.FLOOR_S
    assert sm.weight_floor_sum(x[11200:], xs) < sm.FLOOR_S / 4
    assert sm.table_state(x[11200:], xs, False)[0] == sm.USABLE


@pytest.mark.parametrize("net", list(sc.NETS))
@pytest.mark.parametrize("variant", sc.VARIANTS, ids=sc.variant_id)
def test_float32_model_is_inside_half_the_bars(variant, net):
    kind, small = variant
    x_tr, x_te = sc.tables(kind)
    lab_tr, lab_te = sc.labels()
    for x32, lab in ((x_tr, lab_tr), (x_te, lab_te)):
        for w in sc.weight_sets(net, kind, small):
            pred, ll = _errors(net, x32, lab, w, "f32")
            assert pred <= 0.5, (kind, small, net, pred)
            assert ll <= 0.5, (kind, small, net, ll)


# the state of the test table the device test relies on (it asserts the mode of the kinds scale_cases names; the rest are pinned here
# so that a change of the rules shows)
STATES = {
    "same": sm.USABLE, "col_x1e2": sm.USABLE, "col_x1e3": sm.WEIGHT_FLOOR, "col_x1e4": sm.WEIGHT_FLOOR, "all_x100": sm.WEIGHT_FLOOR,
    "one_entry_2e5": sm.WEIGHT_FLOOR, "one_entry_1e6": sm.OUT_OF_RANGE, "col_x1e-3": sm.POOR_COLUMN, "col_x1e-6": sm.POOR_COLUMN,
    "zero_in_training": sm.USABLE, "zero_in_training_x1000": sm.WEIGHT_FLOOR, "col_zero_in_test": sm.USABLE,
}


@pytest.mark.parametrize("kind", list(sc.KINDS))
def test_state_of_the_test_table(kind):
    x_tr, x_te = sc.tables(kind)
    tr, te, shift = sm.states(x_tr, x_te)
    assert tr == sm.USABLE, "the training table left the pair"
    if kind in STATES:
        assert te == STATES[kind], (kind, te)
    expect = sc.KINDS[kind][4]
    if expect is not None:
        assert ("f16-split" if te == sm.USABLE else "f32") == expect
    if kind.startswith("moved_train"):
        assert (shift > 0).sum() > 0 and shift.max() <= sm.MAX_SHIFT
    else:
        assert not shift.any()


def test_the_tables_are_what_their_names_say():
    x_tr, x_te = sc.tables("one_entry_2e5")
    xs, ws, _, _ = sm.ensure_scales(x_tr)
    assert xs[sc.ECOL] == 0.25 and x_te[sc.ROW, sc.ECOL] * xs[sc.ECOL] == 5e4 < sm.F16_SAFE
    assert sc.tables("one_entry_1e6")[1][sc.ROW, sc.ECOL] * xs[sc.ECOL] > sm.F16_SAFE
    x_tr, x_te = sc.tables("zero_in_training")
    xs, ws, _, _ = sm.ensure_scales(x_tr)
    assert not x_tr[:, sc.COL].any() and xs[sc.COL] == 1.0 and ws[sc.COL] == 1.0 and x_te[:, sc.COL].any()
    assert not sc.tables("col_zero_in_test")[1][:, sc.COL].any()
    for kind in ("col_x1e-3", "col_x1e-6"):
        x_tr, x_te = sc.tables(kind)
        state, col, _ = sm.table_state(x_te, sm.ensure_scales(x_tr)[0], False)
        assert (state, col) == (sm.POOR_COLUMN, sc.COL)


def test_scales_and_split():
    rs = np.random.default_rng(0)
    m = np.array([0.0, 0.4999, 0.5, 1.0, 3.2, 4.0, np.inf], dtype=np.float32)
    xs, ws = sm.col_scale(m)
    np.testing.assert_array_equal(xs, np.array([1, 2, 1, 0.5, 0.25, 0.125, 1], dtype=np.float32))
    np.testing.assert_array_equal(xs * ws, np.ones(7, dtype=np.float32))
    np.testing.assert_array_equal(sm.col_scale(m[:6], np.array([0, 0, 0, 0, 3, 12]))[0][4:], np.array([2.0, 512.0], dtype=np.float32))
    v = (rs.standard_normal(20000) * 10.0 ** rs.uniform(-9, 4, 20000)).astype(np.float32)
    hi, lo = sm.split_f16(v)
    err = np.abs(v.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64))
    # 22 bits of the entry, or half of fp16's subnormal spacing once the low part is subnormal
    assert np.all(err <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25))
    assert err[np.abs(v) < 2.0 ** -3].max() > 2.0 ** -26        # (the floor is reached)
    assert abs(sm.FLOOR_S - 167.77216) < 1e-9


# (not the moved_train kinds: there the TRAINING table's own rule decides, which is not this module's subject.  With layer 0's weights
# divided by the columns' mean |value| the pair model of the log-normal training table itself reaches 0.86 (linear) and 1.49 (tanh) of
# the prediction bar, its log-normal test table 0.80 and 1.01: 33 of 40 columns sit near the 2^-17 bound at once - NOTES.md)
@pytest.mark.parametrize("net", list(sc.NETS))
@pytest.mark.parametrize("variant", [v for v in sc.VARIANTS if not v[0].startswith("moved_train")], ids=sc.variant_id)
def test_pair_model_is_inside_the_bar_wherever_the_rule_keeps_the_pair(variant, net):
    kind, small = variant
    x_tr, x_te = sc.tables(kind)
    lab_te = sc.labels()[1]
    xs, ws, _, _ = sm.ensure_scales(x_tr)
    state = sm.table_state(x_te, xs, False)[0]
    worst = max(_errors(net, x_te, lab_te, w, "pair", (xs, ws))[0] for w in sc.weight_sets(net, kind, small)) \
        if state != sm.OUT_OF_RANGE else np.inf
    if state == sm.USABLE:
        assert worst <= 0.5, (kind, small, net, worst)
    elif net == "linear" and small and kind in ("col_x1e3", "col_x1e4", "one_entry_2e5"):
        # what the rule is for: kept on the pair (as before the rule), these leave the bar
        assert worst > 1.0, (kind, worst)
