"""Posterior calibration on the GPU: npbnn_predict_sets_calibration (the replay's float32 pre-output values folded into float64 per-row
accumulators, integer tables counted exactly, floating-point sums from per-workgroup partials) and ``get_posterior_calibration``,
against the definition on the host and against the reference's values (tests/golden/calibration.npz).

Two bounds are measured figures (they are printed by the tests before they are asserted):
  KERNEL_TOL  the kernels against ``posterior_calibration`` on the float64 outputs the host computes from the very float32 values
              ``predict_sets(apply_out_fn=False)`` returns: only exp / log / erfc rounding and the order of sums separate the two.
              Deviation = |got - want| / max(1, |want|) over every pointwise value, sum_confidence and every score of every case.
              Measured on an MI355X, per case: relu_h1_c2_s1 2.776e-16, tanh_h2_c4_s7 3.331e-16, swish_h3_c3_s4 3.943e-16,
              genrelu_h2_c10_s64 5.051e-16, genrelu_h2_c4_s3 2.220e-16, tanh_h2_c10_s2 4.441e-16, relu_h2_c3_s64 2.430e-16,
              tanh_h2_reg1_s7 2.220e-16, swish_h1_reg3_s4 4.441e-16, genrelu_h3_reg3_s3 4.441e-16, relu_h2_reg4_s64 3.331e-16,
              tanh_h2_err2_s7 3.331e-16, genrelu_h2_err1_s3 1.110e-16, swish_h1_err3_s1 3.918e-16, relu_h3_err3_s7 4.441e-16; the
              grid-stride table (against the restatement; its scores are sums over half a million rows) 1.682e-14, the largest.
              The bound is 10 x that (the cap is 1e-10).
  POINT_TOL   pointwise values against the golden file on the default, float32 and weight-streamed paths: the float32 network is the
              error source.  Largest absolute deviation measured per path: 1.931e-05 (default), 6.710e-06 (f32), 1.931e-05
              (streamed), all in swish_h1_err3_s1; next swish_h3_c3_s4 at 4.4e-06 to 6.0e-06 and genrelu_h2_err1_s3 at 2.9e-06 to
              4.6e-06, every other case below 2.0e-06.  The bound is 4 x the worst path, the margin test_hip_uncertainty.py gives the
              same float32-network error.
Rows that may fall either way.  In test 1 a row whose host confidence or transform lies within 1e-12 of an edge, or whose two largest
mean probabilities differ by at most 1e-12 without being equal, is excused from the equality of the integer tables and of
``predicted_class``; more than 2 such rows in a case fail the test.  Rows whose two largest mean probabilities are exactly equal (the
four rows of relu_h1_c2_s1 on which every hidden unit is off: both logits are 0 and both means exactly 0.5 on the host and on the
device) are not excused and do not count: their class is the first one on both sides, and the test holds them to it."""
import pickle
import types

import numpy as np
import pytest

import npbnn_amd as bn
import calibration_cases as cc
from npbnn_amd import HipContext, _capi as capi
from npbnn_amd.backend import pack_weights

pytestmark = pytest.mark.gpu

PATHS = {"default": {}, "f32": {"NPBNN_L0": "f32"}, "streamed": {"NPBNN_FORCE_WIDE": "1"}}
BUDGET = 1e-4                                      # relative, README: the float32 forward pass against float64
MEASURED_KERNEL_DEVIATION = 1.682e-14              # the grid-stride table; the largest case genrelu_h2_c10_s64 at 5.051e-16
KERNEL_TOL = min(10 * MEASURED_KERNEL_DEVIATION, 1e-10)
MEASURED_POINT_DEVIATION = {"default": 1.931e-05, "f32": 6.710e-06, "streamed": 1.931e-05}    # swish_h1_err3_s1 on each path
POINT_TOL = 4 * max(MEASURED_POINT_DEVIATION.values())
EXCUSED = 1e-12
OUT_KINDS = {"classification": capi.OUT_SOFTMAX, "regression": capi.OUT_IDENTITY, "regression-error": capi.OUT_SOFTPLUS_HALF}
OUT_FNS = {"classification": bn.SoftMax, "regression": bn.RegressTransform, "regression-error": bn.RegressTransformError}
CHECKPOINT_CASES = ["genrelu_h2_c10_s64", "genrelu_h3_reg3_s3", "tanh_h2_err2_s7"]


def _set_path(path, monkeypatch):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)


def _context(inp, kind, labels=None):
    ctx = HipContext(0)
    ctx.set_data(inp["x"])
    ctx.set_arch_from_weights(inp["samples"][0]["weights"], inp["x"].shape[1], cc.act_for(bn, inp["fun"], len(inp["nodes"])).device_kind(),
                              OUT_KINDS[kind], capi.LIK_NONE)
    labels = inp["labels"] if labels is None else labels
    if kind == "classification":
        ctx.set_labels(labels)
    else:
        ctx.set_targets(labels)
    return ctx


def _call(ctx, inp, name, slopes="own", **kw):
    n_bins, levels = cc.params(name)
    return ctx.predict_sets_calibration([s["weights"] for s in inp["samples"]], n_bins=n_bins, levels=levels, sigma_sets=cc.sigmas_of(inp),
                                        act_prm_sets=cc.slopes_of(inp) if isinstance(slopes, str) else slopes, **kw)


def _tables(kind):
    return ("count", "n_correct") if kind == "classification" else cc.REGRESSION_TABLES


def _deviation(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    inf = np.isinf(want)
    assert np.array_equal(inf, np.isinf(got)) and np.array_equal(got[inf], want[inf])       # (an infinite nll is infinite on both sides)
    if inf.all():
        return 0.0
    return float(np.max(np.abs(got[~inf] - want[~inf]) / np.maximum(1.0, np.abs(want[~inf]))))


def _kernel_check(got, want, name, kind, top_two_gap=None):
    """Test 1's comparison of a device dict with the host definition's on the same values; returns the deviation."""
    value = want["confidence" if kind == "classification" else "pit"]
    excused = cc.rows_near_an_edge(name, value, EXCUSED)
    if top_two_gap is not None:
        close = (top_two_gap > 0) & (top_two_gap <= EXCUSED)
        excused += int(close.sum())
    assert excused <= 2, (name, excused)
    floats = [f for f in cc.point_fields_of(name) if f != "predicted_class"]
    worst = max(_deviation(got[f], want[f]) for f in floats)
    if excused == 0:
        for f in _tables(kind) + (("predicted_class",) if kind == "classification" else ()):
            np.testing.assert_array_equal(got[f], want[f], err_msg="%s %s" % (name, f))
        scores = [f for f in cc.score_fields_of(name) if want[f] is not None] + (["sum_confidence"] if kind == "classification" else [])
        worst = max([worst] + [_deviation(got[f], want[f]) for f in scores])
    else:
        for f in _tables(kind):
            assert np.abs(np.asarray(got[f]) - np.asarray(want[f])).sum() <= 2 * excused, (name, f)
        if kind == "classification":
            assert np.sum(got["predicted_class"] != want["predicted_class"]) <= excused, name
    return worst


def _golden_check(res, name, path, labels, flip=False):
    """Test 2's bounds of a device dict against the golden file; returns the largest pointwise deviation."""
    kind = cc.kind_of(name)
    n_bins, levels = cc.params(name)
    want = cc.golden_scores(name)
    if flip:
        want.update({f: want[f][::-1] for f in cc.point_fields_of(name) + (("top_two_gap",) if kind == "classification" else ())})
    floats = [f for f in cc.point_fields_of(name) if f != "predicted_class"]
    finite = {f: np.isfinite(want[f]) for f in floats}
    point = max(float(np.max(np.abs(res[f][finite[f]] - want[f][finite[f]]))) for f in floats)
    print("golden deviation %s %s: pointwise %.3e" % (name, path, point))
    assert point <= POINT_TOL, (name, path, point)
    # the device's tables are the tables of the device's own pointwise values
    if kind == "classification":
        lab = np.asarray(labels, dtype=np.int64)
        bins = np.minimum(n_bins - 1, np.floor(res["confidence"] * n_bins).astype(np.int64))
        np.testing.assert_array_equal(res["count"], np.bincount(bins, minlength=n_bins))
        np.testing.assert_array_equal(res["n_correct"], np.bincount(bins[res["predicted_class"] == lab], minlength=n_bins))
        np.testing.assert_allclose(res["sum_confidence"], np.bincount(bins, weights=res["confidence"], minlength=n_bins), rtol=1e-12, atol=0)
        m = cc.rows_near_an_edge(name, want["confidence"], POINT_TOL, want["top_two_gap"], 2 * POINT_TOL)
    else:
        bins = np.minimum(n_bins - 1, np.floor(res["pit"] * n_bins).astype(np.int64))
        for t in range(bins.shape[1]):
            np.testing.assert_array_equal(res["pit_hist"][t], np.bincount(bins[:, t], minlength=n_bins))
            for j, lv in enumerate(levels):
                assert res["covered"][t, j] == np.sum(np.abs(res["pit"][:, t] - 0.5) <= lv / 2)
        m = cc.rows_near_an_edge(name, want["pit"], POINT_TOL)
    assert m <= 4, (name, m)
    slack = POINT_TOL + 2.0 * m / cc.N_ROWS
    if kind == "classification":
        assert abs(res["ece"] - want["ece"]) <= slack, (name, path, res["ece"], want["ece"])
        for f in ("accuracy", "brier", "nll"):
            assert abs(res[f] - want[f]) <= BUDGET * abs(want[f]), (name, path, f, res[f], want[f])
    else:
        assert np.all(np.abs(res["coverage"] - want["coverage"]) <= slack), (name, path)
        assert np.all(np.abs(res["rmse"] - want["rmse"]) <= BUDGET * want["rmse"]), (name, path)
    return point


# ---- 1. kernel arithmetic ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.CASES)
def test_kernels_against_the_definition_on_the_same_float32_values(name):
    inp, kind = cc.inputs(name), cc.kind_of(name)
    n_bins, levels = cc.params(name)
    ctx = _context(inp, kind)
    try:
        z = ctx.predict_sets([s["weights"] for s in inp["samples"]], act_prm_sets=cc.slopes_of(inp), apply_out_fn=False)
        got = _call(ctx, inp, name)
    finally:
        ctx.close()
    assert np.array_equal(z, z.astype(np.float32))                          # (the float32 values themselves)
    y = cc.outputs_from_values(z, kind)
    want = bn.posterior_calibration(y, inp["labels"], kind, n_bins, levels, cc.sigmas_of(inp))
    gap = None
    if kind == "classification":
        top = np.sort(np.sum(y, axis=0) / len(y), axis=1)
        gap = top[:, -1] - top[:, -2]
    worst = _kernel_check(got, want, name, kind, gap)
    print("kernel deviation %s: %.3e" % (name, worst))
    assert worst <= KERNEL_TOL, (name, worst)
    assert sorted(got) == sorted(want)
    assert (got["n_samples"], got["n_rows"], got["n_bins"]) == (len(z), cc.N_ROWS, n_bins)


# ---- 2. against the reference's numbers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", cc.CASES)
def test_golden_values_on_every_path(name, path, monkeypatch):
    _set_path(path, monkeypatch)
    inp, kind = cc.inputs(name), cc.kind_of(name)
    ctx = _context(inp, kind)
    try:
        got = _call(ctx, inp, name)
        assert ctx.is_wide() == (path == "streamed") and ctx.l0_mode() == ("f32" if path == "f32" else "f16-split")
    finally:
        ctx.close()
    _golden_check(got, name, path, inp["labels"])


# ---- 3. grouping, 4. determinism -----------------------------------------------------------------------------------------------------
def _same_bytes(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert (a[k] is None and b[k] is None) or np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("name", ["tanh_h2_c4_s7", "tanh_h2_err2_s7"])
def test_grouping_of_the_sets_does_not_matter(name):
    """Seven sets replayed as they come (groups of three, three and one) and with a distinct slope vector each, which splits them into
    groups of one (tanh ignores the slopes): the same bytes in every field."""
    inp = cc.inputs(name)
    ctx = _context(inp, cc.kind_of(name))
    try:
        together = _call(ctx, inp, name)
        assert ctx.replay_info()[1] > 1
        alone = _call(ctx, inp, name, slopes=[np.full(2, 0.01 * (i + 1)) for i in range(7)])
        assert ctx.replay_info()[1] == 1
    finally:
        ctx.close()
    _same_bytes(together, alone)


@pytest.mark.parametrize("name", ["genrelu_h2_c10_s64", "relu_h2_reg4_s64", "relu_h3_err3_s7"])
def test_two_calls_give_the_same_bytes(name):
    inp, kind = cc.inputs(name), cc.kind_of(name)
    ctx = _context(inp, kind)
    try:
        a, b = _call(ctx, inp, name), _call(ctx, inp, name)
        lean = _call(ctx, inp, name, pointwise=False)
    finally:
        ctx.close()
    _same_bytes(a, b)
    assert sorted(lean) == sorted(a) and all(lean[k] is None for k in cc.point_fields_of(name))
    for k in a:
        if k not in cc.point_fields_of(name):
            assert (a[k] is None and lean[k] is None) or np.array_equal(np.asarray(lean[k]), np.asarray(a[k])), k


# ---- 5. grid-stride -------------------------------------------------------------------------------------------------------------------
def test_a_workgroup_takes_a_second_stride():
    """2048 * 256 + 77 rows: the smallest table at which a workgroup of the 2048-workgroup grid takes a second stride."""
    rs = np.random.default_rng(41)
    n, f, c, s, n_bins = 2048 * 256 + 77, 4, 3, 4, 15
    x = rs.standard_normal((n, f))
    teacher = [rs.normal(0, 0.8, (4, f + 1)), rs.normal(0, 0.8, (c, 5))]
    sets = [[t + rs.normal(0, 0.3, t.shape) for t in teacher] for _ in range(s)]
    labels = rs.integers(0, c, n)
    ctx = HipContext(0)
    try:
        ctx.set_data(x)
        ctx.set_labels(labels)
        ctx.set_arch_from_weights(sets[0], f, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
        z = ctx.predict_sets(sets, apply_out_fn=False)
        got = ctx.predict_sets_calibration(sets, n_bins=n_bins)
    finally:
        ctx.close()
    want = cc.restatement(z, labels, "classification", None, n_bins, ())
    floats = ("confidence", "brier_i", "nll_i", "sum_confidence", "brier", "nll", "accuracy", "ece", "mce")
    worst = max(_deviation(got[k], want[k]) for k in floats)
    print("grid-stride kernel deviation: %.3e" % worst)
    assert worst <= KERNEL_TOL
    edges = np.arange(1, n_bins) / n_bins
    top = np.sort(cc.outputs_from_values(z, "classification").mean(axis=0), axis=1)
    excused = int(np.sum(np.min(np.abs(want["confidence"][:, None] - edges[None, :]), axis=1) <= EXCUSED) + np.sum(top[:, -1] - top[:, -2] <= EXCUSED))
    assert excused <= 2
    if excused == 0:
        for k in ("count", "n_correct", "predicted_class"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["count"].sum() == n and got["n_correct"].sum() == round(got["accuracy"] * n) == np.sum(got["predicted_class"] == labels)


# ---- 6. extremes ------------------------------------------------------------------------------------------------------------------------
def test_targets_a_million_sigmas_away():
    """Two targets of an ordinary regression case replaced by +-1e6: their transforms are exactly 1 and 0, in the last and the first
    bin, covered at no level; every other value of the case stays what it was."""
    name = "relu_h2_reg4_s64"
    inp = cc.inputs(name)
    n_bins, levels = cc.params(name)
    far = inp["labels"].copy()
    far[0, 0], far[1, 2] = 1e6, -1e6
    ctx = _context(inp, "regression")
    try:
        plain = _call(ctx, inp, name)
        ctx.set_targets(far)
        got = _call(ctx, inp, name)
    finally:
        ctx.close()
    assert got["pit"][0, 0] == 1.0 and got["pit"][1, 2] == 0.0 and np.all(np.isfinite(got["sq_err"]))
    moved = np.zeros(far.shape, dtype=bool)
    moved[0, 0] = moved[1, 2] = True
    for f in ("pit", "mean", "sq_err"):
        np.testing.assert_array_equal(got[f][~moved], plain[f][~moved])
    np.testing.assert_array_equal(got["mean"], plain["mean"])
    d = 1e6 - got["mean"][0, 0]
    assert got["sq_err"][0, 0] == d * d
    bins = np.minimum(n_bins - 1, np.floor(plain["pit"] * n_bins).astype(np.int64))
    in_level = np.abs(plain["pit"] - 0.5)[:, :, None] <= (np.array(levels) / 2)[None, None, :]
    for (r, t), b in (((0, 0), n_bins - 1), ((1, 2), 0)):
        hist = plain["pit_hist"][t].copy()
        hist[bins[r, t]] -= 1
        hist[b] += 1
        np.testing.assert_array_equal(got["pit_hist"][t], hist)
        np.testing.assert_array_equal(got["covered"][t], plain["covered"][t] - in_level[r, t])
    for t in (1, 3):
        np.testing.assert_array_equal(got["pit_hist"][t], plain["pit_hist"][t])
        np.testing.assert_array_equal(got["covered"][t], plain["covered"][t])


# ---- 7. error paths through ctypes ------------------------------------------------------------------------------------------------------
def test_errors_launch_no_evaluation(monkeypatch):
    monkeypatch.setenv("NPBNN_FI_TIMING", "1")
    cat, reg, err = cc.inputs("tanh_h2_c4_s7"), cc.inputs("swish_h1_reg3_s4"), cc.inputs("tanh_h2_err2_s7")
    i64 = capi.C.POINTER(capi.C.c_int64)

    def raw(ctx, inp, n_out_cols, softmax, n_sets=None, which=capi.TRAIN, handle="own", sigma=None, n_bins=10, levels=(0.5, 0.9), n_levels=None,
            totals="own", counts="own", bin_sums="own", pred=None, packed=None):
        packed = np.stack([pack_weights(s["weights"]) for s in inp["samples"]]) if packed is None else packed
        lv = np.asarray(levels, dtype=np.float64)
        n_levels = len(lv) if n_levels is None else n_levels
        totals = np.zeros(3 if softmax else (2, n_out_cols)) if isinstance(totals, str) else totals
        counts = np.zeros((2, 64) if softmax else (n_out_cols, 64 + 16), dtype=np.int64) if isinstance(counts, str) else counts
        bin_sums = (np.zeros(64) if softmax else None) if isinstance(bin_sums, str) else bin_sums
        sigma = None if sigma is None else capi.as_f64(sigma)
        rc = ctx._lib.npbnn_predict_sets_calibration(
            ctx._ctx if handle == "own" else handle, capi.dptr(packed), None, len(packed) if n_sets is None else n_sets, which, capi.dptr(sigma), n_bins,
            capi.dptr(lv) if len(lv) else None, n_levels, None, None, None, None if pred is None else pred.ctypes.data_as(i64),
            None if counts is None else counts.ctypes.data_as(i64), capi.dptr(bin_sums), capi.dptr(totals))
        return rc, ctx._lib.npbnn_last_error(ctx._ctx).decode(), ctx.info(capi.INFO_SUMMARY_PASS_NS), ctx.info(capi.INFO_CALIBRATION_FINAL_NS)

    def refused(ctx, inp, cols, softmax, code, **kw):
        rc, msg, ns, fin = raw(ctx, inp, cols, softmax, **kw)
        assert rc == code and ns == 0 and fin == 0, (kw, rc, msg, ns, fin)
        return msg

    ctx = _context(cat, "classification")
    try:
        rc, _, ns, fin = raw(ctx, cat, 1, True)
        assert rc == 0 and ns > 0 and fin > 0                                  # (a call that runs leaves the time of its passes)
        assert raw(ctx, cat, 1, True, handle=None)[0] == capi.E_ARG            # (no context: nothing to zero, nothing launched)
        for kw in (dict(n_sets=0), dict(n_sets=-1), dict(which=2), dict(which=-1), dict(n_bins=0), dict(n_bins=65), dict(n_levels=-1), dict(n_levels=17),
                   dict(levels=(0.0,)), dict(levels=(0.5, 1.0)), dict(levels=(np.nan,)), dict(levels=(-0.1,)), dict(totals=None), dict(counts=None),
                   dict(bin_sums=None), dict(sigma=np.ones((7, 4)))):
            refused(ctx, cat, 1, True, capi.E_ARG, **kw)
        refused(ctx, cat, 1, True, capi.E_STATE, which=capi.TEST)              # no data on the test slot
        ctx.set_labels(np.where(np.arange(cc.N_ROWS) == 200, 4, cat["labels"]))
        assert "label" in refused(ctx, cat, 1, True, capi.E_ARG)               # a label outside [0, 4)
        ctx.set_labels(cat["labels"])
        bad = np.stack([pack_weights(s["weights"]) for s in cat["samples"]])
        bad[3, -1] = np.nan
        rc, msg, _, _ = raw(ctx, cat, 1, True, packed=bad)
        assert rc == capi.E_ARG and "NaN" in msg
        with pytest.raises(capi.NpbnnError) as e:
            ctx.predict_sets_calibration(bad)
        assert e.value.code == capi.E_ARG
        rc, _, ns, fin = raw(ctx, cat, 1, True)
        assert rc == 0 and ns > 0 and fin > 0
    finally:
        ctx.close()
    ctx = HipContext(0)
    try:
        ctx.set_data(cat["x"])
        assert "set_arch" in refused(ctx, cat, 1, True, capi.E_STATE)
        ctx.set_arch_from_weights(cat["samples"][0]["weights"], cc.N_FEATURES, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
        assert "labels" in refused(ctx, cat, 1, True, capi.E_STATE)            # no labels on the table
    finally:
        ctx.close()
    # an odd number of outputs cannot be means and sigmas
    ctx = _context(reg, "regression-error")
    try:
        assert "odd" in refused(ctx, reg, 3, False, capi.E_ARG)
    finally:
        ctx.close()
    # the identity output takes its sigma from the caller
    sig = cc.sigmas_of(reg)
    ctx = _context(reg, "regression")
    try:
        refused(ctx, reg, 3, False, capi.E_ARG)                                # no sigma_sets
        for entry in (0.0, -1.0, np.inf, np.nan):
            worse = sig.copy()
            worse[2, 1] = entry
            assert "sigma" in refused(ctx, reg, 3, False, capi.E_ARG, sigma=worse)
        refused(ctx, reg, 3, False, capi.E_ARG, sigma=sig, bin_sums=np.zeros(64))
        refused(ctx, reg, 3, False, capi.E_ARG, sigma=sig, pred=np.zeros(cc.N_ROWS, dtype=np.int64))
        ctx.set_targets(reg["labels"][:, :2])
        assert "columns" in refused(ctx, reg, 3, False, capi.E_ARG, sigma=sig)    # targets of another width
        ctx.set_targets(reg["labels"])
        rc, _, ns, fin = raw(ctx, reg, 3, False, sigma=sig)
        assert rc == 0 and ns > 0 and fin > 0
    finally:
        ctx.close()
    ctx = HipContext(0)
    try:
        ctx.set_data(reg["x"])
        ctx.set_arch_from_weights(reg["samples"][0]["weights"], cc.N_FEATURES, capi.ACT_SWISH, capi.OUT_IDENTITY, capi.LIK_NONE)
        assert "targets" in refused(ctx, reg, 3, False, capi.E_STATE, sigma=sig)  # no targets on the table
    finally:
        ctx.close()
    # the softplus-half output predicts its own
    ctx = _context(err, "regression-error")
    try:
        refused(ctx, err, 2, False, capi.E_ARG, sigma=np.ones((7, 2)))
        totals, counts = np.zeros((2, 2)), np.zeros((2, 12), dtype=np.int64)
        rc, _, ns, fin = raw(ctx, err, 2, False, totals=totals, counts=counts)
        assert rc == 0 and ns > 0 and fin > 0
        assert np.all(counts[:, :10].sum(axis=1) == cc.N_ROWS) and np.all(counts[:, 10] <= counts[:, 11]) and totals.min() > 0
    finally:
        ctx.close()


# ---- 8. checkpoints ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", CHECKPOINT_CASES)
def test_get_posterior_calibration_on_a_checkpoint(name, path, monkeypatch, tmp_path):
    _set_path(path, monkeypatch)
    inp, kind = cc.inputs(name), cc.kind_of(name)
    n_bins, levels = cc.params(name)
    model = types.SimpleNamespace(_data=inp["x"][::-1].copy(), _labels=inp["labels"][::-1].copy(), _test_data=inp["x"], _test_labels=inp["labels"],
                                  _act_fun=cc.act_for(bn, inp["fun"], len(inp["nodes"])), _output_act_fun=OUT_FNS[kind], _estimation_mode=kind)
    pkl = str(tmp_path / "run.pkl")
    with open(pkl, "wb") as fh:
        pickle.dump([model, None, types.SimpleNamespace(_post_weight_samples=inp["samples"])], fh)
    res = bn.get_posterior_calibration(pkl, n_bins=n_bins, levels=levels)
    assert (res["n_samples"], res["n_rows"], res["n_bins"]) == (cc.CASES[name]["s"], cc.N_ROWS, n_bins)
    _golden_check(res, name, path, inp["labels"])
    _golden_check(bn.get_posterior_calibration(pkl, features="train", n_bins=n_bins, levels=levels), name, path, inp["labels"][::-1], flip=True)
    given = bn.get_posterior_calibration(pkl, features=inp["x"], labels=inp["labels"], n_bins=n_bins, levels=levels)
    _golden_check(given, name, path, inp["labels"])
    lean = bn.get_posterior_calibration(pkl, n_bins=n_bins, levels=levels, pointwise=False)
    assert not any(k in lean for k in cc.point_fields_of(name))
    for k in lean:
        assert (lean[k] is None and res[k] is None) or np.array_equal(np.asarray(lean[k]), np.asarray(res[k])), k
