"""The three set-statistic folds on the GPU over their whole envelope: npbnn_predict_sets_lppd, npbnn_predict_sets_uncertainty and
npbnn_predict_sets_calibration on every case of fold_envelope_cases.CASES - row counts at the wave and workgroup edges, one to four
workgroups, widths that give every float4 and float2 loop a second and a later iteration, every pattern of groups the replay forms from
one to six sets, and the test table under a training table of another row count and other labels.

Every case is held to the float64 restatement of the entry's definition on the very float32 values predict_sets(apply_out_fn=False)
returns from the same context: deviation = |got - want| / max(1, |want|) over every floating-point field, printed before it is
asserted; the integer tables and the predicted class through test_hip_calibration._kernel_check, whose rule for rows that may fall
either way is kept as it is.  tests/test_host_fold_envelope.py shows on the CPU that a fold with a wrong vector, class, pair, partial,
reload, first set, label slot or row count lies at least 100 bounds away from these restatements on every case it can differ on.

Measured on an MI355X (fold_envelope_cases.MEASURED_DEVIATION; the bound is 10 x the figure, capped at 1e-10), the largest deviation per
entry and its case:
  lppd          4.140e-15  targets_12 (twelve Gaussian terms per row; next targets_8 at 2.699e-15), 51 cases
  uncertainty   7.483e-15  runs_1_cat (one genReLU set with logits up to 49, where the restatement's unshifted lse(z) - sum p z
                           cancels; next runs_2_cat at 2.487e-15, classes_32 at 2.220e-15), 65 cases
  calibration   1.221e-15  runs_21_err (next runs_231_err at 8.882e-16), 65 cases
In test_route (both routes) the largest figures were 3.371e-15, 2.220e-15 and 8.535e-16; they are held to the same bounds."""
import numpy as np
import pytest

import fold_envelope_cases as fc
import lppd_cases as lc
import npbnn_amd as bn
from npbnn_amd import HipContext, _capi as capi
from test_hip_calibration import _kernel_check

pytestmark = pytest.mark.gpu

OUT_KINDS = {"cat": capi.OUT_SOFTMAX, "reg": capi.OUT_IDENTITY, "err": capi.OUT_SOFTPLUS_HALF}
ROUTES = {"default": {}, "streamed": {"NPBNN_FORCE_WIDE": "1"}}
PAIRS = [(e, n) for e in fc.ENTRIES for n in fc.cases_of(e)]
# per entry: the pointwise arrays of a call, and the totals that are sums over the rows with the pointwise array each sums
POINTWISE = {"lppd": ("lppd_i", "mean_log_lik_i", "p_waic_i"),
             "uncertainty": ("mean_prob", "predicted_class", "predictive_entropy_i", "expected_entropy_i", "mutual_information_i", "mean", "total_var",
                             "aleatoric_var", "epistemic_var"),
             "calibration": ("confidence", "predicted_class", "brier_i", "nll_i", "pit", "mean", "sq_err")}
SUMS = {"lppd": {"lppd": "lppd_i", "mean_log_lik": "mean_log_lik_i", "p_waic": "p_waic_i"},
        "uncertainty": {"predictive_entropy": "predictive_entropy_i", "expected_entropy": "expected_entropy_i", "mutual_information": "mutual_information_i",
                        "mean_avg": "mean", "total_var_avg": "total_var", "aleatoric_var_avg": "aleatoric_var", "epistemic_var_avg": "epistemic_var"},
        "calibration": {"brier": "brier_i", "nll": "nll_i", "mean_pit": "pit"}}


def _pairs_of(names):
    return [(e, n) for e in fc.ENTRIES for n in names if e in fc.CASES[n]["entries"]]


def _context(inp, entry):
    """One context with the table or tables, the labels or targets on every slot (uncertainty reads none and gets none) and the
    architecture; returns it with the slot the statistic is taken on."""
    case = inp["case"]
    ctx = HipContext(0)
    try:
        slots = [(capi.TRAIN, inp["x"], inp["labels"])]
        if case["train_rows"]:
            slots = [(capi.TRAIN, inp["train_x"], inp["train_labels"]), (capi.TEST, inp["x"], inp["labels"])]
        for which, x, labels in slots:
            ctx.set_data(x, which)
            if entry != "uncertainty":
                (ctx.set_labels if case["kind"] == "cat" else ctx.set_targets)(labels, which)
        ctx.set_arch_from_weights(inp["samples"][0]["weights"], fc.N_FEATURES, lc.act_for(bn, inp["fun"], len(inp["nodes"])).device_kind(),
                                  OUT_KINDS[case["kind"]], capi.LIK_NONE)
    except Exception:
        ctx.close()
        raise
    return ctx, slots[-1][0]


def _sets(inp):
    return [s["weights"] for s in inp["samples"]]


def _call(ctx, entry, inp, which, slopes="own", **kw):
    case = inp["case"]
    slopes = inp["slopes"] if isinstance(slopes, str) else slopes
    if entry == "lppd":
        return ctx.predict_sets_lppd(_sets(inp), capi.LIK_CATEGORICAL if case["kind"] == "cat" else capi.LIK_GAUSS, sigma_sets=inp["sigma"],
                                     act_prm_sets=slopes, which=which, **kw)
    if entry == "uncertainty":
        return ctx.predict_sets_uncertainty(_sets(inp), act_prm_sets=slopes, which=which, **kw)
    return ctx.predict_sets_calibration(_sets(inp), n_bins=case["n_bins"], levels=case["levels"], sigma_sets=inp["sigma"], act_prm_sets=slopes,
                                        which=which, **kw)


def _passes(groups):
    return len(groups), max(g for _, g in groups)


def _same_bytes(a, b, but=()):
    assert sorted(a) == sorted(b)
    for k in a:
        if k not in but:
            assert (a[k] is None and b[k] is None) or np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def _check(entry, name, wide=False):
    """A case on one context: its values, the entry, and every assertion of test_case; returns the deviation."""
    inp = fc.inputs(name)
    case, kind = inp["case"], fc.KINDS[inp["kind"]]
    n_rows, n_sets = case["rows"], case["sets"]
    ctx, which = _context(inp, entry)
    try:
        z = ctx.predict_sets(_sets(inp), act_prm_sets=inp["slopes"], which=which, apply_out_fn=False)
        got = _call(ctx, entry, inp, which)
        # (a last layer of more than one 16-output tile - 31 and 32 classes - takes the resident path's one-set builds: the runs of those
        # widths travel together on the weight-streamed route only, which test_route forces)
        alone = not wide and case["n_out"] > 16
        assert ctx.replay_info() == ((n_sets, 1) if alone else _passes(inp["groups"])), (name, ctx.replay_info(), inp["groups"])
        assert ctx.is_wide() == wide
    finally:
        ctx.close()
    assert z.shape == (n_sets, n_rows, case["n_out"]) and np.array_equal(z, z.astype(np.float32))      # (the float32 values themselves)
    want = fc.want_of(entry, name, z)
    if entry != "calibration":
        worst = fc.worst_deviation(got, want)
    else:
        # every pointwise value, and by _kernel_check's rule for rows that may fall either way the tables, the predicted class and the
        # scores that rest on them
        assert {k for k in got if got[k] is not None} == {k for k in want if want[k] is not None} | {"n_bins", "n_rows", "n_samples"} \
            | ({"levels"} if kind != "classification" else set())
        worst = _kernel_check(got, want, name, kind, fc.top_two_gap(z) if kind == "classification" else None)
        assert (got["n_samples"], got["n_rows"], got["n_bins"]) == (n_sets, n_rows, case["n_bins"])
        table = got["count"] if kind == "classification" else got["pit_hist"]
        assert np.all(np.asarray(table).reshape(-1, case["n_bins"]).sum(axis=1) == n_rows)
        if kind == "classification":
            assert got["n_correct"].sum() == round(got["accuracy"] * n_rows) == np.sum(got["predicted_class"] == inp["labels"])
            bins = np.minimum(case["n_bins"] - 1, np.floor(got["confidence"] * case["n_bins"]).astype(np.int64))
            np.testing.assert_allclose(got["sum_confidence"], np.bincount(bins, weights=got["confidence"], minlength=case["n_bins"]), rtol=1e-9, atol=0)
        else:
            np.testing.assert_allclose(got["rmse"] ** 2 * n_rows, got["sq_err"].sum(axis=0), rtol=1e-9, atol=0)
    if entry == "uncertainty":
        if kind == "classification":
            np.testing.assert_array_equal(got["predicted_class"], np.argmax(got["mean_prob"], axis=1))
        if kind == "regression":
            assert all(got[k] is None for k in ("aleatoric_var", "total_var", "aleatoric_var_avg", "total_var_avg"))
        if n_sets == 1:
            assert not got["mutual_information_i" if kind == "classification" else "epistemic_var"].any()
            assert (got["mutual_information"] if kind == "classification" else got["epistemic_var_avg"].max()) == 0.0
    # the totals are the sums of the device's own pointwise arrays (the averages times the row count)
    for total, field in SUMS[entry].items():
        if got.get(total) is not None and got.get(field) is not None:
            scale = 1 if entry == "lppd" else n_rows
            own = np.asarray(got[field]).sum(axis=0)
            if not np.all(np.isfinite(own)):             # (an infinite nll: held to the restatement's above)
                continue
            assert np.all(np.abs(np.asarray(got[total]) * scale - own) <= 1e-9 * np.abs(own)), (name, total)
    return worst


# ---- 1. every case against the definition on the same float32 values ----------------------------------------------------------------
@pytest.mark.parametrize("entry,name", PAIRS)
def test_case(entry, name):
    worst = _check(entry, name)
    print("fold envelope deviation %s %s: %.3e" % (entry, name, worst))
    assert worst <= fc.TOL[entry], (entry, name, worst)


# ---- 2. both routes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("entry,name", _pairs_of(fc.CROSSED + fc.TEST_TABLE + ("classes_31", "classes_32")))
def test_route(entry, name, route, monkeypatch):
    """The crossed edges and the test table on both routes; 31 and 32 classes, which only the weight-streamed route replays three sets
    at a time."""
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    worst = _check(entry, name, wide=route == "streamed")
    print("fold envelope deviation %s %s %s: %.3e" % (entry, name, route, worst))
    assert worst <= fc.TOL[entry], (entry, name, route, worst)


# ---- 3. the same bytes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,name", _pairs_of(("rows_513", "rows_769", "rows_513_classes_12", "rows_513_outputs_12")))
def test_same_bytes_without_pointwise(entry, name):
    """Three and four workgroups: every total and table of a call that leaves the pointwise arrays on the device."""
    inp = fc.inputs(name)
    ctx, which = _context(inp, entry)
    try:
        full = _call(ctx, entry, inp, which)
        lean = _call(ctx, entry, inp, which, pointwise=False)
    finally:
        ctx.close()
    assert all(lean[k] is None for k in POINTWISE[entry] if k in lean)
    _same_bytes(full, lean, but=POINTWISE[entry])


@pytest.mark.parametrize("entry,name", _pairs_of(fc.CROSSED))
def test_same_bytes_every_call(entry, name):
    """Two calls on one context and a third on a fresh one."""
    inp = fc.inputs(name)
    ctx, which = _context(inp, entry)
    try:
        a, b = _call(ctx, entry, inp, which), _call(ctx, entry, inp, which)
    finally:
        ctx.close()
    ctx, which = _context(inp, entry)
    try:
        c = _call(ctx, entry, inp, which)
    finally:
        ctx.close()
    _same_bytes(a, b)
    _same_bytes(a, c)


# six sets in passes of every pattern; the slope vectors tanh ignores differ from run to run
SIX = ((3, 3), (2, 3, 1), (1, 1, 3, 1), (1, 3, 2), (1, 2, 3), (2, 1, 2, 1), (1, 1, 1, 1, 1, 1))


@pytest.mark.parametrize("entry,name", _pairs_of(fc.GROUPING))
def test_grouping_same_bytes(entry, name):
    inp = fc.inputs(name)
    assert inp["fun"] == "tanh" and inp["slopes"] is None and len(inp["samples"]) == 6
    ctx, which = _context(inp, entry)
    try:
        results = []
        for runs in SIX:
            slopes = [np.full(2, 0.01 * (i + 1)) for i, run in enumerate(runs) for _ in range(run)]
            results.append(_call(ctx, entry, inp, which, slopes=slopes))
            assert ctx.replay_info() == (len(runs), max(runs)), runs
        together = _call(ctx, entry, inp, which)
        assert ctx.replay_info() == (2, 3)
    finally:
        ctx.close()
    for runs, res in zip(SIX, results):
        _same_bytes(together, res)
