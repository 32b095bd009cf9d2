"""Posterior uncertainty decomposition on the GPU: npbnn_predict_sets_uncertainty (the replay's float32 pre-output values folded into
float64 per-row accumulators, totals from per-workgroup partials) and ``get_posterior_uncertainty``, against the definition on the host
and against the reference's values (tests/golden/uncertainty.npz).

Two bounds are measured figures (they are printed by the tests before they are asserted):
  KERNEL_TOL  the kernels against ``posterior_uncertainty`` on the float64 outputs the host computes from the very float32 values
              ``predict_sets(apply_out_fn=False)`` returns: only exp / log rounding and the order of sums separate the two.  Deviation
              = |got - want| / max(1, |want|) over every pointwise value and every mean over the rows of every case.  Measured on an
              MI355X, per case: relu_h1_c2_s1 2.220e-16, tanh_h2_c4_s7 4.441e-16, swish_h3_c3_s4 2.220e-16, genrelu_h2_c10_s64
              6.661e-16, genrelu_h2_c4_s3 3.331e-16, tanh_h2_c10_s2 1.110e-15, relu_h2_c3_s64 2.220e-16, tanh_h2_reg1_s7 2.776e-17,
              swish_h1_reg3_s4 5.551e-17, genrelu_h3_reg3_s3 4.449e-16, relu_h2_reg4_s64 2.637e-16, tanh_h2_err2_s7 6.661e-16,
              genrelu_h2_err1_s3 4.742e-16, swish_h1_err3_s1 6.530e-16, relu_h3_err3_s7 4.400e-16; the grid-stride table (against
              the restatement) 1.221e-15, the largest.  The bound is 10 x that (the cap is 1e-10).
  POINT_TOL   pointwise values against the golden file on the default, float32 and weight-streamed paths: the float32 network is the
              error source.  Largest absolute deviation measured per path: 6.783e-06 (default), 5.725e-06 (f32), 6.783e-06
              (streamed), all in swish_h1_err3_s1 (predicted variances up to 22); next genrelu_h2_err1_s3 at 3.5e-06 to 4.4e-06,
              the largest classification case swish_h3_c3_s4 at 1.7e-06, every other case below 1.3e-06.  The bound is 4 x the worst
              path.
Means over the rows are held to the project's log-likelihood budget of 1e-4 relative (measured: 3.4e-07 at most, genrelu_h3_reg3_s3)."""
import pickle
import types

import numpy as np
import pytest

import npbnn_amd as bn
import uncertainty_cases as uc
from npbnn_amd import HipContext, _capi as capi
from npbnn_amd.backend import pack_weights

pytestmark = pytest.mark.gpu

PATHS = {"default": {}, "f32": {"NPBNN_L0": "f32"}, "streamed": {"NPBNN_FORCE_WIDE": "1"}}
BUDGET = 1e-4                                      # relative, README: the float32 forward pass against float64 on a log-likelihood
MEASURED_KERNEL_DEVIATION = 1.221e-15              # the grid-stride table; the largest case tanh_h2_c10_s2 at 1.110e-15
KERNEL_TOL = min(10 * MEASURED_KERNEL_DEVIATION, 1e-10)
MEASURED_POINT_DEVIATION = {"default": 6.783e-06, "f32": 5.725e-06, "streamed": 6.783e-06}    # swish_h1_err3_s1 on each path
POINT_TOL = 4 * max(MEASURED_POINT_DEVIATION.values())
OUT_KINDS = {"classification": capi.OUT_SOFTMAX, "regression": capi.OUT_IDENTITY, "regression-error": capi.OUT_SOFTPLUS_HALF}
OUT_FNS = {"classification": bn.SoftMax, "regression": bn.RegressTransform, "regression-error": bn.RegressTransformError}
CLASS_MEANS = tuple(uc.CLASS_TOTALS)
REGRESSION_ARRAYS = ("mean", "epistemic_var", "aleatoric_var", "total_var")


def _set_path(path, monkeypatch):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)


def _context(inp, kind):
    ctx = HipContext(0)
    ctx.set_data(inp["x"])
    ctx.set_arch_from_weights(inp["samples"][0]["weights"], inp["x"].shape[1], uc.act_for(bn, inp["fun"], len(inp["nodes"])).device_kind(),
                              OUT_KINDS[kind], capi.LIK_NONE)
    return ctx


def _call(ctx, inp, slopes="own", **kw):
    return ctx.predict_sets_uncertainty([s["weights"] for s in inp["samples"]],
                                        act_prm_sets=uc.slopes_of(inp) if isinstance(slopes, str) else slopes, **kw)


def _device_fields(kind):
    """The fields the device call itself returns (under "regression" the aleatoric part is the caller's)."""
    if kind == "classification":
        return uc.CLASS_FIELDS, CLASS_MEANS
    arrays = REGRESSION_ARRAYS if kind == "regression-error" else ("mean", "epistemic_var")
    return arrays, tuple(k + "_avg" for k in arrays)


def _deviation(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _golden(name):
    g = uc.load()
    want = {f: g[uc.key(name, f)] for f in uc.fields_of(name)}
    if uc.CASES[name]["kind"] != "cat":
        want["total_var"] = want["epistemic_var"] + want["aleatoric_var"]
    return want


# ---- 1. kernel arithmetic ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", uc.CASES)
def test_kernels_against_the_definition_on_the_same_float32_values(name):
    inp, kind = uc.inputs(name), uc.kind_of(name)
    ctx = _context(inp, kind)
    try:
        z = ctx.predict_sets([s["weights"] for s in inp["samples"]], act_prm_sets=uc.slopes_of(inp), apply_out_fn=False)
        got = _call(ctx, inp)
    finally:
        ctx.close()
    assert np.array_equal(z, z.astype(np.float32))                          # (the float32 values themselves)
    want = bn.posterior_uncertainty(uc.outputs_from_values(z, kind), kind, None if kind != "regression" else np.ones((len(z), z.shape[2])))
    arrays, means = _device_fields(kind)
    worst = max(_deviation(got[k], want[k]) for k in arrays + means)
    print("kernel deviation %s: %.3e" % (name, worst))
    assert worst <= KERNEL_TOL, (name, worst)
    if kind == "classification":
        np.testing.assert_array_equal(got["predicted_class"], np.argmax(got["mean_prob"], axis=1))
    if kind == "regression":
        assert got["aleatoric_var"] is None and got["total_var"] is None and got["aleatoric_var_avg"] is None and got["total_var_avg"] is None
    if len(z) == 1:
        assert not got["mutual_information_i" if kind == "classification" else "epistemic_var"].any()
        assert (got["mutual_information"] if kind == "classification" else got["epistemic_var_avg"].max()) == 0.0


# ---- 2. against the reference's numbers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", uc.CASES)
def test_golden_values_on_every_path(name, path, monkeypatch):
    _set_path(path, monkeypatch)
    inp, kind, want = uc.inputs(name), uc.kind_of(name), _golden(name)
    ctx = _context(inp, kind)
    try:
        got = _call(ctx, inp)
        assert ctx.is_wide() == (path == "streamed") and ctx.l0_mode() == ("f32" if path == "f32" else "f16-split")
    finally:
        ctx.close()
    arrays, means = _device_fields(kind)
    point = max(float(np.max(np.abs(got[f] - want[f]))) for f in arrays)
    rel = max(float(np.max(np.abs(got[m] - np.mean(want[f], axis=0)) / np.abs(np.mean(want[f], axis=0))))
              for f, m in zip(arrays[1:] if kind == "classification" else arrays, means) if np.all(np.mean(want[f], axis=0) != 0))
    print("golden deviation %s %s: pointwise %.3e, means over the rows %.3e" % (name, path, point, rel))
    assert rel <= BUDGET, (name, path, rel)
    assert point <= POINT_TOL, (name, path, point)


# ---- 3. grouping, 4. determinism -----------------------------------------------------------------------------------------------------
def _same_bytes(a, b):
    for k in a:
        assert (a[k] is None and b[k] is None) or np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("name", ["tanh_h2_c4_s7", "tanh_h2_err2_s7"])
def test_grouping_of_the_sets_does_not_matter(name):
    """Seven sets replayed as they come (groups of three, three and one) and with a distinct slope vector each, which splits them into
    groups of one (tanh ignores the slopes): the same bytes."""
    inp = uc.inputs(name)
    ctx = _context(inp, uc.kind_of(name))
    try:
        together = _call(ctx, inp)
        alone = _call(ctx, inp, slopes=[np.full(2, 0.01 * (i + 1)) for i in range(7)])
    finally:
        ctx.close()
    _same_bytes(together, alone)


@pytest.mark.parametrize("name", ["genrelu_h2_c10_s64", "relu_h2_reg4_s64", "relu_h3_err3_s7"])
def test_two_calls_give_the_same_bytes(name):
    inp, kind = uc.inputs(name), uc.kind_of(name)
    ctx = _context(inp, kind)
    try:
        a, b = _call(ctx, inp), _call(ctx, inp)
        lean = _call(ctx, inp, pointwise=False)
    finally:
        ctx.close()
    _same_bytes(a, b)
    arrays, means = _device_fields(kind)
    assert all(lean[k] is None for k in arrays) and lean.get("predicted_class") is None
    for m in means:
        np.testing.assert_array_equal(lean[m], a[m])


# ---- 5. grid-stride -------------------------------------------------------------------------------------------------------------------
def test_a_workgroup_takes_a_second_stride():
    """2048 * 256 + 77 rows: the smallest table at which a workgroup of the 2048-workgroup grid takes a second stride."""
    rs = np.random.default_rng(31)
    n, f, c, s = 2048 * 256 + 77, 4, 3, 4
    x = rs.standard_normal((n, f))
    teacher = [rs.normal(0, 0.8, (4, f + 1)), rs.normal(0, 0.8, (c, 5))]
    sets = [[t + rs.normal(0, 0.3, t.shape) for t in teacher] for _ in range(s)]
    ctx = HipContext(0)
    try:
        ctx.set_data(x)
        ctx.set_arch_from_weights(sets[0], f, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
        z = ctx.predict_sets(sets, apply_out_fn=False)
        got = ctx.predict_sets_uncertainty(sets)
    finally:
        ctx.close()
    want = uc.restatement(z, "classification")
    worst = max(_deviation(got[k], want[k]) for k in uc.CLASS_FIELDS)
    worst = max(worst, max(_deviation(got[m], np.mean(want[f_])) for m, f_ in uc.CLASS_TOTALS.items()))
    print("grid-stride kernel deviation: %.3e" % worst)
    assert worst <= KERNEL_TOL
    for m, f_ in uc.CLASS_TOTALS.items():
        assert abs(got[m] * n - got[f_].sum()) <= 1e-9 * abs(got[f_].sum()), m


# ---- 6. error paths through ctypes ------------------------------------------------------------------------------------------------------
def test_errors_launch_no_evaluation(monkeypatch):
    monkeypatch.setenv("NPBNN_FI_TIMING", "1")
    inp, reg, err = uc.inputs("tanh_h2_c4_s7"), uc.inputs("swish_h1_reg3_s4"), uc.inputs("tanh_h2_err2_s7")
    packed = np.stack([pack_weights(s["weights"]) for s in inp["samples"]])
    totals = np.zeros(3)

    def raw(ctx, packed, n_sets, totals, which=capi.TRAIN, handle="own", total=None, aleatoric=None):
        rc = ctx._lib.npbnn_predict_sets_uncertainty(ctx._ctx if handle == "own" else handle, capi.dptr(packed), None, n_sets, which, None, capi.dptr(total),
                                                     capi.dptr(aleatoric), None, capi.dptr(totals))
        return rc, ctx._lib.npbnn_last_error(ctx._ctx).decode(), ctx.info(capi.INFO_SUMMARY_PASS_NS), ctx.info(capi.INFO_UNCERTAINTY_FINAL_NS)

    ctx = _context(inp, "classification")
    try:
        rc, _, ns, fin = raw(ctx, packed, 7, totals)
        assert rc == 0 and ns > 0 and fin > 0 and totals[0] > 0             # (a call that runs leaves the time of its passes)
        rc, _, ns, _ = raw(ctx, packed, 7, totals, handle=None)
        assert rc == capi.E_ARG                                              # (no context: nothing to zero, nothing launched)
        for kw in (dict(n_sets=0), dict(n_sets=-1), dict(n_sets=7, which=2), dict(n_sets=7, which=-1), dict(n_sets=7, totals=None)):
            rc, msg, ns, fin = raw(ctx, packed, kw.pop("n_sets"), kw.pop("totals", totals), **kw)
            assert rc == capi.E_ARG and ns == 0 and fin == 0, kw
        rc, msg, ns, fin = raw(ctx, packed, 7, totals, which=capi.TEST)
        assert rc == capi.E_STATE and ns == 0 and fin == 0                   # no data on the test slot
        bad = packed.copy()
        bad[3, -1] = np.nan
        rc, msg, _, _ = raw(ctx, bad, 7, totals)
        assert rc == capi.E_ARG and "NaN" in msg
        with pytest.raises(capi.NpbnnError) as e:
            ctx.predict_sets_uncertainty(bad)
        assert e.value.code == capi.E_ARG
        rc, _, ns, fin = raw(ctx, packed, 7, totals)
        assert rc == 0 and ns > 0 and fin > 0
    finally:
        ctx.close()
    ctx = HipContext(0)
    try:
        ctx.set_data(inp["x"])
        rc, msg, ns, fin = raw(ctx, packed, 7, totals)
        assert rc == capi.E_STATE and "set_arch" in msg and ns == 0 and fin == 0
    finally:
        ctx.close()
    # an odd number of outputs cannot be means and sigmas
    ctx = _context(reg, "regression-error")
    packed = np.stack([pack_weights(s["weights"]) for s in reg["samples"]])
    totals = np.zeros((4, 3))
    try:
        rc, msg, ns, fin = raw(ctx, packed, 4, totals)
        assert rc == capi.E_ARG and "odd" in msg and ns == 0 and fin == 0
    finally:
        ctx.close()
    # the identity output predicts no sigma
    ctx = _context(reg, "regression")
    point = np.zeros((uc.N_ROWS, 3))
    try:
        rc, msg, ns, fin = raw(ctx, packed, 4, totals, aleatoric=point)
        assert rc == capi.E_ARG and "aleatoric" in msg and ns == 0 and fin == 0
        rc, msg, ns, fin = raw(ctx, packed, 4, totals, total=point)
        assert rc == capi.E_ARG and ns == 0 and fin == 0
        rc, _, ns, fin = raw(ctx, packed, 4, totals)
        assert rc == 0 and ns > 0 and fin > 0 and not totals[1:3].any() and totals[3].min() > 0
    finally:
        ctx.close()
    ctx = _context(err, "regression-error")
    packed = np.stack([pack_weights(s["weights"]) for s in err["samples"]])
    totals, point = np.zeros((4, 2)), np.zeros((uc.N_ROWS, 2))
    try:
        rc, _, ns, fin = raw(ctx, packed, 7, totals, aleatoric=point)
        assert rc == 0 and ns > 0 and fin > 0
        np.testing.assert_allclose(point.sum(axis=0), totals[2], rtol=1e-12)
        np.testing.assert_allclose(totals[1], totals[2] + totals[3], rtol=1e-12)
    finally:
        ctx.close()


# ---- 7. checkpoints ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["genrelu_h2_c10_s64", "swish_h3_c3_s4", "genrelu_h3_reg3_s3", "genrelu_h2_err1_s3", "tanh_h2_err2_s7"])
def test_get_posterior_uncertainty_on_a_checkpoint(name, path, monkeypatch, tmp_path):
    _set_path(path, monkeypatch)
    inp, kind, want = uc.inputs(name), uc.kind_of(name), _golden(name)
    model = types.SimpleNamespace(_data=inp["x"][:50], _test_data=inp["x"], _act_fun=uc.act_for(bn, inp["fun"], len(inp["nodes"])),
                                  _output_act_fun=OUT_FNS[kind], _estimation_mode=kind)
    pkl = str(tmp_path / "run.pkl")
    with open(pkl, "wb") as fh:
        pickle.dump([model, None, types.SimpleNamespace(_post_weight_samples=inp["samples"])], fh)
    res = bn.get_posterior_uncertainty(pkl)
    assert (res["n_samples"], res["n_rows"]) == (uc.CASES[name]["s"], uc.N_ROWS)
    if kind == "classification":
        assert max(float(np.max(np.abs(res[f] - want[f]))) for f in uc.CLASS_FIELDS) <= POINT_TOL
        for m, f in uc.CLASS_TOTALS.items():
            assert abs(res[m] - want[f].mean()) <= BUDGET * want[f].mean(), m
        np.testing.assert_array_equal(res["predicted_class"], np.argmax(res["mean_prob"], axis=1))
        flips = res["predicted_class"] != np.argmax(want["mean_prob"], axis=1)      # (only where the two largest means are within the bound)
        top2 = np.sort(want["mean_prob"], axis=1)[:, -2:]
        assert np.all(top2[flips, 1] - top2[flips, 0] <= 2 * POINT_TOL)
    else:
        assert max(float(np.max(np.abs(res[f] - want[f]))) for f in REGRESSION_ARRAYS) <= POINT_TOL
        for f in REGRESSION_ARRAYS:
            ref = want[f].mean(axis=0)
            assert np.all(np.abs(res[f + "_avg"] - ref) <= BUDGET * np.abs(ref)), f
        np.testing.assert_array_equal(res["total_var"], res["epistemic_var"] + res["aleatoric_var"])
    train = bn.get_posterior_uncertainty(pkl, features="train", pointwise=False)
    assert train["n_rows"] == 50 and not any(k in train for k in uc.CLASS_FIELDS + REGRESSION_ARRAYS + ("predicted_class",))
    assert np.all(np.isfinite(train["mutual_information" if kind == "classification" else "total_var_avg"]))
