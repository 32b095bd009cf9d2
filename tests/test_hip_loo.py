"""PSIS-LOO on the GPU: npbnn_op_psis (``device_ops.psis``) against ``posterior_loo``, npbnn_predict_sets_loo against the definition
on the matrix it returns and against npbnn_predict_sets_lppd, and ``get_posterior_loo`` on a checkpoint.

The bar of a case is worked out on the CPU from the case's own input (tests/loo_cases.py: 16 times the float64-to-longdouble
distance of the restatement, never below 16 * 2^-52 of the largest magnitude), per array.  MEASURED_DEVIATIONS below holds, per
group of cases, the largest device deviation seen on an MI355X and the smallest bar in the group (the tests print every figure
before they assert).  The matrix ``log_lik`` is held to test_hip_lppd.py's KERNEL_TOL rule against the float64 log-likelihoods the
host computes from the very float32 values ``predict_sets(apply_out_fn=False)`` returns."""
import functools
import pickle
import types

import numpy as np
import pytest

import loo_cases as lc
import lppd_cases as lpc
import npbnn_amd as bn
import test_hip_lppd as thl
from npbnn_amd import _capi as capi, device_ops
from npbnn_amd.backend import pack_weights
from npbnn_amd.hpd import stack_rows
from npbnn_amd.posterior import _SamplePredictor

pytestmark = pytest.mark.gpu

# Measured on an MI355X, all 106 tests of this file in 3.7 s: the largest device deviation / the smallest bar over the group's cases, for
# elpd_loo_i, lppd_i and the finite pareto_k (npbnn_op_psis: the 1, 3, 65 and 130 columns of a sample count together).  No case is
# over a third of its own bar; +inf in pareto_k sits in the same places everywhere.
MEASURED_DEVIATIONS = {
    "psis S=2 float64": ("8.9e-16 / 3.9e-14", "4.4e-16 / 3.1e-14", "every k +inf"),
    "psis S=2 float32": ("4.4e-16 / 3.9e-14", "4.4e-16 / 3.1e-14", "every k +inf"),
    "psis S=20 float64": ("1.8e-15 / 3.7e-14", "8.9e-16 / 2.3e-14", "every k +inf"),
    "psis S=20 float32": ("1.8e-15 / 3.7e-14", "8.9e-16 / 2.3e-14", "every k +inf"),
    "psis S=21 float64": ("1.3e-15 / 4.3e-14", "8.9e-16 / 3.4e-14", "6.4e-15 / 1.9e-13"),
    "psis S=21 float32": ("1.8e-15 / 4.3e-14", "8.9e-16 / 3.4e-14", "4.9e-15 / 1.5e-13"),
    "psis S=64 float64": ("1.8e-15 / 4.5e-14", "8.9e-16 / 3.4e-14", "1.0e-15 / 4.1e-14"),
    "psis S=64 float32": ("1.8e-15 / 4.5e-14", "4.4e-16 / 3.4e-14", "1.3e-15 / 4.2e-14"),
    "psis S=65 float64": ("1.8e-15 / 3.8e-14", "8.9e-16 / 3.1e-14", "4.0e-15 / 4.5e-14"),
    "psis S=65 float32": ("1.8e-15 / 3.8e-14", "8.9e-16 / 3.1e-14", "1.7e-15 / 1.5e-14"),
    "psis S=257 float64": ("6.2e-15 / 1.3e-13", "8.9e-16 / 2.7e-14", "2.9e-15 / 4.6e-14"),
    "psis S=257 float32": ("1.8e-14 / 1.1e-13", "8.9e-16 / 2.7e-14", "7.6e-15 / 6.0e-14"),
    "psis S=1025 float64": ("2.8e-14 / 4.3e-13", "1.8e-15 / 2.6e-14", "8.7e-15 / 1.5e-13"),
    "psis S=1025 float32": ("8.9e-15 / 2.8e-13", "8.9e-16 / 2.6e-14", "4.9e-15 / 1.2e-13"),
    "psis S=16384 float64": ("5.8e-15 / 2.5e-14", "0 / 1.8e-14", "1.5e-15 / 3.4e-14"),
    "psis S=16384 float32": ("5.3e-15 / 2.3e-14", "0 / 2.1e-14", "5.0e-15 / 5.4e-14"),
    "psis special columns": ("8.9e-16 / 3.6e-09", "0 / 3.6e-09", "4.4e-16 / 1.5e-14"),
    # npbnn_predict_sets_loo, the three paths of a case together (S <= 7: every k +inf)
    "entry genrelu_h2_c10_s64": ("7.1e-15 / 1.7e-13", "8.9e-16 / 6.4e-14", "6.2e-15 / 5.8e-14"),
    "entry relu_h2_c3_s64": ("3.6e-15 / 6.0e-14", "8.9e-16 / 1.4e-14", "3.7e-13 / 1.9e-12"),
    "entry relu_h2_reg4_s64": ("1.8e-15 / 3.7e-14", "8.9e-16 / 2.6e-14", "2.2e-15 / 2.5e-14"),
    "entry, the seven cases of 2 to 7 samples": ("1.8e-15 / 1.1e-14", "8.9e-16 / 1.0e-14", "every k +inf"),
    # log_lik and log_lik_sample against the host on the same float32 values, and lppd_i / log_lik_sample against
    # npbnn_predict_sets_lppd, |got - want| / max(1, |want|): 3.6e-15 and 8.9e-16 at most over the 30 (case, path) pairs (KERNEL_TOL 1.3e-13)
}
SAMPLE_COUNTS = (2, 20, 21, 64, 65, 257, 1025)
COLUMN_COUNTS = (1, 3, 65, 130)
LOO_CASES = [n for n, c in lpc.CASES.items() if c["s"] >= 2]      # S in 2, 3, 4, 7, 64; classification and regression


@functools.lru_cache(maxsize=None)
def _case(S, dtype):
    """(the matrix of S samples and 130 columns - 3 for 16384 samples - in dtype, posterior_loo of it, its bars): computed once"""
    ll = lc.matrix(S, 3 if S == 16384 else max(COLUMN_COUNTS)).astype(dtype)
    _, bars = lc.reference(ll.astype(np.float64))
    return ll, bn.posterior_loo(ll.astype(np.float64)), bars


def _hold(got, want, bars, label, cols=slice(None)):
    for i, f in enumerate(lc.FIELDS):
        dev = lc.deviation({f: got[i] if isinstance(got, tuple) else got[f]}, {f: want[f][cols]}, f)
        print("device %s %s: deviation %.3e, bar %.3e" % (label, f, dev, bars[f]))
        assert dev <= bars[f], (label, f, dev, bars[f])


# ---- 1. the column kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n_cols", COLUMN_COUNTS)
@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_psis_against_posterior_loo(S, n_cols, dtype):
    ll, want, bars = _case(S, dtype)
    got = device_ops.psis(np.ascontiguousarray(ll[:, :n_cols]))
    _hold(got, want, bars, "S=%d cols=%d %s" % (S, n_cols, dtype), slice(0, n_cols))
    if S <= 20:
        assert np.all(got[2] == np.inf)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_psis_of_16384_samples(dtype):
    ll, want, bars = _case(16384, dtype)
    _hold(device_ops.psis(ll), want, bars, "S=16384 cols=3 %s" % dtype)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("S,n_cols", [(21, 3), (65, 65), (257, 130)])
def test_a_strided_array_gives_the_packed_calls_bytes(S, n_cols, dtype):
    ll = _case(S, dtype)[0][:, :n_cols]
    packed = device_ops.psis(np.ascontiguousarray(ll))
    lib, dev = device_ops._lib()
    wide = np.full((S, n_cols + 3), -7.0, dtype=dtype)
    wide[:, :n_cols] = ll
    out = [np.empty(n_cols) for _ in range(3)]
    rc = lib.npbnn_op_psis(dev, wide.ctypes.data, capi.VALUE_F32 if dtype == "float32" else capi.VALUE_F64, S, n_cols, n_cols + 3,
                           capi.dptr(out[0]), capi.dptr(out[1]), capi.dptr(out[2]))
    assert rc == 0
    for a, b in zip(out, packed):
        assert a.tobytes() == b.tobytes()
    again = device_ops.psis(np.ascontiguousarray(ll))
    for a, b in zip(again, packed):
        assert a.tobytes() == b.tobytes()


def test_psis_of_the_special_columns():
    """a constant column, a column of two tied values, two equal columns, one shifted by 1e6, one near -700"""
    ll = lc.special_matrix()
    want, bars = bn.posterior_loo(ll), lc.reference(ll)[1]
    got = device_ops.psis(ll)
    _hold(got, want, bars, "special")
    assert got[2][0] == np.inf and got[0][0] == -1.25 and got[1][0] == -1.25 and got[2][1] == np.inf
    for a in got:
        assert a[2] == a[3]


def test_psis_refusals():
    lib, dev = device_ops._lib()
    ok = lc.matrix(8, 4)
    out = [np.empty(4) for _ in range(3)]

    def raw(a, S, n_cols, stride, kind=capi.VALUE_F64):
        return lib.npbnn_op_psis(dev, a.ctypes.data, kind, S, n_cols, stride, capi.dptr(out[0]), capi.dptr(out[1]), capi.dptr(out[2]))

    assert raw(ok, 8, 4, 4) == 0 and raw(ok, 8, 0, 4) == 0
    assert raw(ok, 1, 4, 4) == capi.E_ARG and raw(ok, 16385, 4, 4) == capi.E_ARG and raw(ok, 8, 4, 3) == capi.E_ARG and raw(ok, 8, 4, 4, 7) == capi.E_ARG
    for v in (np.nan, np.inf, -np.inf):
        bad = ok.copy()
        bad[5, 1] = v
        assert raw(bad, 8, 4, 4) == capi.E_ARG
        with pytest.raises(ValueError):
            device_ops.psis(bad)
    assert all(len(a) == 0 for a in device_ops.psis(np.zeros((8, 0))))


# ---- 2. the entry over stored sets ---------------------------------------------------------------------------------------------------
def _call(ctx, inp, slopes="own", **kw):
    sets = [s["weights"] for s in inp["samples"]]
    return ctx.predict_sets_loo(sets, capi.LIK_GAUSS if inp["kind"] == "reg" else capi.LIK_CATEGORICAL, sigma_sets=lpc.sigmas_of(inp),
                                act_prm_sets=lpc.slopes_of(inp) if isinstance(slopes, str) else slopes, **kw)


@pytest.mark.parametrize("path", sorted(thl.PATHS))
@pytest.mark.parametrize("name", LOO_CASES)
def test_entry_against_the_definition_on_every_path(name, path, monkeypatch):
    thl._set_path(path, monkeypatch)
    inp = lpc.inputs(name)
    ctx = thl._context(inp)
    try:
        z = ctx.predict_sets([s["weights"] for s in inp["samples"]], act_prm_sets=lpc.slopes_of(inp), apply_out_fn=False)
        got = _call(ctx, inp, log_lik=True)
        assert ctx.is_wide() == (path == "streamed") and ctx.l0_mode() == ("f32" if path == "f32" else "f16-split")
        lppd = thl._call(ctx, inp)
    finally:
        ctx.close()
    ll = lpc.log_lik_from_values(z, inp["labels"], inp["kind"], lpc.sigmas_of(inp))
    worst = max(thl._deviation(got["log_lik"], ll), thl._deviation(got["log_lik_sample"], ll.sum(axis=1)))
    against = max(thl._deviation(got["lppd_i"], lppd["lppd_i"]), thl._deviation(got["log_lik_sample"], lppd["log_lik_sample"]))
    print("log-likelihood deviation %s %s: %.3e; lppd_i and log_lik_sample against predict_sets_lppd: %.3e" % (name, path, worst, against))
    assert worst <= thl.KERNEL_TOL and against <= thl.KERNEL_TOL, (name, path, worst, against)
    assert got["log_lik"].shape == (lpc.CASES[name]["s"], lpc.N_ROWS)
    _hold(got, bn.posterior_loo(got["log_lik"]), lc.reference(got["log_lik"])[1], "%s %s" % (name, path))
    if lpc.CASES[name]["s"] <= 20:
        assert np.all(got["pareto_k"] == np.inf)


def _same_bytes(a, b, keys=("elpd_loo_i", "lppd_i", "pareto_k", "log_lik_sample", "log_lik")):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


@pytest.mark.parametrize("name", ["genrelu_h2_c10_s64", "relu_h2_reg4_s64"])
def test_two_calls_give_the_same_bytes(name):
    inp = lpc.inputs(name)
    ctx = thl._context(inp)
    try:
        a, b = _call(ctx, inp, log_lik=True), _call(ctx, inp, log_lik=True)
        lean = _call(ctx, inp)
    finally:
        ctx.close()
    _same_bytes(a, b)
    assert lean["log_lik"] is None
    _same_bytes(a, lean, ("elpd_loo_i", "lppd_i", "pareto_k", "log_lik_sample"))


@pytest.mark.parametrize("name", ["tanh_h2_c4_s7", "tanh_h2_reg1_s7"])
def test_grouping_of_the_sets_does_not_matter(name):
    """Seven sets replayed as they come and with a distinct slope vector each, which splits them into groups of one (tanh ignores
    the slopes): the same bytes."""
    inp = lpc.inputs(name)
    ctx = thl._context(inp)
    try:
        together = _call(ctx, inp, log_lik=True)
        alone = _call(ctx, inp, slopes=[np.full(2, 0.01 * (i + 1)) for i in range(7)], log_lik=True)
    finally:
        ctx.close()
    _same_bytes(together, alone)


@pytest.mark.parametrize("name", ["genrelu_h2_c10_s64", "relu_h2_reg4_s64"])
def test_three_row_blocks_give_the_whole_tables_bytes(name, monkeypatch):
    inp = lpc.inputs(name)
    reg = inp["kind"] == "reg"
    kind = capi.LIK_GAUSS if reg else capi.LIK_CATEGORICAL
    S = len(inp["samples"])
    with _SamplePredictor(lpc.N_FEATURES, inp["samples"], lpc.act_for(bn, inp["fun"], len(inp["nodes"])), bn.RegressTransform if reg else bn.SoftMax) as pred:
        whole = pred.loo(inp["x"], inp["labels"], kind, sigma_sets=lpc.sigmas_of(inp), log_lik=True)
        monkeypatch.setenv("NPBNN_HPD_STACK_BYTES", str(S * 8 * 68))
        assert stack_rows(S, 2) == 68                                          # 203 rows: blocks of 68, 68 and 67
        with pytest.raises(capi.NpbnnError) as e:
            pred.loo(inp["x"], inp["labels"], kind, sigma_sets=lpc.sigmas_of(inp))
        assert e.value.code == capi.E_NOMEM and "at most 68 rows fit" in str(e.value)
        blocked = pred.loo(inp["x"], inp["labels"], kind, sigma_sets=lpc.sigmas_of(inp), log_lik=True, block_rows=stack_rows(S, 2))
    _same_bytes(whole, blocked, ("elpd_loo_i", "lppd_i", "pareto_k", "p_loo_i", "log_lik"))
    for k in ("elpd_loo", "se_elpd_loo", "p_loo", "looic", "lppd", "n_bad_k"):
        assert whole[k] == blocked[k], k


# ---- 3. checkpoints ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["genrelu_h2_c10_s64", "relu_h2_reg4_s64", "tanh_h2_c4_s7"])
def test_get_posterior_loo_on_a_checkpoint(name, tmp_path):
    inp = lpc.inputs(name)
    reg = inp["kind"] == "reg"
    model = types.SimpleNamespace(_data=inp["x"][:50], _labels=inp["labels"][:50], _test_data=inp["x"], _test_labels=inp["labels"],
                                  _act_fun=lpc.act_for(bn, inp["fun"], len(inp["nodes"])), _output_act_fun=bn.RegressTransform if reg else bn.SoftMax,
                                  _estimation_mode="regression" if reg else "classification")
    pkl = str(tmp_path / "run.pkl")
    with open(pkl, "wb") as fh:
        pickle.dump([model, None, types.SimpleNamespace(_post_weight_samples=inp["samples"])], fh)
    res = bn.get_posterior_loo(pkl, pointwise=True, log_lik=True)
    S = lpc.CASES[name]["s"]
    assert (res["n_samples"], res["n_rows"]) == (S, lpc.N_ROWS) and res["log_lik"].shape == (S, lpc.N_ROWS)
    g = lpc.load()                                                                  # (the float32 network is the error source)
    assert float(np.max(np.abs(res["lppd_i"] - g[lpc.key(name, "lppd_i")]))) <= thl.POINT_TOL
    trace = g[lpc.key(name, "log_lik_sample")]
    assert float(np.max(np.abs(res["log_lik_sample"] - trace) / np.abs(trace))) <= thl.LL_BUDGET
    want = bn.posterior_loo(res["log_lik"])
    _hold(res, want, lc.reference(res["log_lik"])[1], "checkpoint %s" % name)
    for k in ("elpd_loo", "se_elpd_loo", "p_loo", "lppd"):
        assert abs(res[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])) * lpc.N_ROWS, k
    assert res["looic"] == -2.0 * res["elpd_loo"] and res["k_threshold"] == want["k_threshold"] and res["n_bad_k"] == want["n_bad_k"]
    lppd = bn.get_posterior_lppd(pkl)
    assert abs(res["lppd"] - lppd["lppd"]) <= 1e-10 * abs(lppd["lppd"])
    np.testing.assert_allclose(res["log_lik_sample"], lppd["log_lik_sample"], rtol=1e-12)
    train = bn.get_posterior_loo(pkl, features="train")
    assert train["n_rows"] == 50 and "elpd_loo_i" not in train and "log_lik" not in train and np.isfinite(train["looic"])
    other = bn.get_posterior_loo(pkl, features="train", pointwise=True)
    assert bn.loo_compare(other, other)["elpd_diff"] == 0.0


# ---- 4. error paths through ctypes ------------------------------------------------------------------------------------------------------
def test_errors_launch_no_evaluation(monkeypatch):
    monkeypatch.setenv("NPBNN_FI_TIMING", "1")
    inp, reg = lpc.inputs("tanh_h2_c4_s7"), lpc.inputs("swish_h1_reg3_s4")
    packed = np.stack([pack_weights(s["weights"]) for s in inp["samples"]])
    out = [np.zeros(lpc.N_ROWS) for _ in range(3)]

    def raw(ctx, packed, n_sets, lik, sigma, outs=out):
        rc = ctx._lib.npbnn_predict_sets_loo(ctx._ctx, capi.dptr(packed), None, n_sets, capi.TRAIN, lik, capi.dptr(sigma), capi.dptr(outs[0]),
                                             capi.dptr(outs[1]), capi.dptr(outs[2]), None, None)
        return rc, ctx._lib.npbnn_last_error(ctx._ctx).decode(), ctx.info(capi.INFO_SUMMARY_PASS_NS), ctx.info(capi.INFO_LOO_FINAL_NS)

    ctx = thl._context(inp)
    try:
        rc, _, ns, fin = raw(ctx, packed, 7, capi.LIK_CATEGORICAL, None)
        assert rc == 0 and ns > 0 and fin > 0 and np.all(out[0] < 0)              # (a call that runs leaves the time of its passes)
        for n_sets, word in ((1, "at least 2"), (0, "at least 2")):
            rc, msg, ns, fin = raw(ctx, packed, n_sets, capi.LIK_CATEGORICAL, None)
            assert rc == capi.E_ARG and word in msg and ns == 0 and fin == 0
        many = np.zeros((16385, packed.shape[1]))
        rc, msg, ns, fin = raw(ctx, many, 16385, capi.LIK_CATEGORICAL, None)
        assert rc == capi.E_ARG and "at most 16384" in msg and ns == 0
        rc, msg, ns, fin = raw(ctx, packed, 7, 99, None)
        assert rc == capi.E_ARG and ns == 0
        for kind in (capi.LIK_GAUSS_PRED_SIGMA, capi.LIK_POISSON, capi.LIK_NEGBIN, capi.LIK_NEGBIN2D, capi.LIK_NEGBIN_BASE10):
            rc, msg, ns, fin = raw(ctx, packed, 7, kind, None)
            assert rc == capi.E_ARG and "out of scope" in msg and ns == 0
        rc, msg, ns, fin = raw(ctx, packed, 7, capi.LIK_CATEGORICAL, None, [None, out[1], out[2]])
        assert rc == capi.E_ARG and ns == 0
        rc, msg, ns, fin = raw(ctx, packed, 7, capi.LIK_GAUSS, np.ones((7, 4)))      # a softmax network has no Gaussian likelihood
        assert rc == capi.E_ARG and ns == 0
        monkeypatch.setenv("NPBNN_HPD_STACK_BYTES", "1000")                          # 7 sets: 56 bytes a row, 17 rows fit
        rc, msg, ns, fin = raw(ctx, packed, 7, capi.LIK_CATEGORICAL, None)
        assert rc == capi.E_NOMEM and "at most 17 rows fit" in msg and ns == 0 and fin == 0
        monkeypatch.delenv("NPBNN_HPD_STACK_BYTES")
        lab = inp["labels"].copy()
        lab[77] = 4
        ctx.set_labels(lab)
        rc, msg, ns, fin = raw(ctx, packed, 7, capi.LIK_CATEGORICAL, None)
        assert rc == capi.E_ARG and "label" in msg and ns == 0 and fin == 0
        with pytest.raises(capi.NpbnnError) as e:
            _call(ctx, inp)
        assert e.value.code == capi.E_ARG
        ctx.set_labels(inp["labels"])
        poisoned = packed.copy()
        poisoned[3, 5] = np.nan                                                      # (found after the passes: a prediction is NaN)
        rc, msg, ns, fin = raw(ctx, poisoned, 7, capi.LIK_CATEGORICAL, None)
        assert rc == capi.E_ARG and "NaN" in msg
    finally:
        ctx.close()
    ctx = thl._context(inp, labels=False)
    try:
        rc, msg, ns, fin = raw(ctx, packed, 7, capi.LIK_CATEGORICAL, None)
        assert rc == capi.E_STATE and "labels" in msg and ns == 0
    finally:
        ctx.close()
    packed = np.stack([pack_weights(s["weights"]) for s in reg["samples"]])
    ctx = thl._context(reg, labels=False)
    try:
        rc, msg, ns, fin = raw(ctx, packed, 4, capi.LIK_GAUSS, lpc.sigmas_of(reg))
        assert rc == capi.E_STATE and "targets" in msg and ns == 0
        ctx.set_targets(reg["labels"][:, :2])
        rc, msg, ns, fin = raw(ctx, packed, 4, capi.LIK_GAUSS, lpc.sigmas_of(reg))
        assert rc == capi.E_ARG and ns == 0                                          # two target columns, three outputs
        ctx.set_targets(reg["labels"])
        for bad in (0.0, -0.5, np.inf, np.nan):
            sig = lpc.sigmas_of(reg).copy()
            sig[2, 1] = bad
            rc, msg, ns, fin = raw(ctx, packed, 4, capi.LIK_GAUSS, sig)
            assert rc == capi.E_ARG and "sigma" in msg and ns == 0
        rc, msg, ns, fin = raw(ctx, packed, 4, capi.LIK_GAUSS, None)
        assert rc == capi.E_ARG and ns == 0
        rc, msg, ns, fin = raw(ctx, packed, 4, capi.LIK_GAUSS, lpc.sigmas_of(reg))
        assert rc == 0 and ns > 0 and fin > 0
    finally:
        ctx.close()
