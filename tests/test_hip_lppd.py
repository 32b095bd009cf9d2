"""Log pointwise predictive density and WAIC on the GPU: npbnn_predict_sets_lppd (the replay's float32 pre-output values folded into
float64 per-row accumulators, per-sample totals from per-workgroup partials) and ``get_posterior_lppd``, against the definition on the
host and against the reference's values (tests/golden/lppd.npz).

Two bounds are measured figures (they are printed by the tests before they are asserted):
  KERNEL_TOL  the kernels against ``posterior_lppd`` on the float64 log-likelihoods the host computes from the very float32 values
              ``predict_sets(apply_out_fn=False)`` returns: only exp / log rounding and the order of sums separate the two.  Deviation
              = |got - want| / max(1, |want|) over every pointwise value, per-sample total and total of every case.  Measured on an
              MI355X: 1.326e-14 at most (genrelu_h2_c10_s64; every other case below 4.2e-15; the same on two boxes); the bound is 10 x
              that (the cap is 1e-10).
  POINT_TOL   pointwise values against the golden file on the default, float32 and weight-streamed paths: the float32 network is the
              error source.  Largest absolute deviation measured per path: 8.848e-05 (default), 1.178e-04 (f32), 1.236e-04 (streamed), all in
              swish_h3_c3_s4, every other case below 2.7e-05; the bound is 4 x the worst path.
Totals (lppd, log_lik_sample) are held to the project's log-likelihood budget of 1e-4 relative."""
import pickle
import types

import numpy as np
import pytest

import lppd_cases as lc
import npbnn_amd as bn
import oracle as orc
from npbnn_amd import HipContext, _capi as capi
from npbnn_amd.backend import pack_weights

pytestmark = pytest.mark.gpu

PATHS = {"default": {}, "f32": {"NPBNN_L0": "f32"}, "streamed": {"NPBNN_FORCE_WIDE": "1"}}
LL_BUDGET = 1e-4                                   # relative, README: the float32 forward pass against float64 on a log-likelihood
MEASURED_KERNEL_DEVIATION = 1.326e-14              # genrelu_h2_c10_s64; every other case below 4.2e-15
KERNEL_TOL = min(10 * MEASURED_KERNEL_DEVIATION, 1e-10)
MEASURED_POINT_DEVIATION = {"default": 8.848e-05, "f32": 1.178e-04, "streamed": 1.236e-04}    # swish_h3_c3_s4 on each path (ll down to -37)
POINT_TOL = 4 * max(MEASURED_POINT_DEVIATION.values())
POINT_FIELDS = ("lppd_i", "mean_log_lik_i", "p_waic_i")


def _set_path(path, monkeypatch):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)


def _context(inp, labels=True, lik=capi.LIK_NONE):
    ctx = HipContext(0)
    ctx.set_data(inp["x"])
    reg = inp["kind"] == "reg"
    if labels:
        (ctx.set_targets if reg else ctx.set_labels)(inp["labels"])
    ctx.set_arch_from_weights(inp["samples"][0]["weights"], inp["x"].shape[1], lc.act_for(bn, inp["fun"], len(inp["nodes"])).device_kind(),
                              capi.OUT_IDENTITY if reg else capi.OUT_SOFTMAX, lik)
    return ctx


def _call(ctx, inp, slopes="own", **kw):
    sets = [s["weights"] for s in inp["samples"]]
    return ctx.predict_sets_lppd(sets, capi.LIK_GAUSS if inp["kind"] == "reg" else capi.LIK_CATEGORICAL, sigma_sets=lc.sigmas_of(inp),
                                 act_prm_sets=lc.slopes_of(inp) if isinstance(slopes, str) else slopes, **kw)


def _deviation(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


# ---- 1. kernel arithmetic ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.CASES)
def test_kernels_against_the_definition_on_the_same_float32_values(name):
    inp = lc.inputs(name)
    ctx = _context(inp)
    try:
        z = ctx.predict_sets([s["weights"] for s in inp["samples"]], act_prm_sets=lc.slopes_of(inp), apply_out_fn=False)
        got = _call(ctx, inp)
    finally:
        ctx.close()
    assert np.array_equal(z, z.astype(np.float32))                          # (the float32 values themselves)
    want = bn.posterior_lppd(lc.log_lik_from_values(z, inp["labels"], inp["kind"], lc.sigmas_of(inp)))
    worst = max(_deviation(got[k], want[k]) for k in POINT_FIELDS + ("log_lik_sample", "lppd", "mean_log_lik", "p_waic"))
    print("kernel deviation %s: %.3e" % (name, worst))
    assert worst <= KERNEL_TOL, (name, worst)


# ---- 2. against the reference's numbers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", lc.CASES)
def test_golden_values_on_every_path(name, path, monkeypatch):
    _set_path(path, monkeypatch)
    inp, g = lc.inputs(name), lc.load()
    ctx = _context(inp)
    try:
        got = _call(ctx, inp)
        assert ctx.is_wide() == (path == "streamed") and ctx.l0_mode() == ("f32" if path == "f32" else "f16-split")
    finally:
        ctx.close()
    point = max(float(np.max(np.abs(got[f] - g[lc.key(name, f)]))) for f in POINT_FIELDS)
    trace = g[lc.key(name, "log_lik_sample")]
    total = g[lc.key(name, "lppd_i")].sum()
    rel_trace = float(np.max(np.abs(got["log_lik_sample"] - trace) / np.abs(trace)))
    rel_total = abs(got["lppd"] - total) / abs(total)
    print("golden deviation %s %s: pointwise %.3e, lppd %.3e, log_lik_sample %.3e, p_waic %.3e"
          % (name, path, point, rel_total, rel_trace, abs(got["p_waic"] - g[lc.key(name, "p_waic_i")].sum()) / max(1.0, g[lc.key(name, "p_waic_i")].sum())))
    assert rel_total <= LL_BUDGET and rel_trace <= LL_BUDGET, (name, path, rel_total, rel_trace)
    assert point <= POINT_TOL, (name, path, point)
    if lc.CASES[name]["s"] == 1:
        assert not got["p_waic_i"].any() and got["p_waic"] == 0.0


# ---- 3. grouping, 4. determinism -----------------------------------------------------------------------------------------------------
def _same_bytes(a, b):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("name", ["tanh_h2_c4_s7", "tanh_h2_reg1_s7"])
def test_grouping_of_the_sets_does_not_matter(name):
    """Seven sets replayed as they come (groups of three, three and one) and with a distinct slope vector each, which splits them into
    groups of one (tanh ignores the slopes): the same bytes."""
    inp = lc.inputs(name)
    ctx = _context(inp)
    try:
        together = _call(ctx, inp)
        alone = _call(ctx, inp, slopes=[np.full(2, 0.01 * (i + 1)) for i in range(7)])
    finally:
        ctx.close()
    _same_bytes(together, alone)


@pytest.mark.parametrize("name", ["genrelu_h2_c10_s64", "relu_h2_reg4_s64"])
def test_two_calls_give_the_same_bytes(name):
    inp = lc.inputs(name)
    ctx = _context(inp)
    try:
        a, b = _call(ctx, inp), _call(ctx, inp)
        lean = _call(ctx, inp, pointwise=False)
    finally:
        ctx.close()
    _same_bytes(a, b)
    assert lean["lppd_i"] is None and lean["p_waic_i"] is None
    assert (lean["lppd"], lean["mean_log_lik"], lean["p_waic"]) == (a["lppd"], a["mean_log_lik"], a["p_waic"])
    np.testing.assert_array_equal(lean["log_lik_sample"], a["log_lik_sample"])


# ---- 5. full size ---------------------------------------------------------------------------------------------------------------------
def test_config2_shape():
    """100k x 256, [32, 8], 10 classes, 100 samples: finite, the totals against the float64 oracle and log_lik_sample against
    npbnn_eval's log-likelihood of the same weights, within the log-likelihood budget."""
    rs = np.random.default_rng(21)
    n, f, c, s = 100000, 256, 10, 100
    x = rs.standard_normal((n, f))
    dims = [f, 32, 8, c]
    teacher = [rs.normal(0, 0.25, (dims[i + 1], dims[i] + 1)) for i in range(3)]
    sets = [[t + rs.normal(0, 0.08, t.shape) for t in teacher] for _ in range(s)]
    act = orc.Act("tanh")
    labels = np.argmax(orc.forward_logits(x, teacher, act), axis=1)
    flip = rs.random(n) < 0.05
    labels = np.where(flip, (labels + rs.integers(1, c, n)) % c, labels).astype(np.int64)
    ctx = HipContext(0)
    try:
        ctx.set_data(x)
        ctx.set_labels(labels)
        ctx.set_arch_from_weights(sets[0], f, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_CATEGORICAL)
        got = ctx.predict_sets_lppd(sets, capi.LIK_CATEGORICAL)
        evals = np.array([ctx.eval(w)["loglik"] for w in sets])
    finally:
        ctx.close()
    assert all(np.all(np.isfinite(got[k])) for k in POINT_FIELDS + ("log_lik_sample",))
    # the oracle in row blocks: [S, block] log-likelihoods at a time
    tot = np.zeros(3)
    trace = np.zeros(s)
    for r in range(0, n, 20000):
        z = np.array([orc.forward_logits(x[r:r + 20000], w, act) for w in sets])
        res = bn.posterior_lppd(lc.log_lik_from_values(z, labels[r:r + 20000], "cat"))
        tot += [res["lppd"], res["mean_log_lik"], res["p_waic"]]
        trace += res["log_lik_sample"]
    dev = [abs(got[k] - w) / abs(w) for k, w in zip(("lppd", "mean_log_lik", "p_waic"), tot)]
    dev_trace = float(np.max(np.abs(got["log_lik_sample"] - trace) / np.abs(trace)))
    dev_eval = float(np.max(np.abs(got["log_lik_sample"] - evals) / np.abs(evals)))
    print("config-2 shape: totals %s, log_lik_sample against the oracle %.3e, against npbnn_eval %.3e" % (["%.3e" % d for d in dev], dev_trace, dev_eval))
    assert max(dev) <= LL_BUDGET and dev_trace <= LL_BUDGET and dev_eval <= LL_BUDGET
    for k, f_ in (("lppd", "lppd_i"), ("mean_log_lik", "mean_log_lik_i"), ("p_waic", "p_waic_i")):
        assert abs(got[k] - got[f_].sum()) <= 1e-9 * abs(got[k])


# ---- 6. error paths through ctypes ------------------------------------------------------------------------------------------------------
def test_errors_launch_no_evaluation(monkeypatch):
    monkeypatch.setenv("NPBNN_FI_TIMING", "1")
    inp, reg = lc.inputs("tanh_h2_c4_s7"), lc.inputs("swish_h1_reg3_s4")
    packed = np.stack([pack_weights(s["weights"]) for s in inp["samples"]])
    totals = np.zeros(3)

    def raw(ctx, packed, n_sets, lik, sigma, totals):
        rc = ctx._lib.npbnn_predict_sets_lppd(ctx._ctx, capi.dptr(packed), None, n_sets, capi.TRAIN, lik, capi.dptr(sigma), None, None, None, None,
                                              capi.dptr(totals))
        return rc, ctx._lib.npbnn_last_error(ctx._ctx).decode(), ctx.info(capi.INFO_SUMMARY_PASS_NS)

    ctx = _context(inp)
    try:
        rc, _, ns = raw(ctx, packed, 7, capi.LIK_CATEGORICAL, None, totals)
        assert rc == 0 and ns > 0 and totals[0] < 0                          # (a call that runs leaves the time of its passes)
        rc, msg, ns = raw(ctx, packed, 7, 99, None, totals)
        assert rc == capi.E_ARG and ns == 0
        for kind in (capi.LIK_GAUSS_PRED_SIGMA, capi.LIK_POISSON, capi.LIK_NEGBIN, capi.LIK_NEGBIN2D, capi.LIK_NEGBIN_BASE10):
            rc, msg, ns = raw(ctx, packed, 7, kind, None, totals)
            assert rc == capi.E_ARG and "out of scope" in msg and ns == 0
        rc, msg, ns = raw(ctx, packed, 7, capi.LIK_CATEGORICAL, None, None)
        assert rc == capi.E_ARG and ns == 0
        rc, msg, ns = raw(ctx, packed, 7, capi.LIK_GAUSS, np.ones((7, 4)), totals)      # a softmax network has no Gaussian likelihood
        assert rc == capi.E_ARG and ns == 0
        lab = inp["labels"].copy()
        lab[77] = 4
        ctx.set_labels(lab)
        rc, msg, ns = raw(ctx, packed, 7, capi.LIK_CATEGORICAL, None, totals)
        assert rc == capi.E_ARG and "label" in msg and ns == 0
        with pytest.raises(capi.NpbnnError) as e:
            _call(ctx, inp)
        assert e.value.code == capi.E_ARG
    finally:
        ctx.close()
    ctx = _context(inp, labels=False)
    try:
        rc, msg, ns = raw(ctx, packed, 7, capi.LIK_CATEGORICAL, None, totals)
        assert rc == capi.E_STATE and "labels" in msg and ns == 0
    finally:
        ctx.close()
    packed = np.stack([pack_weights(s["weights"]) for s in reg["samples"]])
    ctx = _context(reg, labels=False)
    try:
        rc, msg, ns = raw(ctx, packed, 4, capi.LIK_GAUSS, lc.sigmas_of(reg), totals)
        assert rc == capi.E_STATE and "targets" in msg and ns == 0
        ctx.set_targets(reg["labels"][:, :2])
        rc, msg, ns = raw(ctx, packed, 4, capi.LIK_GAUSS, lc.sigmas_of(reg), totals)
        assert rc == capi.E_ARG and ns == 0                                   # two target columns, three outputs
        ctx.set_targets(reg["labels"])
        for bad in (0.0, -0.5, np.inf, np.nan):
            sig = lc.sigmas_of(reg).copy()
            sig[2, 1] = bad
            rc, msg, ns = raw(ctx, packed, 4, capi.LIK_GAUSS, sig, totals)
            assert rc == capi.E_ARG and "sigma" in msg and ns == 0
        rc, msg, ns = raw(ctx, packed, 4, capi.LIK_GAUSS, None, totals)
        assert rc == capi.E_ARG and ns == 0
        rc, msg, ns = raw(ctx, packed, 4, capi.LIK_GAUSS, lc.sigmas_of(reg), totals)
        assert rc == 0 and ns > 0
    finally:
        ctx.close()


# ---- checkpoints ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", ["genrelu_h2_c10_s64", "swish_h3_c3_s4", "genrelu_h3_reg3_s3", "tanh_h2_reg1_s7"])
def test_get_posterior_lppd_on_a_checkpoint(name, path, monkeypatch, tmp_path):
    _set_path(path, monkeypatch)
    inp, g = lc.inputs(name), lc.load()
    reg = inp["kind"] == "reg"
    model = types.SimpleNamespace(_data=inp["x"][:50], _labels=inp["labels"][:50], _test_data=inp["x"], _test_labels=inp["labels"],
                                  _act_fun=lc.act_for(bn, inp["fun"], len(inp["nodes"])), _output_act_fun=bn.RegressTransform if reg else bn.SoftMax,
                                  _estimation_mode="regression" if reg else "classification")
    pkl = str(tmp_path / "run.pkl")
    with open(pkl, "wb") as fh:
        pickle.dump([model, None, types.SimpleNamespace(_post_weight_samples=inp["samples"])], fh)
    res = bn.get_posterior_lppd(pkl, pointwise=True)
    total, pw = g[lc.key(name, "lppd_i")].sum(), g[lc.key(name, "p_waic_i")].sum()
    assert abs(res["lppd"] - total) <= LL_BUDGET * abs(total)
    assert np.max(np.abs(res["log_lik_sample"] - g[lc.key(name, "log_lik_sample")]) / np.abs(g[lc.key(name, "log_lik_sample")])) <= LL_BUDGET
    assert max(float(np.max(np.abs(res[f] - g[lc.key(name, f)]))) for f in POINT_FIELDS) <= POINT_TOL
    assert res["elpd_waic"] == res["lppd"] - res["p_waic"] and res["waic"] == -2.0 * res["elpd_waic"]
    assert (res["n_samples"], res["n_rows"]) == (lc.CASES[name]["s"], lc.N_ROWS)
    assert abs(res["p_waic"] - pw) <= lc.N_ROWS * POINT_TOL + LL_BUDGET * pw   # (a sum of N_ROWS pointwise values, each within POINT_TOL)
    train = bn.get_posterior_lppd(pkl, features="train")
    assert train["n_rows"] == 50 and "lppd_i" not in train and np.isfinite(train["waic"])
