"""The weight gradient of the log-likelihood on the GPU (npbnn_loglik_grad, HipContext.loglik_grad, bn.log_posterior_grad,
bn.map_estimate) against the float64 restatement of tests/grad_cases.py on the table the device holds.

The gradient bar, per layer, is 16 times the larger of two reference-only quantities: the float32 restatement's distance to float64
on that input, and 2^-24 A with A the largest entry of sum_i |delta_i| |h_i|, the scale float32 rounding acts on.  The 16 is the
margin tests/test_hip_loo.py gives over a restatement's distance: it pays for the device's fast exponential and reciprocal and its
different order of sums.  The returned log-likelihood is held to a relative 1e-4, the README's log-likelihood budget.
tests/test_host_grad.py checks on the host that these references tell a wrong kernel from a right one."""
import contextlib
import io

import numpy as np
import pytest

import grad_cases as gc
import npbnn_amd as bn
import oracle as orc
from npbnn_amd import _capi as capi
from oracle_backend import serve_from_oracle

pytestmark = pytest.mark.gpu

KINDS = {"cat": (capi.OUT_SOFTMAX, capi.LIK_CATEGORICAL), "gauss": (capi.OUT_IDENTITY, capi.LIK_GAUSS),
         "pred": (capi.OUT_SOFTPLUS_HALF, capi.LIK_GAUSS_PRED_SIGMA)}
LL_TOL = 1e-4


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **k)


def _context(case, inp, lik_kind=None):
    ctx = bn.HipContext()
    ctx.set_data(inp["x"])
    if inp["x_test"] is not None:
        ctx.set_data(inp["x_test"], capi.TEST)
    for which, y in ((capi.TRAIN, inp["y"]), (capi.TEST, inp["y_test"])):
        if y is not None:
            (ctx.set_labels if case["lik"] == "cat" else ctx.set_targets)(y, which)
    if inp["inst_w"] is not None or inp["class_w"] is not None:
        ctx.set_row_weights(instance_w=inp["inst_w"], class_w=inp["class_w"])
    out_kind, lik = KINDS[case["lik"]]
    ctx.set_arch_from_weights(inp["w"], inp["x"].shape[1], bn.ActFun(fun=case["fun"], trainable=case["trainable"]).device_kind(), out_kind,
                              lik if lik_kind is None else lik_kind, n_targets=case["k"])
    return ctx


def _device(case, inp, calls=1):
    ctx = _context(case, inp)
    try:
        return [ctx.loglik_grad(inp["w"], act_prm=inp["slopes1"], col_override=inp["override"], lik_temp=case["lik_temp"], sigma=inp["sigma"],
                                which=case["which"]) for _ in range(calls)]
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(gc.CASES))
def test_case(name, monkeypatch):
    case, inp, want, want32 = gc.case_data(name)
    for k, v in case["env"]:
        monkeypatch.setenv(k, v)
    (r, grads), = _device(case, inp)
    bar, a, b = gc.bars(want, want32)
    errs = [float(np.abs(g - w).max()) for g, w in zip(grads, want["grads"])]
    rel = abs(r["loglik"] - want["loglik"]) / abs(want["loglik"])
    print("\ngrad %-24s %-5s loglik rel %.2e  device error / bar per layer %s  (float32 restatement / 2^-24 A: %s)"
          % (name, case["lik"], rel, " ".join("%.3f" % (e / x) for e, x in zip(errs, bar)), " ".join("%.2f" % (x / y) for x, y in zip(a, b))))
    assert rel <= LL_TOL
    assert r["n_rows"] == inp["table"].shape[0]
    assert len(grads) == len(want["grads"])
    for l, (g, w, e, x) in enumerate(zip(grads, want["grads"], errs, bar)):
        assert g.shape == w.shape and e <= x, (l, e, x)
    if case["lik"] == "gauss":
        assert np.array_equal(r["sigma"], inp["sigma"])
        assert np.allclose(r["sum_r2"], want["sum_r2"], rtol=LL_TOL) and np.abs(r["sum_r"] - want["sum_r"]).max() <= LL_TOL * np.sqrt(want["sum_r2"].max() * r["n_rows"])
    if inp["override"] is not None:
        # an overridden column's gradient is c_j times layer 0's bias sum (all layers of this case have a bias column)
        for col in np.flatnonzero(~np.isnan(inp["override"])):
            assert np.array_equal(grads[0][:, 1 + col], inp["override"][col] * grads[0][:, 0])


@pytest.mark.parametrize("name", ["rows_2111", "scratch_in_chunks", "gauss_k3"])
def test_same_bits_every_call(name, monkeypatch):
    case, inp, _, _ = gc.case_data(name)
    for k, v in case["env"]:
        monkeypatch.setenv(k, v)
    (ra, ga), (rb, gb) = _device(case, inp, calls=2)
    (rc, gcc), = _device(case, inp)
    assert ra["loglik"] == rb["loglik"] == rc["loglik"]
    for x, y, z in zip(ga, gb, gcc):
        assert np.array_equal(x, y) and np.array_equal(x, z) and np.abs(x).max() > 0


def test_refusals_leave_the_outputs_untouched():
    case, inp, _, _ = gc.case_data("rows_257")
    ctx = _context(case, inp)
    try:
        w = capi.as_f64(bn.pack_weights(inp["w"]))
        out, grad = capi.EvalOut(), np.full(w.size, 7.0)
        out.loglik = 7.0

        def call(W=w, o=out, g=grad, which=capi.TRAIN, c=ctx):
            import ctypes as C
            return c._lib.npbnn_loglik_grad(c._ctx, capi.dptr(W), None, None, 1.0, None, which, None if o is None else C.byref(o), capi.dptr(g))

        for tag, kw in dict(null_weights=dict(W=None), null_out=dict(o=None), null_grad=dict(g=None), which=dict(which=2)).items():
            assert call(**kw) == capi.E_ARG, tag
            assert b"loglik_grad" in ctx._lib.npbnn_last_error(ctx._ctx), tag
        assert call(which=capi.TEST) == capi.E_STATE                      # (no test table)
        # a context that holds a share of the rows (one rank, no communicator: npbnn_set_row_shard takes it on one GPU)
        ctx.set_row_shard(None, None, 0, 1, case["rows"])
        assert call() == capi.E_STATE
        assert b"loglik_grad" in ctx._lib.npbnn_last_error(ctx._ctx) and b"npbnn_set_row_shard" in ctx._lib.npbnn_last_error(ctx._ctx)
        assert out.loglik == 7.0 and np.all(grad == 7.0)
        ctx.set_row_shard(None, None, 0, 0, 0)
        assert call() == 0 and out.loglik < 0 and np.all(grad != 7.0)
        # ("a table without rows" cannot be built through the ABI: npbnn_set_data refuses n_rows < 1; the entry's check stands behind it)
        with pytest.raises(capi.NpbnnError):
            ctx.set_data(np.zeros((0, inp["x"].shape[1])))
    finally:
        ctx.close()
    # the likelihoods without a gradient, each by its own name (the message ends with it); the Gaussian one without sigma
    one, two = gc.case_data("gauss_k1"), gc.case_data("pred_sigma_k1")          # (1 output and 1 target; 2 outputs and 1 target)
    for g, lik, word in ((one, capi.LIK_POISSON, b"NPBNN_LIK_POISSON"), (two, capi.LIK_NEGBIN, b"NPBNN_LIK_NEGBIN"),
                         (two, capi.LIK_NEGBIN2D, b"NPBNN_LIK_NEGBIN2D"), (two, capi.LIK_NEGBIN_BASE10, b"NPBNN_LIK_NEGBIN_BASE10"),
                         (one, capi.LIK_NONE, b"NPBNN_LIK_NONE"), (one, capi.LIK_GAUSS, b"needs sigma (the empirical sigma has no gradient here)")):
        ctx = _context(g[0], g[1], lik_kind=lik)
        try:
            out.loglik = 7.0
            grad = np.full(bn.pack_weights(g[1]["w"]).size, 7.0)
            assert call(W=capi.as_f64(bn.pack_weights(g[1]["w"])), g=grad, c=ctx) == capi.E_ARG, word
            assert ctx._lib.npbnn_last_error(ctx._ctx).endswith(word), (word, ctx._lib.npbnn_last_error(ctx._ctx))
            assert out.loglik == 7.0 and np.all(grad == 7.0)
        finally:
            ctx.close()


def test_block_mask_through_the_backend():
    """a config-5-style block mask: the masked entries of log_posterior_grad are exactly 0, the others the restatement's"""
    rs = np.random.default_rng(11)
    x = rs.standard_normal((500, 24))
    y = np.tanh(x[:, :2]) + 0.1 * rs.standard_normal((500, 2))
    dat = dict(data=x, labels=y, test_data=np.zeros((0, 24)), test_labels=np.zeros((0, 2)))
    np.random.seed(3)
    bnn = quiet(bn.npBNN, dat, n_nodes=[8, 4], estimation_mode="regression", actFun=bn.ActFun(fun="tanh"), use_bias_node=-1)
    m = bn.create_mask(bnn._w_layers, indx_input_list=[list(np.repeat(np.arange(4), 6)), [], []], nodes_per_feature_list=[[2] * 4, [], []])
    quiet(bnn.apply_mask, m)
    ll, lp, grad, sigma = bn.log_posterior_grad(bnn)
    want = gc.restate(x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64), bnn._w_layers, orc.Act("tanh"), "gauss",
                      sigma=np.ones(2))
    want32 = gc.restate(x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64), bnn._w_layers, orc.Act("tanh"), "gauss",
                        sigma=np.ones(2), dtype=np.float32)
    bar, _, _ = gc.bars(want, want32)
    assert abs(ll - want["loglik"]) <= LL_TOL * abs(ll) and lp == bnn.calc_prior()
    assert (m[0] == 0).sum() == 8 * 24 * 3 // 4
    for g, w, k, b, layer in zip(grad, want["grads"], m, bar, bnn._w_layers):
        assert np.all(g[k == 0] == 0)
        assert np.abs(g - (w - layer) * k).max() <= b                          # (normal prior, scale 1: -w)


def test_map_estimate_against_the_float64_seam():
    device = gc.teacher_model()
    start = [np.array(w, copy=True) for w in device._w_layers]
    got = bn.map_estimate(device, n_iter=gc.TEACHER_STEPS)
    twin = gc.teacher_model()
    # (tests/conftest.py puts the real builder back after the test; `device` keeps the HIP backend it already holds)
    serve_from_oracle(lambda m: gc.GradOracleBackend(m, out_kind=0))
    want = bn.map_estimate(twin, n_iter=gc.TEACHER_STEPS)
    rel = np.abs(got["log_posterior"] / want["log_posterior"] - 1)
    print("\nmap_estimate: log posterior %.3f -> %.3f, largest relative distance to the float64 seam's trace %.2e"
          % (got["log_posterior"][0], got["log_posterior"].max(), rel.max()))
    assert got["n_iter"] == gc.TEACHER_STEPS == 60 and len(got["log_posterior"]) == 61
    assert rel.max() <= LL_TOL

    def accuracy(w):
        y = device.__dict__["_npbnn_backend"].predict(w)
        return float(np.mean(np.argmax(y, axis=1) == device._labels))

    assert accuracy(got["weights"]) > accuracy(start)
    best = int(np.argmax(got["log_posterior"]))
    assert all(np.array_equal(a, b) for a, b in zip(device._w_layers, got["weights"]))
    mcmc = quiet(bn.MCMC, device, n_iteration=10)
    assert abs(mcmc._logLik - got["log_lik"][best]) <= LL_TOL * abs(got["log_lik"][best])
