"""The posterior predictive distribution on the GPU: npbnn_op_mixture (device_ops.mixture) and npbnn_predict_sets_predictive
(HipContext.predict_sets_predictive, get_posterior_predictive) against the independent restatement of tests/predictive_cases.py, under
its acceptance rules: a quantile passes by its residual |F(q) - p| <= 4 (S + 8) 2^-53 max(p, 1 - p) or within 4 ulp of the restated
root, a CRPS within (64 + ceil(S (S - 1) / 128)) 2^-53 (T1 + T2 / 2); no cell is left out.  The fused entry is held to the restatement
applied to the float64 array npbnn_predict_sets returns."""
import math
import pickle
import types

import numpy as np
import pytest

import calibration_cases as cc
import predictive_cases as pc
import npbnn_amd as bn
from npbnn_amd import _capi as capi
from npbnn_amd import device_ops

pytestmark = pytest.mark.gpu

S_VALUES = (1, 2, 63, 64, 65, 257)                # one lane, and the lane-stride edge on either side of 64
COL_VALUES = (1, 3, 65, 130)                      # one cell, and partial last tiles
# every family at every S; the column counts, the value types and the three sigma layouts rotate through them
OP_CASES = [(fam, S, COL_VALUES[(fi + si) % 4], ("float32", "float64")[(fi + si // 2) % 2], (0, 1, 3)[(fi + si) % 3])
            for fi, fam in enumerate(pc.FAMILIES) for si, S in enumerate(S_VALUES)]


def test_the_rotation_covers_every_value():
    for k, values in ((1, S_VALUES), (2, COL_VALUES), (3, ("float32", "float64")), (4, (0, 1, 3))):
        assert {c[k] for c in OP_CASES} == set(values)
        for fam in pc.FAMILIES:
            assert len({c[k] for c in OP_CASES if c[0] == fam}) >= 2


def _mixture(mu, sg, dtype, probs, y):
    per_cell = sg.shape == mu.shape
    return device_ops.mixture(mu.astype(dtype), sg.astype(dtype) if per_cell else sg, probs, y)


@pytest.mark.parametrize("fam,S,n_cols,dtype,sigma_cols", OP_CASES, ids=lambda v: str(v))
def test_mixture_against_the_restatement(fam, S, n_cols, dtype, sigma_cols):
    mu, sg, y = pc.make(fam, S, n_cols, sigma_cols)
    if sigma_cols == 1:
        sg = sg[:, 0]                                      # ([S] is taken as [S, 1])
    q, mean, crps = _mixture(mu, sg, dtype, pc.PROBS, y)
    sg2 = sg.reshape(S, -1)
    label = "%s S=%d cols=%d %s sigma_cols=%d" % (fam, S, n_cols, dtype, sigma_cols)
    worst, by_root = pc.check_quantiles(q, mu, sg2, pc.PROBS, sigma_cols > 0, label)
    worst_crps = pc.check_crps(crps, mu, sg2, y, sigma_cols > 0, label)
    print("%s: largest residual / bound %.3f, %d cells by the root, largest CRPS difference / bound %.4f" % (label, worst, by_root, worst_crps))
    assert q.dtype == np.float64 and mean.dtype == np.float64 and crps.dtype == np.float64
    assert np.array_equal(mean, pc.mean_of(mu))            # bit for bit: the cases' sums of mu - K are exact
    if fam == "identical":                                 # S equal components: mu + sigma z_p
        sig = pc.sigma_of_cells(sg2, n_cols, sigma_cols > 0)
        for j, p in enumerate(pc.PROBS):
            np.testing.assert_allclose(q[j], mu[0] + sig[0] * pc.normal_quantile(p), rtol=1e-13, atol=0)
    assert np.all(np.diff(q, axis=0) >= 0)                 # non-decreasing in p


def test_mixture_sixteen_probabilities_in_one_call():
    mu, sg, y = pc.make("random", 65, 3)
    q, mean, crps = device_ops.mixture(mu, sg, pc.PROBS16)
    assert crps is None and q.shape == (16, 3)
    worst, by_root = pc.check_quantiles(q, mu, sg, pc.PROBS16, False, "16 probabilities")
    print("16 probabilities: largest residual / bound %.3f, %d cells by the root" % (worst, by_root))
    order = np.argsort(pc.PROBS16)
    assert np.all(np.diff(q[order], axis=0) > 0)
    alone = device_ops.mixture(mu, sg, pc.PROBS16[3:4])[0]
    assert np.array_equal(alone[0], q[3])                  # a probability's result does not depend on its neighbours


def test_mixture_1025_samples():
    mu, sg, y = pc.make("random", 1025, 3)
    q, mean, crps = device_ops.mixture(mu.astype(np.float32), sg.astype(np.float32), pc.PROBS, y)
    worst, by_root = pc.check_quantiles(q, mu, sg, pc.PROBS, False, "S=1025")
    worst_crps = pc.check_crps(crps, mu, sg, y, False, "S=1025")
    print("S=1025: largest residual / bound %.3f, %d cells by the root, largest CRPS difference / bound %.4f" % (worst, by_root, worst_crps))
    assert np.array_equal(mean, pc.mean_of(mu))


def test_mixture_global_memory_route():
    """float64 mu and sigma at S = 16384 are 256 KiB a cell: not staged, every pass reads them where they lie."""
    mu, sg, _ = pc.make("random", 16384, 3)
    q, mean, _ = device_ops.mixture(mu, sg, pc.PROBS)
    worst, by_root = pc.check_quantiles(q, mu, sg, pc.PROBS, False, "S=16384")
    print("S=16384: largest residual / bound %.3f, %d cells by the root" % (worst, by_root))
    assert np.array_equal(mean, pc.mean_of(mu))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("sigma_cols", [0, 3], ids=["per_cell", "per_sample"])
@pytest.mark.parametrize("S,n_cols", [(S, n) for S in (2, 65) for n in (1, 65)])
def test_mixture_strided_equals_packed_and_a_cell_does_not_depend_on_its_tile(S, n_cols, sigma_cols, dtype):
    """mu (and a per-cell sigma beside it) sit in wider arrays (col_stride = n_cols + 3): quantiles, mean and CRPS byte for byte
    those of the packed call.  The cells are six distinct ones over and over (cell c of a [S, 3] sigma reads column c % 3, which
    c % 6 fixes), so of 65 cells - a tile of 64 and one of 1 - a copy lands in the other tile and at other places, and gives the
    bytes of the first."""
    mu6, sg6, y6 = pc.make("random", S, 6, sigma_cols)
    idx = np.arange(n_cols) % 6
    mu = np.ascontiguousarray(mu6[:, idx]).astype(dtype)
    sg = sg6 if sigma_cols else np.ascontiguousarray(sg6[:, idx]).astype(dtype)
    y = np.ascontiguousarray(y6[idx])
    q, mean, crps = device_ops.mixture(mu, sg, pc.PROBS, y)
    for j in range(n_cols):
        for a in (q.T, mean, crps):
            assert a[j].tobytes() == a[idx[j]].tobytes(), j
    lib, dev = device_ops._lib()
    wide = np.full((S, n_cols + 3), 7.0, dtype=dtype)
    wide[:, :n_cols] = mu
    wide_sg = sg
    if not sigma_cols:
        wide_sg = np.full((S, n_cols + 3), 7.0, dtype=dtype)
        wide_sg[:, :n_cols] = sg
    pr = np.asarray(pc.PROBS, dtype=np.float64)
    q2, mean2, crps2 = np.empty((len(pr), n_cols)), np.empty(n_cols), np.empty(n_cols)
    rc = lib.npbnn_op_mixture(dev, wide.ctypes.data, wide_sg.ctypes.data, capi.VALUE_F32 if dtype == "float32" else capi.VALUE_F64, S, n_cols,
                              n_cols + 3, sigma_cols, capi.dptr(pr), len(pr), capi.dptr(y), capi.dptr(q2), capi.dptr(mean2), capi.dptr(crps2))
    assert rc == 0 and q2.tobytes() == q.tobytes() and mean2.tobytes() == mean.tobytes() and crps2.tobytes() == crps.tobytes()


def test_mixture_keeps_the_trailing_shape_and_refuses():
    mu, sg, y = pc.make("random", 7, 6)
    flat = device_ops.mixture(mu, sg, (0.1, 0.9), y)
    q, mean, crps = device_ops.mixture(mu.reshape(7, 2, 3), sg.reshape(7, 2, 3), (0.1, 0.9), y.reshape(2, 3))
    assert q.shape == (2, 2, 3) and mean.shape == (2, 3) and crps.shape == (2, 3)
    assert np.array_equal(q.reshape(2, 6), flat[0]) and np.array_equal(crps.ravel(), flat[2])
    per_sample = device_ops.mixture(mu.reshape(7, 2, 3), sg[:, :3], (0.1, 0.9))[0]
    assert np.array_equal(per_sample.reshape(2, 6), device_ops.mixture(mu, sg[:, [0, 1, 2, 0, 1, 2]], (0.1, 0.9))[0])
    for bad in (dict(probs=(0.0,)), dict(probs=(1.0,)), dict(probs=(1e-13,)), dict(probs=np.linspace(0.1, 0.9, 17)), dict(y=y[:5]),
                dict(y=np.where(np.arange(6) == 2, np.nan, y))):
        with pytest.raises(ValueError):
            device_ops.mixture(mu, sg, **dict(dict(probs=(0.5,)), **bad))
    for bad_mu, bad_sg in ((np.where(mu == mu[3, 1], np.inf, mu), sg), (mu, np.where(sg == sg[2, 2], 0.0, sg)), (mu, -sg), (mu.reshape(7, 2, 3), sg[:, :2]),
                           (np.zeros((16385, 1)), np.ones((16385, 1)))):
        with pytest.raises(ValueError):
            device_ops.mixture(bad_mu, bad_sg, (0.5,))
    # the library's own checks, behind the binding's
    lib, dev = device_ops._lib()
    out = np.empty(6)

    def rc(mu_, sg_, probs, y_, oq, om, oc, n=7):
        pr = np.asarray(probs, dtype=np.float64)
        return lib.npbnn_op_mixture(dev, mu_.ctypes.data, sg_.ctypes.data, capi.VALUE_F64, n, 6, 6, 0, capi.dptr(pr) if len(pr) else None, len(pr),
                                    capi.dptr(y_), capi.dptr(oq), capi.dptr(om), capi.dptr(oc))
    assert rc(mu, sg, (), None, None, out, None) == 0 and np.array_equal(out, pc.mean_of(mu))
    bad_sigma = sg.copy()
    bad_sigma[4, 4] = np.inf
    bad_mu = mu.copy()
    bad_mu[0, 0] = np.nan
    for args in ((mu, sg, (), None, None, None, None), (mu, sg, (0.5,), None, None, out, None), (mu, sg, (), y, None, out, None),
                 (mu, sg, (), None, None, out, out.copy()), (mu, sg, (2.0,), None, out, None, None), (mu, sg, [0.5] * 17, None, np.empty(17 * 6), None, None),
                 (mu, bad_sigma, (), None, None, out, None), (bad_mu, sg, (), None, None, out, None), (mu, sg, (), y * np.inf, None, None, out),
                 (mu, sg, (), None, None, out, None, 16385)):
        assert rc(*args) == capi.E_ARG


# ---- the fused entry: replay into a device stack, the two kernels on it
N_FEATURES = 5
N_SETS = 12
CONFIGS = {"identity": dict(out=capi.OUT_IDENTITY, n_out=2, fun="tanh"), "softplus_half": dict(out=capi.OUT_SOFTPLUS_HALF, n_out=4, fun="swish")}


def _net(n_out, genrelu, seed=11):
    rs = np.random.default_rng([seed, n_out, int(genrelu)])
    dims = [N_FEATURES, 7, 4, n_out]
    weights = [[rs.normal(0, 0.6, (dims[i + 1], dims[i] + 1)) for i in range(3)] for _ in range(N_SETS)]
    slopes = None
    if genrelu:
        slopes = [rs.uniform(0.01, 0.4, 2) for _ in range(N_SETS)]
        slopes[1] = slopes[0]
        slopes[7] = slopes[6] = slopes[5]                    # groups of two and three that share their slopes, the rest alone
    sigma = np.exp(rs.normal(-0.5, 0.4, (N_SETS, n_out)))
    return weights, slopes, sigma


def _open(cfg, genrelu, n_rows, wide, monkeypatch, which):
    if wide:
        monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    rs = np.random.default_rng([3, n_rows])
    x = rs.standard_normal((n_rows, N_FEATURES))
    weights, slopes, sigma = _net(cfg["n_out"], genrelu)
    ctx = bn.HipContext()
    ctx.set_data(x if which == capi.TRAIN else rs.standard_normal((37, N_FEATURES)))
    if which == capi.TEST:
        ctx.set_data(x, capi.TEST)
    fun = "genReLU" if genrelu else cfg["fun"]
    act = bn.ActFun(fun=fun, prm=np.zeros(2)) if genrelu else bn.ActFun(fun=fun)
    ctx.set_arch_from_weights(weights[0], N_FEATURES, act.device_kind(), cfg["out"], capi.LIK_NONE)
    assert ctx.is_wide() == wide
    targets = rs.standard_normal((n_rows, 2)) * 1.5
    return ctx, weights, slopes, (sigma if cfg["out"] == capi.OUT_IDENTITY else None), targets


def _check_against_stack(got, stack, sigma, targets, label):
    n_sets, n_rows = stack.shape[:2]
    if sigma is None:
        mu, sg, per_sample = stack[:, :, :2].reshape(n_sets, -1), stack[:, :, 2:].reshape(n_sets, -1), False
    else:
        mu, sg, per_sample = stack.reshape(n_sets, -1), sigma, True
    q = got["quantiles"].reshape(len(pc.PROBS), -1)
    worst, by_root = pc.check_quantiles(q, mu, sg, pc.PROBS, per_sample, label)
    worst_crps = pc.check_crps(got["crps_i"].ravel(), mu, sg, targets.ravel(), per_sample, label)
    print("%s: largest residual / bound %.3f, %d cells by the root, largest CRPS difference / bound %.4f" % (label, worst, by_root, worst_crps))
    # mean = K + (1/S) sum (mu - K): S - 1 additions, a division and an addition, each within 2^-53 of what it rounds
    exact = np.array([math.fsum((mu[:, c] - mu[0, c]).tolist()) for c in range(mu.shape[1])])
    tol = (n_sets + 2) * 2.0 ** -53 * (np.abs(mu[0]) + np.sum(np.abs(mu - mu[0]), axis=0) / n_sets)
    assert np.all(np.abs(got["mean"].ravel() - (mu[0] + exact / n_sets)) <= tol), label
    crps_i = got["crps_i"]
    for t in range(crps_i.shape[1]):
        assert abs(got["crps_total"][t] - math.fsum(crps_i[:, t].tolist())) <= n_rows * 2.0 ** -53 * math.fsum(np.abs(crps_i[:, t]).tolist()), label


@pytest.mark.parametrize("wide", [False, True], ids=["resident", "streamed"])
@pytest.mark.parametrize("which", [capi.TRAIN, capi.TEST], ids=["train", "test"])
@pytest.mark.parametrize("n_rows", [130, 1])
@pytest.mark.parametrize("genrelu", [False, True], ids=["plain", "slopes"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_predict_sets_predictive_equals_restatement_of_predict_sets(name, genrelu, n_rows, which, wide, monkeypatch):
    ctx, weights, slopes, sigma, targets = _open(CONFIGS[name], genrelu, n_rows, wide, monkeypatch, which)
    try:
        stack = ctx.predict_sets(weights, act_prm_sets=slopes, which=which)
        got = ctx.predict_sets_predictive(weights, pc.PROBS, sigma_sets=sigma, targets=targets, act_prm_sets=slopes, which=which)
        again = ctx.predict_sets_predictive(weights, pc.PROBS, sigma_sets=sigma, targets=targets, act_prm_sets=slopes, which=which)
        if genrelu:
            assert ctx.replay_info()[0] > 1                 # (several groups)
    finally:
        ctx.close()
    assert got["quantiles"].shape == (5, n_rows, 2) and got["mean"].shape == (n_rows, 2) and got["crps_i"].shape == (n_rows, 2)
    _check_against_stack(got, stack, sigma, targets, "%s slopes=%s rows=%d which=%d wide=%s" % (name, genrelu, n_rows, which, wide))
    for k in got:                                           # two calls, the same bits
        assert np.array_equal(got[k], again[k]), k
    # a cell's bits depend on its values and on S alone: the same float32 values laid out as a plain [S, cells] array, in another
    # tile, grid and stride than the stack's, give them again
    s32 = stack.astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), stack)
    plain = device_ops.mixture(s32, sigma, pc.PROBS, targets) if sigma is not None else device_ops.mixture(s32[:, :, :2], s32[:, :, 2:], pc.PROBS, targets)
    for k, v in zip(("quantiles", "mean", "crps_i"), plain):
        assert np.array_equal(got[k], v), k


def test_predict_sets_predictive_refusals(monkeypatch):
    ctx, weights, slopes, sigma, targets = _open(CONFIGS["identity"], False, 130, False, monkeypatch, capi.TRAIN)
    try:
        # the budget: NPBNN_E_NOMEM naming the largest row count that fits
        monkeypatch.setenv("NPBNN_HPD_STACK_BYTES", str(N_SETS * 2 * 4 * 44))
        with pytest.raises(capi.NpbnnError) as e:
            ctx.predict_sets_predictive(weights, pc.PROBS, sigma_sets=sigma)
        assert e.value.code == capi.E_NOMEM and "predict_sets_predictive" in str(e.value) and "at most 44 rows fit" in str(e.value)
        monkeypatch.delenv("NPBNN_HPD_STACK_BYTES")
        # an infinite prediction
        huge = [[w.copy() for w in weights[0]]] + weights[1:]
        huge[0][1][:, :] = 0.0
        huge[0][1][:, 0] = 50.0                              # (the bias column: every unit of the second hidden layer is tanh(50) = 1)
        huge[0][2][:, :] = 3e38                              # five times 3e38 is past the largest float32
        with pytest.raises(capi.NpbnnError) as e:
            ctx.predict_sets_predictive(huge, pc.PROBS, sigma_sets=sigma)
        assert e.value.code == capi.E_ARG
        for kw in (dict(sigma_sets=None), dict(sigma_sets=sigma[:5]), dict(sigma_sets=-sigma), dict(sigma_sets=sigma, targets=targets[:7]),
                   dict(sigma_sets=sigma, probs=(0.0,)), dict(sigma_sets=sigma, probs=[0.5] * 17), dict(sigma_sets=sigma, probs=(), want_mean=False)):
            with pytest.raises(ValueError):
                ctx.predict_sets_predictive(weights, **dict(dict(probs=pc.PROBS), **kw))
    finally:
        ctx.close()
    # a predicted sigma of 0: the softplus of a large negative value underflows in float32 and is refused, not divided by
    ctx, weights, slopes, _, targets = _open(CONFIGS["softplus_half"], False, 130, False, monkeypatch, capi.TRAIN)
    try:
        with pytest.raises(ValueError):
            ctx.predict_sets_predictive(weights, pc.PROBS, sigma_sets=np.ones((N_SETS, 2)))
        dead = [[w.copy() for w in weights[0]]] + weights[1:]
        dead[0][-1][2:, :] = 0.0
        dead[0][-1][2:, 0] = -200.0                         # (the bias column: softplus(-200) = 1.4e-87, 0 in float32)
        with pytest.raises(capi.NpbnnError) as e:
            ctx.predict_sets_predictive(dead, pc.PROBS)
        assert e.value.code == capi.E_ARG and "sigma" in str(e.value)
    finally:
        ctx.close()
    # a softmax context
    ctx = bn.HipContext()
    try:
        ctx.set_data(np.random.default_rng(0).standard_normal((20, N_FEATURES)))
        ctx.set_arch_from_weights(weights[0], N_FEATURES, bn.ActFun(fun="tanh").device_kind(), capi.OUT_SOFTMAX, capi.LIK_NONE)
        with pytest.raises(ValueError):
            ctx.predict_sets_predictive(weights, pc.PROBS)
        out = np.empty((20, 4))
        w = np.stack([np.concatenate([layer.ravel() for layer in ws]) for ws in weights])
        rc = ctx._lib.npbnn_predict_sets_predictive(ctx._ctx, capi.dptr(w), None, N_SETS, 0, None, None, 0, None, None, capi.dptr(out), None, None)
        assert rc == capi.E_ARG
    finally:
        ctx.close()


# ---- from a checkpoint
CHECKPOINTS = {"swish_h1_reg3_s4": (bn.RegressTransform, "regression"), "tanh_h2_err2_s7": (bn.RegressTransformError, "regression-error")}


def _checkpoint(tmp_path, name):
    inp = cc.inputs(name)
    out_fn, mode = CHECKPOINTS[name]
    model = types.SimpleNamespace(_data=inp["x"][::-1].copy(), _labels=inp["labels"][::-1].copy(), _test_data=inp["x"], _test_labels=inp["labels"],
                                  _act_fun=cc.act_for(bn, inp["fun"], len(inp["nodes"])), _output_act_fun=out_fn, _estimation_mode=mode)
    pkl = str(tmp_path / "run.pkl")
    with open(pkl, "wb") as fh:
        pickle.dump([model, None, types.SimpleNamespace(_post_weight_samples=inp["samples"])], fh)
    return pkl, inp, model


@pytest.mark.parametrize("name", sorted(CHECKPOINTS))
def test_get_posterior_predictive_on_a_checkpoint(name, tmp_path, monkeypatch):
    pkl, inp, model = _checkpoint(tmp_path, name)
    samples = inp["samples"]
    res = bn.get_posterior_predictive(pkl)
    assert sorted(res) == ["crps", "crps_i", "mean", "n_rows", "n_samples", "probs", "quantiles"]
    assert (res["n_samples"], res["n_rows"]) == (len(samples), cc.N_ROWS) and np.array_equal(res["probs"], (0.025, 0.5, 0.975))
    stack, _ = bn.get_posterior_cat_prob(inp["x"], samples, actFun=cc.act_for(bn, inp["fun"], len(inp["nodes"])), output_act_fun=CHECKPOINTS[name][0])
    sigma = np.array([np.ones(inp["n_out"]) * s["error_prm"] for s in samples]) if CHECKPOINTS[name][1] == "regression" else None
    host = bn.posterior_predictive(stack, CHECKPOINTS[name][1], sigma_sets=sigma, targets=inp["labels"])
    n_sets, n_t = len(samples), res["mean"].shape[1]
    if sigma is None:
        mu, sg, per_sample = stack[:, :, :n_t].reshape(n_sets, -1), stack[:, :, n_t:].reshape(n_sets, -1), False
    else:
        mu, sg, per_sample = stack.reshape(n_sets, -1), sigma, True
    for label, r in (("device", res), ("host", host)):
        worst, by_root = pc.check_quantiles(r["quantiles"].reshape(3, -1), mu, sg, res["probs"], per_sample, name + " " + label)
        worst_crps = pc.check_crps(r["crps_i"].ravel(), mu, sg, np.asarray(inp["labels"], dtype=np.float64).ravel(), per_sample, name + " " + label)
        print("%s %s: largest residual / bound %.3f, %d cells by the root, largest CRPS difference / bound %.4f" % (name, label, worst, by_root, worst_crps))
    np.testing.assert_allclose(res["mean"], host["mean"], rtol=0, atol=(n_sets + 2) * 2.0 ** -52 * np.max(np.abs(mu)))
    np.testing.assert_allclose(res["crps"], np.sum(res["crps_i"], axis=0) / cc.N_ROWS, rtol=1e-15)
    lean = bn.get_posterior_predictive(pkl, crps=False)
    assert sorted(lean) == ["mean", "n_rows", "n_samples", "probs", "quantiles"] and np.array_equal(lean["quantiles"], res["quantiles"])
    unlabelled = bn.get_posterior_predictive(pkl, features=inp["x"], probs=(0.5,))
    assert "crps" not in unlabelled and np.array_equal(unlabelled["quantiles"][0], res["quantiles"][1])
    train = bn.get_posterior_predictive(pkl, features="train")
    # (the training table is the test table upside down: the same cells to the rounding of the float32 forward pass)
    np.testing.assert_allclose(train["quantiles"][:, ::-1], res["quantiles"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(train["crps_i"][::-1], res["crps_i"], rtol=1e-4, atol=1e-4)
    # three row blocks under a small budget: the bits of the unblocked call
    rows = -(-cc.N_ROWS // 3)
    monkeypatch.setenv("NPBNN_HPD_STACK_BYTES", str(n_sets * inp["n_out"] * 4 * rows))
    from npbnn_amd import predictive
    assert predictive.stack_rows(n_sets, inp["n_out"]) == rows and -(-cc.N_ROWS // rows) == 3
    blocked = bn.get_posterior_predictive(pkl)
    for k in res:
        assert np.array_equal(np.asarray(blocked[k]), np.asarray(res[k])), k
