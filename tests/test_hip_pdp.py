"""Partial dependence on the GPU (npbnn_predict_pdp, bn.get_pdp / bn.pdp) against the reference's outputs (tests/golden/pdp.npz) and
the float64 oracle, on both routes: the grid-batched kernel (NPBNN_INFO_PDP_ROUTE 1) and one pass per grid point (2)."""
import contextlib
import io

import numpy as np
import pytest

import npbnn_amd as bn
import oracle as orc
import pdp_cases
from attrib_common import softmax_np
from npbnn_amd import _capi as capi

pytestmark = pytest.mark.gpu

TOL = 2e-5      # probabilities and regression outputs: float32 forward pass against float64
CASES = pdp_cases.load()


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **k)


def device_means(x, weights, focal, grid, fun="tanh", out_kind=capi.OUT_SOFTMAX, slopes=None, override=None, which=capi.TRAIN,
                 apply_out_fn=True, x_test=None, trainable=False, want_l0=False):
    """(per grid point and row of the table ``which`` the mean over the sets, route taken[, layer-0 path of the last launch])"""
    ctx = bn.HipContext()
    try:
        ctx.set_data(x)
        if x_test is not None:
            ctx.set_data(x_test, capi.TEST)
        ctx.set_arch_from_weights(weights[0], x.shape[1], bn.ActFun(fun=fun, trainable=trainable).device_kind(), out_kind, capi.LIK_NONE)
        y = ctx.predict_pdp(weights, focal, grid, act_prm_sets=slopes, col_override=override, which=which, apply_out_fn=apply_out_fn)
        route = ctx.info(capi.INFO_PDP_ROUTE)
        return (y, route, ctx.l0_mode()) if want_l0 else (y, route)
    finally:
        ctx.close()


def oracle_means(x, weights, focal, grid, fun="tanh", out_fn=orc.out_softmax, slopes=None):
    res = []
    for point in grid:
        xg = np.array(x, copy=True)
        xg[:, focal] = point
        preds = [out_fn(orc.forward_logits(xg, w, orc.Act(fun, prm=None if slopes is None else np.asarray(slopes[i]))))
                 for i, w in enumerate(weights)]
        res.append(np.mean(preds, axis=0))
    return np.array(res)


@pytest.mark.parametrize("wide", [False, True], ids=["resident", "streamed"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_get_pdp_matches_reference(name, wide, monkeypatch):
    if wide:
        monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    c = CASES[name]
    args = pdp_cases.call_args(bn, c)
    res = bn.get_pdp(*args)
    assert np.array_equal(res["feature"], c["feature"])
    np.testing.assert_allclose(res["pdp"], c["pdp"], rtol=0, atol=TOL)
    assert np.array_equal(np.asarray(args[4]._prm, dtype=float), c["last_prm"])


@pytest.mark.parametrize("wide", [False, True], ids=["resident", "streamed"])
@pytest.mark.parametrize("name", ["continuous", "onehot", "genrelu", "regression_onehot"])
def test_route_taken(name, wide, monkeypatch):
    if wide:
        monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    c = CASES[name]
    out_kind = capi.OUT_SOFTMAX if c["mode"] == "classification" else capi.OUT_IDENTITY
    slopes = [np.asarray(a)[: len(c["weights"][0]) - 1] for a in c["alphas"]] if c["fun"] == "genReLU" else None
    y, route = device_means(c["x"], c["weights"], c["focal"], c["grid"], c["fun"], out_kind, slopes)
    assert route == (2 if wide else 1)
    want = oracle_means(c["x"], c["weights"], c["focal"], c["grid"], c["fun"],
                        orc.out_softmax if out_kind == capi.OUT_SOFTMAX else orc.out_identity, slopes)
    np.testing.assert_allclose(y, want, rtol=0, atol=TOL)


def _drawn(n_rows, n_features, n_nodes, n_out, n_sets, seed):
    rs = np.random.default_rng(seed)
    x = rs.standard_normal((n_rows, n_features))
    dims = [n_features] + list(n_nodes) + [n_out]
    weights = [[rs.normal(0, 1.0 / np.sqrt(dims[i] + 1), (dims[i + 1], dims[i] + 1)) for i in range(len(dims) - 1)]
               for _ in range(n_sets)]
    return x, weights


def test_routes_agree_on_config2_shapes(monkeypatch):
    """[32, 8] on 256 features, 10 classes, one continuous focal feature with 100 grid points: the grid-batched kernel against the
    per-grid route."""
    x, weights = _drawn(30000, 256, (32, 8), 10, 7, seed=5)
    grid = bn.make_pdp_features(x, [3])
    y1, r1 = device_means(x, weights, [3], grid)
    monkeypatch.setenv("NPBNN_PDP_PER_GRID", "1")
    y2, r2 = device_means(x, weights, [3], grid)
    assert (r1, r2) == (1, 2)
    assert np.abs(y1 - y2).max() < 1e-5
    np.testing.assert_allclose(y1[::9], oracle_means(x, weights, [3], grid[::9]), rtol=0, atol=TOL)


@pytest.mark.parametrize("per_grid", [False, True])
def test_grid_in_chunks(per_grid, monkeypatch):
    """An accumulator budget of three grid points: 11 grid points run in four chunks and give what one chunk gives."""
    x, weights = _drawn(5003, 40, (20, 6), 5, 4, seed=9)
    grid = np.linspace(-2, 2, 22).reshape(11, 2)
    if per_grid:
        monkeypatch.setenv("NPBNN_PDP_PER_GRID", "1")
    whole, _ = device_means(x, weights, [1, 7], grid)
    monkeypatch.setenv("NPBNN_PDP_ACC_BYTES", str(3 * 5003 * 5 * 4))
    chunked, route = device_means(x, weights, [1, 7], grid)
    assert route == (2 if per_grid else 1)
    assert np.array_equal(whole, chunked)
    np.testing.assert_allclose(chunked, oracle_means(x, weights, [1, 7], grid), rtol=0, atol=TOL)


@pytest.mark.parametrize("per_grid", [False, True])
@pytest.mark.parametrize("n_nodes", [(24, 7), (50, 5), (16, 12, 6)])
def test_more_sets_than_a_pass_with_their_own_slopes(per_grid, n_nodes, monkeypatch):
    """genReLU with a different slope per set and layer, more sets than one pass of either route carries."""
    x, weights = _drawn(2111, 33, n_nodes, 4, 7, seed=len(n_nodes) * 100 + n_nodes[0])
    rs = np.random.default_rng(1)
    slopes = [rs.uniform(0.01, 0.5, len(n_nodes)) for _ in weights]
    grid = np.linspace(-1.5, 2.5, 9).reshape(9, 1)
    if per_grid:
        monkeypatch.setenv("NPBNN_PDP_PER_GRID", "1")
    y, route = device_means(x, weights, [5], grid, fun="genReLU", slopes=slopes)
    assert route == (2 if per_grid else 1)
    np.testing.assert_allclose(y, oracle_means(x, weights, [5], grid, fun="genReLU", slopes=slopes), rtol=0, atol=TOL)


def test_get_pdp_with_a_custom_output_callable():
    """A softmax the package does not know has no device kind: get_pdp runs one pass per (grid point, sample) for the last layer's
    values and applies the callable on the host.  257 rows (one past a block), genReLU with a slope per sample, an ordinal focal
    column of three levels: against the float64 restatement on the table the device holds, and against the same call with
    bn.SoftMax, whose softmax runs on the device."""
    x, weights = _drawn(257, 5, (4,), 3, 2, seed=21)
    x[:, 1] = np.random.default_rng(22).integers(0, 3, 257)
    slopes = [np.array([0.1]), np.array([0.35])]

    def call(out_fn):
        return bn.get_pdp(x, [1], "classification", 3, bn.ActFun(fun="genReLU"), out_fn, weights, slopes, None)

    res, same = call(softmax_np), call(bn.SoftMax)
    assert res["feature"].shape == (3, 1) and np.array_equal(res["feature"], same["feature"]) and res["pdp"].shape == (3, 3, 3)
    held = x.astype(np.float32).astype(np.float64)
    means = np.cumsum(oracle_means(held, weights, [1], res["feature"], fun="genReLU", out_fn=softmax_np, slopes=slopes), axis=2)
    want = np.stack([means.mean(axis=1)] + list(np.quantile(means, (0.025, 0.975), axis=1)), axis=-1)
    print("\npdp custom callable: max|host branch - float64| %.3e, max|host branch - device softmax| %.3e (bar %.1e)"
          % (np.abs(res["pdp"] - want).max(), np.abs(res["pdp"] - same["pdp"]).max(), TOL))
    assert np.ptp(want[:, :, 0], axis=0).max() > 100 * TOL
    np.testing.assert_allclose(res["pdp"], want, rtol=0, atol=TOL)
    np.testing.assert_allclose(res["pdp"], same["pdp"], rtol=0, atol=TOL)


def test_pdp_of_a_checkpoint(tmp_path):
    """bn.pdp on a checkpoint written by postLogger, against an oracle loop over grid points and stored samples."""
    rs = np.random.default_rng(4)
    n = 300
    x = np.zeros((n, 7))
    x[:, 0] = rs.normal(0, 1, n)
    x[:, 1] = rs.integers(0, 4, n)
    x[:, 2:4] = rs.normal(0, 1, (n, 2))
    x[np.arange(n), 4 + rs.integers(0, 3, n)] = 1
    labels = (x[:, 0] + 0.5 * x[:, 1] > 1).astype(int) + (x[:, 4] > 0)
    dat = dict(data=x, labels=labels, test_data=np.zeros((0, 7)), test_labels=np.zeros(0))
    np.random.seed(1234)
    bnn = bn.npBNN(dat, n_nodes=[6, 4], actFun=bn.ActFun(fun="tanh"), use_bias_node=2)
    mcmc = bn.MCMC(bnn, n_iteration=200, sampling_f=20, print_f=1000, n_post_samples=10)
    logger = bn.postLogger(bnn, wdir=str(tmp_path), filename="pdp", log_all_weights=0)
    quiet(bn.run_mcmc, bnn, mcmc, logger)
    res = bn.pdp(logger._pklfile, [[0], [1], [4, 5, 6]])
    _, _, lg = bn.load_obj(logger._pklfile)
    samples = lg._post_weight_samples
    weights = [s["weights"] for s in samples]
    assert [r["feature"].shape for r in res] == [(100, 1), (4, 1), (3, 3)]
    for focal, r in zip([[0], [1], [4, 5, 6]], res):
        assert r["pdp"].shape == (r["feature"].shape[0], 3, 3)
        means = np.cumsum(oracle_means(x, weights, focal, r["feature"]), axis=2)
        np.testing.assert_allclose(r["pdp"][:, :, 0], means.mean(axis=1), rtol=0, atol=TOL)
        q = np.quantile(means, (0.025, 0.975), axis=1)
        np.testing.assert_allclose(r["pdp"][:, :, 1], q[0], rtol=0, atol=TOL)
        np.testing.assert_allclose(r["pdp"][:, :, 2], q[1], rtol=0, atol=TOL)
