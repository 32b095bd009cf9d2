"""Convergence diagnostics on the GPU: npbnn_op_convergence (one wave per column, the tile in LDS), npbnn_predict_sets_convergence (the
replay's float32 stack read once, the summary reduced on the device) and ``get_posterior_convergence``.

Bounds (every figure is printed by its test before it is asserted):
  RHAT_RTOL / ESS_RTOL  1e-9 / 1e-8 relative, the kernel against the longdouble restatement of tests/convergence_cases.py on the very
              values it was given.  Basis: on these columns the float64 restatement departs from the longdouble one by 1.07e-11 (rhat)
              and 3.47e-11 (ess) at most (the -1e6 + 10 x column at n = 4, where the mean carries the rounding of 1e6), so the bound
              leaves two to three orders for the device's other summation order.  A column whose smallest stop / monotone margin is
              below 1e-6 may be left out of the ess comparison, 1 % of the columns at most; with the seeds of convergence_cases.py
              the smallest margin is 8.87e-06 and none is left out, which (a) asserts.
              Measured on an MI355X, the kernel against the longdouble restatement over every shape and dtype of (a): rhat 2.714e-12
              at most ((1, 9) float64; every float32 case below 5.4e-13), ess 1.741e-11 at most ((4, 250) float64; float32 below
              2.8e-12) - MEASURED_OP_DEVIATION, the float64 restatement's own distance.  The stored-sets entry against
              ``posterior_convergence`` on the float32 values ``predict_sets`` returns: rhat 2.220e-16, ess 3.678e-15 at most.
  PATH_TOL    rhat of the default, float32 and weight-streamed paths against rhat of the float64 forward pass of the test helpers
              (oracle.forward): the float32 network is the error source, relative to a spread between samples that the small
              perturbations of these cases keep near 1e-2.  Measured on an MI355X, largest relative deviation per path, all in swish_c10:
              9.646e-07 (default), 7.788e-07 (f32), 1.275e-06 (streamed); tanh_c2 and genrelu_err2 stay below 1.6e-07 on every
              path.  The bound is 4 x the worst path.  ESS is not compared across paths: a rounding may legitimately move a
              truncation."""
import contextlib
import io
import os

import numpy as np
import pytest

import npbnn_amd as bn
import cases
import convergence_cases as cc
import oracle as orc
from npbnn_amd import HipContext, _capi as capi, device_ops
from npbnn_amd.backend import pack_weights

pytestmark = pytest.mark.gpu

PATHS = {"default": {}, "f32": {"NPBNN_L0": "f32"}, "streamed": {"NPBNN_FORCE_WIDE": "1"}}
MEASURED_OP_DEVIATION = {"rhat": 2.714e-12, "ess": 1.741e-11}                                  # (1, 9) and (4, 250), float64
MEASURED_PATH_DEVIATION = {"default": 9.646e-07, "f32": 7.788e-07, "streamed": 1.275e-06}     # swish_c10 on each path
PATH_TOL = 4 * max(MEASURED_PATH_DEVIATION.values())


# ---- (a) the operator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_op_against_the_longdouble_restatement(shape, dtype):
    ref = cc.reference(shape[0], shape[1], dtype)
    rhat, ess = device_ops.convergence(ref["values"], shape[0])
    dr, de, left = cc.compare(rhat, ess, ref)
    print("op deviation %s %s: rhat %.3e ess %.3e, %d of %d columns left out" % (shape, dtype, dr, de, left, len(rhat)))
    assert left == 0
    assert dr <= cc.RHAT_RTOL and de <= cc.ESS_RTOL


def _tiled(shape, dtype, reps):
    """A shape's 17 columns ``reps`` times over, each copy in another column order; with the reference's index per column."""
    ref = cc.reference(shape[0], shape[1], dtype)
    rs = np.random.default_rng(reps)
    idx = np.concatenate([rs.permutation(17) for _ in range(reps)])
    return ref, idx, np.ascontiguousarray(ref["values"][:, idx])


@pytest.mark.parametrize("shape,dtype,reps", [((2, 50), "float32", 9), ((3, 341), "float64", 5), ((64, 8), "float32", 23), ((2, 2048), "float32", 2)])
def test_op_over_several_workgroups_and_a_ragged_last_tile(shape, dtype, reps):
    """153 columns of 100 float32 values (tiles of 64: two full, one of 25); 85 of 1023 float64 (tiles of 8, the last of 5); 391 of
    512 (tiles of 32, the last of 7); 34 of 4096 (tiles of 4, the last of 2).  Every copy of a column gives the bits of the first, in
    whichever tile and wave it lands, and a strided array the same as a packed one."""
    ref, idx, v = _tiled(shape, dtype, reps)
    rhat, ess = device_ops.convergence(v, shape[0])
    sub = {k: ref[k][idx] for k in ("rhat", "ess", "margin", "rhat_ld", "ess_ld", "margin_ld")}
    dr, de, left = cc.compare(rhat, ess, sub)
    print("tiled op deviation %s %s: rhat %.3e ess %.3e" % (shape, dtype, dr, de))
    assert left == 0 and dr <= cc.RHAT_RTOL and de <= cc.ESS_RTOL
    first = {c: int(np.flatnonzero(idx == c)[0]) for c in range(17)}
    for j, c in enumerate(idx):
        assert rhat[j].tobytes() == rhat[first[c]].tobytes() and ess[j].tobytes() == ess[first[c]].tobytes(), j
    # strided: the columns sit in a wider array
    lib, dev = device_ops._lib()
    wide = np.full((v.shape[0], v.shape[1] + 3), 7.0, dtype=v.dtype)
    wide[:, :v.shape[1]] = v
    r2, e2 = np.empty(v.shape[1]), np.empty(v.shape[1])
    rc = lib.npbnn_op_convergence(dev, wide.ctypes.data, capi.VALUE_F32 if dtype == "float32" else capi.VALUE_F64, shape[0], shape[1],
                                  v.shape[1], wide.shape[1], capi.dptr(r2), capi.dptr(e2))
    assert rc == 0 and r2.tobytes() == rhat.tobytes() and e2.tobytes() == ess.tobytes()


def test_op_refusals():
    lib, dev = device_ops._lib()
    v = np.random.default_rng(0).standard_normal((16, 5))
    r, e = np.empty(5), np.empty(5)

    def raw(values, kind, m, n, n_cols, stride, rp=r, ep=e):
        return lib.npbnn_op_convergence(dev, None if values is None else values.ctypes.data, kind, m, n, n_cols, stride, capi.dptr(rp), capi.dptr(ep))

    assert raw(v, capi.VALUE_F64, 2, 8, 5, 5) == 0
    for args in ((None, capi.VALUE_F64, 2, 8, 5, 5), (v, 2, 2, 8, 5, 5), (v, capi.VALUE_F64, 0, 16, 5, 5), (v, capi.VALUE_F64, 65, 8, 5, 5),
                 (v, capi.VALUE_F64, 4, 4, 5, 5), (v, capi.VALUE_F64, 2, 8193, 5, 5), (v, capi.VALUE_F64, 2, 8, 5, 4), (v, capi.VALUE_F64, 2, 8, -1, 5)):
        assert raw(*args) == capi.E_ARG, args[1:]
    assert raw(v, capi.VALUE_F64, 2, 8, 5, 5, rp=None) == capi.E_ARG
    assert raw(v, capi.VALUE_F64, 2, 8, 0, 5) == 0                       # no columns: nothing to do
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[11, 3] = bad
        assert raw(w, capi.VALUE_F64, 2, 8, 5, 5) == capi.E_ARG and b"NaN or infinite" in lib.npbnn_last_error(None)
        with pytest.raises(capi.NpbnnError):
            device_ops.convergence(w.astype(np.float32), 2)
    with pytest.raises(ValueError):
        device_ops.convergence(v, 3)
    with pytest.raises(ValueError):
        device_ops.convergence(v[:, 0], 1)


# ---- (b) the stored-sets entry --------------------------------------------------------------------------------------------------------
# name -> activation, hidden layers, outputs, bias mode, output kind, rows
NETS = {
    "tanh_c2": dict(fun="tanh", nodes=(5,), n_out=2, bias=1, kind=capi.OUT_SOFTMAX, rows=37),
    "swish_c10": dict(fun="swish", nodes=(8, 6), n_out=10, bias=2, kind=capi.OUT_SOFTMAX, rows=64),
    "genrelu_err2": dict(fun="genReLU", nodes=(6, 5), n_out=4, bias=3, kind=capi.OUT_SOFTPLUS_HALF, rows=51),
    "tanh_c2_long": dict(fun="tanh", nodes=(5,), n_out=2, bias=1, kind=capi.OUT_SOFTMAX, rows=70001),
}
N_FEATURES = 7
N_SETS = 100
OUT_FNS = {capi.OUT_SOFTMAX: orc.out_softmax, capi.OUT_SOFTPLUS_HALF: orc.out_regress_error}
_inputs = {}


def inputs(name):
    """x and 100 weight sets: small weights (no probability saturates) moving as an AR(1) around a teacher, so that a row's
    predictions are a correlated series; the second half starts elsewhere, so that two chains of 50 disagree on some rows."""
    if name not in _inputs:
        spec = NETS[name]
        rs = np.random.default_rng(cases.hash_name("convergence/" + name) % (2 ** 31))
        x = rs.standard_normal((spec["rows"], N_FEATURES))
        shapes = cases.layer_shapes(N_FEATURES, list(spec["nodes"]), spec["n_out"], spec["bias"])
        teacher = [rs.normal(0, 0.3, s) for s in shapes]
        sets, slopes = [], []
        state = [np.zeros(s) for s in shapes]
        for i in range(N_SETS):
            if i == N_SETS // 2:
                state = [rs.normal(0, 0.05, s) for s in shapes]
            state = [0.7 * w + rs.normal(0, 0.03, w.shape) for w in state]
            sets.append([t + w for t, w in zip(teacher, state)])
            slopes.append(rs.uniform(0.0, 0.3, len(spec["nodes"])) if spec["fun"] == "genReLU" else np.zeros(1))
        _inputs[name] = dict(x=x, sets=sets, slopes=slopes, spec=spec)
    return _inputs[name]


def _context(inp):
    spec = inp["spec"]
    act = bn.ActFun(fun=spec["fun"], prm=np.zeros(len(spec["nodes"]))) if spec["fun"] == "genReLU" else bn.ActFun(fun=spec["fun"])
    ctx = HipContext(0)
    ctx.set_data(inp["x"])
    ctx.set_arch_from_weights(inp["sets"][0], N_FEATURES, act.device_kind(), spec["kind"], capi.LIK_NONE)
    return ctx


def _slopes(inp, n_sets):
    return inp["slopes"][:n_sets] if inp["spec"]["fun"] == "genReLU" else None


def _summary_of(rhat, ess, threshold):
    """[outputs, 4] from the pointwise arrays, in numpy."""
    out = np.full((rhat.shape[1], 4), np.nan)
    for o in range(rhat.shape[1]):
        a, e = rhat[:, o], ess[:, o]
        live = ~np.isnan(a)
        if live.any():
            out[o, 0], out[o, 1] = a[live].max(), e[live].min()
        out[o, 2], out[o, 3] = np.count_nonzero(a[live] > threshold), np.count_nonzero(~live)
    return out


def _against_the_definition(got, stack, n_chains):
    """Deviations of the device's rhat / ess from posterior_convergence on ``stack``; an ess beyond the bound is excused only by a
    decision margin of the column below cc.MARGIN (the restatement's), and is counted."""
    want = bn.posterior_convergence(stack, n_chains)
    assert np.array_equal(np.isnan(got["rhat"]), np.isnan(want["rhat"])) and np.array_equal(np.isnan(got["ess"]), np.isnan(want["ess"]))
    live = ~np.isnan(want["rhat"])
    dr = np.abs(got["rhat"][live] - want["rhat"][live]) / want["rhat"][live]
    de = np.zeros(live.shape)
    de[live] = np.abs(got["ess"][live] - want["ess"][live]) / want["ess"][live]
    left = 0
    for r, o in np.argwhere(de > cc.ESS_RTOL):
        assert cc.restate(stack[:, r, o], n_chains)[2] < cc.MARGIN, (r, o, de[r, o])
        de[r, o] = 0.0
        left += 1
    return float(dr.max()), float(de.max()), left


def _sets_entry_case(name, n_sets, n_chains):
    inp = inputs(name)
    sets, slopes = inp["sets"][:n_sets], _slopes(inp, n_sets)
    ctx = _context(inp)
    try:
        y = ctx.predict_sets(sets, act_prm_sets=slopes)
        got = ctx.predict_sets_convergence(sets, n_chains, rhat_threshold=1.05, act_prm_sets=slopes)
        lean = ctx.predict_sets_convergence(sets, n_chains, rhat_threshold=1.05, act_prm_sets=slopes, pointwise=False)
    finally:
        ctx.close()
    assert np.array_equal(y, y.astype(np.float32))                          # (the float32 values themselves)
    dr, de, left = _against_the_definition(got, y, n_chains)
    print("sets deviation %s %d sets in %d chains: rhat %.3e ess %.3e, %d of %d columns left out; max rhat %.3f min ess %.1f"
          % (name, n_sets, n_chains, dr, de, left, got["rhat"].size, got["max_rhat"], got["min_ess"]))
    assert dr <= cc.RHAT_RTOL and de <= cc.ESS_RTOL and left <= got["rhat"].size // 100
    assert (got["n_chains"], got["n_draws"]) == (n_chains, n_sets // n_chains) and got["n_constant"] == 0
    # the summary, reduced on the device, is the pointwise arrays' - exactly - and does not need them on the host
    assert got["per_output"].tobytes() == _summary_of(got["rhat"], got["ess"], 1.05).tobytes()
    assert lean["rhat"] is None and lean["ess"] is None and lean["per_output"].tobytes() == got["per_output"].tobytes()
    assert got["max_rhat"] == got["rhat"].max() and got["min_ess"] == got["ess"].min()
    assert got["frac_rhat_above"] == np.count_nonzero(got["rhat"] > 1.05) / got["rhat"].size


@pytest.mark.parametrize("n_sets,n_chains", [(16, 1), (16, 2), (100, 1), (100, 2)])
@pytest.mark.parametrize("name", ["tanh_c2", "swish_c10", "genrelu_err2"])
def test_sets_entry_against_the_definition_on_its_own_float32_values(name, n_sets, n_chains):
    _sets_entry_case(name, n_sets, n_chains)


def test_sets_entry_on_a_long_table():
    """70001 rows, 140002 columns of 16 values: the evaluation kernels stride over the rows, the diagnostic launch has 2188 workgroups
    (the last with 34 columns) and a workgroup of the summary kernel strides 274 times."""
    _sets_entry_case("tanh_c2_long", 16, 2)


def _same_bytes(a, b):
    for k in ("rhat", "ess", "per_output"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_grouping_of_the_sets_does_not_matter(monkeypatch):
    """100 sets replayed as they come (groups of up to three) and with a distinct slope vector each, which splits them into groups of
    one (tanh ignores the slopes): the same bytes.  On the weight-streamed path, whose replay carries one set per pass whatever
    NPBNN_WIDE_MAX_CAND allows a fused chain pass, that setting changes no bit either."""
    inp = inputs("tanh_c2")
    ctx = _context(inp)
    try:
        together = ctx.predict_sets_convergence(inp["sets"], 2)
        alone = ctx.predict_sets_convergence(inp["sets"], 2, act_prm_sets=[np.full(1, 0.001 * (i + 1)) for i in range(N_SETS)])
        again = ctx.predict_sets_convergence(inp["sets"], 2)
    finally:
        ctx.close()
    _same_bytes(together, alone)
    _same_bytes(together, again)
    monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    res = []
    for cap in (None, "1"):
        if cap:
            monkeypatch.setenv("NPBNN_WIDE_MAX_CAND", cap)
        ctx = _context(inp)
        try:
            assert ctx.is_wide()
            res.append(ctx.predict_sets_convergence(inp["sets"], 2))
        finally:
            ctx.close()
    _same_bytes(res[0], res[1])


def test_constant_columns_through_the_sets_entry():
    """An output whose last-layer weights are zero in every set predicts the same value everywhere: its columns are constant, NaN,
    counted per output, and take no part in the largest rhat and the smallest ess."""
    inp = inputs("genrelu_err2")
    sets = [[w.copy() for w in s] for s in inp["sets"][:16]]
    for s in sets:
        s[-1][1, :] = 0.0
    ctx = _context(inp)
    try:
        got = ctx.predict_sets_convergence(sets, 2, act_prm_sets=_slopes(inp, 16))
    finally:
        ctx.close()
    rows = NETS["genrelu_err2"]["rows"]
    assert np.all(np.isnan(got["rhat"][:, 1])) and np.all(np.isnan(got["ess"][:, 1])) and got["n_constant"] == rows
    np.testing.assert_array_equal(got["per_output"][:, 3], [0, rows, 0, 0])
    assert np.isnan(got["per_output"][1, 0]) and np.isnan(got["per_output"][1, 1]) and got["per_output"][1, 2] == 0
    assert np.isfinite(got["max_rhat"]) and got["max_rhat"] == np.nanmax(got["rhat"]) and got["min_ess"] == np.nanmin(got["ess"])


# ---- (c) the paths against float64 ----------------------------------------------------------------------------------------------------
def _oracle_stack(inp, n_sets):
    spec = inp["spec"]
    return np.array([orc.forward(inp["x"], w, orc.Act(spec["fun"], a), OUT_FNS[spec["kind"]]) for w, a in zip(inp["sets"][:n_sets], inp["slopes"][:n_sets])])


@pytest.mark.parametrize("path", sorted(PATHS))
def test_rhat_on_every_path_against_the_float64_forward_pass(path, monkeypatch):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    worst = 0.0
    for name in ("tanh_c2", "swish_c10", "genrelu_err2"):
        inp = inputs(name)
        want = bn.posterior_convergence(_oracle_stack(inp, N_SETS), 2)
        ctx = _context(inp)
        try:
            got = ctx.predict_sets_convergence(inp["sets"], 2, act_prm_sets=_slopes(inp, N_SETS))
            assert ctx.is_wide() == (path == "streamed") and ctx.l0_mode() == ("f32" if path == "f32" else "f16-split")
        finally:
            ctx.close()
        dev = float(np.max(np.abs(got["rhat"] - want["rhat"]) / want["rhat"]))
        print("path deviation %s %s: rhat %.3e" % (path, name, dev))
        worst = max(worst, dev)
    print("path deviation %s: %.3e (bound %.3e)" % (path, worst, PATH_TOL))
    assert worst <= PATH_TOL


# ---- (d) checkpoints ----------------------------------------------------------------------------------------------------------------
def _quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **k)


def test_get_posterior_convergence_end_to_end(tmp_path, monkeypatch):
    """Two checkpoints written by the package - a run of 12 samples and its continuation of 10 - and a third with the first's samples
    and a constant added to one class's output bias: the first two give finite diagnostics on every row; the first against the third
    has rhat above the threshold on every row."""
    dat = cases.classification_data(7, 160, 6, 3, 40)
    np.random.seed(1234)
    bnn = _quiet(bn.npBNN, dat, n_nodes=[5], actFun=bn.ActFun(fun="tanh"), use_bias_node=3, prior_f=1, p_scale=1, seed=1234, init_std=0.1)
    files = []
    for i, n_it in enumerate((600, 500)):
        mcmc = bn.MCMC(bnn, update_f=[0.05, 0.05], update_ws=[0.075, 0.075], n_iteration=n_it, sampling_f=50, print_f=1000, mcmc_id=i)
        logger = bn.postLogger(bnn, filename="chain%d" % i, wdir=str(tmp_path), log_all_weights=0)
        _quiet(bn.run_mcmc, bnn, mcmc, logger)
        files.append(logger._pklfile)
    model, mc, lg = bn.load_obj(files[0])
    assert len(lg._post_weight_samples) == 12 and len(bn.load_obj(files[1])[2]._post_weight_samples) == 10
    for s in lg._post_weight_samples:
        s["weights"][-1][0, 0] += 3.0
    shifted = os.path.join(str(tmp_path), "shifted.pkl")
    bn.SaveObject([model, mc, lg], shifted)

    res = bn.get_posterior_convergence(files)
    assert (res["n_chains"], res["n_draws"]) == (2, 10) and res["rhat"].shape == (40, 3) and res["n_constant"] == 0
    assert np.all(np.isfinite(res["rhat"])) and np.all(res["ess"] > 0) and np.all(res["ess"] <= 20 * np.log10(20) * (1 + 1e-12))
    assert res["max_rhat"] == res["rhat"].max() and res["min_ess"] == res["ess"].min()
    # the same numbers from the host stack of the very predictions
    kept = bn.load_obj(files[0])[2]._post_weight_samples[2:] + bn.load_obj(files[1])[2]._post_weight_samples
    ctx = HipContext(0)
    try:
        ctx.set_data(model._test_data)
        ctx.set_arch_from_weights(kept[0]["weights"], 6, bn.ActFun(fun="tanh").device_kind(), capi.OUT_SOFTMAX, capi.LIK_NONE)
        y = ctx.predict_sets([s["weights"] for s in kept])
    finally:
        ctx.close()
    dr, de, left = _against_the_definition(res, y, 2)
    print("checkpoint deviation: rhat %.3e ess %.3e, %d left out; max rhat %.3f" % (dr, de, left, res["max_rhat"]))
    assert dr <= cc.RHAT_RTOL and de <= cc.ESS_RTOL and left <= 1
    single = bn.get_posterior_convergence(files[0], features="train", pointwise=False)
    assert (single["n_chains"], single["n_draws"]) == (1, 12) and "rhat" not in single and np.isfinite(single["max_rhat"])

    apart = bn.get_posterior_convergence([files[0], shifted], rhat_threshold=1.01)
    print("shifted chain: smallest rhat %.3f" % apart["rhat"].min())
    assert (apart["n_chains"], apart["n_draws"]) == (2, 12)
    assert np.all(apart["rhat"].max(axis=1) > 1.01) and np.all(apart["rhat"][:, 0] > 1.01)
    assert apart["frac_rhat_above"] >= 1 / 3 and apart["per_output"][0, 2] == 40

    # refusals of the entry itself: a stack over the budget, sets that do not divide into the chains
    packed = np.stack([pack_weights(s["weights"]) for s in kept])
    summary = np.zeros((3, 4))
    monkeypatch.setenv("NPBNN_FI_TIMING", "1")
    ctx = HipContext(0)
    try:
        ctx.set_data(model._test_data)
        ctx.set_arch_from_weights(kept[0]["weights"], 6, bn.ActFun(fun="tanh").device_kind(), capi.OUT_SOFTMAX, capi.LIK_NONE)

        def raw(n_sets, n_chains, which=capi.TRAIN, out=summary, threshold=1.01):
            rc = ctx._lib.npbnn_predict_sets_convergence(ctx._ctx, capi.dptr(packed), None, n_sets, n_chains, which, 1, threshold, None, None, capi.dptr(out))
            return rc, ctx._lib.npbnn_last_error(ctx._ctx).decode(), [ctx.info(i) for i in (capi.INFO_SUMMARY_PASS_NS, capi.INFO_SUMMARY_ACC_NS,
                                                                                              capi.INFO_CONVERGENCE_FINAL_NS)]
        rc, _, ns = raw(20, 2)
        assert rc == 0 and ns[0] > 0 and ns[2] > 0 and summary.tobytes() == res["per_output"].tobytes()
        for args, code, word in (((20, 3), capi.E_ARG, "divide"), ((20, 4), capi.E_ARG, "at least 8"), ((20, 0), capi.E_ARG, ""),
                                 ((0, 1), capi.E_ARG, ""), ((20, 2, 2), capi.E_ARG, "which"), ((20, 2, capi.TEST), capi.E_STATE, ""),
                                 ((20, 2, capi.TRAIN, None), capi.E_ARG, ""), ((20, 2, capi.TRAIN, summary, float("nan")), capi.E_ARG, "NaN")):
            rc, msg, ns = raw(*args)
            assert rc == code and word in msg and ns == [0, 0, 0], args
        monkeypatch.setenv("NPBNN_HPD_STACK_BYTES", str(20 * 39 * 3 * 4))
        rc, msg, ns = raw(20, 2)
        assert rc == capi.E_NOMEM and "predict_sets_convergence" in msg and "at most 39 rows fit" in msg and ns == [0, 0, 0]
        with pytest.raises(capi.NpbnnError) as e:
            ctx.predict_sets_convergence(packed, 2)
        assert e.value.code == capi.E_NOMEM
        monkeypatch.setenv("NPBNN_HPD_STACK_BYTES", str(20 * 40 * 3 * 4))
        assert raw(20, 2)[0] == 0
        with pytest.raises(ValueError):
            ctx.predict_sets_convergence(packed, 3)
    finally:
        ctx.close()
