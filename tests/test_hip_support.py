"""Confidence thresholds and Bayes-factor support on the GPU: npbnn_predict_sets_support (threshold cube, Bayes-factor table, NaN-masked
summary and keep mask from one pass over the accumulator npbnn_predict_sets_summary's replay leaves), ``get_posterior_threshold`` and
``predictBNN``'s threshold / prior keywords, against the reference's values (tests/golden/support.npz).

The device's forward pass is float32, the reference's float64: class probabilities agree within ``TOL`` (test_hip_posterior.TOL).
A row is BORDERLINE (support_cases.candidate_cells, from the golden values alone) when that much can move it to another cell: mode 1 -
its largest summary value within TOL of a threshold or of the second largest; mode 0 - votes are integers and the quotient
votes / n_sets is the reference's own, so only a sample whose two leading probabilities lie within TOL can vote otherwise.  Every cube
cell must lie between the counts with the borderline rows left out and put in; with no borderline row the cube, the sweep table and
the selected row are the reference's exactly (every mode-0 case but two, which have one such row)."""
import contextlib
import importlib
import io
import os

import numpy as np
import pytest

import npbnn_amd as bn
import support_cases as sc
from npbnn_amd import HipContext, _capi as capi
from test_hip_posterior import TOL

pytestmark = pytest.mark.gpu

posterior = importlib.import_module("npbnn_amd.posterior")
support = importlib.import_module("npbnn_amd.support")

assert TOL == sc.TOL
PATHS = {"default": {}, "f32": {"NPBNN_L0": "f32"}, "streamed": {"NPBNN_FORCE_WIDE": "1"}}


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = f(*a, **k)
    return res, out.getvalue()


def _set_path(path, monkeypatch):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("NPBNN_FI_HOST", raising=False)


def _context(inp, path):
    ctx = HipContext(0)
    ctx.set_data(inp["x"])
    ctx.set_arch_from_weights(inp["samples"][0]["weights"], inp["x"].shape[1], sc.act_for(bn, inp["fun"]).device_kind(), capi.OUT_SOFTMAX,
                              capi.LIK_NONE)
    return ctx


def _sets(inp):
    slopes = [np.asarray(s["alphas"], dtype=float)[:2] for s in inp["samples"]] if inp["fun"] == "genReLU" else None
    return [s["weights"] for s in inp["samples"]], slopes


def _bf_table(summary, prior, labels, thresholds):
    call = np.argmax(summary, axis=1)
    p, r = summary[np.arange(len(call)), call], prior[np.arange(len(call)), call]
    with np.errstate(divide="ignore", invalid="ignore"):
        factor = (p / (1e-10 + 1 - p)) / (r / (1e-10 + 1 - r))
    table = np.zeros((len(thresholds) + 1, 2), dtype=np.int64)
    np.add.at(table, (np.sum(factor[:, None] > np.asarray(thresholds)[None, :], axis=1), (call == labels).astype(int)), 1)
    return table


def _check_against_golden(cube, case, label):
    """The borderline rule on a cube; with no borderline row, the reference's cube, table and selected row exactly."""
    name, n_samples, mode = case
    g, k = sc.load(), sc.key(*case)
    labels = sc.inputs(name, n_samples)["labels"]
    n_border = sc.assert_cube_within_borderline(cube, g[k + "/summary"], labels, mode, n_samples, g[sc.key(name, n_samples) + "/near_ties"],
                                                label=label)
    exact = np.array_equal(cube, g[k + "/cube"])
    print("%s: %d borderline rows of %d, cube %s the reference's" % (label, n_border, len(labels), "is" if exact else "is not"))
    assert n_border <= 0.02 * len(labels)
    if n_border == 0:
        np.testing.assert_array_equal(cube, g[k + "/cube"], err_msg=label)
    if exact:
        table = support.table_from_cube(cube, sc.GRID)
        np.testing.assert_array_equal(table, g[k + "/table"], err_msg=label)
        np.testing.assert_array_equal(table[np.min(np.where(np.round(table[:, 1], 2) >= g[k + "/target"]))], g[k + "/selected"])
    return exact


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_cube_and_bayes_factor_table(case, path, monkeypatch):
    name, n_samples, mode = case
    _set_path(path, monkeypatch)
    inp = sc.inputs(name, n_samples)
    labels, prior = inp["labels"], sc.load()[name + "/prior_mean"]
    sets, slopes = _sets(inp)
    ctx = _context(inp, path)
    try:
        res = ctx.predict_sets_support(sets, mode, labels, sc.GRID, prior_summary=prior, bf_thresholds=sc.BF_GRID, act_prm_sets=slopes,
                                       want_summary=True, want_keep=True)
        assert ctx.is_wide() == (path == "streamed") and ctx.l0_mode() == ("f32" if path == "f32" else "f16-split")
        summary, table = ctx.predict_sets_summary(sets, mode, labels=labels, act_prm_sets=slopes)
        cube, bf = res["cube"], res["bf"]
        assert cube.dtype == np.int64 and cube.shape == (100, inp["n_classes"], inp["n_classes"]) and bf.shape == (5, 2)
        # the two entries share their replay: the same summary bit for bit, the same confusion table
        np.testing.assert_array_equal(res["summary"], summary)
        np.testing.assert_array_equal(cube.sum(axis=0), table)
        assert res["keep"].all()
        # the tables are those of the device's own summary, exactly: float64 comparisons against the caller's thresholds, the Bayes
        # factor in CalcTP_BF's order of operations
        np.testing.assert_array_equal(cube, sc.cube_of(summary, labels))
        np.testing.assert_array_equal(bf, _bf_table(summary, prior, labels, sc.BF_GRID))
        for i, t in enumerate(sc.BF_GRID):
            with np.errstate(divide="ignore", invalid="ignore"):
                assert bf[i + 1:, 1].sum() / len(labels) == bn.CalcTP_BF(summary, prior, labels, threshold=t)
                assert bf[i + 1:, 0].sum() / len(labels) == bn.CalcFP_BF(summary, prior, labels, threshold=t)
        # ... and the reference's, up to the rows float32 can move
        exact = _check_against_golden(cube, case, "%s %s" % (sc.case_id(case), path))
        if exact and mode == 0:
            np.testing.assert_array_equal(bf, _bf_table(sc.load()[sc.key(*case) + "/summary"], prior, labels, sc.BF_GRID))
        # thresholds of the caller's: none, one, and more than are staged in LDS (the search then reads global memory)
        none = ctx.predict_sets_support(sets, mode, labels, [], act_prm_sets=slopes)
        np.testing.assert_array_equal(none["cube"][0], table)
        assert none["bf"] is None and none["summary"] is None and none["keep"] is None
        many = np.linspace(0.001, 0.999, 999)
        np.testing.assert_array_equal(ctx.predict_sets_support(sets, mode, labels, many, act_prm_sets=slopes)["cube"],
                                      sc.cube_of(summary, labels, many))
    finally:
        ctx.close()


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("case", [("tanh", 10, 0), ("genrelu", 9, 1), ("swish_bias3", 10, 1)], ids=sc.case_id)
def test_cutoff_masks_the_summary(case, path, monkeypatch):
    name, n_samples, mode = case
    _set_path(path, monkeypatch)
    inp = sc.inputs(name, n_samples)
    sets, slopes = _sets(inp)
    ctx = _context(inp, path)
    try:
        summary = ctx.predict_sets_summary(sets, mode, act_prm_sets=slopes)[0]
        for cutoff in (0.7, 0.0, 1.0):
            res = ctx.predict_sets_support(sets, mode, inp["labels"], [cutoff], cutoff=cutoff, act_prm_sets=slopes, want_summary=True,
                                           want_keep=True)
            keep = res["keep"]
            np.testing.assert_array_equal(keep, summary.max(axis=1) > cutoff)
            np.testing.assert_array_equal(np.isnan(res["summary"]).all(axis=1), ~keep)
            np.testing.assert_array_equal(np.isnan(res["summary"]).any(axis=1), ~keep)
            np.testing.assert_array_equal(res["summary"][keep], summary[keep])
            assert res["cube"][1].sum() == keep.sum()
        assert 0 < (summary.max(axis=1) > 0.7).sum() < len(summary)
    finally:
        ctx.close()


def test_errors():
    inp = sc.inputs("tanh", 9)
    sets, _ = _sets(inp)
    ctx = _context(inp, "default")
    try:
        for bad in (4, -1):
            lab = inp["labels"].copy()
            lab[77] = bad
            with pytest.raises(capi.NpbnnError) as e:
                ctx.predict_sets_support(sets, 0, lab, sc.GRID)
            assert e.value.code == capi.E_ARG and "label" in str(e.value)
        # the C entry checks its thresholds itself, before any launch
        from npbnn_amd.backend import pack_weights
        import ctypes as C
        packed = np.stack([pack_weights(w) for w in sets])
        lab = np.ascontiguousarray(inp["labels"], dtype=np.int64)
        cube = np.zeros((3, 4, 4), dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        for thr in (np.array([0.5, 0.4]), np.array([0.1, np.nan])):
            rc = ctx._lib.npbnn_predict_sets_support(ctx._ctx, capi.dptr(packed), None, len(sets), capi.TRAIN, 1, 0, lab.ctypes.data_as(i64),
                                                     capi.dptr(thr), 2, None, None, 0, None, cube.ctypes.data_as(i64), None, None, None)
            assert rc == capi.E_ARG and not cube.any()
    finally:
        ctx.close()


# ---- end to end on a checkpoint written by this package ---------------------------------------------------------------------------
def _checkpoint(tmp_path, inp, n_samples):
    dat = dict(data=inp["x"], labels=inp["labels"], test_data=inp["x"], test_labels=inp["labels"])
    np.random.seed(1234)
    bnn = bn.npBNN(dat, n_nodes=list(sc.N_NODES), actFun=sc.act_for(bn, inp["fun"]), use_bias_node=inp["bias"])
    mcmc = bn.MCMC(bnn, n_iteration=50, sampling_f=10, print_f=1000, n_post_samples=n_samples)
    logger = bn.postLogger(bnn, wdir=str(tmp_path), filename="run", log_all_weights=0)
    logger._post_weight_samples = inp["samples"]
    pkl = os.path.join(str(tmp_path), "run.pkl")
    bn.SaveObject([bnn, mcmc, logger], pkl)
    return pkl


@pytest.fixture
def cubes(monkeypatch):
    """The cubes HipContext.predict_sets_support hands back during a test."""
    seen = []
    real = HipContext.predict_sets_support

    def wrapped(self, *a, **kw):
        res = real(self, *a, **kw)
        seen.append(res["cube"])
        return res
    monkeypatch.setattr(HipContext, "predict_sets_support", wrapped)
    return seen


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("case", [("tanh", 10, 0), ("tanh", 9, 1), ("genrelu", 10, 1), ("swish_bias3", 9, 0), ("swish_bias3", 10, 1)], ids=sc.case_id)
def test_threshold_and_predictbnn_end_to_end(case, path, cubes, monkeypatch, tmp_path):
    name, n_samples, mode = case
    _set_path(path, monkeypatch)
    g, k = sc.load(), sc.key(*case)
    inp = sc.inputs(name, n_samples)
    labels, golden = inp["labels"], g[k + "/summary"]
    pkl = _checkpoint(tmp_path, inp, n_samples)
    target = float(g[k + "/target"])
    out_file = str(tmp_path / "sweep.txt")
    (row, printed) = quiet(bn.get_posterior_threshold, pkl, target, mode, out_file, write_predictions=False)
    assert len(cubes) == 1 and not [f for f in os.listdir(str(tmp_path)) if "_pred_" in f]
    exact = _check_against_golden(cubes[0], case, "%s %s end to end" % (sc.case_id(case), path))
    table = support.table_from_cube(cubes[0], sc.GRID)
    np.testing.assert_array_equal(row, table[np.min(np.where(np.round(table[:, 1], 2) >= target))])
    np.testing.assert_array_equal(np.loadtxt(out_file, skiprows=1), np.round(table, 3))
    assert printed.startswith("Selected threshold: PP = %s yielding" % np.round(row[0], 3))
    if exact:
        np.testing.assert_array_equal(row, g[k + "/selected"])
    # the device route and this package's host route give the same row; the default call leaves predictBNN's files
    monkeypatch.setenv("NPBNN_FI_HOST", "1")
    (host_row, _) = quiet(bn.get_posterior_threshold, pkl, target, mode)
    monkeypatch.delenv("NPBNN_FI_HOST")
    np.testing.assert_array_equal(host_row, row)
    (again, _) = quiet(bn.get_posterior_threshold, pkl, target, mode)
    np.testing.assert_array_equal(again, row)
    assert len(cubes) == 2 and os.path.exists(str(tmp_path / "run_pred_pr.npy")) and os.path.exists(str(tmp_path / "run_accuracy.txt"))
    # predictBNN: a target accuracy, then a cutoff with prior samples
    res, _ = quiet(bn.predictBNN, inp["x"], pkl, test_labels=labels, target_acc=target, post_summary_mode=mode, verbose=0, fname="t")
    masked = np.isnan(res["post_prob_predictions"]).all(axis=1)
    clear = np.abs(golden.max(axis=1) - row[0]) > TOL if mode == 1 else \
        ~np.isin(np.arange(len(labels)), g[sc.key(name, n_samples) + "/near_ties"][:, 0])
    np.testing.assert_array_equal(masked[clear], ~(golden.max(axis=1) > row[0])[clear])
    assert np.mean(~masked) == row[2]
    stack = np.load(str(tmp_path / "t_run_pred_pr.npy"))
    assert stack.shape == (n_samples,) + golden.shape and np.isnan(stack[:, masked]).all() and not np.isnan(stack[:, ~masked]).any()
    prior_pkl = str(tmp_path / "prior.pkl")
    bn.SaveObject(inp["prior"], prior_pkl)
    res, printed = quiet(bn.predictBNN, inp["x"], pkl, test_labels=labels, post_cutoff=0.7, threshold=0.6, bf=20.0,
                         pickle_file_prior=prior_pkl, post_summary_mode=mode, fname="c")
    assert sorted(res) == ['confusion_matrix', 'mean_accuracy', 'post_prob_predictions']
    assert res["confusion_matrix"].shape == (inp["n_classes"],) * 2 and res["confusion_matrix"].sum() == len(labels)
    masked = np.isnan(res["post_prob_predictions"]).all(axis=1)
    clear = np.abs(golden.max(axis=1) - 0.7) > TOL if mode == 1 else clear
    np.testing.assert_array_equal(masked[clear], ~(golden.max(axis=1) > 0.7)[clear])
    if mode == 1:
        np.testing.assert_allclose(res["post_prob_predictions"][~masked], golden[~masked], atol=TOL, rtol=0)
    # the rates printed: within the rows float32 can move (one row is 1 / n) of the reference's
    lines = dict(line.split(": ") for line in printed.splitlines() if line.startswith(("True positive", "False positive")))
    want = dict(zip(("True positive rate", "False positive rate"), g[k + "/tp_fp"][1]))
    want.update(zip(("True positive rate (BF)", "False positive rate (BF)"), g[k + "/tp_fp_bf"][list(sc.BF_GRID).index(20.0)]))
    n_border = len(sc.candidate_cells(golden, labels, mode, n_samples, g[sc.key(name, n_samples) + "/near_ties"]))
    for what, value in want.items():
        print("%s %s: %s, the reference's %s" % (sc.case_id(case), what, lines[what], value))
        if "(BF)" not in what:
            assert abs(float(lines[what]) - value) <= (n_border + 0.5) / len(labels), what
    assert "(TP: %s; FP: %s)" % (lines["True positive rate"], lines["False positive rate"]) in open(str(tmp_path / "c_run_accuracy.txt")).read()


# ---- a larger shape ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_config2_shape_device_route_is_the_host_route(mode, monkeypatch):
    """100k x 256, 10 classes, 30 samples, no golden: the cube against this package's host functions on the downloaded stack, under the
    borderline rule with the stack's own summary as the yardstick (both rest on the same float32 predictions: equality is expected,
    and printed)."""
    _set_path("default", monkeypatch)
    rs = np.random.default_rng(12)
    n, f, c, s = 100000, 256, 10, 30
    x = rs.standard_normal((n, f))
    dims = [f, 32, 8, c]
    teacher = [rs.normal(0, 0.25, (dims[i + 1], dims[i] + 1)) for i in range(3)]
    sets = [[t + rs.normal(0, 0.08, t.shape) for t in teacher] for _ in range(s)]
    ctx = HipContext(0)
    try:
        ctx.set_data(x)
        ctx.set_arch_from_weights(sets[0], f, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
        labels = np.argmax(ctx.predict(teacher), axis=1)
        flip = rs.random(n) < 0.05
        labels = np.where(flip, (labels + rs.integers(1, c, n)) % c, labels).astype(np.int64)
        stack = ctx.predict_sets(sets)
        summary = posterior._summarise(stack, mode)
        cube = ctx.predict_sets_support(sets, mode, labels, sc.GRID)["cube"]
    finally:
        ctx.close()
    n_border = sc.assert_cube_within_borderline(cube, summary, labels, mode, s, sc.near_ties_of(stack), label="config-2 shape, mode %d" % mode)
    print("config-2 shape, mode %d: %d borderline rows, cube %s the host's" % (mode, n_border, "is" if np.array_equal(cube, sc.cube_of(summary, labels)) else "is not"))
    rows = []
    for t in sc.GRID:
        try:
            r = bn.get_accuracy_threshold(summary, labels, threshold=t)
            rows.append([t, r['accuracy'], r['retained_samples']])
        except ZeroDivisionError:
            pass
    if np.array_equal(cube, sc.cube_of(summary, labels)):
        np.testing.assert_array_equal(support.table_from_cube(cube, sc.GRID), np.array(rows))
