"""The host side of the four attribution drivers' device seams (no GPU): what ``_pdp_row_means``, ``_ale_local_effects``,
``_saliency_means`` and ``_shapley_device`` hand the library, and the branch of ``get_pdp`` / ``get_ale`` that runs a custom output
callable on the host.  ``HipContext`` is replaced, where the seams look it up (npbnn_amd.backend, at call time), by a stand-in that
records every call, answers ``predict`` with the oracle's float64 forward pass and the ``predict_*`` entries with a sentinel."""
import importlib
import inspect

import numpy as np
import pytest

import ale_cases
import npbnn_amd as bn
import oracle as orc
from attrib_common import _apply_override, softmax_np
from npbnn_amd import _capi as capi

backend = importlib.import_module("npbnn_amd.backend")
posterior = importlib.import_module("npbnn_amd.posterior")
PDP, ALE, SAL, SHAP = (importlib.import_module("npbnn_amd." + m) for m in ("pdp", "ale", "saliency", "shapley"))
REAL = backend.HipContext

N_ROWS, N_FEATURES, NODES, N_OUT, N_SETS = 37, 5, (4, 3), 3, 3
N_HIDDEN = len(NODES)
ENTRIES = ("predict_pdp", "predict_ale", "predict_saliency", "predict_shapley")
SENTINEL = {name: object() for name in ENTRIES}


def _bound(name, ctx, a, kw):
    """the arguments of a call by the real method's names, defaults filled in"""
    b = inspect.signature(getattr(REAL, name)).bind(ctx, *a, **kw)
    b.apply_defaults()
    return dict(b.arguments)


def _entry(name):
    def entry(self, *a, **kw):
        self.calls.append((name, _bound(name, self, a, kw)))
        if self.fail:
            raise RuntimeError("refused")
        return SENTINEL[name]
    return entry


class _Recorder:
    fun, fail, made = "tanh", False, None

    def __init__(self, device=None):
        self.calls, self.tables, self.n_rows, self.n_out, self.closed = [], {}, {}, None, 0
        self.made.append(self)

    def set_data(self, *a, **kw):
        args = _bound("set_data", self, a, kw)
        self.calls.append(("set_data", args))
        self.tables[args["which"]] = args["X"]
        self.n_rows[args["which"]] = args["X"].shape[0]

    def set_arch_from_weights(self, *a, **kw):
        args = _bound("set_arch_from_weights", self, a, kw)
        self.calls.append(("arch", args))
        self.n_out = args["weights"][-1].shape[0]

    def predict(self, *a, **kw):
        args = _bound("predict", self, a, kw)
        if args["col_override"] is not None:
            args["col_override"] = np.array(args["col_override"], dtype=float, copy=True)
        self.calls.append(("predict", args))
        assert not args["apply_out_fn"]
        x = _apply_override(self.tables[args["which"]], args["col_override"])
        prm = None if args["act_prm"] is None else np.asarray(args["act_prm"], dtype=float)
        return orc.forward_logits(x, args["weights"], orc.Act(self.fun, prm=prm))

    def predict_sets(self, *a, **kw):
        args = _bound("predict_sets", self, a, kw)
        self.calls.append(("predict_sets", args))
        return np.zeros((len(args["weight_sets"]), self.n_rows[args["which"]], self.n_out))

    predict_pdp, predict_ale, predict_saliency, predict_shapley = (_entry(n) for n in ENTRIES)

    def close(self):
        self.closed += 1


@pytest.fixture
def recorder(monkeypatch):
    rec = type("Recorder", (_Recorder,), dict(made=[]))
    monkeypatch.setattr(backend, "HipContext", rec)
    return rec


def _inputs(fun, transform):
    """a table (Fortran order: the seams must hand over a C-contiguous copy) with an ordinal column 1, N_SETS samples with a slope
    vector each - an entry longer than the hidden layers - and the transform that switches columns 2 and 4 off"""
    rs = np.random.default_rng(17)
    x = rs.standard_normal((N_ROWS, N_FEATURES))
    x[:, 1] = rs.integers(0, 3, N_ROWS)
    dims = [N_FEATURES] + list(NODES) + [N_OUT]
    weights = [[rs.normal(0, 1.0 / np.sqrt(dims[i] + 1), (dims[i + 1], dims[i] + 1)) for i in range(len(dims) - 1)] for _ in range(N_SETS)]
    alphas = [rs.uniform(0.01, 0.5, N_HIDDEN + 1) for _ in range(N_SETS)]
    tr = bn.data_transform_obj(np.array([1, 1, 0, 1, 0]), x.mean(axis=0)) if transform else None
    return np.asfortranarray(x), weights, alphas, bn.ActFun(fun=fun), tr


def _slopes(fun, alphas):
    return [np.asarray(a, dtype=float).ravel()[:N_HIDDEN] for a in alphas] if fun == "genReLU" else None


def _override(tr):
    return None if tr is None else np.asarray(tr.column_override(), dtype=float)


SHAPLEY_EXTRA = dict(rows=np.array([0, 5, 5, 36]), bg_rows=np.array([3, 1]), player_of=np.array([0, 1, 1, 2, 3], dtype=np.int32),
                     perms=np.array([[0, 1, 2, 3], [3, 2, 1, 0]], dtype=np.int32))
GRID = np.array([[0.0, -1.0], [2.0, 1.0], [1.0, 0.5]])
EDGES = np.array([-1.5, -0.2, 0.4, 1.5])


def _call_seam(seam, inp, out_fn=bn.SoftMax):
    """(what the seam returned, the tables it must have handed over as (table, slot), the entry's name, its own arguments)"""
    x, weights, alphas, act, tr = inp
    own = dict(SHAPLEY_EXTRA)
    if seam == "pdp":
        return PDP._pdp_row_means(x, [1, 3], GRID, weights, alphas, act, out_fn, tr), [(x, capi.TRAIN)], "predict_pdp", dict(focal=[1, 3], grid=GRID)
    if seam == "ale":
        return ALE._ale_local_effects(x, 2, EDGES, weights, alphas, act, out_fn, tr), [(x, capi.TRAIN)], "predict_ale", dict(focal=2, edges=EDGES)
    if seam == "saliency":
        return SAL._saliency_means(x, weights, alphas, act, out_fn, tr), [(x, capi.TRAIN)], "predict_saliency", {}
    if seam == "shapley":
        own.update(which=capi.TRAIN, which_bg=capi.TRAIN, want_phi=False)
        got = SHAP._shapley_device(x, own["rows"], None, own["bg_rows"], own["player_of"], own["perms"], weights, alphas, act, out_fn, tr, False)
        return got, [(x, capi.TRAIN)], "predict_shapley", own
    bg = np.asfortranarray(np.asarray(x)[::2] + 0.5)
    own.update(which=capi.TEST, which_bg=capi.TRAIN, want_phi=True)
    got = SHAP._shapley_device(x, own["rows"], bg, own["bg_rows"], own["player_of"], own["perms"], weights, alphas, act, out_fn, tr, True)
    return got, [(bg, capi.TRAIN), (x, capi.TEST)], "predict_shapley", own


SEAMS = ("pdp", "ale", "saliency", "shapley", "shapley_background")


def _check_tables_and_arch(ctx, tables, weights, act, out_kind):
    assert [c[0] for c in ctx.calls[:len(tables) + 1]] == ["set_data"] * len(tables) + ["arch"]
    for (_, got), (want, slot) in zip(ctx.calls, tables):
        assert got["which"] == slot and got["X"].dtype == np.float64 and got["X"].flags.c_contiguous and np.array_equal(got["X"], want)
    arch = ctx.calls[len(tables)][1]
    assert arch["weights"] is weights[0] and arch["in_dim"] == N_FEATURES and arch["act_kind"] == act.device_kind()
    assert arch["out_kind"] == out_kind and arch["lik_kind"] == capi.LIK_NONE and arch["n_targets"] == 0 and not arch["final_activation"]


@pytest.mark.parametrize("transform", [False, True], ids=["plain", "transform"])
@pytest.mark.parametrize("fun", ["tanh", "genReLU"])
@pytest.mark.parametrize("seam", SEAMS)
def test_what_the_library_is_handed(seam, fun, transform, recorder):
    inp = _inputs(fun, transform)
    x, weights, alphas, act, tr = inp
    got, tables, name, own = _call_seam(seam, inp)
    assert got is SENTINEL[name]
    (ctx,) = recorder.made
    assert ctx.closed == 1 and len(ctx.calls) == len(tables) + 2 and ctx.calls[-1][0] == name
    _check_tables_and_arch(ctx, tables, weights, act, capi.OUT_SOFTMAX)
    args = ctx.calls[-1][1]
    assert np.stack(list(args["weight_sets"])).tobytes() == np.stack([bn.pack_weights(w) for w in weights]).tobytes()
    if fun == "genReLU":
        assert len(args["act_prm_sets"]) == N_SETS
        for given, want in zip(args["act_prm_sets"], _slopes(fun, alphas)):
            assert np.shape(given) == (N_HIDDEN,) and np.array_equal(given, want)
        assert len({tuple(s) for s in args["act_prm_sets"]}) == N_SETS
    else:
        assert args["act_prm_sets"] is None
    if tr is None:
        assert args["col_override"] is None      # (no row of NaN: to the library the two are one path, and the drivers say it one way)
    else:
        assert np.array_equal(args["col_override"], tr.column_override(), equal_nan=True) and np.isnan(args["col_override"]).sum() == 3
    assert args["apply_out_fn"] is True
    for key, want in own.items():
        assert np.array_equal(args[key], want), key
    if seam in ("pdp", "ale", "saliency"):
        assert args["which"] == capi.TRAIN


@pytest.mark.parametrize("out_fn,applied", [(None, False), (bn.RegressTransform, True)], ids=["none", "regress"])
@pytest.mark.parametrize("seam", SEAMS)
def test_output_kinds(seam, out_fn, applied, recorder):
    """no output function: the last layer's values (identity, not applied); RegressTransform: identity, applied"""
    inp = _inputs("tanh", False)
    _, tables, name, _ = _call_seam(seam, inp, out_fn=out_fn)
    (ctx,) = recorder.made
    _check_tables_and_arch(ctx, tables, inp[1], inp[3], capi.OUT_IDENTITY)
    assert ctx.calls[-1][0] == name and ctx.calls[-1][1]["apply_out_fn"] is applied and ctx.closed == 1


@pytest.mark.parametrize("seam", SEAMS)
def test_the_context_is_closed_once_when_the_entry_raises(seam, recorder):
    recorder.fail = True
    with pytest.raises(RuntimeError, match="refused"):
        _call_seam(seam, _inputs("genReLU", True))
    (ctx,) = recorder.made
    assert ctx.closed == 1


@pytest.mark.parametrize("seam,text", [("saliency", "get_saliency: a custom output callable has no device kind and cannot be differentiated"),
                                       ("shapley", "get_shapley: a custom output callable has no device kind"),
                                       ("shapley_background", "get_shapley: a custom output callable has no device kind")])
def test_saliency_and_shapley_refuse_a_custom_callable_before_the_device(seam, text, recorder):
    with pytest.raises(ValueError, match="^%s$" % text):
        _call_seam(seam, _inputs("tanh", False), out_fn=softmax_np)
    assert recorder.made == []


def test_no_samples_fail_as_before(recorder):
    """get_pdp has no check of its own for an empty posterior: the seam fails on the first sample it asks for, the table already
    uploaded, and closes the context."""
    x, _, _, act, _ = _inputs("tanh", False)
    with pytest.raises(IndexError):
        bn.get_pdp(np.asarray(x), [1], "classification", N_OUT, act, bn.SoftMax, [], [], None)
    (ctx,) = recorder.made
    assert [c[0] for c in ctx.calls] == ["set_data"] and ctx.closed == 1


# ---- a custom output callable: pdp and ale run it on the host, pass by pass -----------------------------------------------------------
def _check_host_passes(ctx, x, weights, act, want):
    """``want``: per pass (index of the sample, its slopes or None, the override row)"""
    _check_tables_and_arch(ctx, [(x, capi.TRAIN)], weights, act, capi.OUT_IDENTITY)
    passes = ctx.calls[2:]
    assert [c[0] for c in passes] == ["predict"] * len(want) and ctx.closed == 1
    for (_, args), (i, slopes, co) in zip(passes, want):
        assert args["weights"] is weights[i] and args["which"] == capi.TRAIN and args["apply_out_fn"] is False
        assert (args["act_prm"] is None) if slopes is None else np.array_equal(args["act_prm"], slopes)
        assert np.array_equal(args["col_override"], co, equal_nan=True)


@pytest.mark.parametrize("focal", [[1, 3], [1], [2]], ids=["two_columns", "ordinal", "switched_off"])
@pytest.mark.parametrize("transform", [False, True], ids=["plain", "transform"])
@pytest.mark.parametrize("fun", ["tanh", "genReLU"])
def test_get_pdp_runs_a_custom_callable_on_the_host(fun, transform, focal, recorder):
    recorder.fun = fun
    x, weights, alphas, act, tr = _inputs(fun, transform)
    res = bn.get_pdp(x, focal, "classification", N_OUT, act, softmax_np, weights, alphas, tr)
    grid = bn.make_pdp_features(x, focal)
    assert np.array_equal(res["feature"], grid) and len(grid) == (2 if len(focal) == 2 else 3 if focal == [1] else 100)
    slopes, override = _slopes(fun, alphas), _override(tr)
    want, means = [], []
    for point in grid:
        co = np.full(N_FEATURES, np.nan) if override is None else override.copy()
        for col, v in zip(focal, point):
            if np.isnan(co[col]):
                co[col] = v
        want += [(i, None if slopes is None else slopes[i], co) for i in range(N_SETS)]
        xg = _apply_override(x, co)
        means.append(np.mean([softmax_np(orc.forward_logits(xg, w, orc.Act(fun, prm=alphas[i]))) for i, w in enumerate(weights)], axis=0))
    (ctx,) = recorder.made
    _check_host_passes(ctx, x, weights, act, want)
    means = np.cumsum(np.array(means), axis=2)
    assert res["pdp"].shape == (len(grid), N_OUT, 3)
    assert np.abs(res["pdp"][:, :, 0] - means.mean(axis=1)).max() < 1e-12
    q = np.quantile(means, (0.025, 0.975), axis=1)
    assert np.abs(res["pdp"][:, :, 1] - q[0]).max() < 1e-12 and np.abs(res["pdp"][:, :, 2] - q[1]).max() < 1e-12
    if transform and focal == [2]:
        assert np.ptp(res["pdp"], axis=0).max() == 0
    else:
        assert np.ptp(res["pdp"][:, :, 0], axis=0).max() > 1e-3
    assert act._prm is alphas[-1]


@pytest.mark.parametrize("focal", [0, 2], ids=["free", "switched_off"])
@pytest.mark.parametrize("transform", [False, True], ids=["plain", "transform"])
@pytest.mark.parametrize("fun", ["tanh", "genReLU"])
def test_get_ale_runs_a_custom_callable_on_the_host(fun, transform, focal, recorder):
    recorder.fun = fun
    x, weights, alphas, act, tr = _inputs(fun, transform)
    res = bn.get_ale(x, focal, "classification", N_OUT, act, softmax_np, weights, alphas, tr, n_bins=5)
    edges = bn.make_ale_edges(x, focal, n_bins=5)
    assert np.array_equal(res["feature"], edges) and len(edges) == 6
    slopes, override = _slopes(fun, alphas), _override(tr)
    want = []
    for i in range(N_SETS):
        for z in edges:
            co = np.full(N_FEATURES, np.nan) if override is None else override.copy()
            if np.isnan(co[focal]):
                co[focal] = z
            want.append((i, None if slopes is None else slopes[i], co))
    (ctx,) = recorder.made
    _check_host_passes(ctx, x, weights, act, want)
    counts, effects = ale_cases.local_effects(x, focal, edges, weights, fun=fun, out_fn=softmax_np, slopes=alphas, override=override)
    assert np.array_equal(res["counts"], counts) and res["counts"].dtype == np.int64 and counts.sum() == N_ROWS
    assert res["local_effects"].shape == (N_SETS, 5, N_OUT) and np.abs(res["local_effects"] - effects).max() < 1e-12
    curve = ale_cases.curve(counts, effects)
    assert np.abs(res["ale_samples"] - curve).max() < 1e-12 and np.abs(res["ale"][:, :, 0] - curve.mean(axis=0)).max() < 1e-12
    q = np.quantile(curve, (0.025, 0.975), axis=0)
    assert np.abs(res["ale"][:, :, 1] - q[0]).max() < 1e-12 and np.abs(res["ale"][:, :, 2] - q[1]).max() < 1e-12
    if transform and focal == 2:
        assert np.all(res["local_effects"] == 0)
    else:
        assert np.abs(res["local_effects"]).max() > 1e-3
    assert act._prm is alphas[-1]


# ---- the predictor of the statistics drivers describes the network from the same place ------------------------------------------------
@pytest.mark.parametrize("form", ["vector", "column", "row", "matrix"])
def test_sample_predictor_hands_over_the_same_slope_bytes(form, recorder):
    """The slopes ``_SamplePredictor`` passes on reach ``_pack_sets`` as the bytes of ``np.asarray(alphas)[:n_hidden]`` through it,
    whatever the shape the checkpoint stored them in."""
    x, weights, alphas, act, _ = _inputs("genReLU", False)
    shape = dict(vector=(-1,), column=(-1, 1), row=(1, -1), matrix=(N_HIDDEN + 1, 2))[form]
    if form == "matrix":
        alphas = [np.concatenate([a, a + 0.5]) for a in alphas]
    alphas = [a.reshape(shape) for a in alphas]
    samples = [dict(weights=w, alphas=a) for w, a in zip(weights, alphas)]
    with posterior._SamplePredictor(N_FEATURES, samples, act, bn.SoftMax) as pred:
        y = pred.predict(np.ascontiguousarray(x))
    assert y.shape == (N_SETS, N_ROWS, N_OUT)
    (ctx,) = recorder.made
    assert [c[0] for c in ctx.calls] == ["set_data", "arch", "predict_sets"] and ctx.closed == 1
    arch, args = ctx.calls[1][1], ctx.calls[2][1]
    assert arch["weights"] is weights[0] and arch["in_dim"] == N_FEATURES and arch["act_kind"] == act.device_kind()
    assert arch["out_kind"] == capi.OUT_SOFTMAX and arch["lik_kind"] == capi.LIK_NONE and args["apply_out_fn"] is True
    assert np.stack(list(args["weight_sets"])).tobytes() == np.stack([bn.pack_weights(w) for w in weights]).tobytes()
    bare = REAL.__new__(REAL)
    bare._ctx = None
    bare.arch = capi.Arch()
    bare.arch.n_layers = N_HIDDEN + 1
    zeros = np.zeros((N_SETS, 1))
    before = bare._pack_sets(zeros, [np.asarray(a, dtype=float)[:N_HIDDEN] for a in alphas], "t")[1]
    assert before.shape == (N_SETS, N_HIDDEN) and bare._pack_sets(zeros, args["act_prm_sets"], "t")[1].tobytes() == before.tobytes()
