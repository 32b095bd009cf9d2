"""GPU: npbnn_predict_sets_support over its whole envelope (tests/support_envelope_cases.py; the CPU guards of the case table and of the
restatement are tests/test_host_support_envelope.py).

On one context a case runs ``predict_sets`` and then ``predict_sets_support`` in both modes; the cube, the Bayes-factor table, the keep
mask and the NaN-masked summary must be the bytes of the plain numpy restatement on the float32 predictions ``predict_sets`` returned
(a summary's NaNs compared by position).  Nothing is excused and nothing has a tolerance: the tables are integers, the quotients one
float64 division.  A case that names an edge - a row whose p IS a threshold or the cutoff, a row whose Bayes factor IS a threshold, a
tied vote - asserts on the device's own summary that the edge occurred."""
import numpy as np
import pytest

import support_envelope_cases as sec
from npbnn_amd import HipContext, _capi as capi

pytestmark = pytest.mark.gpu

TRAIN, TEST = capi.TRAIN, capi.TEST
PATHS = {"default": {}, "f32": {"NPBNN_L0": "f32"}, "streamed": {"NPBNN_FORCE_WIDE": "1"}}        # test_hip_support.PATHS


@pytest.fixture
def opened():
    """contexts a test opened: closed whatever the test's end"""
    held = []
    yield held
    for ctx in held:
        ctx.close()


@pytest.fixture(scope="module")
def n_cu():
    ctx = HipContext(0)
    try:
        n = ctx.info(capi.INFO_N_CU)
    finally:
        ctx.close()
    assert n > 0
    return n


def _set_path(path, monkeypatch):
    for k in ("NPBNN_L0", "NPBNN_FORCE_WIDE", "NPBNN_FI_HOST"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)


def _open(opened, inp):
    """(context, slot of the table the statistic is taken on)"""
    ctx = HipContext(0)
    opened.append(ctx)
    which = TRAIN
    if inp["train_x"] is not None:
        ctx.set_data(inp["train_x"])
        ctx.set_data(inp["x"], TEST)
        which = TEST
    else:
        ctx.set_data(inp["x"])
    ctx.set_arch_from_weights(inp["sets"][0], inp["x"].shape[1], capi.ACT_LEAKY if inp["slopes"] else capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
    return ctx, which


def _assert_path(ctx, path):
    assert ctx.is_wide() == (path == "streamed") and ctx.l0_mode() == ("f32" if path == "f32" else "f16-split")


def _support(ctx, inp, which, mode, prior, bft, labels=None, want_summary=True, want_keep=True):
    return ctx.predict_sets_support(inp["sets"], mode, inp["labels"] if labels is None else labels, inp["thresholds"], prior_summary=prior,
                                    bf_thresholds=() if bft is None else bft, cutoff=inp["cutoff"], act_prm_sets=inp["slopes"], which=which,
                                    want_summary=want_summary, want_keep=want_keep)


def _assert_same(got, want, label):
    assert got["cube"].dtype == np.int64 and (got["bf"] is None or got["bf"].dtype == np.int64) and got["summary"].dtype == np.float64
    wrong = sec.differing_fields(got, want)
    assert wrong == [], "%s: %s differ from the restatement" % (label, wrong)


def _run_case(name, path, opened, n_cu, monkeypatch):
    _set_path(path, monkeypatch)
    inp = sec.inputs(name, n_cu)
    case, labels, thr = inp["case"], inp["labels"], inp["thresholds"]
    plan = sec.launch_plan(case, n_cu)
    ctx, which = _open(opened, inp)
    stack = ctx.predict_sets(inp["sets"], act_prm_sets=inp["slopes"], which=which)
    _assert_path(ctx, path)
    assert stack.shape == (case["sets"], plan["n_rows"], case["n_out"])
    print("\n  %s on the %s path: %d rows in %d workgroups (%d strides), %d cells %s, %d thresholds %s" % (
        name, path, plan["n_rows"], plan["grid"], plan["strides"], plan["cells"], "in LDS" if plan["lds_cube"] else "global", len(thr),
        "in LDS" if plan["lds_thr"] else "global"))
    for mode in sec.MODES:
        label = "%s mode %d %s" % (name, mode, path)
        summary = sec.summarise(stack, mode)
        prior, bft = inp["prior"], inp["bf_thresholds"]
        if case["prior"] == "built":
            # a first call's returned summary: the restatement's own, and the prior is built from what the device returned
            first = _support(ctx, inp, which, mode, None, None)
            assert sec.same_bytes(first["summary"], summary), label
            prior, bft = sec.built_prior(name, first["summary"])
        want = sec.restatement(summary, labels, thr, prior, bft, inp["cutoff"])
        got = _support(ctx, inp, which, mode, prior, bft)
        _assert_path(ctx, path)
        # the replay's passes: sets that share a slope vector travel together, as many as the launch plan carries (three at the most)
        passes, widest = ctx.replay_info()
        assert passes >= len(inp["groups"]) and 1 <= widest <= sec.MAX_GROUP, label
        if path == "default" and name in ("default", "slopes_aabbba"):
            assert (passes, widest) == (len(inp["groups"]), max(g for _, g in inp["groups"])), label
        _assert_same(got, want, label)
        assert got["cube"].sum() == plan["n_rows"] and (got["bf"] is None or got["bf"].sum() == plan["n_rows"])
        # the edge the case names, on the device's own summary (without a cutoff's NaN rows: a call that masks nothing)
        dev = got["summary"] if inp["cutoff"] is None else ctx.predict_sets_summary(inp["sets"], mode, act_prm_sets=inp["slopes"], which=which)[0]
        assert sec.same_bytes(dev, summary), label
        mine = sec.restatement(dev, labels, thr, prior, bft, inp["cutoff"])
        edge = sec.edge_count(case, mode, mine, dev, thr, bft, inp["cutoff"])
        if edge is not None:
            print("    mode %d: %d rows on the %s edge" % (mode, edge, case["edge"]))
            assert edge > 0, label
        assert not sec.must_tie(case, mode) or sec.tied_rows(dev) > 0, label
        if case["outputs"]:
            for ws in (False, True):
                for wk in (False, True):
                    res = _support(ctx, inp, which, mode, prior, bft, want_summary=ws, want_keep=wk)
                    assert res["cube"].tobytes() == got["cube"].tobytes(), (label, ws, wk)
                    assert (res["summary"] is None) == (not ws) and (res["keep"] is None) == (not wk)
                    assert not ws or sec.same_bytes(res["summary"], want["summary"])
                    assert not wk or sec.same_bytes(res["keep"], want["keep"])


@pytest.mark.parametrize("name", list(sec.CASES))
def test_case(name, opened, n_cu, monkeypatch):
    _run_case(name, "default", opened, n_cu, monkeypatch)


@pytest.mark.parametrize("path", ["f32", "streamed"])
@pytest.mark.parametrize("name", sec.ROUTED)
def test_route(name, path, opened, n_cu, monkeypatch):
    _run_case(name, path, opened, n_cu, monkeypatch)


def _bytes(res):
    return [None if res[k] is None else np.asarray(res[k]).tobytes() for k in sec.FIELDS]


@pytest.mark.parametrize("name", sec.SAME_BYTES)
def test_same_bytes_every_call(name, opened, n_cu, monkeypatch):
    """The counts are integer atomics: two calls on one context and one on a fresh context give the same bytes."""
    _set_path("default", monkeypatch)
    inp = sec.inputs(name, n_cu)
    ctx, which = _open(opened, inp)
    for mode in sec.MODES:
        first = _support(ctx, inp, which, mode, inp["prior"], inp["bf_thresholds"])
        second = _support(ctx, inp, which, mode, inp["prior"], inp["bf_thresholds"])
        fresh_ctx, _ = _open(opened, inp)
        fresh = _support(fresh_ctx, inp, which, mode, inp["prior"], inp["bf_thresholds"])
        fresh_ctx.close()
        assert first["cube"].sum() == len(inp["labels"])
        assert _bytes(first) == _bytes(second) == _bytes(fresh), (name, mode)


@pytest.mark.parametrize("name,position", [("default", "last row of the ragged last workgroup"), ("grid_capped", "second stride of the capped grid")])
def test_bad_label_is_refused_and_the_next_call_is_right(name, position, opened, n_cu, monkeypatch):
    _set_path("default", monkeypatch)
    inp = sec.inputs(name, n_cu)
    case, plan = inp["case"], sec.launch_plan(inp["case"], n_cu)
    n = plan["n_rows"]
    row = n - 1
    # the row is the last of a ragged last workgroup; on the capped grid it is reached only in a second stride
    assert n % sec.WORKGROUP != 0 and (plan["strides"] == 2 and row >= plan["grid"] * sec.WORKGROUP) == (name == "grid_capped")
    ctx, which = _open(opened, inp)
    stack = ctx.predict_sets(inp["sets"], act_prm_sets=inp["slopes"], which=which)
    for mode in sec.MODES:
        want = sec.restatement(sec.summarise(stack, mode), inp["labels"], inp["thresholds"], cutoff=inp["cutoff"])
        for bad in (case["n_out"], -1):
            lab = np.array(inp["labels"])
            lab[row] = bad
            with pytest.raises(capi.NpbnnError) as e:
                _support(ctx, inp, which, mode, None, None, labels=lab)
            assert e.value.code == capi.E_ARG and "label" in str(e.value), position
            _assert_same(_support(ctx, inp, which, mode, None, None), want, "%s mode %d after a refusal" % (name, mode))
