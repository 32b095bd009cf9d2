"""Every stored-sample entry through the fp16-range float32 repeat on the GPU, on the resident and on the weight-streamed path
(tests/repeat_cases.py has the cases, the model of the replay loop and the comparisons; tests/test_host_sets_repeat.py checks those
without a GPU).  A set whose scaled layer-0 weight leaves the fp16 range makes replay_sets (npbnn_sets.hip) or run_point_passes
(npbnn_pdp.hip) repeat work on the float32 path; per case and path, on one context:

  1. ctx.replay_info() and ctx.l0_mode() after predict_sets and after every entry equal repeat_cases.expected_replay - no case passes
     on inputs that never repeat;
  2. the stack is finite, every set's bytes are those of its own single prediction on the path the model names for it, and under tanh
     within TOL of the float64 oracle;
  3. every entry against its definition on that same stack, by the comparison and the bar of the entry's own GPU module;
  4. a byte-exact twin: with a planted set in every group the call's outputs are those of a context under set_l0_precision("f32");
     on the streamed path a tanh case with a distinct slope vector per set (groups of one) gives the bytes of the sets together;
  5. no state is left: the same entry on clean sets on the same context runs fp16-split and gives a fresh context's bytes; under
     set_l0_precision("f16") every entry raises E_RANGE in its own name, and the next clean call is the fresh context's again;
  6. route 2 of predict_pdp and predict_ale: the bytes of the same call under set_l0_precision("f32"), within the modules' bars of the
     float64 references, ALE's counts exact.

No tolerance is this module's: every bar is imported.  The largest deviation per entry and path is printed (NOTES.md has the figures
measured on an MI355X)."""
import numpy as np
import pytest

import npbnn_amd as bn
import predictive_cases as pc
import repeat_cases as rc
import support_cases as sc
from npbnn_amd import HipContext, _capi as capi
from test_hip_wide_replay import _flat_bytes

pytestmark = pytest.mark.gpu

OUT_KINDS = {"cat": capi.OUT_SOFTMAX, "reg": capi.OUT_IDENTITY, "err": capi.OUT_SOFTPLUS_HALF}
WHO = {"summary0": "predict_sets_summary", "summary1": "predict_sets_summary", "hpd": "predict_sets_hpd", "support0": "predict_sets_support",
       "support1": "predict_sets_support", "lppd": "predict_sets_lppd", "loo": "predict_sets_loo", "uncertainty": "predict_sets_uncertainty",
       "calibration": "predict_sets_calibration", "convergence": "predict_sets_convergence", "predictive": "predict_sets_predictive"}
PAIRS = [(name, path) for name, c in rc.CASES.items() for path in c["paths"]]
_fresh = {}                     # (family, path, entry) -> bytes of the entry on the family's clean sets on a fresh context
_worst = {}                     # (entry, path) -> largest deviation in units of its bar seen in this process


def _set_path(path, monkeypatch):
    if path == "streamed":
        monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")


def _which(case):
    return capi.TEST if case["test_rows"] else capi.TRAIN


def _context(inp, path, l0=None):
    case = inp["case"]
    ctx = HipContext(0)
    try:
        which = _which(case)
        if case["test_rows"]:
            ctx.set_data(inp["train_x"], capi.TRAIN)
        ctx.set_data(inp["x"], which)
        if inp["labels"] is not None:
            ctx.set_labels(inp["labels"], which)
        else:
            ctx.set_targets(inp["targets"], which)
        if l0:
            ctx.set_l0_precision(l0)
        act = capi.ACT_TANH if case["fun"] == "tanh" else bn.ActFun(fun="genReLU", prm=np.zeros(2)).device_kind()
        ctx.set_arch_from_weights(inp["sets"][0], case["features"], act, OUT_KINDS[case["kind"]], capi.LIK_NONE)
        assert ctx.is_wide() == (path == "streamed")
    except Exception:
        ctx.close()
        raise
    return ctx


def _call(ctx, entry, inp, sets, slopes, sigma):
    """the entry on ``sets`` (as many as the entry takes: repeat_cases.sets_for), with their slopes and sigmas"""
    case = inp["case"]
    kind, which = case["kind"], _which(case)
    kw = dict(act_prm_sets=slopes, which=which)
    lik = capi.LIK_CATEGORICAL if kind == "cat" else capi.LIK_GAUSS
    if entry in ("summary0", "summary1"):
        return ctx.predict_sets_summary(sets, int(entry[-1]), labels=inp["labels"], **kw)
    if entry == "hpd":
        return ctx.predict_sets_hpd(sets, rc.HPD_LEVEL, **kw)
    if entry in ("support0", "support1"):
        return ctx.predict_sets_support(sets, int(entry[-1]), inp["labels"], sc.GRID, want_summary=True, **kw)
    if entry == "lppd":
        return ctx.predict_sets_lppd(sets, lik, sigma_sets=sigma, **kw)
    if entry == "loo":
        return ctx.predict_sets_loo(sets, lik, sigma_sets=sigma, log_lik=True, **kw)
    if entry == "uncertainty":
        return ctx.predict_sets_uncertainty(sets, **kw)
    if entry == "calibration":
        return ctx.predict_sets_calibration(sets, n_bins=rc.N_BINS, levels=rc._levels(kind), sigma_sets=sigma, **kw)
    if entry == "convergence":
        return ctx.predict_sets_convergence(sets, 1, **kw)
    assert entry == "predictive", entry
    return ctx.predict_sets_predictive(sets, pc.PROBS, sigma_sets=sigma, targets=inp["targets"], **kw)


def _args(entry, inp, sets=None):
    """(sets, slopes, sigma) of the entry's call on the case's planted sets, or on ``sets``"""
    n, sigma = rc.sets_for(entry, inp)
    slopes = rc.slopes_of(inp["case"], n)
    return (inp["sets"] if sets is None else sets)[:n], None if slopes is None else slopes[:n], sigma


def _distinct_slopes(n):
    return [np.full(2, 0.001 * (i + 1)) for i in range(n)]


def _clean_sets(inp):
    return rc.family(inp["case"]["family"])["sets"]


def _fresh_bytes(entry, inp, path):
    """the entry on the family's clean sets on a fresh context (computed once per process and path)"""
    key = (inp["case"]["family"], path, entry)
    if key not in _fresh:
        ctx = _context(inp, path)
        try:
            _fresh[key] = _flat_bytes(_call(ctx, entry, inp, *_args(entry, inp, _clean_sets(inp))))
            assert ctx.l0_mode() == "f16-split"
        finally:
            ctx.close()
    return _fresh[key]


def _stack(ctx, inp, n, want, apply_out_fn):
    slopes = rc.slopes_of(inp["case"], n)
    y = ctx.predict_sets(inp["sets"][:n], act_prm_sets=slopes, which=_which(inp["case"]), apply_out_fn=apply_out_fn)
    got = ctx.replay_info() + (ctx.l0_mode(),)
    assert got == want[:3], ("predict_sets", n, got, want[:3])
    assert np.all(np.isfinite(y)) and np.array_equal(y, y.astype(np.float32))
    return y


# ---- 1 - 3, the streamed twin of 4 and the clean call of 5: per case and path, on one context --------------------------------------------
@pytest.mark.parametrize("name,path", PAIRS)
def test_case(name, path, monkeypatch):
    _set_path(path, monkeypatch)
    inp = rc.inputs(name)
    case = inp["case"]
    kind, n, which, planted = case["kind"], inp["n"], _which(case), case["planted"]
    caps = rc.caps_of(case, path)
    want = {m: rc.expected_replay(m, rc.slopes_of(case, m), planted, path, *caps) for m in {n, rc.sets_for("convergence", inp)[0]}}
    ctx = _context(inp, path)
    try:
        # 1. and 2.: the stacks, as the entries see them (with and without the output function; eight sets for convergence)
        stacks = {(m, out): _stack(ctx, inp, m, want[m], out) for m in want if m == n or "convergence" in case["entries"] for out in (True, False)}
        print("%s %s: sets per pass %s, replay %s, computed on %s" % (name, path, caps, want[n][:3], want[n][3]))
        assert "f32" in want[n][3] and want[n][0] > rc.expected_replay(n, rc.slopes_of(case, n), (), path, *caps)[0]       # (it does repeat)
        y = stacks[(n, True)]
        slopes = rc.slopes_of(case, n)
        single = {}
        for mode in ("f32", "f16-split"):
            ctx.set_l0_precision("f32" if mode == "f32" else "auto")
            for i in range(n):
                if want[n][3][i] == mode:
                    single[i] = ctx.predict(inp["sets"][i], act_prm=None if slopes is None else slopes[i], which=which)
                    assert ctx.l0_mode() == mode, (i, mode)
        worst_oracle = 0.0
        for i in range(n):
            np.testing.assert_array_equal(y[i], single[i], err_msg="set %d, computed on %s" % (i, want[n][3][i]))
            if case["fun"] == "tanh":
                err = float(np.max(np.abs(y[i] - rc.outputs_of(inp["z64"][i], kind))))
                worst_oracle = max(worst_oracle, err)
                assert err <= rc.TOL, (i, err)
        print("%s %s: max |device - float64 oracle| over the sets %.3e (TOL %.1e)" % (name, path, worst_oracle, rc.TOL))
        # 3., 4. (streamed: groups of one give the same bytes) and 5. (a clean call behind the planted one)
        for entry in case["entries"]:
            sets, slopes, sigma = _args(entry, inp)
            m = len(sets)
            got = _call(ctx, entry, inp, sets, slopes, sigma)
            info = ctx.replay_info() + (ctx.l0_mode(),)
            assert info == want[m][:3], (entry, info, want[m][:3])
            res = rc.compare(entry, inp, got, stacks[(m, True)], stacks[(m, False)], sigma)
            print("%s %s %-12s %s, %d excused (%.2f %%)" % (name, path, entry, "%d outputs differ" % res["worst"] if entry in rc.EXACT else
                  "deviation %.3e of bar %.3e" % (res["worst"], res["bound"]), res["excused"], 100 * res["share"]))
            _worst[(entry, path)] = max(_worst.get((entry, path), 0.0), res["worst"] / res["bound"] if res["bound"] else res["worst"])
            assert res["share"] <= rc.EXCUSED_SHARE, (entry, res)
            assert res["worst"] <= res["bound"], (entry, res)
            if path == "streamed" and case["fun"] == "tanh":
                alone = _call(ctx, entry, inp, sets, _distinct_slopes(m), sigma)
                info = ctx.replay_info() + (ctx.l0_mode(),)
                assert info == rc.expected_replay(m, _distinct_slopes(m), planted, path, *caps)[:3], (entry, info)
                assert _flat_bytes(alone) == _flat_bytes(got), entry
            clean = _call(ctx, entry, inp, *_args(entry, inp, _clean_sets(inp)))
            assert ctx.l0_mode() == "f16-split", entry
            assert ctx.replay_info() == rc.expected_replay(m, slopes, (), path, *caps)[:2], entry
            assert _flat_bytes(clean) == _fresh_bytes(entry, inp, path), entry
    finally:
        ctx.close()
    for key in sorted(_worst):
        if key[1] == path:
            print("largest so far %-12s %-9s %.3e %s" % (key + (_worst[key], "outputs" if key[0] in rc.EXACT else "of its bar")))


# ---- 4. the whole call in float32 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", rc.PATHS)
@pytest.mark.parametrize("kind", ["cat", "reg", "err"])
def test_a_planted_set_in_every_group_gives_the_float32_contexts_bytes(kind, path, monkeypatch):
    """Resident: sets 1, 4 and 6, one per group; streamed: all seven.  Every pass that delivers runs in float32, so every entry's
    outputs are those of the same call on a context under set_l0_precision("f32").  (The convergence entry's eighth set is clean: on
    the streamed path it runs fp16-split behind the seven, and that entry has no float32 twin there.)"""
    _set_path(path, monkeypatch)
    inp = rc.inputs("%s_planted_%s" % (kind, rc._tag(rc.EVERY_GROUP[path])))
    case = inp["case"]
    caps = rc.caps_of(case, path)
    auto, f32 = _context(inp, path), None
    try:
        f32 = _context(inp, path, l0="f32")
        for entry in case["entries"]:
            if entry == "convergence" and path == "streamed":
                continue
            args = _args(entry, inp)
            m = len(args[0])
            a = _call(auto, entry, inp, *args)
            want = rc.expected_replay(m, None, case["planted"], path, *caps)
            assert auto.replay_info() + (auto.l0_mode(),) == want[:3] and set(want[3]) == {"f32"}, (entry, want)
            b = _call(f32, entry, inp, *args)
            assert f32.replay_info() + (f32.l0_mode(),) == rc.expected_f32(m, None, caps[1])[:3], entry
            assert _flat_bytes(a) == _flat_bytes(b), entry
    finally:
        auto.close()
        if f32 is not None:
            f32.close()


# ---- 5. fp16 only: an error in the entry's name, and nothing left behind ----------------------------------------------------------------
@pytest.mark.parametrize("path", rc.PATHS)
@pytest.mark.parametrize("kind", ["cat", "reg", "err"])
def test_under_f16_every_entry_raises_e_range_and_leaves_no_state(kind, path, monkeypatch):
    _set_path(path, monkeypatch)
    inp = rc.inputs("%s_planted_4" % kind)
    ctx = _context(inp, path)
    try:
        for entry in inp["case"]["entries"]:
            ctx.set_l0_precision("f16")
            with pytest.raises(capi.NpbnnError) as e:
                _call(ctx, entry, inp, *_args(entry, inp))
            assert e.value.code == capi.E_RANGE and WHO[entry] + ":" in str(e.value) and "fp16 range" in str(e.value), (entry, str(e.value))
            ctx.set_l0_precision("auto")
            clean = _call(ctx, entry, inp, *_args(entry, inp, _clean_sets(inp)))
            assert ctx.l0_mode() == "f16-split", entry
            assert _flat_bytes(clean) == _fresh_bytes(entry, inp, path), entry
    finally:
        ctx.close()


# ---- 6. route 2 of predict_pdp and predict_ale --------------------------------------------------------------------------------------------
def _point_call(case, inp, l0=None):
    """(result, route, replay-independent layer-0 path the call ended on) of the case on a fresh context"""
    ctx = HipContext(0)
    try:
        ctx.set_data(inp["x"])
        if l0:
            ctx.set_l0_precision(l0)
        ctx.set_arch_from_weights(inp["weights"][0], inp["x"].shape[1], capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
        if case["what"] == "ale":
            res = ctx.predict_ale(inp["weights"], inp["column"], inp["edges"])
            route = ctx.info(capi.INFO_ALE_ROUTE)
        else:
            res = ctx.predict_pdp(inp["weights"], inp["focal"], inp["grid"])
            route = ctx.info(capi.INFO_PDP_ROUTE)
        mode = ctx.l0_mode()
        # nothing is left behind: a clean prediction runs fp16-split again (under "auto")
        if not l0:
            clean = [[np.array(a) for a in w] for w in inp["weights"]]
            for w in clean:
                w[0][rc.PLANT_AT] = 0.0
            ctx.predict(clean[0])
            assert ctx.l0_mode() == "f16-split"
        return res, route, mode
    finally:
        ctx.close()


@pytest.mark.parametrize("path", rc.PATHS)
@pytest.mark.parametrize("planted", rc.POINT_PLANTED, ids=lambda p: "set_%d" % p[0])
@pytest.mark.parametrize("name", sorted(rc.POINT_CASES))
def test_route_2_restarts_on_float32(name, planted, path, monkeypatch):
    """Any flag of a chunk starts the call again from its first point on the float32 path, after the chunk's passes were folded into
    the accumulators: the outputs are the bytes of the same call under set_l0_precision("f32") and within the modules' bars of the
    float64 references; ALE's counts are exact.  pdp_two_chunks: the accumulator holds three of the five grid points."""
    from test_hip_ale import BAR as ALE_BAR
    from test_hip_pdp import TOL as PDP_TOL
    case, inp, want = rc.point_inputs(name, planted)
    for k, v in rc.POINT_ENV[path][case["what"]] + tuple(case["env"]):
        monkeypatch.setenv(k, v)
    got, route, mode = _point_call(case, inp)
    twin, route_twin, mode_twin = _point_call(case, inp, l0="f32")
    assert (route, route_twin) == (2, 2) and (mode, mode_twin) == ("f32", "f32")
    assert _flat_bytes(got) == _flat_bytes(twin)
    if case["what"] == "ale":
        counts, effects = got
        err = float(np.abs(effects - want[1]).max())
        print("%s %s planted %s: max |device - float64| %.3e (bar %.1e)" % (name, path, planted, err, ALE_BAR))
        assert counts.dtype == np.int64 and np.array_equal(counts, want[0]) and counts.sum() == case["rows"]
        assert effects.shape == want[1].shape and err <= ALE_BAR
    else:
        err = float(np.abs(got - want).max())
        print("%s %s planted %s: max |device - float64| %.3e (bar %.1e)" % (name, path, planted, err, PDP_TOL))
        assert got.shape == want.shape and err <= PDP_TOL


# ---- a repeat that leaves the resident path -----------------------------------------------------------------------------------------------
def test_a_repeat_that_leaves_the_resident_path():
    """768 features under [33, 8]: resident on the fp16 build, and the float32 build is the weight-streamed path's
    (test_host_sets_repeat.test_a_context_can_be_resident_where_its_float32_build_is_not).  A planted set there gives a correct
    float32 result - the bytes of its single prediction under set_l0_precision("f32"), within TOL of the oracle - or an error that
    names the entry and the cause; a clean call behind it is resident and fp16-split again, with a fresh context's bytes."""
    c = rc.FALLBACK
    inp = rc.fallback_inputs()
    clean = [[np.array(a) for a in w] for w in inp["sets"]]
    for i in c["planted"]:
        clean[i][0][rc.PLANT_AT] = 0.0

    def context():
        ctx = HipContext(0)
        ctx.set_data(inp["x"])
        ctx.set_arch_from_weights(inp["sets"][0], c["features"], capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
        return ctx

    ctx = context()
    try:
        fresh = ctx.predict_sets(clean)
        assert not ctx.is_wide() and ctx.l0_mode() == "f16-split"
    finally:
        ctx.close()
    ctx = context()
    try:
        try:
            y = ctx.predict_sets(inp["sets"])
        except capi.NpbnnError as e:
            print("refused: %s" % e)
            assert "predict_sets:" in str(e) and ("fp16 range" in str(e) or "LDS" in str(e)), str(e)
            y = None
        if y is not None:
            print("replay_info %s, ends on %s, streamed %s" % (ctx.replay_info(), ctx.l0_mode(), ctx.is_wide()))
            assert np.all(np.isfinite(y))
            for i in range(c["sets"]):
                err = float(np.max(np.abs(y[i] - rc.outputs_of(inp["z64"][i], "cat"))))
                print("set %d: max |device - float64 oracle| %.3e" % (i, err))
                assert err <= rc.TOL, (i, err)
            ctx.set_l0_precision("f32")
            for i in c["planted"]:
                np.testing.assert_array_equal(y[i], ctx.predict(inp["sets"][i]), err_msg="set %d" % i)
            ctx.set_l0_precision("auto")
        again = ctx.predict_sets(clean)
        assert not ctx.is_wide() and ctx.l0_mode() == "f16-split"
        assert again.tobytes() == fresh.tobytes()
    finally:
        ctx.close()
