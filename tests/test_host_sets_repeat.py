"""tests/repeat_cases.py without a GPU: the model of the replay loop against the tables the two existing repeat tests state, the sets
a pass carries from the host plan rule, the conditions on the planted inputs, and the guards - every entry's comparison "definition on
the stack" tells a stack with the planted set counted twice, dropped or not finite from the right one.  tests/test_hip_sets_repeat.py
runs the same cases and comparisons on the device."""
import numpy as np
import pytest

import fold_envelope_cases as fc
import repeat_cases as rc
import support_cases as sc
import test_host_resident_plan as rp
from range_cases import F16_MAX

FAMILIES = sorted({c["family"] for c in rc.CASES.values()})


def _of_family(name):
    return [c for c in rc.CASES.values() if c["family"] == name]


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def test_the_model_reproduces_the_existing_tests_tables():
    """test_hip_wide_replay.PLANTED (streamed: passes and the path the call ends on, groups of three at most) and
    test_hip_posterior's ``repeated``: (3, 4, 5) on the resident path, (4,) on the streamed path."""
    import test_hip_wide_replay
    planted_table = test_hip_wide_replay.PLANTED
    assert sorted(planted_table) == [(3,), (3, 4), (4,), (5,), (6,)]
    for planted, (passes, ends) in planted_table.items():
        got = rc.expected_replay(7, None, planted, "streamed", 3, 3)
        assert got[:3] == (passes, 3, ends), planted
        assert [i for i, p in enumerate(got[3]) if p == "f32"] == list(planted)
    for path, repeated in (("resident", (3, 4, 5)), ("streamed", (4,))):
        passes, group, ends, on = rc.expected_replay(7, None, (4,), path, 3, 3)
        assert tuple(i for i, p in enumerate(on) if p == "f32") == repeated and ends == "f16-split" and (passes, group) == (4, 3)
    # nothing planted: fold_envelope_cases.expected_groups; a slope vector per set: groups of one
    assert rc.expected_replay(7, None, (), "resident", 3, 3)[:3] == (3, 3, "f16-split")
    slopes = rc.slopes_of(rc.CASES["slopes_planted_3"])
    assert rc.expected_replay(7, slopes, (), "streamed", 3, 3)[:2] == (4, 3)                     # (0 1)(2 3 4)(5)(6): part E
    assert [g for _, g in fc.expected_groups(slopes, 7)] == [2, 3, 1, 1]
    assert rc.expected_replay(7, [np.full(2, 0.001 * (i + 1)) for i in range(7)], (2,), "streamed", 3, 3)[:3] == (8, 1, "f16-split")
    assert rc.expected_f32(7, None, 3)[:3] == (3, 3, "f32")


def test_sets_per_pass_from_the_plan_rule():
    """The base shape carries three sets per pass on both builds; 256 features under [50, 5] two on the fp16 build and one on the float32
    build, at 257 and 999 rows, 3 and 10 classes, with and without labels.  The modelled sequences on that shape (caps 2, 1), resident:
      planted (0,): (0 1) flagged, 0 alone in float32, then (1 2) and (3) on fp16                                4 passes
      planted (1,): (0 1) flagged, 0 alone in float32, (1 2) flagged, 1 alone in float32, (2 3)                  5 passes;
                    set 0 ends in float32 although it is in range
      planted (3,): (0 1), (2 3) flagged, 2 alone in float32, (3) flagged, 3 alone in float32                    5 passes, ends on float32"""
    assert rc.resident_caps(6, (5, 4), 3, 999) == (3, 3)
    for n_out in (3, 4):
        assert rc.caps_of(dict(features=6, nodes=(5, 4), kind="err" if n_out == 4 else "reg", rows=999), "resident") == (3, 3)
    for rows in (257, 999):
        for n_out in (3, 10):
            for lab in (0, 1):
                assert rc.resident_caps(256, (50, 5), n_out, rows, has_labels=lab) == (2, 1), (rows, n_out, lab)
    shrink = rc.CASES["shrink_planted_0"]
    assert rc.caps_of(shrink, "resident") == (2, 1) and rc.caps_of(shrink, "streamed") == (3, 3)
    assert rc.expected_replay(4, None, (0,), "resident", 2, 1) == (4, 2, "f16-split", ["f32", "f16-split", "f16-split", "f16-split"])
    assert rc.expected_replay(4, None, (1,), "resident", 2, 1) == (5, 2, "f16-split", ["f32", "f32", "f16-split", "f16-split"])
    assert rc.expected_replay(4, None, (3,), "resident", 2, 1) == (5, 2, "f32", ["f16-split", "f16-split", "f32", "f32"])
    # the whole call in float32 where every group holds a planted set
    for path in rc.PATHS:
        passes, group, ends, on = rc.expected_replay(7, None, rc.EVERY_GROUP[path], path, 3, 3)
        assert set(on) == {"f32"} and ends == "f32"


def test_the_case_table():
    for kind in ("cat", "reg", "err"):
        assert sorted(c["planted"] for c in _of_family(kind)) == sorted(rc.POSITIONS)
        assert all((c["rows"], c["features"], c["nodes"], c["sets"], c["fun"], c["paths"]) == (999, 6, (5, 4), 7, "tanh", rc.PATHS) for c in _of_family(kind))
    assert [c["planted"] for c in _of_family("slopes")] == [(3,), (6,)]
    assert [(c["planted"], c["paths"]) for c in _of_family("shrink")] == [((0,), ("resident",)), ((1,), ("resident",)), ((3,), ("resident",))]
    t = rc.CASES["test_table_planted_4"]
    assert (t["rows"], t["test_rows"], t["planted"]) == (300, 1000, (4,))
    for name, c in rc.POINT_CASES.items():
        assert c["sets"] == 7 and c["rows"] <= 300 and c["route"] == 2
    assert len(np.linspace(*rc.POINT_CASES["pdp"]["grid"])) <= 5 and rc.POINT_CASES["ale"]["bins"] <= 7
    # the two-chunk case: the accumulator the case asks for holds three of its five grid points (npbnn_attrib_pdp_g_chunk)
    import ctypes as C
    lib = rc.host_lib()
    lib.npbnn_host_attrib_pdp_g_chunk.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int64]
    two = rc.POINT_CASES["pdp_two_chunks"]
    budget = int(dict(two["env"])["NPBNN_PDP_ACC_BYTES"])
    assert lib.npbnn_host_attrib_pdp_g_chunk(two["grid"][2], two["rows"], two["n_out"], budget) == 3 and two["grid"][2] == 5
    assert lib.npbnn_host_attrib_pdp_g_chunk(5, 300, 5, 512 << 20) == 5 and not rc.POINT_CASES["pdp"]["env"]


# ---- the planted inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES)
def test_only_the_planted_weight_leaves_the_fp16_range(name):
    """Every planted weight times the largest |entry| of its float32-rounded column exceeds fp16's largest number; no other scaled
    layer-0 weight of any set exceeds half of it (test_host_chain_f16_range's condition)."""
    for case in _of_family(name):
        inp = rc.inputs(case["name"])
        for i in range(len(inp["sets"])):
            s = rc.scaled_layer0(inp, i)
            at = (rc.PLANT_AT[0], rc.PLANT_AT[1] - 1)
            if i in case["planted"]:
                assert inp["sets"][i][0][rc.PLANT_AT] == rc.PLANT and s[at] > F16_MAX
                s[at] = 0.0
            assert s.max() < F16_MAX / 2, (case["name"], i, s.max())


@pytest.mark.parametrize("name", [f for f in FAMILIES if f != "slopes"])
def test_the_planted_unit_saturates_and_float32_follows_the_oracle(name):
    """tanh: no row of a planted unit has |z| < 20 in the float64 oracle, and a numpy float32 forward pass of every set is within
    TOL / 4 of the oracle on the float32-rounded table - so the device's float32 path can be held to TOL on these inputs."""
    worst = 0.0
    for case in _of_family(name):
        inp = rc.inputs(case["name"])
        kind = case["kind"]
        for i in case["planted"]:
            z = rc.planted_preactivation(inp, i)
            assert np.min(np.abs(z)) >= rc.Z_MIN, (case["name"], i, np.min(np.abs(z)))
        for i in (range(len(inp["sets"])) if case["planted"] == rc.POSITIONS[0] or name in ("shrink", "test_table") else case["planted"]):
            got = rc.outputs_of(rc.forward32(inp["x"], inp["sets"][i], case, i), kind)
            err = float(np.max(np.abs(got - rc.outputs_of(inp["z64"][i], kind))))
            worst = max(worst, err)
            assert err <= rc.TOL / 4, (case["name"], i, err)
    print("%s: numpy float32 forward pass within %.3e of the float64 oracle (TOL / 4 = %.1e)" % (name, worst, rc.TOL / 4))


@pytest.mark.parametrize("name", sorted(rc.POINT_CASES))
def test_the_point_cases_saturate(name):
    """route 2 of predict_pdp / predict_ale: at every grid point or edge the planted unit stays beyond |z| = 20 (the focal column is
    not the planted weight's), and only the planted weight leaves the range"""
    for planted in rc.POINT_PLANTED:
        case, inp, _ = rc.point_inputs(name, planted)
        x = rc.f32(inp["x"])
        for i in planted:
            w0 = inp["weights"][i][0]
            rest = x.copy()
            rest[:, inp["focal"]] = 0.0
            z = rest @ w0[0, 1:] + w0[0, 0]
            reach = np.abs(w0[0, 1:][inp["focal"]]).sum() * max(np.abs(np.asarray(inp.get("edges", inp["grid"]))).max(), np.abs(x[:, inp["focal"]]).max())
            assert np.min(np.abs(z)) - reach >= rc.Z_MIN, (name, planted, i)
            scaled = np.abs(w0[:, 1:]) * np.max(np.abs(x), axis=0)[None, :]
            assert scaled[0, 2] > F16_MAX
            scaled[0, 2] = 0.0
            assert scaled.max() < F16_MAX / 2


# ---- the helpers that excuse ----------------------------------------------------------------------------------------------------------
def _oracle_stack(inp, n):
    z = rc.f32(inp["z64"][:n])
    return rc.f32(rc.outputs_of(z, inp["case"]["kind"])), z


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_the_excusing_helpers_excuse_next_to_nothing(name):
    """On the oracle's float32 stack fold_envelope_cases' rule (rows within 1e-12 of a bin or coverage edge) excuses no row, and
    support_cases' borderline rule no row of the votes and at most 1 % of the rows of the mean (its window of +-TOL around 99
    thresholds covers 0.4 % of the unit interval: a handful of 999 rows lie in it under any seed; the device test holds the cube to
    the summary's own besides, which leaves no row to that rule)."""
    inp = rc.inputs(name)
    case = inp["case"]
    y, z = _oracle_stack(inp, inp["n"])
    sigma = rc.sets_for("calibration", inp)[1]
    if "calibration" in case["entries"]:
        assert rc.excused_rows(inp, z, sigma) == 0
    if case["kind"] == "cat":
        from npbnn_amd import posterior
        for mode in (0, 1):
            summary = posterior._summarise(y, mode)
            n = sc.assert_cube_within_borderline(sc.cube_of(summary, inp["labels"]), summary, inp["labels"], mode, inp["n"], sc.near_ties_of(y))
            print("%s mode %d: %d borderline rows of %d" % (name, mode, n, y.shape[1]))
            assert n <= rc.EXCUSED_SHARE * y.shape[1] and (mode == 1 or n == 0)


# ---- the guards -----------------------------------------------------------------------------------------------------------------------
def _nan_like(v):
    if isinstance(v, tuple):
        return tuple(_nan_like(e) for e in v)
    if isinstance(v, dict):
        return {k: _nan_like(e) for k, e in v.items()}
    if v is None or np.asarray(v).dtype.kind != "f":
        return v
    return np.full(np.shape(v), np.nan) if np.ndim(v) else float("nan")


@pytest.mark.parametrize("kind", ["cat", "reg", "err"])
def test_every_comparison_tells_a_wrong_replay_from_a_right_one(kind):
    """The planted set (2) counted twice (a sink that also ran for the attempt thrown away), dropped, or folded as the non-finite
    values its fp16 pass left: every entry's definition of such a stack, held against the right stack, lies at least WRONG_FACTOR
    bounds away (the exact entries: at least one output differs), while the definition of the right stack passes.  (Set 2 and not 3 or
    4: split R-hat leaves the middle draw of an odd chain out, so eight draws with the fourth or fifth doubled have the halves of the
    right eight, and the convergence entry's definition cannot see that one mistake there.)"""
    inp = rc.inputs("%s_planted_2" % kind)
    for entry in rc.ENTRIES[kind]:
        n, sigma = rc.sets_for(entry, inp)
        y, z = _oracle_stack(inp, n)
        right = rc.define(entry, inp, y, z, sigma)
        res = rc.compare(entry, inp, right, y, z, sigma)
        assert rc.passed(entry, res), (entry, res)
        for how in rc.WRONG:
            yw, zw = rc.wrong_stack(how, y, 2), rc.wrong_stack(how, z, 2)
            sw = None if sigma is None else (sigma if how == "not_finite" else rc.wrong_stack(how, sigma, 2))
            try:
                with np.errstate(all="ignore"):
                    wrong = rc.define(entry, inp, yw, zw, sw)
            except (AssertionError, ValueError, FloatingPointError):
                wrong = _nan_like(right)                   # (the definition has no value on that stack)
            try:
                with np.errstate(all="ignore"):
                    res = rc.compare(entry, inp, wrong, y, z, sigma)
                far = res["worst"] >= 1 if entry in rc.EXACT else res["worst"] >= fc.WRONG_FACTOR * res["bound"]
                figure = res["worst"] / res["bound"] if res["bound"] else res["worst"]
            except AssertionError:                         # (the module's own helper refused it)
                far, figure = True, np.inf
            print("%s %-12s %-14s %s" % (kind, entry, how, "%d outputs differ" % figure if entry in rc.EXACT and np.isfinite(figure) else "%.3g bounds away" % figure))
            assert far, (kind, entry, how, res)


# ---- a float32 build that leaves the resident path ------------------------------------------------------------------------------------
def test_a_context_can_be_resident_where_its_float32_build_is_not():
    """768 features under [33, 8]: the host rule plans the fp16 build on the resident path and refuses the float32 request with
    NPBNN_RESIDENT_FEW_WAVES.  build_net (npbnn_capi.hip) asks wide_needed (npbnn_wide.hip) per layout - resident path bytes at
    kMinResidentWaves waves against the LDS limit - so a context is on the resident path there as long as it runs the fp16 build, and
    rebuild_net(false) moves it to the weight-streamed path: the repeat of a planted set runs streamed
    (test_hip_sets_repeat.test_a_repeat_that_leaves_the_resident_path)."""
    c = rc.FALLBACK
    f16 = rc.plan_of(c["features"], c["nodes"], c["n_out"], c["rows"], True)
    f32 = rc.plan_of(c["features"], c["nodes"], c["n_out"], c["rows"], False)
    assert f16 == dict(layout=rp.OK, stays=True, refusal=rp.OK, n_cand=f16["n_cand"]) and f16["n_cand"] >= 1
    assert (f32["layout"], f32["stays"], f32["refusal"]) == (rp.OK, False, rp.FEW_WAVES)
    inp = rc.fallback_inputs()
    for i in c["planted"]:
        w0 = inp["sets"][i][0]
        z = rc.f32(inp["x"]) @ w0[0, 1:] + w0[0, 0]
        assert np.min(np.abs(z)) >= rc.Z_MIN
    for i, w in enumerate(inp["sets"]):
        err = np.max(np.abs(rc.outputs_of(rc.forward32(inp["x"], w, inp["case"], i), "cat") - rc.outputs_of(inp["z64"][i], "cat")))
        assert err <= rc.TOL / 4, (i, err)
