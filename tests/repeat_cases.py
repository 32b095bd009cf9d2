"""The stored-sample entries through the fp16-range float32 repeat (CPU side; tests/test_hip_sets_repeat.py runs the cases on the GPU,
tests/test_host_sets_repeat.py checks this module without one).

A stored set whose scaled layer-0 weight leaves the fp16 range (PLANT = 3e5 written to layer-0 weight [0, 3], as test_hip_posterior.py
and test_hip_wide_replay.py plant it) makes ``replay_sets`` (npbnn_sets.hip) repeat work on the exact float32 path.  Here are

  * ``expected_replay``: the ``while`` loop of ``replay_sets`` restated in plain Python - what a call launches, which layer-0 path it ends
    on and which path every set's delivered values were computed on;
  * the case table CASES (three kinds on the base shape of the two existing repeat tests, every planted position of its groups, a
    genReLU case whose slopes cut the groups, the shape whose float32 build carries fewer sets per pass than its fp16 build, a test
    table), POINT_CASES (route 2 of predict_pdp / predict_ale) and FALLBACK (a shape whose float32 build leaves the resident path);
  * the inputs of a case, its float64 oracle and a numpy float32 forward pass;
  * per entry its definition on a stack of predictions (``define``) and the comparison the entry's own GPU module uses for "the same
    float32 values" (``compare``): a deviation over an imported bar, or a count of differing outputs for the exact entries.

The planted unit saturates: under tanh a pre-activation of 3e5 x is +-1 in float32 and in float64 alike as long as no row has |z| < 20
(tanh(20) = 1 - 8e-18), which the seeds are chosen for and test_host_sets_repeat.py asserts."""
import ctypes as C
import functools
import math
import os

import numpy as np

import cases
import calibration_cases as cc
import convergence_cases as cvc
import fold_envelope_cases as fc
import hpd_cases
import loo_cases
import lppd_cases as lc
import oracle as orc
import pdp_cases
import ale_cases
import predictive_cases as pc
import support_cases as sc
import uncertainty_cases as uc
from range_cases import PLANT

TOL = 2e-5                      # test_hip_posterior.TOL: float32 forward pass against float64
Z_MIN = 20.0                    # no row of a planted unit may have a pre-activation below this under tanh
EXCUSED_SHARE = 0.01            # the helpers that excuse borderline rows or cells may excuse at most this share of a case
MAX_GROUP = fc.MAX_GROUP        # kMaxCand, kWideMaxCand
PLANT_AT = (0, 3)               # layer-0 weight [node 0, column 3]: feature 2 (column 0 is the bias)
HPD_LEVEL = 0.8
N_BINS = 15
PATHS = ("resident", "streamed")
POSITIONS = ((0,), (2,), (3,), (4,), (6,), (3, 4), (1, 4, 6), (0, 1, 2, 3, 4, 5, 6))
EVERY_GROUP = {"resident": (1, 4, 6), "streamed": (0, 1, 2, 3, 4, 5, 6)}          # a planted set in every group: the whole call in float32
ENTRIES = {"cat": ("summary0", "summary1", "hpd", "support0", "support1", "lppd", "loo", "uncertainty", "calibration", "convergence"),
           "reg": ("hpd", "lppd", "loo", "uncertainty", "calibration", "convergence", "predictive"),
           "err": ("hpd", "uncertainty", "calibration", "convergence", "predictive")}
EXACT = ("summary0", "summary1", "hpd", "support0", "support1")
N_OUT = {"cat": 3, "reg": 3, "err": 4}
# npbnn_amd.convergence.MIN_DRAWS is 8: the convergence entry runs on the case's seven sets and an eighth, clean one behind them
CONVERGENCE_SETS = 8


# ---- the replay loop ----------------------------------------------------------------------------------------------------------------
def _group_len(slopes, s0, n_sets, cap):
    g = 1
    while s0 + g < n_sets and g < cap and (slopes is None or np.array_equal(slopes[s0 + g], slopes[s0])):
        g += 1
    return g


def expected_replay(n_sets, slopes, planted, path, cap_f16, cap_f32):
    """(passes, max_group, layer-0 path the call ends on, [path every set's delivered values were computed on]) of a replay of
    ``n_sets`` sets of which ``planted`` leave the fp16 range; ``slopes``: one vector per set or None; ``path`` "resident" or
    "streamed"; ``cap_f16`` / ``cap_f32``: the sets a pass carries on each build of the first layer.  The loop of ``replay_sets``:
    a resident group that raises the flag runs again as a whole under the float32 plan, which may carry fewer sets - the rest waits
    for the next round; a streamed pass reports per set, delivers the sets before the first offender as computed, repeats that one
    alone in float32 and starts a fresh group behind it."""
    assert path in PATHS
    planted = set(planted)
    passes = max_group = 0
    ends, on = "f16-split", [None] * n_sets
    s0, alone = 0, False
    while s0 < n_sets:
        g = 1 if alone else _group_len(slopes, s0, n_sets, MAX_GROUP)
        attempt = 1 if alone else 0
        alone = False
        while attempt < 2:
            f32 = attempt == 1
            g = min(g, cap_f32 if f32 else cap_f16)
            passes += 1
            max_group = max(max_group, g)
            ends = "f32" if f32 else "f16-split"
            bad = None if f32 else next((j for j in range(g) if s0 + j in planted), None)
            if bad is None:
                break
            if path == "resident":
                attempt += 1
                continue
            if bad > 0:
                g, alone = bad, True
                break
            g = 1
            attempt += 1
        for j in range(g):
            on[s0 + j] = ends
        s0 += g
    return passes, max_group, ends, on


def expected_f32(n_sets, slopes, cap_f32):
    """expected_replay of a context under set_l0_precision("f32"): one build, no flag"""
    passes, max_group, _, _ = expected_replay(n_sets, slopes, (), "streamed", cap_f32, cap_f32)
    return passes, max_group, "f32", ["f32"] * n_sets


# ---- the host plan rule -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_lib():
    """libnpbnn_host.so with the plan rule's entries typed (tests/test_host_resident_plan.py's fixture, without pytest)"""
    import test_host_resident_plan as rp
    from npbnn_amd import _capi, predraw
    if not os.path.exists(predraw.HOST_LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(predraw.HOST_LIB_PATH)
    i32p = C.POINTER(C.c_int32)
    lib.npbnn_host_resident_layout.argtypes = [C.POINTER(_capi.Arch), i32p, C.c_char_p, C.POINTER(rp.Layout)]
    lib.npbnn_host_resident_path_bytes.argtypes = [C.POINTER(rp.Layout), C.c_int, C.c_int]
    lib.npbnn_host_resident_path_bytes.restype = C.c_longlong
    lib.npbnn_host_resident_launch.argtypes = [C.POINTER(rp.Layout), i32p, C.POINTER(rp.Launch)]
    return lib


MIN_RESIDENT_WAVES = 4          # kMinResidentWaves (npbnn_ctx.hip.h): what wide_needed asks npbnn_resident_path_bytes for below 65536 rows


def plan_of(features, nodes, n_out, rows, f16, has_labels=0, has_targets=0):
    """dict(code of the layout rule, stays: does wide_needed keep this layout on the resident path, refusal and n_cand of a predicting
    launch that wants three sets) of a tanh network on the host rule"""
    import test_host_resident_plan as rp
    from npbnn_amd import _capi
    lib = host_lib()
    arch = rp.make_arch(list(nodes) + [n_out], features, bias=[1] * len(nodes) + [0], lik=_capi.LIK_NONE)
    rc, y = rp.layout_of(lib, arch, f16=1 if f16 else 0)
    stays = rc == rp.OK and lib.npbnn_host_resident_path_bytes(C.byref(y), 0, MIN_RESIDENT_WAVES) <= rp.LDS_LIMIT
    refusal, p = rp.launch_of(lib, y, predict_only=1, want_cand=MAX_GROUP, lik_only=0, has_labels=has_labels, has_targets=has_targets,
                              n_tiles=-(-rows // 16))
    return dict(layout=rc, stays=bool(stays), refusal=refusal, n_cand=p.n_cand)


def resident_caps(features, nodes, n_out, rows, **kw):
    """(sets a pass carries on the fp16 build, on the float32 build) of the resident path"""
    return tuple(plan_of(features, nodes, n_out, rows, f16, **kw)["n_cand"] for f16 in (True, False))


def caps_of(case, path):
    if path == "streamed":
        return (MAX_GROUP, MAX_GROUP)
    return resident_caps(case["features"], case["nodes"], N_OUT[case["kind"]], case["rows"])


# ---- the case table -----------------------------------------------------------------------------------------------------------------
_BASE = dict(rows=999, features=6, nodes=(5, 4), fun="tanh", sets=7, slopes=None, test_rows=None, paths=PATHS, seed=0, entries=None)
CASES = {}


def _case(name, **kw):
    assert name not in CASES and not set(kw) - set(_BASE) - {"kind", "planted"}, name
    c = dict(_BASE, name=name, **kw)
    c["family"] = name.rsplit("_planted_", 1)[0]
    if c["entries"] is None:
        c["entries"] = ENTRIES[c["kind"]]
    CASES[name] = c


def _tag(planted):
    return "all" if len(planted) == 7 else "".join(map(str, planted))


# the seeds: the first of 0, 1, 2, ... under which test_host_sets_repeat.py's conditions on the inputs hold for every planted position
_SEEDS = {"cat": 0, "reg": 0, "err": 0, "slopes": 1, "shrink": 0, "test_table": 0}
for _kind in ("cat", "reg", "err"):
    for _p in POSITIONS:
        _case("%s_planted_%s" % (_kind, _tag(_p)), kind=_kind, planted=_p, seed=_SEEDS[_kind])
# genReLU slopes a a b b b b a (test_hip_wide_replay's part E): groups (0 1)(2 3 4)(5)(6).  The planted unit is not bounded there, so
# the oracle is no yardstick of the float32 pass; every set is held to its own single prediction's bytes and every entry to its
# definition on the stack, as everywhere
for _p in ((3,), (6,)):
    _case("slopes_planted_%s" % _tag(_p), kind="cat", planted=_p, fun="genReLU", slopes="aabbbba", seed=_SEEDS["slopes"])
# 256 features, [50, 5]: two sets per pass on the fp16 build, one on the float32 build - a repeat regroups sets that are in range
for _p in ((0,), (1,), (3,)):
    _case("shrink_planted_%s" % _tag(_p), kind="cat", planted=_p, features=256, nodes=(50, 5), sets=4, paths=("resident",), seed=_SEEDS["shrink"],
          entries=tuple(e for e in ENTRIES["cat"] if e != "convergence"))
_case("test_table_planted_4", kind="cat", planted=(4,), rows=300, test_rows=1000, seed=_SEEDS["test_table"])
# (rows: the table the entries read - the TEST slot, 300 rows; test_rows: the training table above it, 1000 rows)

SLOPES_A, SLOPES_B = np.array([0.05, 0.3]), np.array([0.2, 0.01])


def slopes_of(case, n_sets=None):
    if case["slopes"] is None:
        return None
    s = [SLOPES_A if ch == "a" else SLOPES_B for ch in case["slopes"]]
    return s + [SLOPES_A] * ((n_sets or len(s)) - len(s))


def f32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def family(name):
    """The inputs every planted position of a family shares: ``x`` (the table the entries read), ``train_x`` (the training table above
    it, or None), eight clean sets (seven of the case and the one the convergence entry needs; the shrinking shape: four), ``labels``
    (class indices) or ``targets`` a float32 holds exactly, ``sigma`` [8, T] for the identity regression."""
    case = next(c for c in CASES.values() if c["family"] == name)
    rs = np.random.default_rng([20261021, case["seed"], cases.hash_name(name) % (2 ** 31)])
    kind, f, c = case["kind"], case["features"], N_OUT[case["kind"]]
    x = rs.standard_normal((case["rows"], f))
    train_x = rs.standard_normal((case["test_rows"], f)) if case["test_rows"] else None
    shapes = cases.layer_shapes(f, list(case["nodes"]), c, 2)
    n_draw = CONVERGENCE_SETS if case["sets"] == 7 else case["sets"]
    # (the base shape as the two existing tests draw it, N(0, 0.5); the 256-feature first layer N(0, 1 / sqrt(fan-in)): sums of order 1)
    sets = [[rs.normal(0, 0.5 if s[1] < 64 else 1.0 / np.sqrt(s[1]), s) for s in shapes] for _ in range(n_draw)]
    out = dict(case=case, x=_frozen(x), train_x=None if train_x is None else _frozen(train_x), sets=sets, labels=None, targets=None, sigma=None)
    z = np.array([forward64(x, w, case, i) for i, w in enumerate(sets)])
    if kind == "cat":
        labels = np.argmax(np.mean(_softmax(z), axis=0), axis=1)
        flip = rs.random(len(x)) < 0.1
        out["labels"] = _frozen(np.where(flip, (labels + rs.integers(1, c, len(x))) % c, labels).astype(np.int64))
    else:
        t = c // 2 if kind == "err" else c
        out["targets"] = _frozen(f32(z[0][:, :t] + 0.7 * rs.standard_normal((len(x), t))))
        if kind == "reg":
            out["sigma"] = _frozen(rs.uniform(0.5, 1.5, (n_draw, c)))
    out["z_clean"] = _frozen(z)
    for w in sets:
        for a in w:
            a.setflags(write=False)
    return out


def act_of(case, set_index):
    s = slopes_of(case, CONVERGENCE_SETS)
    return orc.Act(case["fun"], prm=None if s is None else s[set_index])


def forward64(x, w, case, set_index):
    """the float64 oracle's pre-output values on the table as the device holds it (float32 entries)"""
    with np.errstate(over="ignore"):         # (the oracle's tanh of a planted pre-activation: exp overflows to inf, the result is 1)
        return orc.forward_logits(f32(x), w, act_of(case, set_index))


def forward32(x, w, case, set_index):
    """a plain numpy float32 forward pass of the same network: float32 table, float32 weights, float32 sums and activations"""
    h = np.asarray(x, dtype=np.float32)
    slopes = slopes_of(case, CONVERGENCE_SETS)
    for l, a in enumerate(w):
        a = np.asarray(a, dtype=np.float32)
        bias = a.shape[1] == h.shape[1] + 1
        z = h @ a[:, 1:].T + a[:, 0] if bias else h @ a.T
        if l == len(w) - 1:
            return z.astype(np.float64)
        if case["fun"] == "tanh":
            h = np.tanh(z)
        else:
            h = np.where(z < 0, np.float32(slopes[set_index][l]) * z, z).astype(np.float32)


def plant(sets, planted):
    """copies of the sets with PLANT written to layer-0 weight PLANT_AT of every planted one"""
    out = [[np.array(a, copy=True) for a in w] for w in sets]
    for i in planted:
        out[i][0][PLANT_AT] = PLANT
    return out


@functools.lru_cache(maxsize=None)
def inputs(name):
    """A case's inputs: the family's, with ``sets`` planted (all the family drew: the case's own are the first ``case["sets"]``) and
    ``z64`` [sets, rows, outputs] the float64 oracle's pre-output values.  Built once, shared, never changed."""
    case = CASES[name]
    fam = family(case["family"])
    sets = plant(fam["sets"], case["planted"])
    z = np.array(fam["z_clean"], copy=True)
    for i in case["planted"]:
        z[i] = forward64(fam["x"], sets[i], case, i)
    return dict(fam, case=case, sets=sets, z64=_frozen(z), n=case["sets"])


def _softmax(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def outputs_of(z, kind):
    """post-output predictions from pre-output values (softmax; identity; softplus on the second half)"""
    z = np.asarray(z, dtype=np.float64)
    if kind == "cat":
        return _softmax(z)
    if kind == "err":
        t = z.shape[-1] // 2
        return np.concatenate([z[..., :t], np.logaddexp(0.0, z[..., t:])], axis=-1)
    return z


def planted_preactivation(inp, i):
    """[rows] the planted unit's pre-activation of set i in float64"""
    w0 = inp["sets"][i][0]
    return f32(inp["x"]) @ w0[PLANT_AT[0], 1:] + w0[PLANT_AT[0], 0]


def scaled_layer0(inp, i):
    """|w| x the largest |entry| of its float32-rounded column, over the feature columns of set i's first layer"""
    return np.abs(inp["sets"][i][0][:, 1:]) * np.max(np.abs(f32(inp["x"])), axis=0)[None, :]


# ---- rows the python-loop restatements are held on -----------------------------------------------------------------------------------
def rows_held(n_rows, step=13):
    """every ``step``-th row and the last: a repeat that counts a set twice, drops one or keeps a stale accumulator is wrong on every
    row alike, and the restatements with a Python loop per cell (PSIS, R-hat / ESS, the mixture quantiles) cost a millisecond a cell"""
    return np.unique(np.r_[np.arange(0, n_rows, step), n_rows - 1])


# ---- the entries: definition on a stack, and the comparison ---------------------------------------------------------------------------
for _fam, _kind in (("cat", "cat"), ("reg", "reg"), ("err", "err"), ("slopes", "cat"), ("shrink", "cat"), ("test_table", "cat")):
    cc.register("repeat/" + _fam, _kind, N_BINS, () if _kind == "cat" else cc.DEFAULT_LEVELS)


def _cc_name(inp):
    return "repeat/" + inp["case"]["family"]


def _levels(kind):
    return () if kind == "cat" else cc.DEFAULT_LEVELS


def _truth(inp):
    return inp["labels"] if inp["case"]["kind"] == "cat" else inp["targets"]


def _want_uncertainty(z, kind, sigma):
    """fold_envelope_cases.want_of's uncertainty branch, on a case of this table"""
    w = uc.restatement(z, fc.KINDS[kind], sigma)
    if kind == "cat":
        w.update({total: float(np.mean(w[field])) for total, field in uc.CLASS_TOTALS.items()})
        return w
    if kind == "reg":
        w = dict(mean=w["mean"], epistemic_var=w["epistemic_var"])
    w.update({k + "_avg": np.mean(v, axis=0) for k, v in list(w.items())})
    return w


def _mixture_cells(inp, y, sigma, rows):
    kind = inp["case"]["kind"]
    n_sets = y.shape[0]
    t = y.shape[2] // 2 if kind == "err" else y.shape[2]
    mu = y[:, rows, :t].reshape(n_sets, -1)
    if kind == "err":
        return mu, y[:, rows, t:].reshape(n_sets, -1), False, t
    return mu, np.asarray(sigma, dtype=np.float64), True, t


def _convergence_ref(stack_cols):
    """convergence_cases.reference's dict for the columns of a stack [S, cols] (one chain)"""
    f64 = [cvc.restate(stack_cols[:, c], 1, np.float64) for c in range(stack_cols.shape[1])]
    ld = [cvc.restate(stack_cols[:, c], 1, np.longdouble) for c in range(stack_cols.shape[1])]
    return dict(rhat=np.array([r[0] for r in f64], dtype=np.float64), ess=np.array([r[1] for r in f64], dtype=np.float64),
                margin=np.array([r[2] for r in f64]), rhat_ld=np.array([r[0] for r in ld], dtype=np.longdouble),
                ess_ld=np.array([r[1] for r in ld], dtype=np.longdouble), margin_ld=np.array([r[2] for r in ld]))


def define(entry, inp, y, z, sigma=None):
    """The entry's outputs by its definition on a stack: ``y`` [S, rows, outputs] the predictions, ``z`` the pre-output values, both
    float64 arrays of float32 values; under the keys the device call returns (tuples for summary and hpd).  The restatements with a
    Python loop per cell fill the rows of ``rows_held`` and leave NaN elsewhere."""
    from npbnn_amd import posterior
    kind, n_rows = inp["case"]["kind"], y.shape[1]
    rows = rows_held(n_rows)
    if entry in ("summary0", "summary1"):
        return (posterior._summarise(y, int(entry[-1])), None)
    if entry == "hpd":
        lo, hi = hpd_columns(y)
        return (np.mean(y, axis=0), lo, hi)
    if entry in ("support0", "support1"):
        summary = posterior._summarise(y, int(entry[-1]))
        return dict(summary=summary, cube=sc.cube_of(summary, inp["labels"]))
    if entry == "lppd":
        return fc.lppd_restatement(lc.log_lik_from_values(z, _truth(inp), kind, sigma))
    if entry == "loo":
        ll = lc.log_lik_from_values(z, _truth(inp), kind, sigma)
        out = dict(log_lik=ll, log_lik_sample=ll.sum(axis=1))
        cols = loo_cases.loo_columns(ll[:, rows])
        for f in loo_cases.FIELDS:
            out[f] = np.full(n_rows, np.nan)
            out[f][rows] = cols[f]
        return out
    if entry == "uncertainty":
        return _want_uncertainty(z, kind, sigma)
    if entry == "calibration":
        return cc.restatement(z, _truth(inp), fc.KINDS[kind], sigma, N_BINS, _levels(kind))
    if entry == "convergence":
        ref = _convergence_ref(y[:, rows, :].reshape(y.shape[0], -1))
        out = dict(rhat=np.full(y.shape[1:], np.nan), ess=np.full(y.shape[1:], np.nan))
        out["rhat"][rows], out["ess"][rows] = ref["rhat"].reshape(len(rows), -1), ref["ess"].reshape(len(rows), -1)
        return out
    assert entry == "predictive", entry
    rows = rows[::3]
    mu, sg, per_sample, t = _mixture_cells(inp, y, sigma, rows)
    sig = pc.sigma_of_cells(sg, mu.shape[1], per_sample)
    q = np.full((len(pc.PROBS), n_rows, t), np.nan)
    crps = np.full((n_rows, t), np.nan)
    targets = inp["targets"][rows].ravel()
    roots = np.array([[pc.root(mu[:, c], sig[:, c], p, False) for c in range(mu.shape[1])] for p in pc.PROBS])
    q[:, rows, :] = roots.reshape(len(pc.PROBS), len(rows), t)
    parts = [pc.crps_parts(mu[:, c], sig[:, c], float(targets[c]), False) for c in range(mu.shape[1])]
    crps[rows] = np.array([a - b for a, b in parts]).reshape(len(rows), t)
    return dict(quantiles=q, mean=np.mean(y[:, :, :t], axis=0), crps_i=crps)


def hpd_columns(y):
    return hpd_cases.hpd_columns(y, HPD_LEVEL)


def _differing(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.size if a.shape != b.shape else int(np.count_nonzero(~((a == b) | (np.isnan(a) & np.isnan(b)))))


def _bars():
    """the entries' own bars for "the same float32 values", imported from the modules that own them"""
    import test_hip_calibration as thc
    import test_hip_lppd as thl
    import test_hip_uncertainty as thu
    return dict(lppd=min(thl.KERNEL_TOL, fc.TOL["lppd"]), uncertainty=min(thu.KERNEL_TOL, fc.TOL["uncertainty"]),
                calibration=min(thc.KERNEL_TOL, fc.TOL["calibration"]), log_lik=thl.KERNEL_TOL)


def compare(entry, inp, got, y, z, sigma=None):
    """``got`` (a device call's result, or ``define``'s) against the entry's definition on the stack ``y`` / ``z``, by the comparison
    of the entry's own GPU module.  Returns dict(worst, bound, excused, share): the exact entries count differing outputs (bound 0);
    the others report their largest deviation in units of the imported bar (bound 1 for those whose bar differs from cell to cell).
    ``excused``: rows or cells the borderline helpers excuse, ``share`` of how many.  AssertionError where the module's own helper
    raises one."""
    from npbnn_amd import posterior
    kind, n_rows = inp["case"]["kind"], y.shape[1]
    rows = rows_held(n_rows)
    res = dict(worst=0.0, bound=0.0, excused=0, share=0.0)
    if entry in ("summary0", "summary1"):
        res["worst"] = _differing(got[0], posterior._summarise(y, int(entry[-1])))
    elif entry == "hpd":
        lo, hi = hpd_columns(y)
        mean = np.mean(y, axis=0)
        far = np.abs(np.asarray(got[0]) - mean) > 1e-12 * np.abs(mean)         # (test_hip_posterior: rtol 1e-12 on the mean)
        res["worst"] = _differing(got[1], lo) + _differing(got[2], hi) + int(np.count_nonzero(far | np.isnan(np.asarray(got[0]))))
    elif entry in ("support0", "support1"):
        mode = int(entry[-1])
        summary = posterior._summarise(y, mode)
        n_sets = y.shape[0]
        # the cube is the summary's own, whose quotients the device's are bit for bit: no row is left to the borderline rule, which
        # (support_cases' helper, the yardstick of test_hip_support) has to hold besides and excuse at most EXCUSED_SHARE
        res["worst"] = _differing(got["summary"], summary) + _differing(got["cube"], sc.cube_of(summary, inp["labels"]))
        res["excused"] = sc.assert_cube_within_borderline(got["cube"], summary, inp["labels"], mode, n_sets, sc.near_ties_of(y), label=entry)
        res["share"] = res["excused"] / n_rows
    elif entry == "lppd":
        want = fc.lppd_restatement(lc.log_lik_from_values(z, _truth(inp), kind, sigma))
        res.update(worst=fc.worst_deviation(got, want), bound=_bars()["lppd"])
    elif entry == "uncertainty":
        res.update(worst=fc.worst_deviation(got, _want_uncertainty(z, kind, sigma)), bound=_bars()["uncertainty"])
    elif entry == "calibration":
        from test_hip_calibration import _kernel_check
        want = cc.restatement(z, _truth(inp), fc.KINDS[kind], sigma, N_BINS, _levels(kind))
        excused = excused_rows(inp, z, sigma)
        worst = _kernel_check(got, want, _cc_name(inp), fc.KINDS[kind], fc.top_two_gap(z) if kind == "cat" else None)
        res.update(worst=worst, bound=_bars()["calibration"], excused=excused, share=excused / n_rows)
    elif entry == "loo":
        ll = lc.log_lik_from_values(z, _truth(inp), kind, sigma)
        if np.shape(got["log_lik"]) != ll.shape or not np.all(np.isfinite(got["log_lik"])):
            return dict(res, worst=np.inf, bound=1.0)
        worst = max(fc.deviation(got["log_lik"], ll), fc.deviation(got["log_lik_sample"], ll.sum(axis=1))) / _bars()["log_lik"]
        want, bars = loo_cases.reference(np.asarray(got["log_lik"])[:, rows])
        for f in loo_cases.FIELDS:
            dev = loo_cases.deviation({f: np.asarray(got[f])[rows]}, want, f)
            worst = max(worst, dev / bars[f] if bars[f] > 0 else (0.0 if dev == 0 else np.inf))
        res.update(worst=worst, bound=1.0)
    elif entry == "convergence":
        ref = _convergence_ref(y[:, rows, :].reshape(y.shape[0], -1))
        dr, de, left = cvc.compare(np.asarray(got["rhat"])[rows].ravel(), np.asarray(got["ess"])[rows].ravel(), ref)
        res.update(worst=max(dr / cvc.RHAT_RTOL, de / cvc.ESS_RTOL), bound=1.0, excused=left, share=left / (len(rows) * y.shape[2]))
    else:
        assert entry == "predictive", entry
        r3 = rows[::3]
        mu, sg, per_sample, t = _mixture_cells(inp, y, sigma, r3)
        q = np.asarray(got["quantiles"])[:, r3, :].reshape(len(pc.PROBS), -1)
        worst, by_root = pc.check_quantiles(q, mu, sg, pc.PROBS, per_sample, entry)
        worst_crps = pc.check_crps(np.asarray(got["crps_i"])[r3].ravel(), mu, sg, inp["targets"][r3].ravel(), per_sample, entry)
        # test_hip_predictive._check_against_stack's bound on the mean, over every row
        m_all = y[:, :, :t].reshape(y.shape[0], -1)
        exact = np.array([math.fsum((m_all[:, c] - m_all[0, c]).tolist()) for c in range(m_all.shape[1])])
        tol = (y.shape[0] + 2) * 2.0 ** -53 * (np.abs(m_all[0]) + np.sum(np.abs(m_all - m_all[0]), axis=0) / y.shape[0])
        d_mean = np.abs(np.asarray(got["mean"]).ravel() - (m_all[0] + exact / y.shape[0]))
        w_mean = float(np.max(np.where(tol > 0, d_mean / np.where(tol > 0, tol, 1.0), np.where(d_mean > 0, np.inf, 0.0))))
        res.update(worst=max(worst, worst_crps, w_mean if np.isfinite(w_mean) else np.inf), bound=1.0)
    if np.isnan(res["worst"]):                   # (a NaN where a value is defined is as far as it gets)
        res["worst"] = np.inf
    return res


def excused_rows(inp, z, sigma=None):
    """fold_envelope_cases.rows_that_may_fall_either_way on a case of this table"""
    kind = inp["case"]["kind"]
    want = cc.restatement(z, _truth(inp), fc.KINDS[kind], sigma, N_BINS, _levels(kind))
    if kind != "cat":
        return cc.rows_near_an_edge(_cc_name(inp), want["pit"], fc.EXCUSED)
    gap = fc.top_two_gap(z)
    return cc.rows_near_an_edge(_cc_name(inp), want["confidence"], fc.EXCUSED) + int(np.sum((gap > 0) & (gap <= fc.EXCUSED)))


def passed(entry, res):
    return res["worst"] <= res["bound"] and res["share"] <= EXCUSED_SHARE


def sets_for(entry, inp):
    """(number of sets the entry runs on, sigma of those sets or None): the case's own, and CONVERGENCE_SETS for convergence"""
    n = CONVERGENCE_SETS if entry == "convergence" else inp["n"]
    return n, None if inp["sigma"] is None else inp["sigma"][:n]


# ---- wrong stacks for the guards ------------------------------------------------------------------------------------------------------
WRONG = ("counted_twice", "dropped", "not_finite")


def wrong_stack(how, a, i):
    """the stack ``a`` [S, ...] with set i counted twice, dropped, or replaced by what an fp16 pass leaves of it (NaN)"""
    if how == "counted_twice":
        return np.concatenate([a[:i + 1], a[i:]], axis=0)
    if how == "dropped":
        return np.concatenate([a[:i], a[i + 1:]], axis=0)
    out = np.array(a, copy=True)
    out[i] = np.nan
    return out


# ---- route 2 of predict_pdp and predict_ale -------------------------------------------------------------------------------------------
POINT_PLANTED = ((0,), (5,), (6,))
# route 2 forced on the resident path (one pass per point) and taken by itself on the weight-streamed path
POINT_ENV = {"resident": {"pdp": (("NPBNN_PDP_PER_GRID", "1"),), "ale": (("NPBNN_ALE_PER_EDGE", "1"),)},
             "streamed": {"pdp": (("NPBNN_FORCE_WIDE", "1"),), "ale": (("NPBNN_FORCE_WIDE", "1"),)}}
_PDP = dict(pdp_cases._DEFAULTS, route=2, sets=7, rows=300, grid=(-2.0, 2.0, 5))
POINT_CASES = {
    "pdp": dict(_PDP, name="repeat_pdp", what="pdp", seed=9100, env=()),
    # an accumulator of three of the five grid points: the flag of the first chunk restarts the call after its passes were folded
    "pdp_two_chunks": dict(_PDP, name="repeat_pdp_two_chunks", what="pdp", seed=9100, env=(("NPBNN_PDP_ACC_BYTES", str(3 * 300 * 5 * 4)),)),
    "ale": dict(pdp_cases._DEFAULTS, name="repeat_ale", what="ale", route=2, sets=7, rows=300, seed=9100, bins=7, edges=None, ordinal=0, env=()),
}


@functools.lru_cache(maxsize=None)
def point_inputs(name, planted):
    """inputs and float64 reference of a route-2 case with PLANT in layer-0 weight PLANT_AT of the planted sets (the focal column is
    feature 3, the planted weight reads feature 2)"""
    case = POINT_CASES[name]
    inp = ale_cases.inputs(case) if case["what"] == "ale" else pdp_cases.envelope_inputs(case)
    inp["weights"] = plant(inp["weights"], planted)
    assert 2 not in inp["focal"]
    with np.errstate(over="ignore"):
        want = ale_cases.reference(case, inp) if case["what"] == "ale" else pdp_cases.envelope_oracle(case, inp)
    return case, inp, want


# ---- a float32 build that leaves the resident path -------------------------------------------------------------------------------------
# 768 features, [33, 8]: the fp16-split image fits beside four waves, the float32 image does not.  build_net asks wide_needed per
# layout, so the context is resident on the fp16 build and its repeat runs on the weight-streamed path.
FALLBACK = dict(rows=300, features=768, nodes=(33, 8), n_out=3, sets=4, planted=(1,), seed=5)


@functools.lru_cache(maxsize=None)
def fallback_inputs():
    c = FALLBACK
    rs = np.random.default_rng([20261021, c["seed"], 768])
    x = rs.standard_normal((c["rows"], c["features"]))
    shapes = cases.layer_shapes(c["features"], list(c["nodes"]), c["n_out"], 2)
    sets = plant([[rs.normal(0, 1.0 / np.sqrt(s[1]), s) for s in shapes] for _ in range(c["sets"])], c["planted"])
    case = dict(fun="tanh", slopes=None)
    z = np.array([forward64(x, w, case, i) for i, w in enumerate(sets)])
    return dict(case=case, x=_frozen(x), sets=sets, z64=_frozen(z))
