"""The envelope of the three set-statistic folds - npbnn_predict_sets_lppd, npbnn_predict_sets_uncertainty and
npbnn_predict_sets_calibration (npbnn_lppd.hip, npbnn_uncertainty.hip, npbnn_calibration.hip, npbnn_fold.hip.h): the case table CASES,
its seeded inputs, the float64 restatements a case is held to, and the bounds.  tests/test_hip_fold_envelope.py runs the cases on the
device, tests/test_host_fold_envelope.py shows on the CPU that the restatements tell a wrong fold from a right one on every case.
Nothing here needs a GPU.

A case is one or two axes away from the default: 257 rows x 11 features, hidden layers (6, 5), tanh, 4 stored sets, bias mode 2; three
classes, three targets, or two targets with their sigmas.  Every value of an axis is the smallest at which the code it names can go
wrong; none is a workload size.
  rows      wave and workgroup edges (64 lanes, 256 threads), one to four workgroups with a full and a ragged last one, a single row;
  classes   softmax widths: the float4 builds at 4, 8, 12, 16, 32 (8 the smallest with a second vector), the scalar ones between, and
            the degenerate single class (log-likelihood 0, entropies 0);
  targets   identity widths, the Gaussian branch of lppd and the regression folds;
  outputs   means plus sigmas: 8 is T = 4, the smallest with a second float2 pair; at 12 (T = 6) the boundary between means and sigmas
            is 8-byte but not 16-byte aligned;
  runs      a genReLU network whose slope vectors are shared in runs of the sets: the replay carries a run of up to three sets per pass,
            so the run lengths are the groups (``expected_groups``), S from 1 to 6;
  test      the statistic on the test table, 513 rows under 300 training rows, labels or targets set on both slots and drawn
            independently;
  crossed   edges the one-axis cases do not reach together.
Calibration's bins (1, 15, 64) and coverage levels (none, one, the default four) ride along case after case.

The inputs are lppd_cases.inputs' and calibration_cases._error_targets': a teacher network, the samples perturbations of it, labels the
teacher's calls with a share flipped, targets rounded through float32, sigmas from uniform(0.5, 1.5).

The bounds.  A case's reference is the float64 restatement on the very float32 values predict_sets(apply_out_fn=False) returns, so only
exp / log / erfc rounding and the order of sums separate the device from it.  Deviation = |got - want| / max(1, |want|) over every
floating-point field.  MEASURED_DEVIATION is the largest figure test_hip_fold_envelope.test_case printed per entry on an MI355X, with
the case that gave it; the bound is 10 x that, capped at 1e-10 - the rule of KERNEL_TOL in test_hip_lppd.py, test_hip_uncertainty.py
and test_hip_calibration.py."""
import functools

import numpy as np

import calibration_cases as cc
import lppd_cases as lc
import uncertainty_cases as uc

ENTRIES = ("lppd", "uncertainty", "calibration")
# the largest deviation test_hip_fold_envelope.test_case measured per entry (MI355X), and its case
MEASURED_DEVIATION = {"lppd": (4.140e-15, "targets_12"),             # next targets_8 2.699e-15, rows_513_targets_8_runs_231 2.623e-15
                      "uncertainty": (7.483e-15, "runs_1_cat"),      # next runs_2_cat 2.487e-15, runs_21_cat 2.271e-15, classes_32 2.220e-15
                      "calibration": (1.221e-15, "runs_21_err")}     # next runs_231_err 8.882e-16, runs_12_reg 7.182e-16
TOL = {e: min(10 * MEASURED_DEVIATION[e][0], 1e-10) for e in ENTRIES}
HOST_TOL = 1e-12                                 # the numpy model of a right fold against the restatement
WRONG_FACTOR = 100                               # a wrong fold lies at least this many bounds away
EXCUSED = 1e-12                                  # test_hip_calibration.EXCUSED: a row this close to an edge may fall either way
MAX_GROUP = 3                                    # kMaxCand, kWideMaxCand: sets a pass of the replay carries at most
WORKGROUP = 256                                  # kFiThreads
N_FEATURES = lc.N_FEATURES
KINDS = uc.KINDS                                 # "cat" | "reg" | "err" -> the entries' names of the kinds
RUNS = ((1,), (2,), (3,), (2, 1), (1, 2), (1, 3), (1, 1, 3), (2, 3, 1), (3, 3))
_BINS = (15, 64, 1)
_LEVELS = (cc.DEFAULT_LEVELS, (0.9,), ())

_DEFAULTS = dict(rows=257, kind="cat", n_out=None, fun="tanh", nodes=(6, 5), sets=4, runs=None, bias=2, train_rows=None, n_bins=None)
_DEFAULT_WIDTH = {"cat": 3, "reg": 3, "err": 4}
CASES = {}


def _case(name, **kw):
    unknown = set(kw) - set(_DEFAULTS)
    assert not unknown and name not in CASES, (name, unknown)
    c = dict(_DEFAULTS, name=name, **kw)
    if c["n_out"] is None:
        c["n_out"] = _DEFAULT_WIDTH[c["kind"]]
    if c["runs"] is not None:
        c.update(fun="genReLU", sets=sum(c["runs"]))
    i = len(CASES)
    c.update(n_bins=c["n_bins"] or _BINS[i % 3], levels=_LEVELS[(i // 3) % 3] if c["kind"] != "cat" else (),
             entries=tuple(e for e in ENTRIES if not (e == "lppd" and c["kind"] == "err")))
    CASES[name] = c
    cc.register(name, c["kind"], c["n_bins"], c["levels"])


# rows: classification and identity regression in turn, so that both partial layouts see one to four workgroups (the default, 257 rows,
# is every other case's: a ragged second workgroup of one row)
for _i, _n in enumerate((1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 769)):
    _case("rows_%d" % _n, rows=_n, kind=("cat", "reg")[_i % 2])
for _c in (1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 31, 32):
    _case("classes_%d" % _c, n_out=_c)
for _t in (1, 2, 3, 4, 5, 8, 12):
    _case("targets_%d" % _t, kind="reg", n_out=_t)
for _o in (2, 4, 6, 8, 10, 12, 16):
    _case("outputs_%d" % _o, kind="err", n_out=_o)
# every run-length pattern on the softmax fold and on a regression fold (identity and means plus sigmas in turn)
for _i, _r in enumerate(RUNS):
    _tag = "".join(str(v) for v in _r)
    _case("runs_%s_cat" % _tag, runs=_r)
    # (two sets that predict sigmas near 1e-4 - genReLU is unbounded - have transforms of 0 or 1 and a mean transform of exactly 0.5 on
    # dozens of rows: an edge of 64 bins, which the cycle would give that case, and of no odd number of bins)
    _case("runs_%s_%s" % (_tag, ("reg", "err")[_i % 2]), runs=_r, kind=("reg", "err")[_i % 2], n_bins=15 if _r == (2,) else None)
for _k in ("cat", "reg", "err"):
    _case("test_table_%s" % _k, rows=513, train_rows=300, kind=_k)
CROSSED = ("rows_513_classes_12", "rows_513_outputs_12", "rows_513_targets_8_runs_231", "rows_1_classes_8")
_case(CROSSED[0], rows=513, n_out=12)
_case(CROSSED[1], rows=513, kind="err", n_out=12)
_case(CROSSED[2], rows=513, kind="reg", n_out=8, runs=(2, 3, 1))
_case(CROSSED[3], rows=1, n_out=8)
TEST_TABLE = tuple(n for n in CASES if CASES[n]["train_rows"])
# six tanh sets: two passes of three as they come, and the device of test_grouping_of_the_sets_does_not_matter - distinct slope vectors,
# which tanh ignores - splits them into any other pattern (test_hip_fold_envelope.test_grouping_same_bytes)
GROUPING = ("grouping_cat", "grouping_reg", "grouping_err")
for _k in ("cat", "reg", "err"):
    _case("grouping_%s" % _k, sets=6, kind=_k)


def cases_of(entry):
    return [n for n in CASES if entry in CASES[n]["entries"]]


def n_workgroups(n_rows):
    """grid_for: one workgroup per 256 rows (no case comes near the 2048 at which a workgroup takes a second stride)."""
    return max(1, -(-n_rows // WORKGROUP))


def expected_groups(slopes, n_sets):
    """[(s0, g)]: the passes of the replay - sets that share set s0's slope vector travel together, MAX_GROUP at most (no slopes:
    all share)."""
    out, s0 = [], 0
    while s0 < n_sets:
        g = 1
        while s0 + g < n_sets and g < MAX_GROUP and (slopes is None or np.array_equal(slopes[s0 + g], slopes[s0])):
            g += 1
        out.append((s0, g))
        s0 += g
    return out


def kernel_build(entry, case):
    """(fold kernel, its template arguments, iterations of its loop over the row) a case selects in an entry: VEC is on when the outputs
    are a multiple of 4; vectors are float4, in cal_regress_accumulate_kernel<SP = true> float2 pairs of targets."""
    kind, n_out = case["kind"], case["n_out"]
    vec = n_out % 4 == 0
    if kind == "cat":
        if entry == "lppd":
            return "lppd_accumulate_kernel", (False, vec), n_out // 4 if vec else n_out
        return "softmax_mean_accumulate_kernel", (entry == "uncertainty", vec), n_out // 4 if vec else n_out
    sp = kind == "err"
    if entry == "lppd":
        return "lppd_accumulate_kernel", (True, vec), n_out // 4 if vec else n_out
    if entry == "uncertainty":
        return "unc_regress_accumulate_kernel", (sp, vec), n_out // 4 if vec else n_out
    t = n_out // 2 if sp else n_out
    return "cal_regress_accumulate_kernel", (sp, vec), t // ((2 if sp else 4) if vec else 1)


BUILDS = tuple([("lppd_accumulate_kernel", (g, v)) for g in (False, True) for v in (False, True)] +
               [("softmax_mean_accumulate_kernel", (e, v)) for e in (False, True) for v in (False, True)] +
               [(k, (s, v)) for k in ("unc_regress_accumulate_kernel", "cal_regress_accumulate_kernel") for s in (False, True) for v in (False, True)])


def _seed(name):
    return "fold_envelope/" + name


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def inputs(name):
    """What a case hands the device and the restatements: ``x`` and ``labels`` (class indices or targets [rows, T]; drawn for every
    kind, uncertainty reads none) of the table the statistic is taken on, ``train_x`` and ``train_labels`` of the training slot above
    a test table (else None), the stored ``samples``, ``slopes`` (per set, or None), ``sigma`` [S, T] (identity regression, else
    None), and the passes ``groups`` the replay has to report."""
    case = CASES[name]
    spec = dict(fun=case["fun"], nodes=case["nodes"], n_out=case["n_out"], s=case["sets"], bias=case["bias"], kind=case["kind"])
    inp = cc.inputs(name, case["rows"], spec, _seed(name))
    if case["runs"] is not None:
        # (the slopes are the generator's, one vector per set; a run takes its first set's)
        s0 = 0
        for run in case["runs"]:
            for s in range(s0 + 1, s0 + run):
                inp["samples"][s]["alphas"] = inp["samples"][s0]["alphas"]
            s0 += run
    slopes = lc.slopes_of(inp)
    out = dict(inp, case=case, slopes=slopes, sigma=lc.sigmas_of(inp), groups=expected_groups(slopes, case["sets"]), train_x=None, train_labels=None,
               x=_frozen(inp["x"]), labels=_frozen(inp["labels"]))
    if case["runs"] is not None:
        assert tuple(g for _, g in out["groups"]) == case["runs"], (name, out["groups"])
    if case["train_rows"]:
        # the training slot: rows, labels or targets of its own draw (another teacher, another generator)
        train = cc.inputs(name, case["train_rows"], spec, _seed(name) + "/train")
        out.update(train_x=_frozen(train["x"]), train_labels=_frozen(train["labels"]))
    return out


def oracle_z(name):
    """The float64 oracle's pre-output values of a case, as a float32 holds them: what the host tests fold."""
    return uc.oracle_values(inputs(name)).astype(np.float32).astype(np.float64)


# ---- the restatements ---------------------------------------------------------------------------------------------------------------
def lppd_restatement(ll):
    """lppd's quantities from ll [S, N] in float64, by their definitions (no shared code with npbnn_amd.lppd): logsumexp over the
    sets minus log S, the mean, the variance with ddof 1, the per-set row sums, and the totals over the rows."""
    ll = np.asarray(ll, dtype=np.float64)
    n_sets = ll.shape[0]
    top = ll.max(axis=0)
    lppd_i = top + np.log(np.exp(ll - top[None]).sum(axis=0)) - np.log(n_sets)
    mean_i = ll.sum(axis=0) / n_sets
    p_waic_i = ((ll - mean_i[None]) ** 2).sum(axis=0) / (n_sets - 1) if n_sets > 1 else np.zeros(ll.shape[1])
    return dict(lppd_i=lppd_i, mean_log_lik_i=mean_i, p_waic_i=p_waic_i, log_lik_sample=ll.sum(axis=1), lppd=float(lppd_i.sum()),
                mean_log_lik=float(mean_i.sum()), p_waic=float(p_waic_i.sum()))


def want_of(entry, name, z):
    """The float64 restatement of an entry's fields from pre-output values z [S, N, outputs], under the device dict's keys."""
    inp = inputs(name)
    case, kind = inp["case"], KINDS[inp["kind"]]
    if entry == "lppd":
        return lppd_restatement(lc.log_lik_from_values(z, inp["labels"], inp["kind"], inp["sigma"]))
    if entry == "calibration":
        return cc.restatement(z, inp["labels"], kind, inp["sigma"], case["n_bins"], case["levels"])
    w = uc.restatement(z, kind, inp["sigma"])
    if kind == "classification":
        w.update({total: float(np.mean(w[field])) for total, field in uc.CLASS_TOTALS.items()})
        return w
    if kind == "regression":                     # (the identity output predicts no sigma: the aleatoric part is the caller's)
        w = dict(mean=w["mean"], epistemic_var=w["epistemic_var"])
    w.update({k + "_avg": np.mean(v, axis=0) for k, v in list(w.items())})
    return w


def float_fields(want):
    return [k for k, v in want.items() if v is not None and np.asarray(v).dtype.kind == "f"]


def integer_fields(want):
    return [k for k, v in want.items() if v is not None and np.asarray(v).dtype.kind in "iu"]


def deviation(got, want):
    """max |got - want| / max(1, |want|); an infinite value (the nll of a zero probability) has to be the same on both sides, and a
    NaN or a missing value counts as infinitely far."""
    want = np.asarray(want, dtype=np.float64)
    if got is None or np.shape(got) != want.shape:
        return np.inf
    got = np.asarray(got, dtype=np.float64)
    if want.size == 0:
        return 0.0
    fin = np.isfinite(want)
    if not np.array_equal(got[~fin], want[~fin]) or np.any(np.isnan(got)):
        return np.inf
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])))) if fin.any() else 0.0


def worst_deviation(got, want):
    return max(deviation(got[k], want[k]) for k in float_fields(want))


def top_two_gap(z):
    """[N]: the difference of the two largest mean probabilities of a row (infinite with a single class)."""
    m = uc.restatement(z, "classification")["mean_prob"]
    if m.shape[1] < 2:
        return np.full(len(m), np.inf)
    top = np.sort(m, axis=1)
    return top[:, -1] - top[:, -2]


def rows_that_may_fall_either_way(name, z):
    """test_hip_calibration._kernel_check's count on values z: rows whose confidence or transform lies within EXCUSED of a bin or
    coverage edge, and rows whose two largest mean probabilities differ by at most EXCUSED without being equal."""
    want = want_of("calibration", name, z)
    if CASES[name]["kind"] != "cat":
        return cc.rows_near_an_edge(name, want["pit"], EXCUSED)
    gap = top_two_gap(z)
    return cc.rows_near_an_edge(name, want["confidence"], EXCUSED) + int(np.sum((gap > 0) & (gap <= EXCUSED)))
