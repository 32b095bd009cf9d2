"""The cases of tests/golden/calibration.npz (make_calibration_golden.py): seeded inputs, keys, and an independent float64 restatement
of posterior calibration from pre-output values.

Classification and ``"regression"`` inputs are ``lppd_cases.inputs`` (203 ragged rows, 11 features; they carry labels and targets a
float32 holds exactly).  The ``"regression-error"`` inputs are ``uncertainty_cases.ERROR_CASES``' networks; their targets are made
here, seeded: the teacher's mean plus the teacher's softplus sigma times normal noise, rounded through float32.  Every case has its
own number of bins, one of {1, 10, 15, 64}, and its own coverage levels: none, one, or the default four."""
import math
import os

import numpy as np

import cases
import lppd_cases as lc
import uncertainty_cases as uc

N_ROWS = lc.N_ROWS
N_FEATURES = lc.N_FEATURES
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calibration.npz")
DEFAULT_LEVELS = (0.5, 0.8, 0.9, 0.95)
CLASS_POINT = ("confidence", "predicted_class", "brier_i", "nll_i")
CLASS_TABLES = ("count", "sum_confidence", "n_correct")
CLASS_SCORES = ("accuracy", "brier", "nll", "ece", "mce")
REGRESSION_POINT = ("pit", "mean", "sq_err")
REGRESSION_TABLES = ("pit_hist", "covered")
REGRESSION_SCORES = ("rmse", "mean_pit", "coverage", "coverage_error")
# name -> bins, coverage levels (not read by classification)
PARAMS = {
    "relu_h1_c2_s1": dict(n_bins=15, levels=()),
    "tanh_h2_c4_s7": dict(n_bins=10, levels=()),
    "swish_h3_c3_s4": dict(n_bins=1, levels=()),
    "genrelu_h2_c10_s64": dict(n_bins=64, levels=()),
    "genrelu_h2_c4_s3": dict(n_bins=10, levels=()),
    "tanh_h2_c10_s2": dict(n_bins=15, levels=()),
    "relu_h2_c3_s64": dict(n_bins=15, levels=()),
    "tanh_h2_reg1_s7": dict(n_bins=64, levels=DEFAULT_LEVELS),
    "swish_h1_reg3_s4": dict(n_bins=10, levels=(0.9,)),
    "genrelu_h3_reg3_s3": dict(n_bins=1, levels=DEFAULT_LEVELS),
    "relu_h2_reg4_s64": dict(n_bins=10, levels=DEFAULT_LEVELS),
    "tanh_h2_err2_s7": dict(n_bins=64, levels=DEFAULT_LEVELS),
    "genrelu_h2_err1_s3": dict(n_bins=1, levels=(0.9,)),
    "swish_h1_err3_s1": dict(n_bins=10, levels=()),
    "relu_h3_err3_s7": dict(n_bins=15, levels=DEFAULT_LEVELS),
}
CASES = uc.CASES
assert sorted(PARAMS) == sorted(CASES)
# name -> dict(kind, n_bins, levels): the cases of another table (fold_envelope_cases) that go through this module's helpers
EXTRA = {}


def register(name, kind, n_bins, levels):
    """A case of another table under the helpers here that take a case by name (``params``, ``edges_of``, ``rows_near_an_edge``,
    ``point_fields_of``, ``score_fields_of``): its kind in CASES' letters, its bins and its coverage levels."""
    assert name not in CASES and name not in EXTRA, name
    EXTRA[name] = dict(kind=kind, n_bins=n_bins, levels=tuple(levels))


def _kind(name):
    return (CASES[name] if name in CASES else EXTRA[name])["kind"]


def key(name, field):
    return "%s/%s" % (name, field)


kind_of = uc.kind_of
act_for = uc.act_for
slopes_of = uc.slopes_of
sigmas_of = uc.sigmas_of
outputs_from_values = uc.outputs_from_values
oracle_values = uc.oracle_values


def fields_of(name):
    """What the golden file holds of a case: the pointwise arrays and the tables, and for classification ``top_two_gap`` [N], the
    difference of the two largest mean probabilities (the margin of ``predicted_class``; 1 - ... for two classes is just that)."""
    return CLASS_POINT + CLASS_TABLES + ("top_two_gap",) if CASES[name]["kind"] == "cat" else REGRESSION_POINT + REGRESSION_TABLES


def point_fields_of(name):
    return CLASS_POINT if _kind(name) == "cat" else REGRESSION_POINT


def score_fields_of(name):
    return CLASS_SCORES if _kind(name) == "cat" else REGRESSION_SCORES


def params(name):
    p = PARAMS[name] if name in PARAMS else EXTRA[name]
    return p["n_bins"], tuple(p["levels"])


def _error_targets(name, inp, spec=None, seed=None):
    """Targets of a ``"regression-error"`` case: the teacher of ``uncertainty_cases.inputs`` (its generator replayed to the same
    draws), its mean plus its softplus sigma times seeded normal noise, as a float32 holds them.  ``spec`` and ``seed``: as
    ``uncertainty_cases.inputs`` takes them, for a case of another table; the noise is then seeded from ``seed + "/noise"``."""
    import oracle as orc
    spec = uc.ERROR_CASES[name] if spec is None else spec
    rs = np.random.default_rng(cases.hash_name("uncertainty/" + name if seed is None else seed) % (2 ** 31))
    x = rs.standard_normal((len(inp["x"]), N_FEATURES))
    assert np.array_equal(x, inp["x"])
    teacher = [rs.normal(0, 0.6, s) for s in cases.layer_shapes(N_FEATURES, list(spec["nodes"]), spec["n_out"], spec["bias"])]
    z = orc.forward_logits(x, teacher, orc.Act(spec["fun"], np.full(len(spec["nodes"]), 0.15)))
    t = spec["n_out"] // 2
    noise = np.random.default_rng(cases.hash_name("calibration/" + name if seed is None else seed + "/noise") % (2 ** 31)).standard_normal((len(x), t))
    return (z[:, :t] + np.logaddexp(0.0, z[:, t:]) * noise).astype(np.float32).astype(np.float64)


def inputs(name, n_rows=N_ROWS, spec=None, seed=None):
    """x, the stored samples, and labels (class indices) or targets [rows, T], with the case's description.  ``spec`` and ``seed``:
    as ``uncertainty_cases.inputs`` takes them, for a case of another table (fold_envelope_cases)."""
    inp = uc.inputs(name, n_rows, spec, seed)
    if inp["kind"] == "err":
        inp = dict(inp, labels=_error_targets(name, inp, spec, seed))
    return inp


def _phi(u):
    return 0.5 * math.erfc(-u / math.sqrt(2.0))


def restatement(z, labels, kind, sigma=None, n_bins=15, levels=DEFAULT_LEVELS):
    """The definitions, row by row in float64, from pre-output values z [S, N, outputs] (no shared code with the package): tables,
    scores and pointwise values under ``posterior_calibration``'s keys."""
    z = np.asarray(z, dtype=np.float64)
    n_samples, n_rows, n_out = z.shape
    if kind == "classification":
        # (whole arrays at once: the grid-stride table has half a million rows)
        lab = np.asarray(labels, dtype=np.int64)
        rows = np.arange(n_rows)
        e = np.exp(z - z.max(axis=2, keepdims=True))
        m = np.zeros((n_rows, n_out))
        for s in range(n_samples):
            m += e[s] / e[s].sum(axis=1, keepdims=True)
        m /= n_samples
        best = np.argmax(m, axis=1)
        conf = m[rows, best]
        hit = np.zeros((n_rows, n_out))
        hit[rows, lab] = 1.0
        brier = ((m - hit) ** 2).sum(axis=1)
        with np.errstate(divide="ignore"):
            nll = np.where(m[rows, lab] > 0, -np.log(m[rows, lab]), np.inf)
        b = np.minimum(n_bins - 1, np.floor(conf * n_bins).astype(np.int64))
        count = np.bincount(b, minlength=n_bins)
        sum_conf = np.bincount(b, weights=conf, minlength=n_bins)
        n_correct = np.bincount(b[best == lab], minlength=n_bins)
        gaps = [abs(n_correct[j] / count[j] - sum_conf[j] / count[j]) for j in range(n_bins) if count[j]]
        ece = sum(count[j] / n_rows * abs(n_correct[j] / count[j] - sum_conf[j] / count[j]) for j in range(n_bins) if count[j])
        return dict(confidence=conf, predicted_class=best, brier_i=brier, nll_i=nll, count=count, sum_confidence=sum_conf, n_correct=n_correct,
                    accuracy=float(np.mean(best == lab)), brier=float(brier.mean()), nll=float(nll.mean()), ece=float(ece), mce=float(max(gaps)))
    lv = list(levels)
    y = np.asarray(labels, dtype=np.float64).reshape(n_rows, -1)
    n_targets = y.shape[1]
    pit, mean = np.zeros((n_rows, n_targets)), np.zeros((n_rows, n_targets))
    pit_hist, covered = np.zeros((n_targets, n_bins), dtype=np.int64), np.zeros((n_targets, len(lv)), dtype=np.int64)
    for i in range(n_rows):
        for t in range(n_targets):
            acc = 0.0
            for s in range(n_samples):
                if kind == "regression-error":
                    v = z[s, i, n_targets + t]
                    sg = max(v, 0.0) + math.log1p(math.exp(-abs(v)))
                else:
                    sg = float(np.asarray(sigma, dtype=np.float64)[s, t])
                acc += _phi((y[i, t] - z[s, i, t]) / sg)
            pit[i, t] = acc / n_samples
            mean[i, t] = math.fsum(z[:, i, t]) / n_samples
            pit_hist[t, min(n_bins - 1, int(math.floor(pit[i, t] * n_bins)))] += 1
            for j, level in enumerate(lv):
                covered[t, j] += int(abs(pit[i, t] - 0.5) <= level / 2)
    sq_err = (y - mean) ** 2
    coverage = covered / n_rows
    return dict(pit=pit, mean=mean, sq_err=sq_err, pit_hist=pit_hist, covered=covered, rmse=np.sqrt(sq_err.mean(axis=0)), mean_pit=pit.mean(axis=0),
                coverage=coverage, coverage_error=np.mean(np.abs(coverage - np.array(lv)[None, :]), axis=1) if lv else None)


def edges_of(name):
    """The values at which a row changes its place in a case's tables: the interior bin edges j / B (at 0 and at 1 both sides fall
    in the same bin), and for regression the coverage edges (1 +- level) / 2."""
    n_bins, levels = params(name)
    e = [j / n_bins for j in range(1, n_bins)]
    if _kind(name) != "cat":
        e += [(1 - lv) / 2 for lv in levels] + [(1 + lv) / 2 for lv in levels]
    return np.array(e, dtype=np.float64)


def rows_near_an_edge(name, values, margin, mean_prob_gap=None, gap_margin=None):
    """How many rows of a case lie within ``margin`` of an edge in ``values`` (confidence [N] or pit [N, T]), or have their two
    largest mean probabilities within ``gap_margin`` (classification, ``mean_prob_gap`` [N])."""
    v = np.asarray(values, dtype=np.float64).reshape(len(values), -1)
    e = edges_of(name)
    near = np.zeros(len(v), dtype=bool) if not len(e) else np.any(np.abs(v[:, :, None] - e[None, None, :]) <= margin, axis=(1, 2))
    if mean_prob_gap is not None:
        near |= np.asarray(mean_prob_gap) <= gap_margin
    return int(near.sum())


def golden_scores(name, g=None):
    """The scores of a case from the golden file's tables and pointwise arrays, by their formulas (``fields_of``' arrays by name
    included): accuracy, brier, nll, ece for classification; rmse [T], coverage [T, L] for regression."""
    g = load() if g is None else g
    v = {f: g[key(name, f)] for f in fields_of(name)}
    if CASES[name]["kind"] == "cat":
        count, hit, conf = v["count"].astype(np.float64), v["n_correct"].astype(np.float64), v["sum_confidence"]
        full = count > 0
        v.update(accuracy=hit.sum() / N_ROWS, brier=v["brier_i"].mean(), nll=v["nll_i"].mean(),
                 ece=float(np.sum(count[full] / N_ROWS * np.abs(hit[full] / count[full] - conf[full] / count[full]))))
    else:
        v.update(rmse=np.sqrt(v["sq_err"].mean(axis=0)), coverage=v["covered"] / N_ROWS)
    return v


def load():
    return np.load(GOLDEN)
