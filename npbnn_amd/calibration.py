"""Posterior calibration of stored posterior samples: ``posterior_calibration``, ``get_posterior_calibration``.

A Bayesian network is trained to be believed when it says "90 %"; this checks that claim against held-out labels or targets.  The
reference has no such function; the predictions are its own (``RunPredict`` per stored sample with ``SoftMax``,
``RegressTransform`` or ``RegressTransformError``, np_bnn/BNN_lib.py:166-182, 245-256).  Float64 throughout, ``S`` stored samples in
sample order, ``B = n_bins`` equal-width bins on [0, 1]:

  classification, ``p_s`` a sample's class probabilities of a row, ``m = (1/S) sum_s p_s``:
    predicted_class = the first argmax of m        confidence = m[predicted_class]
    brier_i = sum_k (m_k - [k == label])^2         nll_i = -log m[label]  (+inf when m[label] is 0: a value, not an error)
    the reliability table per bin min(B - 1, floor(confidence B)): count, sum_confidence, n_correct
    accuracy, brier, nll: the means over the rows  ece = sum_b (count_b / N) |n_correct_b / count_b - sum_confidence_b / count_b|
    mce = the largest of those gaps (non-empty bins)
  regression, ``mu_s`` / ``sigma_s`` a sample's mean / standard deviation per target, ``y`` the target:
    pit = (1/S) sum_s Phi((y - mu_s) / sigma_s), Phi(u) = 0.5 erfc(-u / sqrt 2): the probability integral transform under the
    posterior predictive mixture - uniform on [0, 1] when the predictive distribution is calibrated
    mean = mu_1 + (1/S) sum_s (mu_s - mu_1)        sq_err = (y - mean)^2
    pit_hist [T, B]: the rows per bin min(B - 1, floor(pit B))
    covered [T, L]: the rows with |pit - 0.5| <= level / 2 - the target lies inside the mixture's central interval of that level
    rmse [T], mean_pit [T], coverage = covered / N, coverage_error [T] = mean over the levels of |coverage - level|
  with sigma from the samples' ``error_prm`` (``"regression"``) or predicted per row (``"regression-error"``: the second half of
  the outputs).

``posterior_calibration`` is that definition on a host ``[S, N, outputs]`` array.  ``get_posterior_calibration`` replays a
checkpoint's stored samples on the device and folds every group of samples into per-row accumulators there
(``npbnn_predict_sets_calibration``): the stack is never built and only the tables and the per-row values come back.  Both derive
their scores from the tables with the same function (``scores_from_table``)."""
import numpy as np

from .files import load_obj
from .stored import choose_table, class_labels, open_checkpoint, open_predictor, sample_sigmas, sigma_matrix, target_matrix

KINDS = ("classification", "regression", "regression-error")
DEFAULT_LEVELS = (0.5, 0.8, 0.9, 0.95)
MAX_BINS = 64
MAX_LEVELS = 16
CLASS_POINT_KEYS = ("confidence", "predicted_class", "brier_i", "nll_i")
REGRESSION_POINT_KEYS = ("pit", "mean", "sq_err")


def check_bins_and_levels(n_bins, levels, who):
    """(n_bins as an int, levels as a float64 array) or ``ValueError``: 1..64 bins, at most 16 levels strictly inside (0, 1)."""
    if isinstance(n_bins, bool) or int(n_bins) != n_bins or not 1 <= int(n_bins) <= MAX_BINS:
        raise ValueError("%s: n_bins must be an integer in 1..%d, got %r" % (who, MAX_BINS, n_bins))
    lv = np.asarray(() if levels is None else levels, dtype=np.float64).ravel()
    if len(lv) > MAX_LEVELS:
        raise ValueError("%s: at most %d levels, got %d" % (who, MAX_LEVELS, len(lv)))
    if not np.all((lv > 0.0) & (lv < 1.0)):
        raise ValueError("%s: every level lies strictly inside (0, 1), got %s" % (who, lv.tolist()))
    return int(n_bins), lv


def scores_from_table(table, n_rows):
    """The scores of a calibration table, a dict of the sums over the rows: classification ``count``, ``sum_confidence``,
    ``n_correct`` [B], ``brier_sum``, ``nll_sum`` -> ``accuracy``, ``brier``, ``nll``, ``ece``, ``mce``; regression ``pit_hist``
    [T, B], ``covered`` [T, L], ``levels`` [L], ``sq_err_sum``, ``pit_sum`` [T] -> ``rmse``, ``mean_pit`` [T], ``coverage`` [T, L],
    ``coverage_error`` [T] (None without levels).  The one place the host definition and the device route compute them."""
    n = float(n_rows)
    if "count" in table:
        count = np.asarray(table["count"], dtype=np.float64)
        filled = count > 0
        gap = np.abs(np.asarray(table["n_correct"], dtype=np.float64)[filled] / count[filled]
                     - np.asarray(table["sum_confidence"], dtype=np.float64)[filled] / count[filled])
        return dict(accuracy=float(np.sum(table["n_correct"]) / n), brier=float(table["brier_sum"] / n), nll=float(table["nll_sum"] / n),
                    ece=float(np.sum(count[filled] / n * gap)), mce=float(np.max(gap)) if len(gap) else 0.0)
    levels = np.asarray(table["levels"], dtype=np.float64)
    coverage = np.asarray(table["covered"], dtype=np.float64) / n
    return dict(rmse=np.sqrt(np.asarray(table["sq_err_sum"], dtype=np.float64) / n), mean_pit=np.asarray(table["pit_sum"], dtype=np.float64) / n,
                coverage=coverage, coverage_error=np.mean(np.abs(coverage - levels[None, :]), axis=1) if len(levels) else None)


def _bin_of(value, n_bins):
    return np.minimum(n_bins - 1, np.floor(value * n_bins).astype(np.int64))


def posterior_calibration(stack, labels, kind="classification", n_bins=15, levels=DEFAULT_LEVELS, sigma_sets=None):
    """The definitions above on ``stack`` [S, N, outputs], the samples' post-output predictions (float64 numpy on the host): class
    probabilities against class indices ``labels`` [N] (``"classification"``), means with ``sigma_sets`` [S, targets] or [S]
    against targets ``labels`` [N, T] (``"regression"``), or means followed by as many sigmas (``"regression-error"``).  Returns a
    dict with ``n_samples``, ``n_rows``, ``n_bins`` and, for classification, the table ``count``, ``sum_confidence``, ``n_correct``
    [B], the scores ``accuracy``, ``brier``, ``nll``, ``ece``, ``mce`` and the pointwise ``confidence``, ``predicted_class``,
    ``brier_i``, ``nll_i`` [N]; for regression ``levels`` [L], the tables ``pit_hist`` [T, B], ``covered`` [T, L], the scores
    ``rmse``, ``mean_pit`` [T], ``coverage`` [T, L], ``coverage_error`` [T] (None without levels) and the pointwise ``pit``,
    ``mean``, ``sq_err`` [N, T].  ``ValueError`` on NaN, on bad shapes and on labels out of range."""
    from scipy.special import erfc
    who = "posterior_calibration"
    if kind not in KINDS:
        raise ValueError("%s: kind %r; one of %s" % (who, kind, ", ".join(KINDS)))
    n_bins, lv = check_bins_and_levels(n_bins, levels, who)
    y = np.asarray(stack, dtype=np.float64)
    if y.ndim != 3 or 0 in y.shape:
        raise ValueError("%s: stack must be a non-empty [samples, rows, outputs] array, got shape %s" % (who, y.shape))
    if np.any(np.isnan(y)):
        raise ValueError("%s: stack holds NaN" % who)
    n_samples, n_rows = y.shape[:2]
    res = dict(n_samples=int(n_samples), n_rows=int(n_rows), n_bins=n_bins)
    if kind == "classification":
        if sigma_sets is not None:
            raise ValueError("%s: sigma_sets goes with kind \"regression\" only" % who)
        lab = class_labels(labels, n_rows, y.shape[2], who)
        rows = np.arange(n_rows)
        mean_prob = np.sum(y, axis=0) / n_samples
        best = np.argmax(mean_prob, axis=1)
        confidence = mean_prob[rows, best]
        one_hot = (np.arange(y.shape[2])[None, :] == lab[:, None]).astype(np.float64)
        brier_i = np.sum((mean_prob - one_hot) ** 2, axis=1)
        with np.errstate(divide="ignore"):
            nll_i = -np.log(mean_prob[rows, lab])
        bins = _bin_of(confidence, n_bins)
        table = dict(count=np.bincount(bins, minlength=n_bins).astype(np.int64),
                     sum_confidence=np.bincount(bins, weights=confidence, minlength=n_bins).astype(np.float64),
                     n_correct=np.bincount(bins[best == lab], minlength=n_bins).astype(np.int64))
        res.update(table)
        res.update(scores_from_table(dict(table, brier_sum=np.sum(brier_i), nll_sum=np.sum(nll_i)), n_rows))
        res.update(confidence=confidence, predicted_class=best.astype(np.int64), brier_i=brier_i, nll_i=nll_i)
        return res
    if kind == "regression-error":
        if y.shape[2] % 2:
            raise ValueError("%s: kind \"regression-error\" takes means followed by as many sigmas, and %d outputs is odd" % (who, y.shape[2]))
        if sigma_sets is not None:
            raise ValueError("%s: kind \"regression-error\" predicts its sigma: sigma_sets goes with kind \"regression\" only" % who)
        n_targets = y.shape[2] // 2
        mu, sig = y[:, :, :n_targets], y[:, :, n_targets:]
    else:
        n_targets = y.shape[2]
        mu, sig = y, sigma_matrix(sigma_sets, n_samples, n_targets, who)[:, None, :]
    t = target_matrix(labels, n_rows, n_targets, who)
    with np.errstate(divide="ignore", invalid="ignore"):
        pit = np.sum(0.5 * erfc(-((t[None] - mu) / sig) / np.sqrt(2.0)), axis=0) / n_samples
    if np.any(np.isnan(pit)):
        raise ValueError("%s: a probability integral transform is NaN (a sigma of 0 at its own mean)" % who)
    mean = mu[0] + np.sum(mu - mu[0], axis=0) / n_samples
    sq_err = (t - mean) ** 2
    bins = _bin_of(pit, n_bins)
    pit_hist = np.array([np.bincount(bins[:, k], minlength=n_bins) for k in range(n_targets)], dtype=np.int64)
    covered = np.sum(np.abs(pit - 0.5)[:, :, None] <= (lv / 2.0)[None, None, :], axis=0).astype(np.int64).reshape(n_targets, len(lv))
    res.update(levels=lv, pit_hist=pit_hist, covered=covered)
    res.update(scores_from_table(dict(levels=lv, covered=covered, sq_err_sum=np.sum(sq_err, axis=0), pit_sum=np.sum(pit, axis=0)), n_rows))
    res.update(pit=pit, mean=mean, sq_err=sq_err)
    return res


def strip_pointwise(res):
    return {k: v for k, v in res.items() if k not in CLASS_POINT_KEYS + REGRESSION_POINT_KEYS}


def get_posterior_calibration(pkl_file, features=None, labels=None, n_bins=15, levels=DEFAULT_LEVELS, pointwise=True):
    """Calibration of a checkpoint's stored samples: on its own test table (default), on its training table
    (``features="train"``), or on ``features`` with ``labels`` given.  The kind follows the model's estimation mode -
    ``"classification"`` (labels are class indices), ``"regression"`` (targets; sigma per sample from the samples' ``error_prm``) or
    ``"regression-error"`` (targets; sigma predicted per row); predictions as ``get_posterior_est`` computes them (per-sample slopes,
    the last sample's slopes left installed).  Returns ``posterior_calibration``'s dict; without ``pointwise`` the [N, ...] arrays
    are left out (they then never leave the device).  ``ValueError`` before any device call: no stored samples, an empty table,
    labels that are not class indices or targets of another shape, ``n_bins`` or ``levels`` out of range, a ``"regression"``
    checkpoint without ``error_prm``, an odd number of outputs under ``"regression-error"``, ``"custom"`` and the count
    likelihoods' estimation modes."""
    who = "get_posterior_calibration"
    n_bins, lv = check_bins_and_levels(n_bins, levels, who)
    model, samples, mode, n_out = open_checkpoint(load_obj(pkl_file), who, KINDS, "%s are served; \"custom\" and the count likelihoods are not" % ", ".join(KINDS))
    x, y = choose_table(model, features, labels, who, need_labels=True)
    sigma = None
    if mode == "classification":
        y = class_labels(y, len(x), n_out, who)
    elif mode == "regression":
        y, sigma = target_matrix(y, len(x), n_out, who), sample_sigmas(samples, n_out, who)
    else:
        if n_out % 2:
            raise ValueError("%s: \"regression-error\" predicts a mean and a sigma per target, and %d outputs is odd" % (who, n_out))
        y = target_matrix(y, len(x), n_out // 2, who)
    with open_predictor(model, samples, x.shape[1]) as pred:
        res = pred.calibration(x, y, mode, n_bins=n_bins, levels=lv, sigma_sets=sigma, pointwise=pointwise)
    res = dict(res, n_samples=len(samples), n_rows=len(x))
    return res if pointwise else strip_pointwise(res)
