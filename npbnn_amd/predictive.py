"""The posterior predictive distribution of stored posterior samples: ``posterior_predictive``, ``get_posterior_predictive``.

``get_posterior_hpd`` gives the interval of the mean function, which covers epistemic uncertainty only, and
``get_posterior_calibration`` evaluates the predictive mixture's distribution function at the observed target.  This module gives
the distribution itself: between which bounds a new observation falls with a given probability, and how good the distribution is as
a whole.  The reference has no such function (its summary code, BNN_plot.py:73-75, takes calcHPD of the means); the predictions are
its own (``RunPredict`` per stored sample with ``RegressTransform`` or ``RegressTransformError``, np_bnn/BNN_lib.py:174-182,
245-256).  Float64 throughout; a cell is one (row, target) pair with ``S`` components ``mu_s``, ``sigma_s``, one per stored sample:

    F(x)       = (1/S) sum_s Phi((x - mu_s) / sigma_s)        Phi(u) = 0.5 erfc(-u / sqrt 2)
    quantile_p = the x with F(x) = p                          (F is continuous and strictly increasing: x is unique)
    mean       = mu_1 + (1/S) sum_s (mu_s - mu_1)
    A(m, v)    = 2 sqrt(v) phi(m / sqrt v) + m erf(m / sqrt(2 v))      (= E|N(m, v)|; both terms are >= 0)
    crps(y)    = (1/S) sum_s A(y - mu_s, sigma_s^2)
                 - (1/(2 S^2)) [sum_s 2 sigma_s / sqrt(pi) + 2 sum_{s<t} A(mu_s - mu_t, sigma_s^2 + sigma_t^2)]

with sigma from the samples' ``error_prm`` (``"regression"``) or predicted per row (``"regression-error"``: the second half of the
outputs).  The CRPS is the continuous ranked probability score, the strictly proper score of a predictive distribution (lower is
better; it has the target's unit), in the closed form of a Gaussian mixture.

Limits: at most 16384 samples, at most 16 probabilities, each with ``min(p, 1 - p) >= 1e-12``, every sigma positive and finite.  The
CRPS costs ``S (S - 1) / 2`` pair terms per cell.

``posterior_predictive`` is that definition on a host ``[S, N, outputs]`` array.  ``get_posterior_predictive`` replays a checkpoint's
stored samples on the device into a float32 stack that never leaves it (``npbnn_predict_sets_predictive``): only the quantiles, the
mean and the scores come back."""
import numpy as np

from .files import load_obj
from .hpd import stack_rows
from .layers import output_kind
from .stored import choose_table, open_checkpoint, open_predictor, sample_sigmas, sigma_matrix, target_matrix

KINDS = ("regression", "regression-error")
DEFAULT_PROBS = (0.025, 0.5, 0.975)
MAX_SAMPLES = 16384
MAX_PROBS = 16
MIN_TAIL = 1e-12


def check_probs(probs, who):
    """``probs`` as a float64 vector, or ``ValueError``: at most 16 of them, each with ``min(p, 1 - p) >= 1e-12``."""
    pr = np.ascontiguousarray(np.asarray(() if probs is None else probs, dtype=np.float64).ravel())
    if len(pr) > MAX_PROBS:
        raise ValueError("%s: at most %d probabilities, got %d" % (who, MAX_PROBS, len(pr)))
    if not np.all(np.minimum(pr, 1.0 - pr) >= MIN_TAIL):
        raise ValueError("%s: every probability needs min(p, 1 - p) >= %g, got %s" % (who, MIN_TAIL, pr.tolist()))
    return pr


def _abs_moment(m, sd):
    """A(m, sd^2) = E|N(m, sd^2)|, with erf: both terms are >= 0"""
    from scipy.special import erf
    z = m / sd
    return 2.0 * sd * (np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)) + m * erf(z / np.sqrt(2.0))


def _h(x, mu, sig, prob):
    """F(x) - prob per cell, on the tail that keeps its precision; x [cells], mu and sig [S, cells]"""
    from scipy.special import erfc
    u = (x[None] - mu) / sig / np.sqrt(2.0)
    upper = prob > 0.5
    tail = 0.5 * np.sum(erfc(np.where(upper, u, -u)), axis=0) / len(mu)
    return np.where(upper, (1.0 - prob) - tail, tail - prob)


def _quantile(mu, sig, prob):
    """The quantile of ``prob`` of every cell by bisection, run until no bracket can narrow; mu and sig [S, cells]."""
    from scipy.special import ndtri
    own = mu + sig * ndtri(prob)
    lo, hi = own.min(axis=0), own.max(axis=0)
    # (every component's own quantile lies inside, up to rounding: widen while an end is on the wrong side)
    w = np.maximum(hi - lo, np.maximum(np.maximum(np.abs(lo), np.abs(hi)) * np.finfo(np.float64).eps, np.finfo(np.float64).tiny))
    for _ in range(128):
        bad = _h(lo, mu, sig, prob) > 0
        if not bad.any():
            break
        lo = np.where(bad, lo - w, lo)
        w = np.where(bad, w + w, w)
    for _ in range(128):
        bad = _h(hi, mu, sig, prob) < 0
        if not bad.any():
            break
        hi = np.where(bad, hi + w, hi)
        w = np.where(bad, w + w, w)
    while True:
        mid = lo + 0.5 * (hi - lo)
        live = (mid > lo) & (mid < hi)
        if not live.any():
            break
        left = _h(mid, mu, sig, prob) < 0
        lo = np.where(live & left, mid, lo)
        hi = np.where(live & ~left, mid, hi)
    # the end of smaller residual
    return np.where(np.abs(_h(lo, mu, sig, prob)) <= np.abs(_h(hi, mu, sig, prob)), lo, hi)


def _crps(mu, sig, y):
    """crps per cell; mu and sig [S, cells], y [cells]"""
    n = len(mu)
    t1 = np.sum(_abs_moment(y[None] - mu, sig), axis=0) / n
    pair = np.zeros(mu.shape[1])
    for s in range(n - 1):                                  # sample row by sample row: [S - 1 - s, cells] terms at once
        pair += np.sum(_abs_moment(mu[s][None] - mu[s + 1:], np.hypot(sig[s][None], sig[s + 1:])), axis=0)
    t2 = (np.sum(2.0 * sig / np.sqrt(np.pi), axis=0) + 2.0 * pair) / (float(n) * float(n))
    return t1 - 0.5 * t2


def posterior_predictive(stack, kind="regression", sigma_sets=None, probs=DEFAULT_PROBS, targets=None):
    """The definitions above on ``stack`` [S, N, outputs], the samples' post-output predictions (float64 numpy on the host): means
    with ``sigma_sets`` [S, targets] or [S] (``"regression"``), or means followed by as many sigmas (``"regression-error"``).
    Returns a dict with ``n_samples``, ``n_rows``, ``probs`` [Q], ``quantiles`` [Q, N, T], ``mean`` [N, T] and, with ``targets``
    [N, T], ``crps_i`` [N, T] and ``crps`` [T], its mean over the rows.  ``ValueError`` on NaN or infinite values, on bad shapes, on
    a sigma that is not positive and finite and on probabilities out of range."""
    who = "posterior_predictive"
    if kind not in KINDS:
        raise ValueError("%s: kind %r; one of %s" % (who, kind, ", ".join(KINDS)))
    pr = check_probs(probs, who)
    y = np.asarray(stack, dtype=np.float64)
    if y.ndim != 3 or 0 in y.shape:
        raise ValueError("%s: stack must be a non-empty [samples, rows, outputs] array, got shape %s" % (who, y.shape))
    if y.shape[0] > MAX_SAMPLES:
        raise ValueError("%s: %d samples, at most %d are supported" % (who, y.shape[0], MAX_SAMPLES))
    if not np.all(np.isfinite(y)):
        raise ValueError("%s: stack holds NaN or infinite values" % who)
    n_samples, n_rows = y.shape[:2]
    if kind == "regression-error":
        if y.shape[2] % 2:
            raise ValueError("%s: kind \"regression-error\" takes means followed by as many sigmas, and %d outputs is odd" % (who, y.shape[2]))
        if sigma_sets is not None:
            raise ValueError("%s: kind \"regression-error\" predicts its sigma: sigma_sets goes with kind \"regression\" only" % who)
        n_targets = y.shape[2] // 2
        mu, sig = y[:, :, :n_targets], y[:, :, n_targets:]
        if not np.all(sig > 0):
            raise ValueError("%s: every predicted sigma must be positive and finite" % who)
    else:
        n_targets = y.shape[2]
        mu = y
        sig = np.broadcast_to(sigma_matrix(sigma_sets, n_samples, n_targets, who)[:, None, :], y.shape)
    t = None if targets is None else target_matrix(targets, n_rows, n_targets, who)
    mu2 = np.ascontiguousarray(mu.reshape(n_samples, -1))
    sig2 = np.ascontiguousarray(sig.reshape(n_samples, -1))
    res = dict(n_samples=int(n_samples), n_rows=int(n_rows), probs=pr)
    res["quantiles"] = np.array([_quantile(mu2, sig2, p) for p in pr]).reshape((len(pr), n_rows, n_targets))
    res["mean"] = (mu2[0] + np.sum(mu2 - mu2[0], axis=0) / n_samples).reshape(n_rows, n_targets)
    if t is not None:
        res["crps_i"] = _crps(mu2, sig2, t.reshape(-1)).reshape(n_rows, n_targets)
        res["crps"] = np.sum(res["crps_i"], axis=0) / n_rows
    return res


def get_posterior_predictive(pkl_file, features=None, labels=None, probs=DEFAULT_PROBS, crps=True):
    """The posterior predictive distribution of a checkpoint's stored samples: on its own test table (default), on its training
    table (``features="train"``), or on ``features`` (with ``labels``, its targets, for the CRPS).  The kind follows the model's
    estimation mode - ``"regression"`` (sigma per sample from the samples' ``error_prm``) or ``"regression-error"`` (sigma predicted
    per row); predictions as ``get_posterior_est`` computes them (per-sample slopes, the last sample's slopes left installed).
    Returns ``posterior_predictive``'s dict; ``crps=False``, or a feature matrix without labels, leaves ``crps_i`` and ``crps`` out
    (the targets are then never sent).  The table is taken in row blocks whose device stack fits the budget of
    ``get_posterior_hpd``, on one predictor; a cell's result does not depend on the blocks.  ``ValueError`` before any device call:
    no stored samples or more than 16384, an empty table, classification, ``"custom"`` and the count likelihoods' estimation
    modes, a ``"regression"`` checkpoint without ``error_prm``, an odd number of outputs under ``"regression-error"``, targets of
    another shape or not finite, probabilities out of range or more than 16 of them, an output callable without a device kind."""
    who = "get_posterior_predictive"
    pr = check_probs(probs, who)
    model, samples, mode, n_out = open_checkpoint(load_obj(pkl_file), who, KINDS,
                                                  "%s are served; classification, \"custom\" and the count likelihoods are not" % ", ".join(KINDS))
    if len(samples) > MAX_SAMPLES:
        raise ValueError("%s: %d samples, at most %d are supported" % (who, len(samples), MAX_SAMPLES))
    want_crps = bool(crps) and not (labels is None and features is not None and not isinstance(features, str))
    x, y = choose_table(model, features, labels, who, need_labels=want_crps)
    sigma = None
    if mode == "regression":
        n_targets, sigma = n_out, sample_sigmas(samples, n_out, who)
    else:
        if n_out % 2:
            raise ValueError("%s: \"regression-error\" predicts a mean and a sigma per target, and %d outputs is odd" % (who, n_out))
        n_targets = n_out // 2
    t = target_matrix(y, len(x), n_targets, who) if want_crps else None
    out_fn = model._output_act_fun
    if out_fn is not None and output_kind(out_fn) is None:            # (the predictor refuses it too; here no context has been built)
        raise ValueError("%s: the model's output function is a custom callable, which has no device kind; build the stack and "
                         "call posterior_predictive" % who)
    with open_predictor(model, samples, x.shape[1]) as pred:
        got = pred.predictive(x, mode, probs=pr, sigma_sets=sigma, targets=t, block_rows=stack_rows(len(samples), n_out), who=who)
    quantiles = got["quantiles"] if len(pr) else np.zeros((0, len(x), n_targets))
    res = dict(n_samples=len(samples), n_rows=len(x), probs=pr, quantiles=quantiles, mean=got["mean"])
    if t is not None:
        # (summed here as posterior_predictive sums it: the same bits whatever the row blocks were)
        res.update(crps_i=got["crps_i"], crps=np.sum(got["crps_i"], axis=0) / len(x))
    return res
