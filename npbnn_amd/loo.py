"""Pareto-smoothed importance-sampling leave-one-out cross-validation of stored posterior samples: ``posterior_loo``,
``get_posterior_loo``, ``loo_compare`` (Vehtari, Gelman, Gabry 2017; Vehtari et al. 2024; the reference has no such function).

With ``ll[s, i]`` the log-likelihood of row ``i`` under stored sample ``s`` (``npbnn_amd.lppd`` has the terms), per row:

    x_s   = -ll_s - max_t(-ll_t)                               (log importance ratios, the largest 0)
    M     = ceil(min(S / 5, 3 sqrt(S)));  cut = max((M + 1)-th largest x, log(DBL_MIN));  ecut = exp(cut)
    tail  = the x_s > cut (strictly), ascending x_(1) <= ... <= x_(n); n may be below M under ties, or 0
    n <= 4:  k = +inf, every log weight lw_s = x_s (plain importance sampling)
    n >  4:  t_j = exp(x_(j)) - ecut;  (k, sigma) = gpdfit(t);  the j-th smallest tail value gets
             lw = min(log(sigma * expm1(-k * log1p(-p_j)) / k + ecut), 0),  p_j = (j - 0.5) / n;  lw_s = x_s outside the tail
    elpd_loo_i = logsumexp_s(lw_s + ll_s) - logsumexp_s(lw_s)
    lppd_i     = logsumexp_s(ll_s) - log S;   p_loo_i = lppd_i - elpd_loo_i;   pareto_k_i = k

``gpdfit`` is Zhang and Stephens (2009) with the weakly informative prior of loo / ArviZ (``_gpdfit``).  Totals:
``elpd_loo = sum_i elpd_loo_i``, ``se_elpd_loo = sqrt(N var_i elpd_loo_i)`` (ddof 1; 0 for one row), ``p_loo``, ``looic = -2 elpd_loo``,
``k_threshold = min(1 - 1 / log10(S), 0.7)`` and ``n_bad_k``, the rows whose ``k`` lies above it: their estimate is not to be trusted
(the importance ratios' tail is too heavy for S samples; ``+inf`` marks a tail of four values or fewer, which is not fitted at all).
``S <= 20`` leaves every tail that short: the estimate is then plain importance sampling, ``-log mean_s exp(-ll_s)``.

``posterior_loo`` is that definition on a host ``[S, N]`` array.  ``get_posterior_loo`` replays a checkpoint's stored samples on the
device, keeps ``ll`` there as a float64 matrix and runs one column kernel over it (``npbnn_predict_sets_loo``); a table whose matrix
is over the budget of ``get_posterior_hpd``'s stack goes block by block of rows.  Not here: the smoothed weights themselves, the
relative-efficiency correction of ``M``, moment matching for rows with a large ``k``."""
import numpy as np

from . import _capi as capi
from .files import load_obj
from .hpd import MAX_SAMPLES, stack_rows
from .stored import choose_table, class_labels, open_checkpoint, open_predictor, sample_sigmas, target_matrix

POINT_KEYS = ("elpd_loo_i", "lppd_i", "p_loo_i", "pareto_k")
MIN_TAIL = 4                     # a tail of this many values or fewer is not fitted
_LOG_TINY = np.log(np.finfo(np.float64).tiny)
_CHUNK = 2048                    # columns fitted at once


def tail_length(n_samples):
    """M: the most values the tail of a column of ``n_samples`` ratios holds."""
    return int(np.ceil(min(n_samples / 5.0, 3.0 * np.sqrt(n_samples))))


def _gpdfit(t):
    """(k, sigma) [K] of the generalized Pareto fit to each column of ``t`` [n, K], ascending along axis 0."""
    n = t.shape[0]
    m = 30 + int(np.floor(np.sqrt(n)))
    q = np.arange(1, m + 1, dtype=np.float64)
    bs = (1.0 - np.sqrt(m / (q - 0.5)))[:, None] / (3.0 * t[int(np.floor(n / 4.0 + 0.5)) - 1])[None] + (1.0 / t[n - 1])[None]   # [m, K]
    ks = np.sum(np.log1p(-bs[:, None, :] * t[None]), axis=1) / n
    big_l = n * (np.log(-bs / ks) - ks - 1.0)
    w = 1.0 / np.sum(np.exp(big_l[None, :, :] - big_l[:, None, :]), axis=1)          # w_q = 1 / sum_r exp(L_r - L_q)
    w = np.where(w >= 10.0 * np.finfo(np.float64).eps, w, 0.0)
    w = w / np.sum(w, axis=0)
    b = np.sum(bs * w, axis=0)
    kp = np.sum(np.log1p(-b[None] * t), axis=0) / n
    return (n * kp + 5.0) / (n + 10.0), -kp / b


def _logsumexp(a):
    top = np.max(a, axis=0)
    # (summed along the contiguous axis: numpy adds pairwise there, and row by row - S roundings deep - along the other)
    return top + np.log(np.sum(np.ascontiguousarray(np.exp(a - top).T), axis=1))


def _pointwise(ll):
    """(elpd_loo_i, lppd_i, k) [N] of ``ll`` [S, N], finite."""
    n_samples, n_rows = ll.shape
    ll = np.sort(ll, axis=0)                                   # ascending: x descending, the tail in front
    neg = -ll
    x = neg - np.max(neg, axis=0)
    m = tail_length(n_samples)
    cut = np.maximum(x[m], _LOG_TINY)
    ecut = np.exp(cut)
    n = np.sum(x[:m] > cut, axis=0)
    lw = x.copy()
    k = np.full(n_rows, np.inf)
    with np.errstate(all="ignore"):
        for nn in np.unique(n[n > MIN_TAIL]):
            cols_all = np.nonzero(n == nn)[0]
            l1 = np.log1p(-((np.arange(1, nn + 1) - 0.5) / nn))[:, None]
            for at in range(0, len(cols_all), _CHUNK):
                cols = cols_all[at:at + _CHUNK]
                kk, sigma = _gpdfit(np.exp(x[:nn][::-1][:, cols]) - ecut[cols])
                quot = np.where(kk == 0.0, -sigma * l1, sigma * np.expm1(-kk * l1) / kk)
                lw[:nn, cols] = np.minimum(np.log(quot + ecut[cols]), 0.0)[::-1]
                k[cols] = kk
    return _logsumexp(lw + ll) - _logsumexp(lw), _logsumexp(ll) - np.log(n_samples), k


def k_threshold(n_samples):
    return min(1.0 - 1.0 / np.log10(n_samples), 0.7)


def loo_totals(elpd_i, lppd_i, k, n_samples):
    """The result dict from the pointwise arrays [N]: the totals, and ``elpd_loo_i``, ``lppd_i``, ``p_loo_i``, ``pareto_k``."""
    elpd_i, lppd_i, k = (np.asarray(a, dtype=np.float64) for a in (elpd_i, lppd_i, k))
    n_rows = len(elpd_i)
    p_i = lppd_i - elpd_i
    elpd = float(np.sum(elpd_i))
    thr = k_threshold(n_samples)
    return dict(elpd_loo=elpd, se_elpd_loo=float(np.sqrt(n_rows * np.var(elpd_i, ddof=1))) if n_rows > 1 else 0.0, p_loo=float(np.sum(p_i)),
                looic=-2.0 * elpd, lppd=float(np.sum(lppd_i)), k_threshold=thr, n_bad_k=int(np.sum(k > thr)), n_samples=int(n_samples),
                n_rows=int(n_rows), elpd_loo_i=elpd_i, lppd_i=lppd_i, p_loo_i=p_i, pareto_k=k)


def check_samples(n_samples, who):
    if n_samples < 2:
        raise ValueError("%s: %d samples, leave-one-out importance sampling needs at least 2" % (who, n_samples))
    if n_samples > MAX_SAMPLES:
        raise ValueError("%s: %d samples, at most %d are supported" % (who, n_samples, MAX_SAMPLES))


def posterior_loo(log_lik):
    """The definitions above on ``log_lik`` [S, N] (float64 numpy on the host), 2 <= S <= 16384.  Returns a dict: ``elpd_loo``,
    ``se_elpd_loo``, ``p_loo``, ``looic``, ``lppd``, ``k_threshold``, ``n_bad_k``, ``n_samples``, ``n_rows`` and the pointwise
    ``elpd_loo_i``, ``lppd_i``, ``p_loo_i``, ``pareto_k`` [N].  ``ValueError`` on NaN or infinite values."""
    who = "posterior_loo"
    ll = np.asarray(log_lik, dtype=np.float64)
    if ll.ndim != 2 or ll.shape[1] < 1:
        raise ValueError("%s: log_lik must be a non-empty [samples, rows] array, got shape %s" % (who, ll.shape))
    check_samples(ll.shape[0], who)
    if not np.all(np.isfinite(ll)):
        raise ValueError("%s: log_lik holds NaN or infinite values" % who)
    return loo_totals(*_pointwise(ll), ll.shape[0])


def loo_compare(a, b):
    """Two pointwise results (``posterior_loo``, ``get_posterior_loo(pointwise=True)``) over the same rows: a dict with
    ``elpd_diff = sum_i (a_i - b_i)`` (positive: ``a`` predicts better), ``se_diff = sqrt(N var_i (a_i - b_i))`` (ddof 1; 0 for
    one row) and ``n_rows``."""
    who = "loo_compare"
    for r in (a, b):
        if not isinstance(r, dict) or r.get("elpd_loo_i") is None:
            raise ValueError("%s: a result without elpd_loo_i (ask for pointwise=True)" % who)
    da, db = np.asarray(a["elpd_loo_i"], dtype=np.float64), np.asarray(b["elpd_loo_i"], dtype=np.float64)
    if da.ndim != 1 or da.shape != db.shape or len(da) == 0:
        raise ValueError("%s: the results cover %s and %s rows; they must be over the same rows" % (who, da.shape, db.shape))
    d = da - db
    return dict(elpd_diff=float(np.sum(d)), se_diff=float(np.sqrt(len(d) * np.var(d, ddof=1))) if len(d) > 1 else 0.0, n_rows=len(d))


def get_posterior_loo(pkl_file, features=None, labels=None, pointwise=False, log_lik=False):
    """PSIS-LOO of a checkpoint's stored samples: on its own test table (default), on its training table (``features="train"``,
    the table the estimate is meant for), or on ``features`` with ``labels`` given.  Classification (labels are class indices) or
    Gaussian regression (targets; sigma per sample from the samples' ``error_prm``); predictions as ``get_posterior_lppd`` computes
    them.  Returns ``posterior_loo``'s dict with ``log_lik_sample`` [S] beside it - the pointwise arrays only when ``pointwise``, and
    with ``log_lik`` the matrix ``ll`` [S, N] itself under that key.  ``ValueError`` before any device call: fewer than 2 stored
    samples or more than 16384, an empty table, labels that are not class indices, a regression checkpoint without ``error_prm``,
    an estimation mode other than classification or regression."""
    who = "get_posterior_loo"
    model, samples, mode, n_out = open_checkpoint(load_obj(pkl_file), who, ("classification", "regression"),
                                                  "classification and Gaussian regression with a sigma per sample are served; "
                                                  "predicted-sigma regression and the count likelihoods are not")
    check_samples(len(samples), who)
    x, y = choose_table(model, features, labels, who, need_labels=True)
    if mode == "classification":
        kind, y, sigma = capi.LIK_CATEGORICAL, class_labels(y, len(x), n_out, who), None
    else:
        kind, y, sigma = capi.LIK_GAUSS, target_matrix(y, len(x), n_out, who), sample_sigmas(samples, n_out, who)
    with open_predictor(model, samples, x.shape[1]) as pred:
        res = pred.loo(x, y, kind, sigma_sets=sigma, log_lik=log_lik, block_rows=stack_rows(len(samples), 2))
    if not pointwise:
        for k in POINT_KEYS:
            res.pop(k, None)
    if not log_lik:
        res.pop("log_lik", None)
    return res
