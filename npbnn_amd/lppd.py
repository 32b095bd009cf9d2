"""Log pointwise predictive density and WAIC of stored posterior samples: ``posterior_lppd``, ``get_posterior_lppd``.

The reference logs accuracy and MSE only; the per-row terms here are its own likelihoods' summands, unweighted and untempered:
``log(prediction[i, label_i])`` (calc_likelihood, np_bnn/BNN_lib.py:121) and ``norm.logpdf(y, mu, sigma)`` summed over the target
columns (calc_likelihood_regression, :131).  With ``ll[s, i]`` the log-likelihood of row ``i`` under stored sample ``s``:

    lppd_i    = logsumexp_s ll[s, i] - log S        mean_ll_i = mean_s ll[s, i]
    p_waic_i  = var_s ll[s, i], ddof 1 (0 for S = 1)    log_lik_sample[s] = sum_i ll[s, i]
    lppd = sum_i lppd_i,  p_waic = sum_i p_waic_i,  elpd_waic = lppd - p_waic,  waic = -2 elpd_waic

``posterior_lppd`` is that definition on a host ``[S, N]`` array.  ``get_posterior_lppd`` replays a checkpoint's stored samples on
the device and folds every group of samples into per-row accumulators there (``npbnn_predict_sets_lppd``): the ``[S, N]`` matrix
is never built and only the results come back.  There is deliberately no function that returns the matrix."""
import numpy as np

from . import _capi as capi
from .files import load_obj
from .stored import choose_table, class_labels, open_checkpoint, open_predictor, sample_sigmas, target_matrix

_HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def posterior_lppd(log_lik):
    """The definitions above on ``log_lik`` [S, N] (float64 numpy on the host).  Returns a dict: ``lppd``, ``mean_log_lik``,
    ``p_waic``, ``elpd_waic``, ``waic``, ``n_samples``, ``n_rows``, ``log_lik_sample`` [S], and the pointwise ``lppd_i``,
    ``mean_log_lik_i``, ``p_waic_i`` [N]."""
    ll = np.asarray(log_lik, dtype=np.float64)
    if ll.ndim != 2 or ll.shape[0] < 1 or ll.shape[1] < 1:
        raise ValueError("posterior_lppd: log_lik must be a non-empty [samples, rows] array, got shape %s" % (ll.shape,))
    if np.any(np.isnan(ll)):
        raise ValueError("posterior_lppd: log_lik holds NaN")
    n_samples, n_rows = ll.shape
    top = np.max(ll, axis=0)
    shift = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide="ignore"):
        lppd_i = shift + np.log(np.sum(np.exp(ll - shift), axis=0)) - np.log(n_samples)
    mean_i = np.mean(ll, axis=0)
    p_waic_i = np.var(ll, axis=0, ddof=1) if n_samples > 1 else np.zeros(n_rows)
    return _finish(dict(lppd=float(np.sum(lppd_i)), mean_log_lik=float(np.sum(mean_i)), p_waic=float(np.sum(p_waic_i)),
                        log_lik_sample=np.sum(ll, axis=1), lppd_i=lppd_i, mean_log_lik_i=mean_i, p_waic_i=p_waic_i), n_samples, n_rows)


def _finish(res, n_samples, n_rows):
    res["elpd_waic"] = res["lppd"] - res["p_waic"]
    res["waic"] = -2.0 * res["elpd_waic"]
    res["n_samples"], res["n_rows"] = int(n_samples), int(n_rows)
    return res


def log_lik_of_stack(stack, labels, lik_kind, sigma_sets=None):
    """``ll`` [S, N] from a host stack of predictions [S, N, outputs] (the route of a custom output callable): class
    probabilities against class indices, or means against targets with ``sigma_sets`` [S, targets]."""
    y = np.asarray(stack, dtype=np.float64)
    if lik_kind == capi.LIK_CATEGORICAL:
        lab = np.asarray(labels, dtype=np.int64).ravel()
        with np.errstate(divide="ignore"):
            return np.log(y[:, np.arange(y.shape[1]), lab])
    t = np.asarray(labels, dtype=np.float64).reshape(y.shape[1], -1)
    sig = np.asarray(sigma_sets, dtype=np.float64).reshape(y.shape[0], 1, -1)
    return np.sum(-_HALF_LOG_2PI - np.log(sig) - 0.5 * ((t[None] - y) / sig) ** 2, axis=2)


def get_posterior_lppd(pkl_file, features=None, labels=None, pointwise=False):
    """lppd and WAIC of a checkpoint's stored samples: on its own test table (default), on its training table
    (``features="train"``), or on ``features`` with ``labels`` given.  Classification (labels are class indices) or Gaussian
    regression (targets; sigma per sample from the samples' ``error_prm``); predictions as ``get_posterior_est`` computes them
    (per-sample slopes, no data transform).  Returns ``posterior_lppd``'s dict - ``lppd``, ``mean_log_lik``, ``p_waic``,
    ``elpd_waic``, ``waic``, ``n_samples``, ``n_rows``, ``log_lik_sample`` [S] - with ``lppd_i``, ``mean_log_lik_i``, ``p_waic_i``
    [N] only when ``pointwise``.  WAIC is meant for the training table; on a held-out table ``lppd`` is the quantity to compare.
    ``ValueError`` before any device call: no stored samples, an empty table, labels that are not class indices, a
    regression checkpoint without ``error_prm``, an estimation mode other than classification or regression."""
    who = "get_posterior_lppd"
    model, samples, mode, n_out = open_checkpoint(load_obj(pkl_file), who, ("classification", "regression"),
                                                  "classification and Gaussian regression with a sigma per sample are served; "
                                                  "predicted-sigma regression and the count likelihoods are not")
    x, y = choose_table(model, features, labels, who, need_labels=True)
    if mode == "classification":
        kind, y, sigma = capi.LIK_CATEGORICAL, class_labels(y, len(x), n_out, who), None
    else:
        kind, y, sigma = capi.LIK_GAUSS, target_matrix(y, len(x), n_out, who), sample_sigmas(samples, n_out, who)
    with open_predictor(model, samples, x.shape[1]) as pred:
        res = pred.lppd(x, y, kind, sigma_sets=sigma, pointwise=pointwise)
    res = _finish(dict(res), len(samples), len(x))
    if not pointwise:
        for k in ("lppd_i", "mean_log_lik_i", "p_waic_i"):
            res.pop(k, None)
    return res
