"""The gradient of the log posterior with respect to the weights, and a deterministic MAP warm start for the sampler:
``loglik_grad``, ``log_posterior_grad``, ``map_estimate``.

np_bnn starts a chain from N(0, 0.1) weights, or from a network trained in another framework and passed in as ``init_weights``
(``get_weights_from_tensorflow_model``, np_bnn/BNN_lib.py:601-624).  Here the data are already resident on the device:
``npbnn_loglik_grad`` returns the log-likelihood and its gradient over all packed weights from the resident matrix, and
``map_estimate`` climbs the log posterior with it, so that

    import npbnn_amd as bn
    bn.map_estimate(bnn)
    mcmc = bn.MCMC(bnn)

starts the chain at a maximum-a-posteriori estimate.  ``loglik_grad`` below is the same definition in float64 numpy on host
arrays: the package's host definition of the entry, which the tests hold the device to."""
import numpy as np

from . import _capi as capi
from .layers import output_kind
from .likelihoods import (calc_likelihood, calc_likelihood_regression, calc_likelihood_regression_error, likelihood_kind)
from .model import CAUCHY, LAPLACE, NORMAL, UNIFORM, data_transform_obj

_HALF_LOG_2PI = 0.5 * np.log(2 * np.pi)
_KINDS = {capi.LIK_CATEGORICAL: "calc_likelihood", capi.LIK_GAUSS: "calc_likelihood_regression",
          capi.LIK_GAUSS_PRED_SIGMA: "calc_likelihood_regression_error"}
_MODE_LIK = {"classification": calc_likelihood, "regression": calc_likelihood_regression,
             "regression-error": calc_likelihood_regression_error}


def _activate(z, kind, slope):
    """(a(z), a'(z)) as the forward pass computes them: the derivative on the branch the activation takes"""
    if kind == capi.ACT_RELU:
        return np.maximum(z, 0.0), (z > 0).astype(np.float64)
    if kind == capi.ACT_LEAKY:
        return np.where(z < 0, slope * z, z), np.where(z < 0, slope, 1.0)
    if kind == capi.ACT_SWISH:
        s = 1.0 / (1.0 + np.exp(-z))
        return z * s, s * (1.0 + z * (1.0 - s))
    t = 1.0 - 2.0 / (np.exp(2.0 * z) + 1.0)
    return t, 1.0 - t * t


def _lik_kind(lik):
    kind = lik if isinstance(lik, (int, np.integer)) else likelihood_kind(lik)
    if kind not in _KINDS:
        name = getattr(lik, "__name__", repr(lik))
        raise ValueError("loglik_grad: no gradient for the likelihood %s (categorical, Gaussian and predicted-sigma only)" % name)
    return int(kind)


def loglik_grad(data, labels, weights, actFun, lik, sigma=None, lik_temp=1.0, class_weight=None, instance_weight=None,
                col_override=None, final_activation=False):
    """``(eval dict, [gradient per layer])`` in float64 numpy: what ``HipContext.loglik_grad`` returns for the same table.

    ``lik``: ``calc_likelihood`` (labels: class indices), ``calc_likelihood_regression`` (``sigma`` per target column is
    required) or ``calc_likelihood_regression_error``, or their ``LIK_*`` kinds.  With ``z`` the last layer's values of row i,

        log-likelihood = sum_i l_i,    gradient = sum_i d l_i / d W,    packed like ``weights`` (bias in column 0)

    categorical ``l_i = lik_temp w_i log softmax(z)[y_i]`` with ``w_i`` the instance weight times the class weight of ``y_i``;
    Gaussian ``l_i = lik_temp sum_t norm.logpdf(y_it, z_t, sigma_t)``; predicted sigma ``mu = z[:k]``, ``s = softplus(z[k:])``.
    A column ``col_override`` replaces by the constant ``c_j`` receives ``c_j`` times the first layer's bias sum: the derivative
    of what the forward pass computes.  The slopes of ``actFun`` are constants; their derivative is not returned."""
    kind = _lik_kind(lik)
    x = np.array(data, dtype=np.float64, copy=True)
    n, f = x.shape
    off = np.zeros(f, dtype=bool)
    if col_override is not None:
        co = np.asarray(col_override, dtype=np.float64)
        off = ~np.isnan(co)
        x[:, off] = co[off]
    weights = [np.asarray(w, dtype=np.float64) for w in weights]
    act_kind = actFun.device_kind()
    slopes = actFun.device_slopes(len(weights) if final_activation else len(weights) - 1)
    if slopes is not None and len(slopes) < len(weights):
        slopes = np.concatenate([slopes, np.zeros(len(weights) - len(slopes))])
    inputs, factors, h = [], [], x
    for l, w in enumerate(weights):
        inputs.append(h)
        bias = w.shape[1] == h.shape[1] + 1
        z = h @ w[:, 1:].T + w[:, 0] if bias else h @ w.T
        if l < len(weights) - 1 or final_activation:
            h, d = _activate(z, act_kind, 0.0 if slopes is None else slopes[l])
        else:
            h, d = z, np.ones_like(z)
        factors.append(d)
    z = h
    out = dict(loglik=0.0, sigma=np.zeros(0), sum_r=np.zeros(0), sum_r2=np.zeros(0), n_rows=n, confusion=None)
    if kind == capi.LIK_CATEGORICAL:
        y = np.asarray(labels).astype(int).ravel()
        m = z.max(axis=1, keepdims=True)
        logp = z - m - np.log(np.exp(z - m).sum(axis=1, keepdims=True))
        wgt = np.ones(n)
        if instance_weight is not None:
            wgt = wgt * np.asarray(instance_weight, dtype=np.float64)
        if class_weight is not None and len(class_weight):
            wgt = wgt * np.asarray(class_weight, dtype=np.float64)[y]
        out["loglik"] = lik_temp * np.sum(wgt * logp[np.arange(n), y])
        g = -np.exp(logp)
        g[np.arange(n), y] += 1.0
        g *= wgt[:, None]
    else:
        t = np.asarray(labels, dtype=np.float64).reshape(n, -1)
        k = t.shape[1]
        if kind == capi.LIK_GAUSS:
            if sigma is None:
                raise ValueError("loglik_grad: calc_likelihood_regression needs sigma (the empirical sigma has no gradient here)")
            s = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (k,))
            res = t - z
            out.update(sigma=np.array(s), sum_r=res.sum(axis=0), sum_r2=(res * res).sum(axis=0))
            out["loglik"] = lik_temp * np.sum(-n * (_HALF_LOG_2PI + np.log(s)) - out["sum_r2"] / (2.0 * s * s))
            g = res / (s * s)
        else:
            if z.shape[1] != 2 * k:
                raise ValueError("loglik_grad: calc_likelihood_regression_error needs 2 k outputs, got %d for k = %d" % (z.shape[1], k))
            mu, zs = z[:, :k], z[:, k:]
            s = np.logaddexp(0.0, zs)
            q = (t - mu) / s
            out["loglik"] = lik_temp * np.sum(-_HALF_LOG_2PI - np.log(s) - 0.5 * q * q)
            g = np.concatenate([q / s, (q * q - 1.0) / s / (1.0 + np.exp(-zs))], axis=1)
    delta = lik_temp * g * factors[-1]
    grads = [None] * len(weights)
    for l in range(len(weights) - 1, -1, -1):
        w, h = weights[l], inputs[l]
        bias = w.shape[1] == h.shape[1] + 1
        gw = delta.T @ h
        if l == 0 and off.any():
            gw[:, off] = np.outer(delta.sum(axis=0), co[off])
        grads[l] = np.concatenate([delta.sum(axis=0)[:, None], gw], axis=1) if bias else gw
        if l > 0:
            delta = (delta @ (w[:, 1:] if bias else w)) * factors[l - 1]
    return out, grads


def prior_grad(bnn, weights):
    """The gradient of the weight prior's log density per layer, on ``bnn._prior_scale`` (scalars, or arrays under ``hyper_p``):
    normal ``-w / s^2``, Cauchy ``-2 w / (s^2 + w^2)``, Laplace ``-sign(w) / s``, uniform 0."""
    kind = bnn._prior if bnn._prior in (UNIFORM, NORMAL, CAUCHY, LAPLACE) else NORMAL
    res = []
    for w, scale in zip(weights, bnn._prior_scale):
        w = np.asarray(w, dtype=np.float64)
        s = np.asarray(scale, dtype=np.float64)
        if kind == UNIFORM:
            g = np.zeros_like(w)
        elif kind == CAUCHY:
            g = -2.0 * w / (s * s + w * w)
        elif kind == LAPLACE:
            g = -np.sign(w) / s * np.ones_like(w)
        else:
            g = -w / (s * s)
        res.append(np.broadcast_to(g, w.shape).copy())
    return res


def _refuse(bnn, likelihood_f, who):
    """the likelihood callable of the model's mode (or the one given), after the refusals the two entries share"""
    mode = bnn._estimation_mode
    if mode == "custom" and likelihood_f is None:
        raise ValueError("%s: estimation_mode 'custom' has no likelihood whose gradient the device returns" % who)
    lik = _MODE_LIK[mode] if likelihood_f is None else likelihood_f
    if likelihood_kind(lik) not in _KINDS:
        raise ValueError("%s: no gradient for the likelihood %s (calc_likelihood, calc_likelihood_regression and "
                         "calc_likelihood_regression_error only)" % (who, getattr(lik, "__name__", repr(lik))))
    if output_kind(bnn._output_act_fun) is None:
        raise ValueError("%s: a custom output callable has no device kind and cannot be differentiated" % who)
    return lik


def _loglik_grad(backend, weights, **kw):
    """The device seam: the model's resident backend returns the log-likelihood and its gradient per layer."""
    return backend.loglik_grad(weights, **kw)


def _masked(bnn, layers):
    mask = bnn._mask
    return layers if mask is None else [g * m for g, m in zip(layers, mask)]


def log_posterior_grad(bnn, weights=None, likelihood_f=None, lik_temp=1.0):
    """``(log_lik, log_prior, [gradient per layer], error_prm)`` of the model at ``weights`` (default: its own), as ``MCMC``
    scores a state: the likelihood on the first layer times the weight indicators and on the feature indicators' column override,
    with ``bnn._error_prm`` as sigma in regression; the prior on the weights themselves (``calc_prior``).  The gradient is the
    likelihood's (the device entry's, times the indicators on the first layer) plus the prior's closed form, times ``bnn._mask``:
    a masked weight stays where it is.  The activation's slopes are constants."""
    return _posterior_grad(bnn, weights, likelihood_f, lik_temp)[:4]


def _posterior_grad(bnn, weights, likelihood_f, lik_temp):
    """log_posterior_grad's tuple, then the entry's eval dict"""
    from .sampler import get_backend
    lik = _refuse(bnn, likelihood_f, "log_posterior_grad")
    w = [np.asarray(x, dtype=np.float64) for x in (bnn._w_layers if weights is None else weights)]
    ind = np.asarray(bnn._indicators, dtype=np.float64)
    fw = [w[0] * ind] + w[1:]
    override = None
    if bnn._feature_indicators is not None:
        override = data_transform_obj(bnn._feature_indicators, bnn._feature_means).column_override()
    sigma = None
    if likelihood_kind(lik) == capi.LIK_GAUSS:
        sigma = np.ones(bnn._labels.shape[1]) * np.asarray(bnn._error_prm, dtype=np.float64)
    backend = get_backend(bnn, lik)
    r, g = _loglik_grad(backend, fw, slopes=bnn._act_fun.device_slopes(bnn._n_layers - 1), col_override=override, lik_temp=lik_temp,
                        sigma=sigma)
    g = [np.asarray(x, dtype=np.float64) for x in g]
    g[0] = g[0] * ind
    grad = _masked(bnn, [a + b for a, b in zip(g, prior_grad(bnn, w))])
    return float(r["loglik"]), float(bnn.calc_prior(w=w)), grad, (r["sigma"] if sigma is not None else bnn._error_prm), r


def map_estimate(bnn, n_iter=500, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, tol=0.0, update_error_prm=True, apply=True, verbose=0,
                 likelihood_f=None, lik_temp=1.0):
    """A maximum-a-posteriori estimate of the weights by plain Adam ascent on the log posterior, from the model's current
    weights: deterministic, no random numbers.  Every step evaluates ``log_posterior_grad`` on the device, moves the weights by
    ``lr * m / (sqrt(v) + eps)`` (bias-corrected moments, ``beta1``, ``beta2``), clips them to ``+-bnn._w_bound`` and re-applies
    ``bnn._mask``.  In ``"regression"`` mode with ``update_error_prm`` each step first sets sigma to its conditional maximum
    ``sqrt(sum_r2 / n)`` from the entry's own residual moments.  It stops early when the largest weight change falls below
    ``tol``, and raises ``FloatingPointError``, naming the step, when a gradient is not finite.

    Returns ``{'weights', 'error_prm', 'log_posterior', 'log_lik', 'grad_norm', 'n_iter'}``: ``weights`` and ``error_prm`` are
    the BEST iterate seen (by log posterior), not the last; the three traces hold a value per evaluated iterate (the start, then
    one per step); ``n_iter`` the steps taken.  With ``apply`` the model is left there (``reset_weights``, in regression
    ``reset_error_prm``), so that ``bn.MCMC(bnn)`` starts from it.

    Trainable activation slopes are held at their current values; ``"custom"`` mode, the count likelihoods and custom output
    callables are refused with ``ValueError``."""
    _refuse(bnn, likelihood_f, "map_estimate")
    regression = bnn._estimation_mode == "regression"
    w = [np.array(x, dtype=np.float64, copy=True) for x in _masked(bnn, bnn._w_layers)]
    saved_sigma = bnn._error_prm
    m = [np.zeros_like(x) for x in w]
    v = [np.zeros_like(x) for x in w]
    trace = dict(log_posterior=[], log_lik=[], grad_norm=[])
    best = None
    t = 0
    try:
        while True:
            if regression and update_error_prm:
                r = _posterior_grad(bnn, w, likelihood_f, lik_temp)[4]
                bnn.reset_error_prm(np.sqrt(np.asarray(r["sum_r2"], dtype=np.float64) / r["n_rows"]))
            ll, lp, g, sigma, _ = _posterior_grad(bnn, w, likelihood_f, lik_temp)
            norm = float(np.sqrt(sum(np.sum(x * x) for x in g)))
            if not np.isfinite(norm) or not np.isfinite(ll + lp):
                raise FloatingPointError("map_estimate: the log posterior or its gradient is not finite at step %d" % t)
            trace["log_posterior"].append(ll + lp)
            trace["log_lik"].append(ll)
            trace["grad_norm"].append(norm)
            if best is None or ll + lp > best[0]:
                best = (ll + lp, [x.copy() for x in w], np.array(sigma, dtype=np.float64, copy=True) if regression else sigma)
            if verbose and t % verbose == 0:
                print("map_estimate: step %d  log posterior %.6f  log likelihood %.6f  |gradient| %.3e" % (t, ll + lp, ll, norm))
            if t >= n_iter:
                break
            change = 0.0
            for i in range(len(w)):
                m[i] = beta1 * m[i] + (1.0 - beta1) * g[i]
                v[i] = beta2 * v[i] + (1.0 - beta2) * g[i] * g[i]
                step = lr * (m[i] / (1.0 - beta1 ** (t + 1))) / (np.sqrt(v[i] / (1.0 - beta2 ** (t + 1))) + eps)
                new = np.clip(w[i] + step, -bnn._w_bound, bnn._w_bound)
                if bnn._mask is not None:
                    new = new * bnn._mask[i]
                change = max(change, float(np.max(np.abs(new - w[i]))) if new.size else 0.0)
                w[i] = new
            t += 1
            if change < tol:
                n_iter = t                       # (the iterate just made is scored, then the run ends)
    finally:
        bnn.reset_error_prm(saved_sigma)
    res = dict(weights=best[1], error_prm=best[2], log_posterior=np.array(trace["log_posterior"]), log_lik=np.array(trace["log_lik"]),
               grad_norm=np.array(trace["grad_norm"]), n_iter=t)
    if apply:
        bnn.reset_weights([x.copy() for x in best[1]])
        if regression:
            bnn.reset_error_prm(np.array(best[2], dtype=np.float64, copy=True))
    return res
