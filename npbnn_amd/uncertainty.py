"""Posterior uncertainty decomposition of stored posterior samples: ``posterior_uncertainty``, ``get_posterior_uncertainty``.

The uncertainty of a prediction splits into the part the data cannot remove (aleatoric) and the part that comes from the posterior
over the weights (epistemic) - the reason to sample a Bayesian network at all.  The reference has no such function; the predictions
are its own (``RunPredict`` per stored sample with ``SoftMax``, ``RegressTransform`` or ``RegressTransformError``,
np_bnn/BNN_lib.py:166-182, 245-256).  Float64 throughout, ``S`` stored samples in sample order:

  classification, ``p_s`` a sample's class probabilities of a row:
    mean_prob = (1/S) sum_s p_s                     predictive_entropy_i = -sum_k m_k log m_k of mean_prob (nats; 0 log 0 = 0)
    expected_entropy_i = (1/S) sum_s H(p_s)         mutual_information_i = max(0, predictive - expected entropy), exactly 0 for S = 1
  regression, ``mu_s`` / ``sigma_s`` a sample's mean / standard deviation per target:
    mean = mean_s mu_s                              epistemic_var = (1/S) sum_s (mu_s - mean)^2 (ddof 0), exactly 0 for S = 1
    aleatoric_var = (1/S) sum_s sigma_s^2           total_var = epistemic_var + aleatoric_var  (the law of total variance)
  with sigma from the samples' ``error_prm`` (``"regression"``, the same for every row) or predicted per row
  (``"regression-error"``: the second half of the outputs).

``posterior_uncertainty`` is that definition on a host ``[S, N, outputs]`` array.  ``get_posterior_uncertainty`` replays a
checkpoint's stored samples on the device and folds every group of samples into per-row accumulators there
(``npbnn_predict_sets_uncertainty``): the stack is never built and only the results come back.  There is deliberately no function
that returns the stack."""
import numpy as np

from .files import load_obj
from .stored import choose_table, open_checkpoint, open_predictor, sample_sigmas, sigma_matrix

KINDS = ("classification", "regression", "regression-error")
CLASS_ROW_KEYS = ("predictive_entropy_i", "expected_entropy_i", "mutual_information_i")
REGRESSION_KEYS = ("mean", "epistemic_var", "aleatoric_var", "total_var")


def posterior_uncertainty(stack, kind="classification", sigma_sets=None):
    """The definitions above on ``stack`` [S, N, outputs], the samples' post-output predictions (float64 numpy on the host): class
    probabilities (``"classification"``), means with ``sigma_sets`` [S, targets] or [S] (``"regression"``), or means followed by as
    many sigmas (``"regression-error"``).  Returns a dict with ``n_samples``, ``n_rows`` and, for classification, ``mean_prob`` [N, C],
    ``predicted_class`` [N] (the first argmax of ``mean_prob``), ``predictive_entropy_i``, ``expected_entropy_i``,
    ``mutual_information_i`` [N] and their means over the rows ``predictive_entropy``, ``expected_entropy``, ``mutual_information``;
    for regression ``mean``, ``epistemic_var``, ``aleatoric_var``, ``total_var`` [N, T] and their means over the rows
    ``mean_avg``, ``epistemic_var_avg``, ``aleatoric_var_avg``, ``total_var_avg`` [T]."""
    who = "posterior_uncertainty"
    if kind not in KINDS:
        raise ValueError("%s: kind %r; one of %s" % (who, kind, ", ".join(KINDS)))
    y = np.asarray(stack, dtype=np.float64)
    if y.ndim != 3 or 0 in y.shape:
        raise ValueError("%s: stack must be a non-empty [samples, rows, outputs] array, got shape %s" % (who, y.shape))
    if np.any(np.isnan(y)):
        raise ValueError("%s: stack holds NaN" % who)
    n_samples, n_rows = y.shape[:2]
    res = dict(n_samples=int(n_samples), n_rows=int(n_rows))
    if kind == "classification":
        mean_prob = np.sum(y, axis=0) / n_samples
        with np.errstate(divide="ignore", invalid="ignore"):
            predictive = -np.sum(np.where(mean_prob > 0, mean_prob * np.log(mean_prob), 0.0), axis=1)
            expected = np.sum(-np.sum(np.where(y > 0, y * np.log(y), 0.0), axis=2), axis=0) / n_samples
        mutual = np.maximum(0.0, predictive - expected) if n_samples > 1 else np.zeros(n_rows)
        res.update(mean_prob=mean_prob, predicted_class=np.argmax(mean_prob, axis=1), predictive_entropy_i=predictive,
                   expected_entropy_i=expected, mutual_information_i=mutual)
        for k in CLASS_ROW_KEYS:
            res[k[:-2]] = float(np.mean(res[k]))
        return res
    if kind == "regression-error":
        if y.shape[2] % 2:
            raise ValueError("%s: kind \"regression-error\" takes means followed by as many sigmas, and %d outputs is odd" % (who, y.shape[2]))
        n_targets = y.shape[2] // 2
        mu, sig2 = y[:, :, :n_targets], y[:, :, n_targets:] ** 2
        aleatoric = np.sum(sig2, axis=0) / n_samples
    else:
        n_targets = y.shape[2]
        mu = y
        sig = sigma_matrix(sigma_sets, n_samples, n_targets, who, positive=False)
        aleatoric = np.broadcast_to(np.sum(sig * sig, axis=0) / n_samples, (n_rows, n_targets)).copy()
    shifted = mu - mu[0]                       # (by the first sample's value: a large mean with a tiny spread does not cancel)
    mean = mu[0] + np.sum(shifted, axis=0) / n_samples
    epistemic = np.var(shifted, axis=0) if n_samples > 1 else np.zeros((n_rows, n_targets))
    res.update(mean=mean, epistemic_var=epistemic, aleatoric_var=aleatoric, total_var=epistemic + aleatoric)
    for k in REGRESSION_KEYS:
        res[k + "_avg"] = np.mean(res[k], axis=0)
    return res


def _strip_pointwise(res):
    return {k: v for k, v in res.items() if k not in CLASS_ROW_KEYS + REGRESSION_KEYS + ("mean_prob", "predicted_class")}


def get_posterior_uncertainty(pkl_file, features=None, pointwise=True):
    """Uncertainty decomposition of a checkpoint's stored samples: on its own test table (default), on its training table
    (``features="train"``), or on a feature matrix.  The kind follows the model's estimation mode - ``"classification"``,
    ``"regression"`` (sigma per sample from the samples' ``error_prm``) or ``"regression-error"`` (sigma predicted per row);
    predictions as ``get_posterior_est`` computes them (per-sample slopes, the last sample's slopes left installed).  Returns
    ``posterior_uncertainty``'s dict; without ``pointwise`` only the means over the rows, ``n_samples`` and ``n_rows`` (the [N, ...]
    arrays then never leave the device).  ``ValueError`` before any device call: no stored samples, an empty table, a
    ``"regression"`` checkpoint without ``error_prm``, an odd number of outputs under ``"regression-error"``, ``"custom"`` and the
    count likelihoods' estimation modes."""
    who = "get_posterior_uncertainty"
    model, samples, mode, n_out = open_checkpoint(load_obj(pkl_file), who, KINDS, "%s are served; \"custom\" and the count likelihoods are not" % ", ".join(KINDS))
    x, _ = choose_table(model, features, None, who, need_labels=False)
    sigma = None
    if mode == "regression":
        sigma = sample_sigmas(samples, n_out, who)
    elif mode == "regression-error" and n_out % 2:
        raise ValueError("%s: \"regression-error\" predicts a mean and a sigma per target, and %d outputs is odd" % (who, n_out))
    with open_predictor(model, samples, x.shape[1]) as pred:
        res = pred.uncertainty(x, mode, sigma_sets=sigma, pointwise=pointwise)
    res = dict(res, n_samples=len(samples), n_rows=len(x))
    return res if pointwise else _strip_pointwise(res)
