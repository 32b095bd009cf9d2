"""Input-gradient saliency of a fitted posterior: ``get_saliency``, ``saliency``.  np_bnn has no counterpart.

Permutation importance, partial dependence and accumulated local effects all move one column at a time and run the network
again.  The derivative of the output with respect to every input gives all features at once: for a stored sample s, row i,
output c and feature j

    G[s, i, c, j] = d f_s(x_i)_c / d x_ij

``npbnn_predict_saliency`` returns, per sample, the means over the rows of G (the average marginal effect), of |G| (the
saliency) and of G^2 from one read of the resident matrix per group of samples; G itself never leaves the device.  The
summary over the samples is taken here in float64: one value per sample, so the band is a credible band of the quantity
itself."""
import numpy as np

from .files import load_obj
from .layers import output_kind
from .stored import Network, check_level, checkpoint_samples, quantile_summary


def _saliency_means(data, weights, alphas, actFun, output_act_fun, data_transform):
    """(mean, abs, sq), each [S, n_out, F]: the row means of G, |G| and G^2 on the table as the device holds it (the device
    seam)."""
    net = Network(weights, alphas, actFun, output_act_fun, data_transform)
    if net.custom_output:
        raise ValueError("get_saliency: a custom output callable has no device kind and cannot be differentiated")
    with net.on(data) as ctx:
        packed, kw = net.sets()
        return ctx.predict_saliency(packed, **kw)


def get_saliency(data, size_output, actFun, output_act_fun, weights, alphas, data_transform, level=0.95):
    """Input gradients of the output on every feature column, a value per stored sample:

    ``'mean_gradient'``     [F, size_output, 3]: the mean over the rows of the gradient (the average marginal effect) - the
                            posterior mean over the samples, then its equal-tailed ``(1 - level) / 2`` and
                            ``1 - (1 - level) / 2`` quantiles over the samples
    ``'saliency'``          likewise for the mean absolute gradient
    ``'rms_gradient'``      likewise for the root of the mean squared gradient
    ``'samples'``           ``{'mean_gradient', 'saliency', 'rms_gradient'}``: every sample's values [S, size_output, F]
    ``'sign_probability'``  [F, size_output]: the share of samples whose mean gradient is positive
    ``'ranking'``           the feature indices by the posterior mean of the saliency summed over the outputs, largest first
                            (ties by index)

    In classification the gradients are those of the class probabilities.  Each sample runs with its own slopes ``alphas``;
    the last sample's stay installed on ``actFun``.  A column ``data_transform`` switches off has gradient 0.  ``ValueError``
    for no samples, a ``level`` outside (0, 1), a ``size_output`` that is not the network's, and a custom output callable
    (it has no device kind, so it cannot be differentiated)."""
    check_level(level, "get_saliency")
    if len(weights) == 0:
        raise ValueError("get_saliency: no stored samples")
    if output_kind(output_act_fun) is None and output_act_fun is not None:
        raise ValueError("get_saliency: a custom output callable has no device kind and cannot be differentiated")
    actFun.reset_prm(alphas[-1])
    mean, absolute, sq = (np.asarray(a, dtype=np.float64) for a in
                          _saliency_means(data, weights, alphas, actFun, output_act_fun, data_transform))
    if mean.shape[1] != size_output:
        raise ValueError("get_saliency: the network has %d outputs, size_output is %d" % (mean.shape[1], size_output))
    samples = {'mean_gradient': mean, 'saliency': absolute, 'rms_gradient': np.sqrt(sq)}
    # ([F, size_output, 3] of samples [S, size_output, F])
    result = {k: np.ascontiguousarray(quantile_summary(v, level).transpose(1, 0, 2)) for k, v in samples.items()}
    result['samples'] = samples
    result['sign_probability'] = (mean > 0).mean(axis=0).T
    result['ranking'] = np.argsort(-result['saliency'][:, :, 0].sum(axis=1), kind="stable")
    return result


def saliency(pickle_file, which="train", level=0.95):
    """``get_saliency`` from a checkpoint ``[bnn, mcmc, logger]`` on the model's training matrix (``which="train"``) or its
    test matrix (``"test"``)."""
    if which not in ("train", "test"):
        raise ValueError("saliency: which must be 'train' or 'test'")
    model, weights, alphas, transform = checkpoint_samples(load_obj(pickle_file))
    data = np.asarray(model._data if which == "train" else model._test_data, dtype=np.float64)
    return get_saliency(data, model._size_output, model._act_fun, model._output_act_fun, weights, alphas, transform, level=level)
