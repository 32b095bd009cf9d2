"""Partial dependence: ``get_feature_summary``, ``make_pdp_features``, ``get_pdp``, ``pdp`` (np_bnn 0.1.23 exports them from its
flat namespace; its driver is bnn_pdp.py).

The partial dependence of the network's output on a set of focal features is the prediction averaged over the rows of the
training matrix with the focal columns set to one point of a grid.  Upstream runs a full forward pass per (grid point, stored
sample).  Here the matrix is uploaded once and ``npbnn_predict_pdp`` returns, per grid point and row, the mean over the stored
samples.  On networks whose weights are resident in LDS one streaming read of X serves every grid point: a grid point only
shifts layer 0's pre-activation by ``sum_f v[f] * W0[:, f]``.  Other networks run one pass per (grid point, sample) with the
grid values folded into layer 0's bias.  The cumulative sum over the classes, the means and the quantiles are taken on the
host in float64."""
import numpy as np

from .files import load_obj
from .stored import Network, checkpoint_samples


def get_feature_summary(data, focal_features):
    """[3, n_focal]: row 0 is 1 when every value of the column is an integer step above its minimum (binary, ordinal, one-hot)
    and 0 otherwise; rows 1 and 2 are the column's smallest and largest value."""
    summary = np.zeros((3, len(focal_features)))
    for i, col in enumerate(focal_features):
        values = np.unique(data[:, col])
        lo, hi = np.nanmin(values), np.nanmax(values)
        summary[0, i] = np.all(np.isin(values, np.arange(lo, hi + 1)))
        summary[1, i] = lo
        summary[2, i] = hi
    return summary


def make_pdp_features(data, focal_features, steps_continuous=100):
    """The grid [n_points, n_focal] along which the partial dependence is computed.  One continuous feature: ``steps_continuous``
    evenly spaced values from its minimum to its maximum.  One binary or ordinal feature: ``int(max) + 1`` evenly spaced values
    from its minimum to ``int(max)`` (not integers when the minimum is not 0, as upstream).  Anything else - a one-hot block,
    but also several continuous features, as upstream - the identity of size n_focal."""
    summary = get_feature_summary(data, focal_features)
    if len(focal_features) == 1:
        lo, hi = summary[1, 0], summary[2, 0]
        if summary[0, 0] == 0:
            return np.linspace(lo, hi, num=steps_continuous).reshape(steps_continuous, 1)
        top = int(hi)
        return np.linspace(lo, top, num=top + 1).reshape(top + 1, 1)
    return np.eye(len(focal_features))


def _pdp_row_means(data, focal_features, grid, weights, alphas, actFun, output_act_fun, data_transform):
    """[n_points, n_rows, n_out]: per grid point and row, the prediction averaged over the stored samples (the device seam)."""
    net = Network(weights, alphas, actFun, output_act_fun, data_transform)
    with net.on(data) as ctx:
        if net.custom_output:
            # a custom output callable has no device kind: one pass per (grid point, sample), the callable on the host
            out = np.zeros((len(grid), np.shape(data)[0], ctx.n_out))
            for g, point in enumerate(grid):
                co = np.full(np.shape(data)[1], np.nan) if net.override is None else net.override.copy()
                cols = np.asarray(focal_features)
                free = np.isnan(co[cols])
                co[cols[free]] = np.asarray(point, dtype=float)[free]
                for i, w in enumerate(weights):
                    y = ctx.predict(w, act_prm=None if net.slopes is None else net.slopes[i], col_override=co, apply_out_fn=False)
                    out[g] += output_act_fun(y)
            return out / len(weights)
        packed, kw = net.sets()
        return ctx.predict_pdp(packed, focal_features, grid, **kw)


def get_pdp(data, focal_features, estimation_mode, size_output, actFun, output_act_fun, weights, alphas, data_transform):
    """Partial dependence of the output on ``focal_features``: ``{'feature': grid [n_points, n_focal], 'pdp': [n_points,
    size_output, 3]}``.  ``[..., 0]`` is the mean prediction over the stored samples and the rows, ``[..., 1]`` and ``[..., 2]``
    the 2.5 % and 97.5 % quantiles over the rows of the per-row mean; in classification the class probabilities are summed
    cumulatively first.  Each sample runs with its own slopes ``alphas``; the last sample's stay installed on ``actFun``.
    ``data_transform`` applies after the grid values are set: a focal column it switches off reads as its mean."""
    grid = make_pdp_features(data, focal_features)
    focal = list(focal_features)
    if len(weights):
        actFun.reset_prm(alphas[-1])        # (upstream installs every sample's slopes in turn; the last one stays)
    means = _pdp_row_means(data, focal, grid, weights, alphas, actFun, output_act_fun, data_transform)
    if estimation_mode == 'classification':
        means = np.cumsum(means, axis=2)
    result = np.zeros((grid.shape[0], size_output, 3))
    result[:, :, 0] = np.mean(means, axis=1)
    quantiles = np.quantile(means, q=(0.025, 0.975), axis=1)
    result[:, :, 1] = quantiles[0]
    result[:, :, 2] = quantiles[1]
    return {'feature': grid, 'pdp': result}


def pdp(pickle_file, pdp_features):
    """Partial dependence from a checkpoint ``[bnn, mcmc, logger]`` on the model's training matrix: one ``get_pdp`` dict per list
    of focal features in ``pdp_features``."""
    model, weights, alphas, transform = checkpoint_samples(load_obj(pickle_file))
    data = np.asarray(model._data, dtype=np.float64)
    return [get_pdp(data, focal, model._estimation_mode, model._size_output, model._act_fun, model._output_act_fun,
                    weights, alphas, transform) for focal in pdp_features]
