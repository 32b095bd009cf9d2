"""Accumulated local effects (Apley & Zhu 2020): ``make_ale_edges``, ``get_ale``, ``ale``.  np_bnn has no counterpart.

Partial dependence (``npbnn_amd.pdp``) sets the focal column to one grid value on every row; with correlated features that
evaluates the network far outside the data.  Here a row only moves to the two edges of its own quantile bin.  With edges
``z_0 < ... < z_K`` of the focal column j, row i belongs to bin ``k(i)``, the smallest k in 1..K with ``x_ij <= z_k`` (bin K
above ``z_K``), and for a stored sample s

    local effect   D[s, k] = mean over the rows of bin k of  f_s(x_i, column j at z_k) - f_s(x_i, column j at z_(k-1))
    curve          A[s, 0] = 0,  A[s, k] = D[s, 1] + ... + D[s, k]
    centred curve  A[s, k] - sum_k n_k (A[s, k-1] + A[s, k]) / (2 n)

``npbnn_predict_ale`` returns the bin counts and D for every stored sample from the resident matrix - on networks whose
weights are resident in LDS both evaluations of a row come from one read of X, as a moved column only shifts layer 0's
pre-activation by a multiple of ``W0[:, j]``.  The sums along the feature, the centring and the summary over the samples are
taken here in float64: one curve per sample, so the band is a credible band of the effect itself."""
import numpy as np

from .files import load_obj
from .pdp import get_feature_summary
from .stored import Network, check_level, checkpoint_samples, quantile_summary


def _focal_column(focal_feature, who):
    cols = np.atleast_1d(np.asarray(focal_feature)).ravel()
    if len(cols) != 1:
        raise ValueError("%s: one focal column at a time (got %d); two-dimensional effects and one-hot blocks are not covered"
                         % (who, len(cols)))
    return int(cols[0])


def make_ale_edges(data, focal_feature, n_bins=40):
    """The bin edges [K + 1] of one focal column.  A column ``get_feature_summary`` calls binary or ordinal: its distinct
    values.  Any other column: the ``n_bins + 1`` evenly spaced quantiles, repeated ones merged (so K may be below ``n_bins``).
    ``ValueError`` when fewer than two distinct edges are left."""
    j = _focal_column(focal_feature, "make_ale_edges")
    col = np.asarray(data, dtype=np.float64)[:, j]
    if get_feature_summary(np.asarray(data), [j])[0, 0]:
        edges = np.unique(col)
    else:
        if n_bins < 1:
            raise ValueError("make_ale_edges: n_bins must be at least 1")
        edges = np.unique(np.quantile(col, np.linspace(0, 1, int(n_bins) + 1)))
    if len(edges) < 2:
        raise ValueError("make_ale_edges: column %d has fewer than two distinct values" % j)
    return edges


def accumulate_and_centre(counts, effects):
    """[S, K + 1, n_out]: the local effects [S, K, n_out] summed along the bins from 0 at the first edge, minus each sample's
    mean over the rows (a row of bin k counts as the midpoint of the curve over its bin)."""
    counts = np.asarray(counts, dtype=np.float64)
    effects = np.asarray(effects, dtype=np.float64)
    curve = np.zeros((effects.shape[0], effects.shape[1] + 1, effects.shape[2]))
    np.cumsum(effects, axis=1, out=curve[:, 1:])
    mid = 0.5 * (curve[:, :-1] + curve[:, 1:])
    centre = np.einsum("k,skc->sc", counts, mid) / counts.sum()
    return curve - centre[:, None, :]


def _ale_local_effects(data, focal, edges, weights, alphas, actFun, output_act_fun, data_transform):
    """(counts [K], local effects [S, K, n_out]) on the table as the device holds it (the device seam)."""
    net = Network(weights, alphas, actFun, output_act_fun, data_transform)
    with net.on(data) as ctx:
        if net.custom_output:
            # a custom output callable has no device kind: one pass per (edge, sample), the callable and the bins on the host
            data = np.asarray(data, dtype=np.float64)
            col = data[:, focal].astype(np.float32)
            k_of_row = np.minimum(np.searchsorted(edges.astype(np.float32)[1:], col, side="left"), len(edges) - 2)
            counts = np.bincount(k_of_row, minlength=len(edges) - 1).astype(np.int64)
            effects = np.zeros((len(weights), len(edges) - 1, ctx.n_out))
            for i, w in enumerate(weights):
                prm = None if net.slopes is None else net.slopes[i]
                lower = None
                for k, z in enumerate(edges):
                    co = np.full(data.shape[1], np.nan) if net.override is None else net.override.copy()
                    if np.isnan(co[focal]):
                        co[focal] = z
                    upper = output_act_fun(ctx.predict(w, act_prm=prm, col_override=co, apply_out_fn=False))
                    if k > 0 and counts[k - 1]:
                        rows = k_of_row == k - 1
                        effects[i, k - 1] = (upper[rows] - lower[rows]).mean(axis=0)
                    lower = upper
            return counts, effects
        packed, kw = net.sets()
        return ctx.predict_ale(packed, focal, edges, **kw)


def get_ale(data, focal_feature, estimation_mode, size_output, actFun, output_act_fun, weights, alphas, data_transform,
            n_bins=40, level=0.95):
    """Accumulated local effects of the output on one focal column, a curve per stored sample:

    ``'feature'``        the edges [K + 1] (``make_ale_edges``)
    ``'counts'``         rows per bin [K]
    ``'ale'``            [K + 1, size_output, 3]: the mean over the samples of the centred curve, then its equal-tailed
                         ``(1 - level) / 2`` and ``1 - (1 - level) / 2`` quantiles over the samples
    ``'ale_samples'``    the centred curve of every sample [S, K + 1, size_output]
    ``'local_effects'``  [S, K, size_output]

    In classification the curves are those of the class probabilities themselves: there is no cumulative sum over the classes
    (``get_pdp``, following np_bnn, reports cumulative ones), so ``estimation_mode`` changes nothing here.  Each sample runs with
    its own slopes ``alphas``; the last sample's stay installed on ``actFun``.  ``data_transform`` applies after the edges are
    set, as in ``get_pdp``: a focal column it switches off gives a flat zero curve.  ``ValueError`` for more than one focal
    column."""
    focal = _focal_column(focal_feature, "get_ale")
    check_level(level, "get_ale")
    if len(weights) == 0:
        raise ValueError("get_ale: no stored samples")
    edges = make_ale_edges(data, focal, n_bins)
    actFun.reset_prm(alphas[-1])
    counts, effects = _ale_local_effects(data, focal, edges, weights, alphas, actFun, output_act_fun, data_transform)
    samples = accumulate_and_centre(counts, effects)
    if samples.shape[2] != size_output:
        raise ValueError("get_ale: the network has %d outputs, size_output is %d" % (samples.shape[2], size_output))
    return {'feature': edges, 'counts': np.asarray(counts), 'ale': quantile_summary(samples, level), 'ale_samples': samples,
            'local_effects': np.asarray(effects)}


def ale(pickle_file, ale_features, n_bins=40):
    """Accumulated local effects from a checkpoint ``[bnn, mcmc, logger]`` on the model's training matrix: one ``get_ale`` dict
    per focal column in ``ale_features`` (a column index, or a list holding one)."""
    model, weights, alphas, transform = checkpoint_samples(load_obj(pickle_file))
    data = np.asarray(model._data, dtype=np.float64)
    return [get_ale(data, focal, model._estimation_mode, model._size_output, model._act_fun, model._output_act_fun,
                    weights, alphas, transform, n_bins=n_bins) for focal in ale_features]
