"""Shapley attributions of single predictions of a fitted posterior: ``get_shapley``, ``shapley``.  np_bnn has no counterpart.

Permutation importance, partial dependence, accumulated local effects and saliency describe a whole table.  Shapley values
answer for one row why the model said what it said, and they are additive: for a stored sample s, explained row e and output c

    sum_p phi[s, e, p, c] = f_s(x_e)_c - mean_b f_s(b)_c

over the players p (a feature column, or a group of columns such as a one-hot block) and the background rows b.  phi is
estimated by permutation sampling: a walk starts at a background row and sets one player after the other, in the order of a
permutation, to the explained row's values; a player's attribution is the mean over the walks of the step that set it.
``npbnn_predict_shapley`` runs the walks on the device, where a step costs one column of the first layer instead of a forward
pass, and returns summaries; every stored sample yields its own attributions, so they come with a credible band."""
from statistics import NormalDist

import numpy as np

from . import _capi as capi
from .files import load_obj
from .layers import output_kind
from .stored import Network, check_level, checkpoint_samples, quantile_summary


def _shapley_device(data, rows, background_data, bg_rows, player_of, perms, weights, alphas, actFun, output_act_fun, data_transform,
                    want_phi):
    """``HipContext.predict_shapley``'s dict for the rows ``rows`` of ``data`` against the rows ``bg_rows`` of
    ``background_data`` (None: of ``data``), the tables as the device holds them (the device seam)."""
    net = Network(weights, alphas, actFun, output_act_fun, data_transform)
    if net.custom_output:
        raise ValueError("get_shapley: a custom output callable has no device kind")
    # (the backgrounds come from the training table: with a table of their own, the explained rows are the test table's)
    tables, which = ((data, None), capi.TRAIN) if background_data is None else ((background_data, data), capi.TEST)
    with net.on(*tables) as ctx:
        packed, kw = net.sets()
        return ctx.predict_shapley(packed, rows, bg_rows, perms, player_of=player_of, which=which, which_bg=capi.TRAIN,
                                   want_phi=want_phi, **kw)


def _players(n_features, feature_indx_list):
    """(column lists, player_of [F]): the groups of ``feature_indx_list`` in its order, then every column it leaves out as a
    player of its own, in column order"""
    groups = [] if feature_indx_list is None else [[int(j) for j in np.atleast_1d(g)] for g in feature_indx_list]
    player_of = np.full(n_features, -1, dtype=np.int32)
    for p, cols in enumerate(groups):
        if len(cols) == 0:
            raise ValueError("get_shapley: group %d of feature_indx_list has no column" % p)
        for j in cols:
            if not 0 <= j < n_features:
                raise ValueError("get_shapley: column %d of feature_indx_list is outside the table's %d columns" % (j, n_features))
            if player_of[j] >= 0:
                raise ValueError("get_shapley: column %d is in more than one group of feature_indx_list" % j)
            player_of[j] = p
    for j in np.flatnonzero(player_of < 0):
        player_of[j] = len(groups)
        groups.append([int(j)])
    return groups, player_of


def get_shapley(data, size_output, actFun, output_act_fun, weights, alphas, data_transform, rows=None, background=100,
                background_data=None, n_perm=16, feature_indx_list=None, antithetic=True, seed=1234, level=0.95,
                return_samples=False):
    """Shapley attributions of the rows ``rows`` of ``data`` (default: all of them), a value per stored sample, against a
    background sample: ``background`` is an index array into ``background_data`` (default: ``data`` itself), or a count of rows
    drawn from it without replacement by ``seed`` (all of them when it has no more).  ``n_perm`` permutations of the players
    are drawn by ``seed``; with ``antithetic`` ``n_perm / 2`` are drawn and each is followed by its reverse.
    ``feature_indx_list`` groups columns into players as ``feature_importance``'s blocks do; a column it leaves out is a
    player of its own, after the groups.  With E rows, P players and C = ``size_output`` outputs:

    ``'attributions'``     [E, P, C, 3]: the posterior mean over the samples, then an equal-tailed ``level`` band.  With
                           ``return_samples`` the band's ends are the quantiles of the per-sample values; without, the
                           per-sample values never leave the device and the band is mean -+ z sd, z the normal quantile of
                           ``1 - (1 - level) / 2`` and sd the samples' standard deviation from the mean of phi^2
    ``'prediction'``       [E, C]: the posterior mean prediction of every explained row
    ``'base_value'``       [C]: the posterior mean of the mean prediction on the background rows; per sample the
                           attributions of a row sum to its prediction minus the base value
    ``'importance'``       [P, C, 3]: the mean over the rows of |phi| - the posterior mean, then the equal-tailed quantiles
                           over the samples
    ``'ranking'``          the players by importance summed over the outputs, largest first (ties by index)
    ``'players'``          every player's column list
    ``'permutations'``     [n_perm, P], ``'background_rows'``: what the walks ran on
    ``'samples'``          with ``return_samples`` only: ``{'attributions' [S, E, P, C], 'prediction' [S, E, C],
                           'base_value' [S, C], 'importance' [S, P, C]}``

    In classification the attributions are those of the class probabilities.  Each sample runs with its own slopes
    ``alphas``; the last sample's stay installed on ``actFun``.  A player whose columns ``data_transform`` switches off is 0.
    ``ValueError`` for no samples, a ``level`` outside (0, 1), a ``size_output`` that is not the network's, a custom output
    callable, ``n_perm`` below 1 or odd with ``antithetic``, no rows, an empty background, and overlapping groups."""
    check_level(level, "get_shapley")
    if len(weights) == 0:
        raise ValueError("get_shapley: no stored samples")
    if output_kind(output_act_fun) is None and output_act_fun is not None:
        raise ValueError("get_shapley: a custom output callable has no device kind")
    if np.shape(weights[0][-1])[0] != size_output:
        raise ValueError("get_shapley: the network has %d outputs, size_output is %d" % (np.shape(weights[0][-1])[0], size_output))
    n_perm = int(n_perm)
    if n_perm < 1 or (antithetic and n_perm % 2):
        raise ValueError("get_shapley: n_perm must be at least 1, and even with antithetic permutations")
    data = np.asarray(data, dtype=np.float64)
    players, player_of = _players(data.shape[1], feature_indx_list)
    rows = np.arange(data.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64).ravel()
    if len(rows) == 0 or rows.min() < 0 or rows.max() >= data.shape[0]:
        raise ValueError("get_shapley: rows must be indices into data, at least one")
    n_bg_table = data.shape[0] if background_data is None else np.shape(background_data)[0]
    rs = np.random.default_rng(seed)
    if np.ndim(background) == 0:
        bg_rows = np.sort(rs.choice(n_bg_table, size=min(int(background), n_bg_table), replace=False)) if int(background) > 0 else np.zeros(0)
    else:
        bg_rows = np.asarray(background, dtype=np.int64).ravel()
    bg_rows = np.asarray(bg_rows, dtype=np.int64)
    if len(bg_rows) == 0 or bg_rows.min() < 0 or bg_rows.max() >= n_bg_table:
        raise ValueError("get_shapley: the background must be indices into its table, at least one")
    n_players = len(players)
    if antithetic:
        drawn = np.array([rs.permutation(n_players) for _ in range(n_perm // 2)])
        perms = np.stack([drawn, drawn[:, ::-1]], axis=1).reshape(n_perm, n_players)
    else:
        perms = np.array([rs.permutation(n_players) for _ in range(n_perm)])
    perms = np.ascontiguousarray(perms, dtype=np.int32)

    actFun.reset_prm(alphas[-1])
    dev = _shapley_device(data, rows, background_data, bg_rows, player_of, perms, weights, alphas, actFun, output_act_fun, data_transform,
                          bool(return_samples))
    mean, sq, absolute, fx, base = (np.asarray(dev[k], dtype=np.float64) for k in ("mean", "sq", "abs", "fx", "base"))
    if return_samples:
        attributions = quantile_summary(np.asarray(dev["phi"], dtype=np.float64), level)
    else:
        z = NormalDist().inv_cdf(1.0 - 0.5 * (1.0 - level))
        sd = np.sqrt(np.maximum(sq - mean * mean, 0.0))
        attributions = np.stack([mean, mean - z * sd, mean + z * sd], axis=-1)
    result = {'attributions': attributions, 'prediction': fx.mean(axis=0), 'base_value': base.mean(axis=0),
              'importance': quantile_summary(absolute, level), 'players': players, 'permutations': perms, 'background_rows': bg_rows}
    result['ranking'] = np.argsort(-result['importance'][:, :, 0].sum(axis=1), kind="stable")
    if return_samples:
        result['samples'] = {'attributions': np.asarray(dev["phi"], dtype=np.float64), 'prediction': fx, 'base_value': base,
                             'importance': absolute}
    return result


def shapley(pickle_file, which="test", **kw):
    """``get_shapley`` from a checkpoint ``[bnn, mcmc, logger]``: the rows of the model's test matrix (``which="test"``) or of
    its training matrix (``"train"``) against a background sample of the training matrix.  The keywords are ``get_shapley``'s
    from ``rows`` on."""
    if which not in ("train", "test"):
        raise ValueError("shapley: which must be 'train' or 'test'")
    model, weights, alphas, transform = checkpoint_samples(load_obj(pickle_file))
    train = np.asarray(model._data, dtype=np.float64)
    data = train if which == "train" else np.asarray(model._test_data, dtype=np.float64)
    kw.setdefault("background_data", None if which == "train" else train)
    return get_shapley(data, model._size_output, model._act_fun, model._output_act_fun, weights, alphas, transform, **kw)
