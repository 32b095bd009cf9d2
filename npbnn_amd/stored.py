"""What the stored-sample drivers share on the host.  The statistics (``get_posterior_lppd``, ``_uncertainty``, ``_calibration``,
``_convergence``, in part ``_hpd`` and ``_threshold``): reading a loaded checkpoint, choosing the table, validating labels, targets and
per-sample sigmas, and opening the predictor.  The attributions (``get_pdp``, ``get_ale``, ``get_saliency``, ``get_shapley``) and the
predictor itself: one description of the samples' network as the device takes it (``Network``), with the context it opens on a table,
the samples of a loaded checkpoint, and the summary over the samples.  A leaf module: the backend is imported inside functions only,
and every error carries the caller's name (``who``)."""
import contextlib

import numpy as np

from . import _capi as capi
from .layers import output_kind


class Network:
    """The network of the stored samples ``weights`` (a per-layer list each) as the library is told of it: ``out_kind`` (OUT_*,
    identity for no output function and for a custom callable), ``apply_out_fn``, ``custom_output`` (a callable without a device
    kind: the device returns the last layer's values and the callable runs on the host), ``slopes`` (genReLU: every sample's
    ``alphas`` cut to the hidden layers; else None) and ``override`` (``data_transform``'s columns, or None without one: to the
    library a missing override and one of NaN alone are the same)."""

    def __init__(self, weights, alphas, actFun, output_act_fun, data_transform=None):
        kind = output_kind(output_act_fun)
        self.weights, self.act_kind = weights, actFun.device_kind()
        self.out_kind = capi.OUT_IDENTITY if kind is None else kind
        self.apply_out_fn = kind is not None
        self.custom_output = kind is None and output_act_fun is not None
        self.slopes = None
        if actFun._function == "genReLU":
            n_hidden = len(weights[0]) - 1
            self.slopes = [np.asarray(a, dtype=float).ravel()[:n_hidden] for a in alphas]
        self.override = None if data_transform is None else np.asarray(data_transform.column_override(), dtype=float)

    def sets(self):
        """what every ``HipContext.predict_*`` entry of the attributions takes: the packed samples and their keywords"""
        from .backend import pack_weights
        return [pack_weights(w) for w in self.weights], dict(act_prm_sets=self.slopes, col_override=self.override,
                                                             apply_out_fn=self.apply_out_fn)

    def describe_to(self, ctx, n_features):
        ctx.set_arch_from_weights(self.weights[0], n_features, self.act_kind, self.out_kind, capi.LIK_NONE)

    @contextlib.contextmanager
    def on(self, data, test_data=None):
        """A ``HipContext`` that holds ``data`` as its training table (and ``test_data`` as its test table), both as contiguous
        float64, and this network; closed on the way out."""
        from .backend import HipContext
        data = np.ascontiguousarray(data, dtype=np.float64)
        ctx = HipContext()
        try:
            ctx.set_data(data)
            if test_data is not None:
                ctx.set_data(np.ascontiguousarray(test_data, dtype=np.float64), capi.TEST)
            self.describe_to(ctx, data.shape[1])
            yield ctx
        finally:
            ctx.close()


def checkpoint_samples(checkpoint):
    """(model, the samples' weights, their alphas, the model's feature indicators as a ``data_transform_obj`` or None) of a loaded
    checkpoint ``[bnn, mcmc, logger]`` (the driver loads it through its own ``load_obj``)."""
    from .model import data_transform_obj
    model, _, logger = checkpoint
    samples = logger._post_weight_samples
    transform = None
    if model._feature_indicators is not None:
        transform = data_transform_obj(model._feature_indicators, model._feature_means)
    return model, [s['weights'] for s in samples], [s['alphas'] for s in samples], transform


def check_level(level, who):
    if not 0.0 < level < 1.0:
        raise ValueError("%s: level must lie in (0, 1)" % who)


def quantile_summary(samples, level):
    """[..., 3] of samples [S, ...]: the mean over the samples, then the equal-tailed quantiles"""
    tail = 0.5 * (1.0 - level)
    res = np.empty(samples.shape[1:] + (3,))
    res[..., 0] = samples.mean(axis=0)
    res[..., 1:] = np.moveaxis(np.quantile(samples, (tail, 1.0 - tail), axis=0), 0, -1)
    return res


def class_labels(labels, n_rows, n_classes, who):
    lab = np.asarray(labels)
    if lab.ndim != 1 or len(lab) != n_rows:
        raise ValueError("%s: %s labels for %d rows" % (who, lab.shape, n_rows))
    if lab.dtype.kind not in "iuf" or not (np.all(lab == np.floor(lab)) and np.all(lab >= 0) and np.all(lab < n_classes)):
        raise ValueError("%s: the labels are not class indices in [0, %d)" % (who, n_classes))
    return lab.astype(np.int64)


def target_matrix(labels, n_rows, n_targets, who):
    t = np.asarray(labels, dtype=np.float64)
    if t.ndim == 1:
        t = t.reshape(-1, 1)
    if t.shape != (n_rows, n_targets):
        raise ValueError("%s: targets are %s, expected %s" % (who, t.shape, (n_rows, n_targets)))
    if not np.all(np.isfinite(t)):
        raise ValueError("%s: the targets hold NaN or infinite values" % who)
    return t


def sigma_matrix(sigma_sets, n_samples, n_targets, who, positive=True):
    """``sigma_sets`` [S, T], [S, 1] or [S] as float64 [S, T].  ``positive``: every entry positive and finite, and the result
    contiguous (it goes to the device: lppd, calibration); otherwise NaN alone is refused and the result is a broadcast view (the
    uncertainty route only squares and sums it)."""
    if sigma_sets is None:
        raise ValueError("%s: kind \"regression\" needs sigma_sets (a sigma per sample and target)" % who)
    sig = np.asarray(sigma_sets, dtype=np.float64)
    if sig.ndim == 1:
        sig = sig.reshape(-1, 1)
    if sig.ndim != 2 or sig.shape[0] != n_samples or sig.shape[1] not in (1, n_targets):
        raise ValueError("%s: sigma_sets is %s, expected (%d, %d)" % (who, sig.shape, n_samples, n_targets))
    if positive:
        if not (np.all(np.isfinite(sig)) and np.all(sig > 0)):
            raise ValueError("%s: every sigma must be positive and finite" % who)
    elif np.any(np.isnan(sig)):
        raise ValueError("%s: sigma_sets holds NaN" % who)
    sig = np.broadcast_to(sig, (n_samples, n_targets))
    return np.ascontiguousarray(sig) if positive else sig


def sample_sigmas(samples, n_out, who):
    """[S, n_out] from the samples' ``error_prm``, the per-sample sigma of the Gaussian likelihood."""
    if any('error_prm' not in s or len(np.atleast_1d(s['error_prm'])) == 0 for s in samples):
        raise ValueError("%s: the checkpoint's samples carry no error_prm (the per-sample sigma of the Gaussian "
                         "likelihood): the run had no error parameters to store" % who)
    sig = np.array([np.ones(n_out) * np.asarray(s['error_prm'], dtype=np.float64) for s in samples])
    if not (np.all(np.isfinite(sig)) and np.all(sig > 0)):
        raise ValueError("%s: a sample's error_prm is not positive and finite" % who)
    return sig


def open_checkpoint(checkpoint, who, modes, out_of_scope):
    """(model, stored samples, estimation mode, outputs of the last layer) of a loaded checkpoint ``[bnn, mcmc, logger]`` (the
    driver loads it through its own ``load_obj``); ``ValueError`` when it holds no samples or its mode is not one of ``modes``
    (``out_of_scope`` says what is served and what is not)."""
    model, _, logger = checkpoint
    samples = logger._post_weight_samples
    if len(samples) == 0:
        raise ValueError("%s: the checkpoint holds no posterior samples" % who)
    mode = getattr(model, "_estimation_mode", "classification")
    if mode not in modes:
        raise ValueError("%s: estimation mode %r is out of scope (%s)" % (who, mode, out_of_scope))
    return model, samples, mode, len(samples[0]['weights'][-1])


def choose_table(model, features, labels, who, need_labels):
    """(x as 2-D float64, y): the model's training table (``features="train"``), its test table (None) or ``features`` with
    ``labels``; ``y`` is None unless ``need_labels``."""
    if isinstance(features, str):
        if features != "train":
            raise ValueError("%s: features=%r; \"train\", None (the test table) or a matrix" % (who, features))
        x, y = model._data, model._labels if need_labels else None
    elif features is None:
        x, y = model._test_data, model._test_labels if need_labels else None
    else:
        if need_labels and labels is None:
            raise ValueError("%s: a feature matrix needs its labels" % who)
        x, y = features, labels if need_labels else None
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2 or len(x) == 0:
        raise ValueError("%s: the table is empty" % who)
    return x, y


def open_predictor(model, samples, n_features):
    """The device predictor of ``samples`` (close it with ``with``), the last sample's slopes left installed on the model's
    activation as ``get_posterior_est`` leaves them."""
    from .posterior import _SamplePredictor
    act = model._act_fun
    act.reset_prm(samples[-1]['alphas'])
    return _SamplePredictor(n_features, samples, act, model._output_act_fun)
