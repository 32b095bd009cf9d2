"""What the attribution tests (partial dependence, accumulated local effects, saliency, Shapley) share: the oracle's activation of one
stored sample, the column override on a copy of a table, an output callable without a device kind, a seam's arguments as the float64 restatements take them, and a stand-in
for a loaded checkpoint."""
import numpy as np

import oracle as orc


def _act(fun, slopes, trainable):
    return orc.Act(fun, prm=None if slopes is None else np.asarray(slopes, dtype=float), trainable=trainable)


def _apply_override(x, override):
    """a float64 copy of ``x`` with ``override``'s columns (NaN = none) at their constants"""
    x = np.array(x, dtype=np.float64, copy=True)
    if override is not None:
        cols = ~np.isnan(override)
        x[:, cols] = np.asarray(override)[cols]
    return x


def softmax_np(z):
    """a softmax the package does not know (``output_kind`` is None): a custom output callable"""
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def seam_to_oracle(alphas, actFun, output_act_fun, data_transform):
    """What a device seam was given, as the restatements' arguments: (the activation's name, the output function's name - a key of
    pdp_cases.OUT_FNS, every sample's slopes as a float array, the feature indicators as a column override or None)."""
    from npbnn_amd import _capi as capi
    from npbnn_amd.layers import output_kind
    out = {capi.OUT_SOFTMAX: "softmax", capi.OUT_IDENTITY: "identity"}[output_kind(output_act_fun)]
    override = None if data_transform is None else np.asarray(data_transform.column_override(), dtype=float)
    return actFun._function, out, [np.asarray(a, dtype=float) for a in alphas], override


class _Holder:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def fake_checkpoint(call_args, case, **model_kw):
    """``[model, None, logger]`` as ``load_obj`` returns it, from pdp_cases.call_args' tuple for the fixture case ``case`` and the
    case's feature indicators; ``model_kw``: further attributes of the model."""
    x, _, mode, n_out, act, out_fn, weights, alphas, _ = call_args
    model = _Holder(_data=x, _estimation_mode=mode, _size_output=n_out, _act_fun=act, _output_act_fun=out_fn,
                    _feature_indicators=case["indicators"], _feature_means=case["means"], **model_kw)
    logger = _Holder(_post_weight_samples=[{"weights": w, "alphas": a} for w, a in zip(weights, alphas)])
    return [model, None, logger]
