"""Stand-alone device operators on host arrays (npbnn_op_* in the C ABI).

These back the reference's small helper callables when user code calls them directly — ``bn.tanh_f(z, 0)``,
``bn.SoftMax(z)``, ``bn.calc_likelihood(y, labels, ids)``, ``bn.CalcAccuracy(y, labels)`` … — so that even the slow,
matrix-in / matrix-out path runs on the GPU.  The sampler itself never takes this route for the built-in functions
(it fuses them into the evaluation kernel)."""
import ctypes as C

import numpy as np

from . import _capi as capi
from .backend import default_device

_I64P = C.POINTER(C.c_int64)


def _lib():
    lib = capi.load_library()
    n = C.c_int(0)
    if lib.npbnn_device_count(C.byref(n)) != 0 or n.value < 1:
        raise capi.BackendUnavailable("no HIP device visible: npbnn_amd operators need an MI355X (there is no CPU fallback)")
    return lib, default_device() % n.value


def _chk(lib, rc):
    capi.check(lib, None, rc)


def activation(z, kind, prm=0):
    """relu / leaky relu mutate their argument like the reference (BNN_lib.py:50-56); swish / tanh return a new array."""
    lib, dev = _lib()
    z = np.asarray(z)
    buf = np.ascontiguousarray(z, dtype=np.float64).copy()
    _chk(lib, lib.npbnn_op_activation(dev, int(kind), float(prm), capi.dptr(buf), buf.size))
    if kind in (capi.ACT_RELU, capi.ACT_LEAKY) and isinstance(z, np.ndarray) and z.dtype == np.float64:
        z[...] = buf.reshape(z.shape)
        return z
    return buf.reshape(z.shape)


def softplus(z):
    lib, dev = _lib()
    buf = np.ascontiguousarray(z, dtype=np.float64).copy()
    _chk(lib, lib.npbnn_op_activation(dev, 4, 0.0, capi.dptr(buf), buf.size))
    return buf.reshape(np.shape(z))


def output_fn(z, kind, ind=None):
    """SoftMax returns a new matrix; RegressTransform returns its argument; RegressTransformError rewrites the
    columns >= ind in place (BNN_lib.py:166-182)."""
    if kind == capi.OUT_IDENTITY:
        return z
    lib, dev = _lib()
    z = np.asarray(z)
    buf = np.ascontiguousarray(z, dtype=np.float64).copy()
    rows, cols = buf.shape
    _chk(lib, lib.npbnn_op_output(dev, int(kind), capi.dptr(buf), rows, cols, -1 if ind is None else int(ind)))
    if kind == capi.OUT_SOFTPLUS_HALF and z.dtype == np.float64:
        z[...] = buf
        return z
    return buf


def _rows_match(what, a, rows, fn):
    """The per-row arguments of an operator must cover exactly the rows it uses: the C operators read ``rows`` entries of each."""
    if len(a) != rows:
        raise ValueError("%s: %s has %d rows, the prediction rows used are %d" % (fn, what, len(a), rows))


def likelihood(kind, prediction, labels, class_weight=None, instance_weight=None, lik_temp=1, sig2=None, sample_id=None):
    """``sample_id`` selects the prediction's rows of a categorical likelihood, ``labels`` aligned to it, as the reference's
    ``prediction[sample_id, labels]`` (BNN_lib.py:100-121); the other kinds ignore it, as upstream does.  Every argument is
    checked against the rows used before the device is touched."""
    pred = capi.as_f64(prediction)
    if pred.ndim != 2:
        raise ValueError("likelihood: the prediction must be a matrix, got shape %s" % (pred.shape,))
    lab = tg = None
    k = 0
    cw = None if class_weight is None or len(class_weight) == 0 else capi.as_f64(class_weight)
    iw = None
    sg = None
    if kind == capi.LIK_CATEGORICAL:
        if cw is not None and instance_weight is not None:
            # upstream sums a vector over axis 1 here and fails (BNN_lib.py:105); keep the failure
            raise np.exceptions.AxisError("axis 1 is out of bounds for array of dimension 1")
        if sample_id is not None:
            pred = np.ascontiguousarray(pred[np.asarray(sample_id)])
            if pred.ndim != 2:
                raise ValueError("likelihood: sample_id must select rows of the prediction")
        lab = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
        _rows_match("labels", lab, pred.shape[0], "likelihood")
        if instance_weight is not None:
            iw = capi.as_f64(instance_weight).reshape(-1)
            _rows_match("instance_weight", iw, pred.shape[0], "likelihood")
    else:
        tg = capi.as_f64(labels)
        if tg.ndim == 1:
            tg = tg.reshape(-1, 1)
        _rows_match("targets", tg, pred.shape[0], "likelihood")
        k = tg.shape[1]
        if kind == capi.LIK_GAUSS:
            sg = capi.as_f64(np.broadcast_to(1 if sig2 is None else sig2, (k,)))
    rows, cols = pred.shape
    out = C.c_double(0)
    lib, dev = _lib()
    _chk(lib, lib.npbnn_op_likelihood(dev, int(kind), capi.dptr(pred), rows, cols,
                                      None if lab is None else lab.ctypes.data_as(_I64P), capi.dptr(tg), k, capi.dptr(iw),
                                      capi.dptr(cw), 0 if cw is None else cw.shape[0], float(lik_temp), capi.dptr(sg),
                                      C.byref(out)))
    return out.value


def _confusion(y, lab):
    pred = capi.as_f64(y)
    if pred.ndim != 2:
        raise ValueError("confusion: the prediction must be a matrix, got shape %s" % (pred.shape,))
    rows, cols = pred.shape
    if lab is not None:
        lab = np.ascontiguousarray(lab, dtype=np.int64).reshape(-1)
        _rows_match("labels", lab, rows, "confusion")
    lib, dev = _lib()
    counts = np.zeros(cols, dtype=np.int64)
    conf = None
    labp = None
    if lab is not None:
        labp = lab.ctypes.data_as(_I64P)
        conf = np.zeros((cols, cols), dtype=np.int64)
    _chk(lib, lib.npbnn_op_confusion(dev, capi.dptr(pred), rows, cols, labp,
                                     None if conf is None else conf.ctypes.data_as(_I64P), counts.ctypes.data_as(_I64P)))
    return conf, counts


def _sse(y, lab, link, first_col_only):
    pred = capi.as_f64(y)
    if pred.ndim != 2:
        raise ValueError("sse: the prediction must be a matrix, got shape %s" % (pred.shape,))
    tg = capi.as_f64(lab)
    if tg.ndim == 1:
        tg = tg.reshape(-1, 1)
    if first_col_only:
        tg = np.ascontiguousarray(tg[:, :1])
    _rows_match("targets", tg, pred.shape[0], "sse")
    k = tg.shape[1]
    if k > pred.shape[1]:
        raise ValueError("sse: %d target columns for a prediction of %d columns" % (k, pred.shape[1]))
    lib, dev = _lib()
    out = np.zeros(k)
    _chk(lib, lib.npbnn_op_sse(dev, capi.dptr(pred), capi.dptr(tg), pred.shape[0], pred.shape[1], k, link, capi.dptr(out)))
    return out, pred.shape[0]


_SSE_KINDS = {"mse": (0, False), "label_mse": (0, False), "mse_exp": (1, False), "mse_exp_col0": (1, True), "mse_pow10_col0": (2, True)}


def statistic_sums(kind, y, lab):
    """What a squared-error statistic is made of, as a vector that adds over rows (a row-sharded chain adds it over its ranks):
    [rows, squared error per column]; None for every other kind."""
    if kind not in _SSE_KINDS:
        return None
    sse, n = _sse(y, lab, *_SSE_KINDS[kind])
    return np.concatenate([[float(n)], sse])


def statistic_of_sums(kind, sums):
    n, sse = sums[0], np.asarray(sums[1:], dtype=float)
    if kind == "label_mse":
        return sse / n
    if kind in ("mse", "mse_exp"):
        return float(np.sum(sse) / (n * len(sse)))
    return float(sse[0] / n)


def statistic(kind, y, lab):
    """The accuracy helpers of the reference on an explicit prediction matrix (BNN_lib.py:195-233, BNN_lik.py:81-99)."""
    if kind == "acc":
        y = np.asarray(y)
        if y.ndim == 3:           # one accuracy per posterior sample (BNN_lib.py:204-205)
            return np.array([statistic("acc", yi, lab) for yi in y])
        conf, _ = _confusion(y, lab)
        return np.trace(conf) / len(lab)
    if kind == "label_acc":
        conf, _ = _confusion(y, lab)
        present = np.unique(np.asarray(lab, dtype=np.int64))
        return np.array([conf[c, c] / conf[c].sum() for c in present])
    if kind == "label_freq":
        _, counts = _confusion(y, None)
        return counts / np.shape(y)[0]
    sums = statistic_sums(kind, y, lab)
    if sums is not None:
        return statistic_of_sums(kind, sums)
    raise ValueError(kind)


def mixture(mu, sigma, probs=(), y=None):
    """npbnn_op_mixture on ``mu`` [S, ...]: quantiles, mean and CRPS of the Gaussian mixtures (1/S) sum_s N(mu_s, sigma_s^2), one per
    trailing cell (npbnn_amd/predictive.py has the definitions).  ``sigma`` has ``mu``'s shape (a sigma per sample and cell), or is
    [S, T] / [S] with T the last axis of ``mu`` (a sigma per sample and target, taken as float64; a flat [S, cells] ``mu`` takes any T, cell c
    reading column c % T).  Returns
    ``(quantiles [len(probs), ...] or None without probs, mean [...], crps [...] or None without y)``, float64, the trailing shape
    kept.  float32 ``mu`` stays float32 on its way to the device (and a per-cell ``sigma`` with it), anything else is taken as
    float64; the arithmetic is float64 either way."""
    from .predictive import MAX_SAMPLES, check_probs
    who = "mixture"
    a = np.asarray(mu)
    if a.ndim < 1 or a.shape[0] < 1:
        raise ValueError("%s: mu must have a leading sample axis" % who)
    if a.shape[0] > MAX_SAMPLES:
        raise ValueError("%s: %d samples, at most %d are supported" % (who, a.shape[0], MAX_SAMPLES))
    pr = check_probs(probs, who)
    n_samples, shape = a.shape[0], a.shape[1:]
    v, kind = capi.value_array(a.reshape(n_samples, -1))
    n_cols = v.shape[1]
    sg = np.asarray(sigma)
    if sg.shape == a.shape:
        sg, sigma_cols = np.ascontiguousarray(sg.reshape(n_samples, -1), dtype=v.dtype), 0
    else:
        n_targets = shape[-1] if len(shape) else 1
        if sg.ndim == 1:
            sg = sg.reshape(-1, 1)
        # (a flat [S, cells] mu takes any [S, T]: cell c reads column c % T, as the library does)
        if sg.ndim != 2 or sg.shape[0] != n_samples or sg.shape[1] < 1 or (sg.shape[1] not in (1, n_targets) and a.ndim != 2):
            raise ValueError("%s: sigma is %s, expected mu's shape %s or (%d, %d)" % (who, sg.shape, a.shape, n_samples, n_targets))
        sg = np.ascontiguousarray(sg, dtype=np.float64)
        sigma_cols = sg.shape[1]
    if not np.all(np.isfinite(v)):
        raise ValueError("%s: mu holds NaN or infinite values" % who)
    if not (np.all(np.isfinite(sg)) and np.all(sg > 0)):
        raise ValueError("%s: every sigma must be positive and finite" % who)
    yy = None
    if y is not None:
        yy = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
        if np.shape(y) != shape:
            raise ValueError("%s: y is %s, the cells are %s" % (who, np.shape(y), shape))
        if not np.all(np.isfinite(yy)):
            raise ValueError("%s: y holds NaN or infinite values" % who)
    quant = np.empty((len(pr), n_cols)) if len(pr) else None
    mean = np.empty(n_cols)
    crps = np.empty(n_cols) if yy is not None else None
    if n_cols:
        lib, dev = _lib()
        _chk(lib, lib.npbnn_op_mixture(dev, v.ctypes.data, sg.ctypes.data, kind, n_samples, n_cols, n_cols, sigma_cols,
                                       capi.dptr(pr) if len(pr) else None, len(pr), capi.dptr(yy), capi.dptr(quant), capi.dptr(mean),
                                       capi.dptr(crps)))
    return (None if quant is None else quant.reshape((len(pr),) + shape), mean.reshape(shape),
            None if crps is None else crps.reshape(shape))


def convergence(values, n_chains=1):
    """npbnn_op_convergence on a [S, n_cols] array, ``n_chains`` chains of S / n_chains draws in chain-major order: (rhat, ess) as
    float64 [n_cols], NaN in a constant column (npbnn_amd/convergence.py has the definition).  float32 stays float32 on its way to
    the device, anything else is taken as float64; the arithmetic is float64 either way."""
    from .convergence import check_shape
    a = np.asarray(values)
    if a.ndim != 2:
        raise ValueError("convergence: values must be [samples, columns], got shape %s" % (a.shape,))
    v, kind = capi.value_array(a)
    n_draws = check_shape("convergence", v.shape[0], n_chains)
    n_cols = v.shape[1]
    rhat, ess = np.empty(n_cols), np.empty(n_cols)
    if n_cols == 0:
        return rhat, ess
    lib, dev = _lib()
    _chk(lib, lib.npbnn_op_convergence(dev, v.ctypes.data, kind, int(n_chains), n_draws, n_cols, n_cols, capi.dptr(rhat), capi.dptr(ess)))
    return rhat, ess


def psis(log_lik):
    """npbnn_op_psis on a [S, n_cols] array of log-likelihoods: (elpd_loo_i, lppd_i, pareto_k) as float64 [n_cols]
    (npbnn_amd/loo.py has the definition).  float32 stays float32 on its way to the device, anything else is taken as float64; the
    arithmetic is float64 either way."""
    from .loo import check_samples
    a = np.asarray(log_lik)
    if a.ndim != 2:
        raise ValueError("psis: log_lik must be [samples, columns], got shape %s" % (a.shape,))
    v, kind = capi.value_array(a)
    check_samples(v.shape[0], "psis")
    if not np.all(np.isfinite(v)):
        raise ValueError("psis: log_lik holds NaN or infinite values")
    n_cols = v.shape[1]
    elpd, lppd, k = np.empty(n_cols), np.empty(n_cols), np.empty(n_cols)
    if n_cols == 0:
        return elpd, lppd, k
    lib, dev = _lib()
    _chk(lib, lib.npbnn_op_psis(dev, v.ctypes.data, kind, v.shape[0], n_cols, n_cols, capi.dptr(elpd), capi.dptr(lppd), capi.dptr(k)))
    return elpd, lppd, k
