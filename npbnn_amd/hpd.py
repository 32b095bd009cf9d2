"""Highest-posterior-density intervals: ``calcHPD``, ``posterior_hpd``, ``get_posterior_hpd`` (reference: np_bnn/BNN_lib.py:286-302;
its summary code applies calcHPD once per prediction row, BNN_plot.py:73-75).

calcHPD sorts S values, takes ``nIn = int(round(level * S))`` of them and returns the bounds of the first narrowest window of
``nIn`` consecutive sorted values.  Here every column of a sample stack is one launch of ``npbnn_op_hpd``, and
``get_posterior_hpd`` replays the stored samples into a float32 stack that stays on the device (``npbnn_predict_sets_hpd``): only
the mean and the two bounds per (row, output) come back.  Differences from upstream: a NaN or infinite value raises
``ValueError`` (upstream's sort is then order-dependent), and at most 16384 samples are taken.  Window widths are computed in the
input's type for float32 input and in float64 for anything else."""
import os
import sys

import numpy as np

from . import _capi as capi
from .files import load_obj

MAX_SAMPLES = 16384
STACK_BYTES = 1 << 30         # default budget of the device stack of get_posterior_hpd (NPBNN_HPD_STACK_BYTES overrides it)


def _window(n_samples, level):
    """calcHPD's argument checks, in its order, then this package's limit on the number of samples."""
    assert (0 < level < 1)
    n_in = int(round(level * n_samples))
    if n_in < 2:
        sys.exit('\n\nToo little data to calculate marginal parameters.')
    if n_samples > MAX_SAMPLES:
        raise ValueError("calcHPD: %d samples, at most %d are supported" % (n_samples, MAX_SAMPLES))
    return n_in


def _values(a):
    """float32 stays float32 (widths in float32, as upstream on a float32 array); anything else is taken as float64."""
    v = capi.value_array(a)[0]
    if not np.all(np.isfinite(v)):
        raise ValueError("calcHPD: the data hold NaN or infinite values")
    return v


def _op_hpd(values, level):
    """npbnn_op_hpd on a contiguous [S, n_cols] float32 / float64 array: (lower, upper) as float64 [n_cols]."""
    from .device_ops import _lib
    n_samples, n_cols = values.shape
    lo, hi = np.empty(n_cols), np.empty(n_cols)
    if n_cols == 0:
        return lo, hi
    lib, dev = _lib()
    values, kind = capi.value_array(values)
    capi.check(lib, None, lib.npbnn_op_hpd(dev, values.ctypes.data, kind, n_samples, n_cols, n_cols, float(level),
                                           capi.dptr(lo), capi.dptr(hi)))
    return lo, hi


def calcHPD(data, level):
    """The highest-posterior-density interval of the 1-D sequence ``data`` at ``level``: ``(lower, upper)``, two scalars of the
    input's type (np_bnn/BNN_lib.py:286-302)."""
    a = np.asarray(data)
    if a.ndim != 1:
        raise ValueError("calcHPD: data must be one-dimensional, got shape %s" % (a.shape,))
    _window(len(a), level)
    v = _values(a)
    lo, hi = _op_hpd(v.reshape(len(v), 1), level)
    return a.dtype.type(lo[0]), a.dtype.type(hi[0])


def posterior_hpd(samples, level=0.95):
    """calcHPD along the first axis of ``samples`` [S, ...], in one device call: ``(lower, upper)``, each of shape [...] and of the
    input's type (float32 stays float32, anything else is float64)."""
    a = np.asarray(samples)
    if a.ndim < 1:
        raise ValueError("posterior_hpd: samples must have a leading sample axis")
    _window(a.shape[0], level)
    v = _values(a.reshape(a.shape[0], -1))
    lo, hi = _op_hpd(v, level)
    return lo.astype(v.dtype).reshape(a.shape[1:]), hi.astype(v.dtype).reshape(a.shape[1:])


def stack_budget():
    """Bytes the float32 device stack [samples, rows, outputs] of one npbnn_predict_sets_hpd may take."""
    try:
        v = int(os.environ.get("NPBNN_HPD_STACK_BYTES", "0"))
    except ValueError:
        v = 0
    return v if v > 0 else STACK_BYTES


def stack_rows(n_samples, n_out):
    """Rows of a table whose float32 device stack [samples, rows, outputs] fits ``stack_budget``."""
    return max(1, stack_budget() // (n_samples * n_out * 4))


def _hpd_row_blocks(blocks, post_samples, actFun, output_act_fun, level):
    """[(mean, lower, upper)] for each block of rows of a feature matrix, every stored sample replayed on it (the device seam).
    One device context serves every block: its matrix is replaced, the packed samples stay."""
    from .posterior import _SamplePredictor
    with _SamplePredictor(blocks[0].shape[1], post_samples, actFun, output_act_fun) as pred:
        return [pred.predict_hpd(b, level) for b in blocks]


def _rows_hpd(matrix, samples, act, output_act_fun, level, n_out):
    """(mean, lower, upper) [rows, n_out] of the stored samples' predictions on ``matrix``, in row blocks whose stack fits the
    budget."""
    if len(matrix) == 0:
        return np.zeros((0, n_out)), np.zeros((0, n_out)), np.zeros((0, n_out))
    x = np.asarray(matrix, dtype=np.float64)
    rows = stack_rows(len(samples), n_out)
    blocks = [x[r:r + rows] for r in range(0, len(x), rows)]
    parts = _hpd_row_blocks(blocks, samples, act, output_act_fun, level)
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def get_posterior_hpd(pkl_file, level=0.95, features=None):
    """Posterior mean and HPD interval of every stored sample's predictions of a checkpoint, on the predictions
    ``get_posterior_est`` computes (per-sample slopes, the last sample's slopes left installed, no data transform).  Keys:
    ``prm_mean``, ``lower``, ``upper`` [row, output] on the training matrix, the same with ``_test`` on the test matrix, and
    ``error_prm``.  With ``features`` the intervals are for that matrix and the ``_test`` keys are left out."""
    model, _, logger = load_obj(pkl_file)
    samples = logger._post_weight_samples
    _window(len(samples), level)
    act = model._act_fun
    act.reset_prm(samples[-1]['alphas'])          # (upstream leaves the last sample's slopes installed)
    n_out = len(samples[0]['weights'][-1])
    out_fn = model._output_act_fun
    res = {}
    if features is None:
        res['prm_mean'], res['lower'], res['upper'] = _rows_hpd(model._data, samples, act, out_fn, level, n_out)
        res['prm_mean_test'], res['lower_test'], res['upper_test'] = _rows_hpd(model._test_data, samples, act, out_fn, level, n_out)
    else:
        res['prm_mean'], res['lower'], res['upper'] = _rows_hpd(features, samples, act, out_fn, level, n_out)
    res['error_prm'] = [s['error_prm'] for s in samples] if 'error_prm' in samples[0] else []
    return res
