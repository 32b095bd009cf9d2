"""Device context of one chain: thin object wrapper over the C ABI.

``HipContext`` owns one ``npbnn_ctx`` (one HIP stream on one MI355X) holding
the resident training / test matrices and the network description.  All
numerics of the hot path run in the hand-written HIP kernels behind it.
"""
import ctypes as C
import os
from operator import is_ as _is
from time import perf_counter as _now

import numpy as np

from . import _capi as capi
from .stored import sigma_matrix


_PACKED_VIEWS = {}      # id(first layer) -> (the layer arrays, the packed vector they are consecutive views of); strong references: ids stay valid


def note_packed_views(layers, base):
    """``layers`` were just made as the consecutive views of the packed vector ``base`` (the state a device batch returns): the next
    pack_weights of exactly these objects is one copy of ``base``."""
    if len(_PACKED_VIEWS) >= 32:
        _PACKED_VIEWS.clear()
    _PACKED_VIEWS[id(layers[0])] = (tuple(layers), base)


def pack_weights(weights):
    """Concatenate the layer matrices (each row-major) into the packed float64 vector the C ABI takes (always a fresh array).
    Layers that are consecutive views of one packed vector - what a device batch leaves in the model - are copied in one piece;
    a set of layer objects once found to be such views is recognised by identity afterwards (a view cannot be moved)."""
    first = weights[0]
    known = _PACKED_VIEWS.get(id(first))
    if known is not None and len(known[0]) == len(weights) and all(map(_is, known[0], weights)):
        return known[1].copy()
    base = getattr(first, "base", None)
    if (isinstance(base, np.ndarray) and base.ndim == 1 and base.dtype == np.float64 and base.flags.c_contiguous
            and base.size == sum(w.size for w in weights)):
        at = base.ctypes.data
        for w in weights:
            if w.base is not base or w.dtype != np.float64 or not w.flags.c_contiguous or w.ctypes.data != at:
                break
            at += w.nbytes
        else:
            if len(_PACKED_VIEWS) >= 32:
                _PACKED_VIEWS.clear()
            _PACKED_VIEWS[id(first)] = (tuple(weights), base)
            return base.copy()
    return np.concatenate([np.ascontiguousarray(w, dtype=np.float64).ravel() for w in weights])


def one_vector(x, copy=False):
    """One weight vector or mask as the C ABI takes it: a list of per-layer matrices is packed (a fresh array), anything else is
    the packed float64 vector itself - copied when ``copy``, for the entries that write the new state into it."""
    if isinstance(x, (list, tuple)):
        return pack_weights(x)
    x = capi.as_f64(x)
    return x.copy() if copy else x


_NO_SIGMA = np.zeros(0)


def _addr(a):
    """Address of an array's first element (a third of the cost of ``a.ctypes.data``, which builds a helper object per use)."""
    try:
        return C.addressof(C.c_char.from_buffer(a))
    except (TypeError, ValueError):          # read-only or empty buffers
        return a.ctypes.data


def default_device():
    """Device of this process: NPBNN_DEVICE, else LOCAL_RANK (one process per
    GPU under torch.distributed.run), else 0."""
    for key in ("NPBNN_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(key)
        if v is not None and v != "":
            return int(v)
    return 0


class HipContext:
    def __init__(self, device=None):
        self._lib = capi.load_library()
        self._ctx = capi._P()
        dev = default_device() if device is None else int(device)
        n = C.c_int(0)
        rc = self._lib.npbnn_device_count(C.byref(n))
        if rc != 0 or n.value < 1:
            raise capi.BackendUnavailable("no HIP device visible: the npbnn_amd hot path needs an MI355X "
                                          "(there is no CPU fallback)")
        capi.check(self._lib, None, self._lib.npbnn_create(dev % n.value, C.byref(self._ctx)))
        self.device = dev % n.value
        opt = os.environ.get("NPBNN_L0", "").lower()
        if opt in ("f32", "f16", "auto"):
            self.set_l0_precision(opt)
        self.arch = None
        self.n_rows = {}
        self.n_out = None
        self.seconds_in_chain_run = 0.0
        self.sync_fallbacks = 0      # batches of the (opt-in) two-stream schedule that timed out and were repeated on one stream

    # -- lifecycle --------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self._lib.npbnn_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        capi.check(self._lib, self._ctx, rc)

    # -- options ----------------------------------------------------------------------
    def set_l0_precision(self, mode):
        """'auto' (default): fp16-split first layer when the data allows, else float32 - a launch whose weights leave the fp16 range
        is repeated on float32; 'f32'; 'f16': the fp16 pair and nothing else - data it cannot hold, or a weight that leaves its range
        in an evaluation, a replay or a chain batch (``chain_run``, ``chains_run_batched``, and with them ``MCMC.run_steps``), raises
        NPBNN_E_RANGE instead of repeating."""
        value = {"auto": capi.L0_AUTO, "f32": capi.L0_F32, "f16": capi.L0_F16}[mode]
        self._chk(self._lib.npbnn_set_option(self._ctx, capi.OPT_L0_PRECISION, value))

    def l0_option(self):
        """The layer-0 precision asked for (the library's own record): 'auto', 'f32' or 'f16'."""
        return {capi.L0_AUTO: "auto", capi.L0_F32: "f32", capi.L0_F16: "f16"}[self.info(capi.INFO_L0_OPTION)]

    def set_fast_tails(self, on):
        """Shape-specialised builds of the evaluation kernel for likelihood-only launches (default on; same results)."""
        self._chk(self._lib.npbnn_set_option(self._ctx, capi.OPT_FAST_TAILS, 1 if on else 0))

    def set_trainable_slopes(self, on):
        """Reserve a slot per hidden layer in the weight image for the activation slope, so that the candidates of a chain pass
        can each carry their own (ActFun(trainable=True) on the device chain); such a network runs on the general builds."""
        on = bool(on)
        if on != getattr(self, "_trainable_slopes", False):
            self._chk(self._lib.npbnn_set_option(self._ctx, capi.OPT_TRAINABLE_SLOPES, 1 if on else 0))
            self._trainable_slopes = on

    def set_row_shard(self, comm_handle, gather_cb, rank, n_ranks, n_rows_total):
        """npbnn_set_row_shard: ``comm_handle`` an npbnn_comm* (ctypes void pointer) or None, ``gather_cb`` a capi.GATHER_FN or None."""
        cb = C.cast(gather_cb, C.c_void_p) if gather_cb is not None else None
        self._chk(self._lib.npbnn_set_row_shard(self._ctx, comm_handle, cb, None, int(rank), int(n_ranks), int(n_rows_total)))

    def set_wide(self, on):
        """Run every network of this context on the weight-streamed path (layers as tiled matrix products, weights streamed from
        HBM), not only those the LDS-resident path cannot hold (layers of more than 128 nodes, weight images that crowd out the
        waves): for A/B timing and tests.  Results agree to rounding, not bit for bit."""
        self._chk(self._lib.npbnn_set_option(self._ctx, capi.OPT_WIDE, 1 if on else 0))

    def is_wide(self):
        """Does the architecture set last run on the weight-streamed path?"""
        return bool(self.info(capi.INFO_WIDE))

    def f16_moved_columns(self):
        """(columns of the training matrix whose fp16 scale was moved up because of heavy tails, largest move in powers of two)."""
        return self.info(capi.INFO_F16_MOVED_COLUMNS), self.info(capi.INFO_F16_MAX_MOVE)

    def set_persistent(self, on):
        """May the library pick the persistent form of the overlapped chain schedule by itself (default on)?"""
        self._chk(self._lib.npbnn_set_option(self._ctx, capi.OPT_PERSISTENT, 1 if on else 0))

    def info(self, what):
        out = C.c_int(0)
        self._chk(self._lib.npbnn_get_info(self._ctx, what, C.byref(out)))
        return out.value

    def replay_info(self):
        """(passes over the data the last replay of stored weight sets launched, float32 repeats included; the most sets one of
        them carried): predict_sets and every entry that summarises it."""
        return self.info(capi.INFO_REPLAY_PASSES), self.info(capi.INFO_REPLAY_MAX_GROUP)

    def l0_mode(self):
        """Layer-0 path of the most recent launch: 'f16-split' or 'f32'."""
        return "f16-split" if self.info(capi.INFO_L0_F16) else "f32"

    # -- resident data ----------------------------------------------------------------
    def set_data(self, X, which=capi.TRAIN):
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError("data must be a 2-D matrix")
        if X.dtype == np.float32:
            Xc = np.ascontiguousarray(X)
            self._chk(self._lib.npbnn_set_data_f32(self._ctx, Xc.ctypes.data_as(C.POINTER(C.c_float)),
                                                   X.shape[0], X.shape[1], which))
        else:
            Xc = capi.as_f64(X)
            self._chk(self._lib.npbnn_set_data_f64(self._ctx, capi.dptr(Xc), X.shape[0], X.shape[1], which))
        self.n_rows[which] = X.shape[0]

    def share_data(self, owner):
        """Use the feature matrices (training and test) resident in ``owner`` (another HipContext on the same device)
        instead of uploading copies (npbnn_share_data); labels / targets / row weights are set per context afterwards."""
        self._chk(self._lib.npbnn_share_data(self._ctx, owner._ctx))
        self.n_rows = dict(owner.n_rows) if isinstance(owner.n_rows, dict) else list(owner.n_rows)
        self._data_owner = owner            # (the library keeps the memory alive by itself; this is for introspection)

    def set_labels(self, labels, which=capi.TRAIN):
        lab = np.ascontiguousarray(labels, dtype=np.int64)
        self._chk(self._lib.npbnn_set_labels_i64(self._ctx, lab.ctypes.data_as(C.POINTER(C.c_int64)), lab.shape[0], which))

    def set_targets(self, targets, which=capi.TRAIN):
        t = capi.as_f64(targets)
        if t.ndim == 1:
            t = t.reshape(-1, 1)
        self._chk(self._lib.npbnn_set_targets_f64(self._ctx, capi.dptr(t), t.shape[0], t.shape[1], which))

    def set_row_weights(self, instance_w=None, class_w=None):
        iw = None if instance_w is None else capi.as_f64(instance_w)
        cw = None if class_w is None or len(class_w) == 0 else capi.as_f64(class_w)
        self._chk(self._lib.npbnn_set_row_weights(self._ctx, capi.dptr(iw), 0 if iw is None else iw.shape[0],
                                                  capi.dptr(cw), 0 if cw is None else cw.shape[0]))

    def set_arch(self, in_dim, out_dims, has_bias, act_kind, out_kind, lik_kind, n_targets=0, final_activation=False):
        if len(out_dims) > capi.MAX_LAYERS:
            raise capi.NpbnnError(-1, "at most %d layers are supported" % capi.MAX_LAYERS)
        a = capi.Arch()
        a.n_layers = len(out_dims)
        a.in_dim = int(in_dim)
        for i, (o, b) in enumerate(zip(out_dims, has_bias)):
            a.out_dim[i] = int(o)
            a.has_bias[i] = int(bool(b))
        a.act_kind, a.out_kind, a.lik_kind, a.n_targets = int(act_kind), int(out_kind), int(lik_kind), int(n_targets)
        a.final_act = 1 if final_activation else 0
        self._chk(self._lib.npbnn_set_arch(self._ctx, C.byref(a)))
        self.arch = a
        self.n_out = int(out_dims[-1])

    def set_layer_mask(self, mask):
        """Declare the 0/1 mask of the network (list of per-layer matrices, a packed vector, or None for dense): blocks of the
        first layer in which it is all zero cost neither device memory nor matrix-core work (npbnn_set_layer_mask).  Weights
        passed afterwards must be zero where the mask is."""
        m = None if mask is None else one_vector(mask)
        self._chk(self._lib.npbnn_set_layer_mask(self._ctx, capi.dptr(m)))

    def set_arch_from_weights(self, weights, in_dim, act_kind, out_kind, lik_kind, n_targets=0, final_activation=False):
        """Derive layer sizes and bias flags from the weight shapes: layer l has a
        bias iff its matrix has in_l + 1 columns (reference: BNN_lib.py:157-161)."""
        out_dims, has_bias = [], []
        cur = in_dim
        for w in weights:
            out_dims.append(w.shape[0])
            if w.shape[1] == cur:
                has_bias.append(0)
            elif w.shape[1] == cur + 1:
                has_bias.append(1)
            else:
                raise ValueError("weight matrix with %d columns does not match %d inputs" % (w.shape[1], cur))
            cur = w.shape[0]
        self.set_arch(in_dim, out_dims, has_bias, act_kind, out_kind, lik_kind, n_targets, final_activation)

    # -- hot path ---------------------------------------------------------------------
    def eval(self, weights, act_prm=None, col_override=None, lik_temp=1.0, sigma=None, which=capi.TRAIN,
             want_confusion=False):
        w = one_vector(weights)
        ap = None if act_prm is None else capi.as_f64(act_prm)
        co = None if col_override is None else capi.as_f64(col_override)
        sg = None if sigma is None else capi.as_f64(np.broadcast_to(sigma, (self.arch.n_targets,)))
        out = capi.EvalOut()
        conf = None
        cptr = None
        if want_confusion:
            conf = np.zeros((self.n_out, self.n_out), dtype=np.int64)
            cptr = conf.ctypes.data_as(C.POINTER(C.c_int64))
        self._chk(self._lib.npbnn_eval(self._ctx, capi.dptr(w), capi.dptr(ap), capi.dptr(co), float(lik_temp),
                                       capi.dptr(sg), which, C.byref(out), cptr))
        k = self.arch.n_targets
        return dict(loglik=out.loglik, sigma=np.array(out.sigma[:k]), sum_r=np.array(out.sum_r[:k]),
                    sum_r2=np.array(out.sum_r2[:k]), n_rows=out.n_rows, confusion=conf)

    def loglik_grad(self, weights, act_prm=None, col_override=None, lik_temp=1.0, sigma=None, which=capi.TRAIN):
        """``(eval dict, [gradient per layer])``: the log-likelihood as :meth:`eval` returns it (no confusion counts) and its
        gradient with respect to every weight, shaped like ``weights`` (npbnn_loglik_grad).  ``weights``: the per-layer matrices.
        Categorical, Gaussian with ``sigma`` given, and predicted-sigma likelihoods."""
        shapes = [np.shape(x) for x in weights]
        w = one_vector(list(weights))
        ap = None if act_prm is None else capi.as_f64(act_prm)
        co = None if col_override is None else capi.as_f64(col_override)
        sg = None if sigma is None else capi.as_f64(np.broadcast_to(sigma, (self.arch.n_targets,)))
        out = capi.EvalOut()
        grad = np.zeros(w.size, dtype=np.float64)
        self._chk(self._lib.npbnn_loglik_grad(self._ctx, capi.dptr(w), capi.dptr(ap), capi.dptr(co), float(lik_temp), capi.dptr(sg), which,
                                              C.byref(out), capi.dptr(grad)))
        k = self.arch.n_targets
        layers, at = [], 0
        for sh in shapes:
            n = int(np.prod(sh))
            layers.append(grad[at:at + n].reshape(sh))
            at += n
        return (dict(loglik=out.loglik, sigma=np.array(out.sigma[:k]), sum_r=np.array(out.sum_r[:k]), sum_r2=np.array(out.sum_r2[:k]),
                     n_rows=out.n_rows, confusion=None), layers)

    def predict(self, weights, act_prm=None, col_override=None, which=capi.TRAIN, apply_out_fn=True):
        w = one_vector(weights)
        ap = None if act_prm is None else capi.as_f64(act_prm)
        co = None if col_override is None else capi.as_f64(col_override)
        y = np.empty((self.n_rows[which], self.n_out), dtype=np.float64)
        self._chk(self._lib.npbnn_predict(self._ctx, capi.dptr(w), capi.dptr(ap), capi.dptr(co), which,
                                          1 if apply_out_fn else 0, capi.dptr(y)))
        return y

    def _pack_sets(self, weight_sets, act_prm_sets, who):
        """What every stored-sample entry hands the library: ``(packed, ap, n_sets)``.  ``packed`` [n_sets, n_w] float64 is
        ``weight_sets`` itself when that is such a matrix, else its items - per-layer lists or packed vectors - stacked; ``ap``
        [n_sets, n_layers - 1] float64 holds the hidden layers' slopes per set, or is None (no ``act_prm_sets``, or no hidden
        layer).  ``ValueError`` in ``who``'s name for no sets and for a number of slope vectors other than the number of sets:
        the library reads one per set."""
        if len(weight_sets) == 0:
            raise ValueError("%s: no weight sets" % who)
        if not (isinstance(weight_sets, np.ndarray) and weight_sets.ndim == 2):
            weight_sets = np.stack([pack_weights(w) if isinstance(w, (list, tuple)) else capi.as_f64(w).ravel() for w in weight_sets])
        packed = capi.as_f64(weight_sets)
        n_sets, n_hidden = packed.shape[0], self.arch.n_layers - 1
        ap = None
        if act_prm_sets is not None and n_hidden > 0:
            if len(act_prm_sets) != n_sets:
                raise ValueError("%s: %d slope vectors for %d weight sets" % (who, len(act_prm_sets), n_sets))
            ap = capi.as_f64(np.stack([np.asarray(a, dtype=np.float64).ravel()[:n_hidden] for a in act_prm_sets]))
        return packed, ap, n_sets

    def predict_sets(self, weight_sets, act_prm_sets=None, which=capi.TRAIN, apply_out_fn=True):
        """Predictions of several weight sets on the resident matrix (npbnn_predict_sets): [n_sets, n_rows, n_out].
        ``weight_sets``: list of per-layer lists (or packed vectors), or the packed matrix; ``act_prm_sets``: per set the
        activation slopes of the hidden layers, or None."""
        packed, ap, n_sets = self._pack_sets(weight_sets, act_prm_sets, "predict_sets")
        out = np.empty((n_sets, self.n_rows[which], self.n_out), dtype=np.float64)
        self._chk(self._lib.npbnn_predict_sets(self._ctx, capi.dptr(packed), capi.dptr(ap), n_sets, which,
                                               1 if apply_out_fn else 0, capi.dptr(out)))
        return out

    def predict_sets_hpd(self, weight_sets, level=0.95, act_prm_sets=None, which=capi.TRAIN, apply_out_fn=True):
        """Posterior mean and HPD interval of several weight sets' predictions on the resident matrix (npbnn_predict_sets_hpd):
        ``(mean, lower, upper)``, each [n_rows, n_out].  The sets replay as in ``predict_sets`` into a float32 stack that stays
        on the device; the bounds equal calcHPD's on the float64 array ``predict_sets`` returns."""
        packed, ap, n_sets = self._pack_sets(weight_sets, act_prm_sets, "predict_sets_hpd")
        shape = (self.n_rows[which], self.n_out)
        mean, lo, hi = np.empty(shape), np.empty(shape), np.empty(shape)
        self._chk(self._lib.npbnn_predict_sets_hpd(self._ctx, capi.dptr(packed), capi.dptr(ap), n_sets, which,
                                                   1 if apply_out_fn else 0, float(level), capi.dptr(mean), capi.dptr(lo),
                                                   capi.dptr(hi)))
        return mean, lo, hi

    def permute_columns(self, cols, perms, which=capi.TRAIN):
        """Shuffle columns of the resident matrix between its rows, on the device (npbnn_permute_columns): column ``cols[j]`` reads
        ``X0[perms[p][r], cols[j]]`` in row ``r``, ``X0`` being the matrix as ``set_data`` left it - ``perms`` [1, n_rows] moves the
        block as a whole, [len(cols), n_rows] every column by its own permutation.  The columns an earlier call moved go back
        first; no columns (or ``perms`` None) only puts them back."""
        c = np.ascontiguousarray(np.asarray(cols, dtype=np.int64).ravel(), dtype=np.int32)
        if perms is None or len(c) == 0:
            self._chk(self._lib.npbnn_permute_columns(self._ctx, which, None, 0, None, 0))
            return
        p = np.ascontiguousarray(perms, dtype=np.int64)
        if p.ndim == 1:
            p = p.reshape(1, -1)
        if p.ndim != 2 or p.shape[0] not in (1, len(c)):
            raise ValueError("permute_columns: %s permutations for %d columns (one for the block, or one per column)" % (p.shape[:-1], len(c)))
        if p.shape[1] != self.n_rows[which]:
            raise ValueError("permute_columns: permutations of %d rows but the matrix has %d" % (p.shape[1], self.n_rows[which]))
        self._chk(self._lib.npbnn_permute_columns(self._ctx, which, c.ctypes.data_as(C.POINTER(C.c_int32)), len(c),
                                                  p.ctypes.data_as(C.POINTER(C.c_int64)), p.shape[0]))

    def predict_sets_summary(self, weight_sets, mode, labels=None, act_prm_sets=None, which=capi.TRAIN, want_summary=True,
                             apply_out_fn=True):
        """Summary over several weight sets' predictions on the resident matrix, and its confusion table against ``labels``
        (npbnn_predict_sets_summary): ``(summary [n_rows, n_out] or None, confusion [n_out, n_out] int64 or None)``.  ``mode`` 0:
        the share of the sets whose largest prediction is the class; 1: the mean prediction.  The sets replay as in
        ``predict_sets``; the per-set predictions stay on the device."""
        if mode not in (0, 1):
            raise ValueError("predict_sets_summary: mode must be 0 (votes) or 1 (mean)")
        if labels is None and not want_summary:
            raise ValueError("predict_sets_summary: nothing asked for (no labels and want_summary off)")
        packed, ap, n_sets = self._pack_sets(weight_sets, act_prm_sets, "predict_sets_summary")
        lab = conf = summary = None
        if labels is not None:
            lab = np.ascontiguousarray(labels, dtype=np.int64).ravel()
            if lab.shape[0] != self.n_rows[which]:
                raise ValueError("predict_sets_summary: %d labels but the matrix has %d rows" % (lab.shape[0], self.n_rows[which]))
            conf = np.zeros((self.n_out, self.n_out), dtype=np.int64)
        if want_summary:
            summary = np.empty((self.n_rows[which], self.n_out), dtype=np.float64)
        i64 = C.POINTER(C.c_int64)
        self._chk(self._lib.npbnn_predict_sets_summary(self._ctx, capi.dptr(packed), capi.dptr(ap), n_sets, which,
                                                       1 if apply_out_fn else 0, int(mode),
                                                       None if lab is None else lab.ctypes.data_as(i64), capi.dptr(summary),
                                                       None if conf is None else conf.ctypes.data_as(i64)))
        return summary, conf

    def predict_sets_support(self, weight_sets, mode, labels, thresholds, prior_summary=None, bf_thresholds=(), cutoff=None,
                             act_prm_sets=None, which=capi.TRAIN, want_summary=False, want_keep=False, apply_out_fn=True):
        """Confidence-threshold and Bayes-factor support of the summary over several weight sets' predictions on the resident
        matrix (npbnn_predict_sets_support).  Per row, ``p`` the largest summary value and ``k`` its (first) class:
        ``cube`` [len(thresholds) + 1, n_out, n_out] int64 counts the row in ``[b, label, k]``, ``b`` the number of ``thresholds``
        (float64, ascending) strictly below ``p`` - the rows retained at ``thresholds[i]`` are ``cube[i + 1:]``; with
        ``prior_summary`` [n_rows, n_out], ``bf`` [len(bf_thresholds) + 1, 2] int64 counts it in ``[b, k == label]``, ``b`` the number
        of ``bf_thresholds`` strictly below CalcTP_BF's Bayes factor.  ``cutoff``: rows with ``p > cutoff`` false are NaN in the
        summary and 0 in the keep mask.  Returns a dict with ``cube``, ``bf``, ``summary``, ``keep`` (None where not asked for).
        The sets replay as in ``predict_sets_summary``, whose quotients these are bit for bit."""
        if mode not in (0, 1):
            raise ValueError("predict_sets_support: mode must be 0 (votes) or 1 (mean)")
        if labels is None:
            raise ValueError("predict_sets_support: labels are required")
        packed, ap, n_sets = self._pack_sets(weight_sets, act_prm_sets, "predict_sets_support")
        n_rows, c = self.n_rows[which], self.n_out
        lab = np.ascontiguousarray(labels, dtype=np.int64).ravel()
        if lab.shape[0] != n_rows:
            raise ValueError("predict_sets_support: %d labels but the matrix has %d rows" % (lab.shape[0], n_rows))
        thr = capi.as_f64(np.asarray(thresholds, dtype=np.float64).ravel())
        bft = capi.as_f64(np.asarray(bf_thresholds, dtype=np.float64).ravel())
        for name, t in (("thresholds", thr), ("bf_thresholds", bft)):
            if np.any(np.isnan(t)) or np.any(np.diff(t) < 0):
                raise ValueError("predict_sets_support: %s must ascend and hold no NaN" % name)
        prior = bf = None
        if prior_summary is not None:
            prior = capi.as_f64(prior_summary)
            if prior.shape != (n_rows, c):
                raise ValueError("predict_sets_support: prior_summary is %s, the summary %s" % (prior.shape, (n_rows, c)))
            bf = np.zeros((len(bft) + 1, 2), dtype=np.int64)
        elif len(bft):
            raise ValueError("predict_sets_support: bf_thresholds without prior_summary")
        if cutoff is not None and np.isnan(cutoff):
            raise ValueError("predict_sets_support: the cutoff is NaN")
        cube = np.zeros((len(thr) + 1, c, c), dtype=np.int64)
        summary = np.empty((n_rows, c), dtype=np.float64) if want_summary else None
        keep = np.empty(n_rows, dtype=np.uint8) if want_keep else None
        cut = None if cutoff is None else C.c_double(float(cutoff))
        i64 = C.POINTER(C.c_int64)
        self._chk(self._lib.npbnn_predict_sets_support(
            self._ctx, capi.dptr(packed), capi.dptr(ap), n_sets, which, 1 if apply_out_fn else 0, int(mode), lab.ctypes.data_as(i64),
            capi.dptr(thr) if len(thr) else None, len(thr), capi.dptr(prior), capi.dptr(bft) if len(bft) else None, len(bft),
            None if cut is None else C.cast(C.byref(cut), capi._DP), cube.ctypes.data_as(i64), None if bf is None else bf.ctypes.data_as(i64),
            capi.dptr(summary), None if keep is None else keep.ctypes.data_as(C.POINTER(C.c_uint8))))
        return dict(cube=cube, bf=bf, summary=summary, keep=None if keep is None else keep.astype(bool))

    def predict_sets_lppd(self, weight_sets, lik_kind, sigma_sets=None, act_prm_sets=None, which=capi.TRAIN, pointwise=True):
        """Log pointwise predictive density and WAIC terms of several weight sets on the resident matrix, against the labels
        (``lik_kind`` LIK_CATEGORICAL) or targets (LIK_GAUSS, ``sigma_sets`` [n_sets, n_targets] or [n_sets]) set on it
        (npbnn_predict_sets_lppd).  With ``ll[s, i]`` the log-likelihood of row ``i`` under set ``s``: a dict with the totals
        ``lppd`` (sum of ``logsumexp_s ll - log S``), ``mean_log_lik`` (sum of ``mean_s ll``), ``p_waic`` (sum of ``var_s ll``,
        ddof 1), ``log_lik_sample`` [n_sets] (``sum_i ll``), and with ``pointwise`` the three [n_rows] arrays ``lppd_i``,
        ``mean_log_lik_i``, ``p_waic_i`` (None otherwise).  The sets replay as in ``predict_sets_summary``; ``ll`` never leaves
        the device."""
        if lik_kind not in (capi.LIK_CATEGORICAL, capi.LIK_GAUSS):
            raise ValueError("predict_sets_lppd: lik_kind must be LIK_CATEGORICAL or LIK_GAUSS (predicted-sigma regression and the "
                             "count likelihoods are out of scope), got %r" % (lik_kind,))
        packed, ap, n_sets = self._pack_sets(weight_sets, act_prm_sets, "predict_sets_lppd")
        n_rows = self.n_rows[which]
        if n_rows < 1:
            raise ValueError("predict_sets_lppd: the matrix has no rows")
        sig = None
        if lik_kind == capi.LIK_GAUSS:
            if sigma_sets is None:
                raise ValueError("predict_sets_lppd: the Gaussian likelihood needs sigma_sets")
            sig = sigma_matrix(sigma_sets, n_sets, self.n_out, "predict_sets_lppd")
        elif sigma_sets is not None:
            raise ValueError("predict_sets_lppd: sigma_sets goes with LIK_GAUSS only")
        point = [np.empty(n_rows, dtype=np.float64) for _ in range(3)] if pointwise else [None] * 3
        trace = np.empty(n_sets, dtype=np.float64)
        totals = np.zeros(3, dtype=np.float64)
        self._chk(self._lib.npbnn_predict_sets_lppd(self._ctx, capi.dptr(packed), capi.dptr(ap), n_sets, which, int(lik_kind), capi.dptr(sig),
                                                    capi.dptr(point[0]), capi.dptr(point[1]), capi.dptr(point[2]), capi.dptr(trace),
                                                    capi.dptr(totals)))
        return dict(lppd=float(totals[0]), mean_log_lik=float(totals[1]), p_waic=float(totals[2]), log_lik_sample=trace,
                    lppd_i=point[0], mean_log_lik_i=point[1], p_waic_i=point[2])

    def predict_sets_loo(self, weight_sets, lik_kind, sigma_sets=None, act_prm_sets=None, which=capi.TRAIN, log_lik=False):
        """PSIS leave-one-out cross-validation of several weight sets on the resident matrix, against the labels (``lik_kind``
        LIK_CATEGORICAL) or targets (LIK_GAUSS, ``sigma_sets`` [n_sets, n_targets] or [n_sets]) set on it
        (npbnn_predict_sets_loo; ``npbnn_amd.loo`` has the definition).  A dict with the pointwise ``elpd_loo_i``, ``lppd_i`` and
        ``pareto_k`` [n_rows], ``log_lik_sample`` [n_sets] and, with ``log_lik``, the float64 matrix ``log_lik`` [n_sets, n_rows]
        (None otherwise).  The sets replay as in ``predict_sets_lppd``; the matrix stays on the device unless asked for, under
        the byte budget of ``predict_sets_hpd``'s stack (NpbnnError E_NOMEM names the rows that fit)."""
        from .loo import check_samples
        who = "predict_sets_loo"
        if lik_kind not in (capi.LIK_CATEGORICAL, capi.LIK_GAUSS):
            raise ValueError("%s: lik_kind must be LIK_CATEGORICAL or LIK_GAUSS (predicted-sigma regression and the count likelihoods "
                             "are out of scope), got %r" % (who, lik_kind))
        packed, ap, n_sets = self._pack_sets(weight_sets, act_prm_sets, who)
        check_samples(n_sets, who)
        n_rows = self.n_rows[which]
        if n_rows < 1:
            raise ValueError("%s: the matrix has no rows" % who)
        sig = None
        if lik_kind == capi.LIK_GAUSS:
            if sigma_sets is None:
                raise ValueError("%s: the Gaussian likelihood needs sigma_sets" % who)
            sig = sigma_matrix(sigma_sets, n_sets, self.n_out, who)
        elif sigma_sets is not None:
            raise ValueError("%s: sigma_sets goes with LIK_GAUSS only" % who)
        elpd, lppd, k = (np.empty(n_rows, dtype=np.float64) for _ in range(3))
        trace = np.empty(n_sets, dtype=np.float64)
        matrix = np.empty((n_sets, n_rows), dtype=np.float64) if log_lik else None
        self._chk(self._lib.npbnn_predict_sets_loo(self._ctx, capi.dptr(packed), capi.dptr(ap), n_sets, which, int(lik_kind), capi.dptr(sig),
                                                   capi.dptr(elpd), capi.dptr(lppd), capi.dptr(k), capi.dptr(trace), capi.dptr(matrix)))
        return dict(elpd_loo_i=elpd, lppd_i=lppd, pareto_k=k, log_lik_sample=trace, log_lik=matrix)

    def predict_sets_uncertainty(self, weight_sets, act_prm_sets=None, which=capi.TRAIN, pointwise=True):
        """Uncertainty decomposition of several weight sets' predictions on the resident matrix (npbnn_predict_sets_uncertainty); the
        kind follows the architecture's output function, and no labels or targets are read.  Softmax: a dict with ``mean_prob``
        [n_rows, n_out], ``predicted_class`` (its first argmax), ``predictive_entropy_i``, ``expected_entropy_i``,
        ``mutual_information_i`` [n_rows] and their means over the rows ``predictive_entropy``, ``expected_entropy``,
        ``mutual_information``.  Regression (T targets: n_out under OUT_IDENTITY, n_out / 2 under OUT_SOFTPLUS_HALF): ``mean``,
        ``epistemic_var``, ``aleatoric_var``, ``total_var`` [n_rows, T] and their means over the rows ``mean_avg``, ... [T];
        OUT_IDENTITY predicts no sigma, and its ``aleatoric_var*`` and ``total_var*`` are None (the caller adds its own).  Without
        ``pointwise`` every [n_rows, ...] array is None and is not copied from the device.  The sets replay as in
        ``predict_sets_lppd``; the predictions never leave the device."""
        packed, ap, n_sets = self._pack_sets(weight_sets, act_prm_sets, "predict_sets_uncertainty")
        n_rows, n_out, kind = self.n_rows[which], self.n_out, self.arch.out_kind
        if n_rows < 1:
            raise ValueError("predict_sets_uncertainty: the matrix has no rows")
        if kind == capi.OUT_SOFTPLUS_HALF and n_out % 2:
            raise ValueError("predict_sets_uncertainty: OUT_SOFTPLUS_HALF splits the outputs into means and sigmas, and %d is odd" % n_out)
        softmax, sigma = kind == capi.OUT_SOFTMAX, kind == capi.OUT_SOFTPLUS_HALF
        t = 1 if softmax else (n_out // 2 if sigma else n_out)
        col = (n_rows,) if softmax else (n_rows, t)
        # mean, total, aleatoric, epistemic
        point = [None] * 4
        if pointwise:
            point = [np.empty((n_rows, n_out if softmax else t), dtype=np.float64), np.empty(col, dtype=np.float64), np.empty(col, dtype=np.float64),
                     np.empty(col, dtype=np.float64)]
            if not (softmax or sigma):
                point[1] = point[2] = None
        totals = np.zeros(3 if softmax else (4, t), dtype=np.float64)
        self._chk(self._lib.npbnn_predict_sets_uncertainty(self._ctx, capi.dptr(packed), capi.dptr(ap), n_sets, which, capi.dptr(point[0]),
                                                           capi.dptr(point[1]), capi.dptr(point[2]), capi.dptr(point[3]), capi.dptr(totals)))
        avg = totals / n_rows
        if softmax:
            return dict(mean_prob=point[0], predicted_class=None if point[0] is None else np.argmax(point[0], axis=1),
                        predictive_entropy_i=point[1], expected_entropy_i=point[2], mutual_information_i=point[3],
                        predictive_entropy=float(avg[0]), expected_entropy=float(avg[1]), mutual_information=float(avg[2]))
        return dict(mean=point[0], total_var=point[1], aleatoric_var=point[2], epistemic_var=point[3], mean_avg=avg[0],
                    total_var_avg=avg[1] if sigma else None, aleatoric_var_avg=avg[2] if sigma else None, epistemic_var_avg=avg[3])

    def predict_sets_calibration(self, weight_sets, n_bins=15, levels=(0.5, 0.8, 0.9, 0.95), sigma_sets=None, act_prm_sets=None, which=capi.TRAIN,
                                 pointwise=True):
        """Calibration of several weight sets' mean prediction on the resident matrix, against the labels or targets set on it
        (npbnn_predict_sets_calibration); the kind follows the architecture's output function.  Softmax: a dict with the reliability
        table ``count``, ``sum_confidence``, ``n_correct`` [n_bins], the scores ``accuracy``, ``brier``, ``nll``, ``ece``, ``mce``
        and the pointwise ``confidence``, ``predicted_class``, ``brier_i``, ``nll_i`` [n_rows].  Regression (T targets: n_out under
        OUT_IDENTITY with ``sigma_sets`` [n_sets, T] or [n_sets], n_out / 2 under OUT_SOFTPLUS_HALF): ``levels``, ``pit_hist``
        [T, n_bins], ``covered`` [T, L], ``rmse``, ``mean_pit`` [T], ``coverage`` [T, L], ``coverage_error`` [T] (None without
        levels) and the pointwise ``pit``, ``mean``, ``sq_err`` [n_rows, T].  ``npbnn_amd.calibration`` has the definitions; the
        scores come from the tables through its ``scores_from_table``.  Without ``pointwise`` every [n_rows, ...] array is None and
        is not copied from the device.  The sets replay as in ``predict_sets_uncertainty``; the predictions never leave the device."""
        from .calibration import check_bins_and_levels, scores_from_table
        who = "predict_sets_calibration"
        n_bins, lv = check_bins_and_levels(n_bins, levels, who)
        packed, ap, n_sets = self._pack_sets(weight_sets, act_prm_sets, who)
        n_rows, n_out, kind = self.n_rows[which], self.n_out, self.arch.out_kind
        if n_rows < 1:
            raise ValueError("%s: the matrix has no rows" % who)
        if kind == capi.OUT_SOFTPLUS_HALF and n_out % 2:
            raise ValueError("%s: OUT_SOFTPLUS_HALF splits the outputs into means and sigmas, and %d is odd" % (who, n_out))
        softmax = kind == capi.OUT_SOFTMAX
        t = 1 if softmax else (n_out // 2 if kind == capi.OUT_SOFTPLUS_HALF else n_out)
        sig = None
        if kind == capi.OUT_IDENTITY:
            sig = sigma_matrix(sigma_sets, n_sets, t, who)
        elif sigma_sets is not None:
            raise ValueError("%s: sigma_sets goes with OUT_IDENTITY only" % who)
        if softmax:
            lv = lv[:0]                                 # (the levels belong to regression)
        point = [np.empty((n_rows,) if softmax else (n_rows, t), dtype=np.float64) for _ in range(3)] if pointwise else [None] * 3
        pred = np.empty(n_rows, dtype=np.int64) if pointwise and softmax else None
        counts = np.zeros((2, n_bins) if softmax else (t, n_bins + len(lv)), dtype=np.int64)
        bin_sums = np.zeros(n_bins, dtype=np.float64) if softmax else None
        totals = np.zeros(3 if softmax else (2, t), dtype=np.float64)
        i64 = C.POINTER(C.c_int64)
        self._chk(self._lib.npbnn_predict_sets_calibration(
            self._ctx, capi.dptr(packed), capi.dptr(ap), n_sets, which, capi.dptr(sig), n_bins, capi.dptr(lv) if len(lv) else None, len(lv),
            capi.dptr(point[0]), capi.dptr(point[1]), capi.dptr(point[2]), None if pred is None else pred.ctypes.data_as(i64),
            counts.ctypes.data_as(i64), capi.dptr(bin_sums), capi.dptr(totals)))
        res = dict(n_samples=int(n_sets), n_rows=int(n_rows), n_bins=n_bins)
        if softmax:
            table = dict(count=counts[0].copy(), sum_confidence=bin_sums, n_correct=counts[1].copy())
            res.update(table)
            res.update(scores_from_table(dict(table, brier_sum=totals[0], nll_sum=totals[1]), n_rows))
            res.update(confidence=point[0], predicted_class=pred, brier_i=point[1], nll_i=point[2])
            return res
        table = dict(levels=lv, pit_hist=counts[:, :n_bins].copy(), covered=counts[:, n_bins:].copy())
        res.update(table)
        res.update(scores_from_table(dict(table, sq_err_sum=totals[0], pit_sum=totals[1]), n_rows))
        res.update(pit=point[0], mean=point[1], sq_err=point[2])
        return res

    def predict_sets_convergence(self, weight_sets, n_chains=1, rhat_threshold=1.01, act_prm_sets=None, which=capi.TRAIN, apply_out_fn=True,
                                 pointwise=True):
        """Split R-hat and effective sample size of several weight sets' predictions on the resident matrix, per (row, output)
        (npbnn_predict_sets_convergence): the sets are ``n_chains`` chains of equal length, chain-major.  Returns
        ``posterior_convergence``'s dict; without ``pointwise`` ``rhat`` and ``ess`` are None and never leave the device.  The sets
        replay as in ``predict_sets_hpd`` into a float32 stack that stays on the device; the results are the definition's on the
        float64 array ``predict_sets`` returns."""
        from .convergence import check_shape, result_dict
        packed, ap, n_sets = self._pack_sets(weight_sets, act_prm_sets, "predict_sets_convergence")
        n_rows, n_out = self.n_rows[which], self.n_out
        n_draws = check_shape("predict_sets_convergence", n_sets, n_chains)
        if n_rows < 1:
            raise ValueError("predict_sets_convergence: the matrix has no rows")
        rhat = np.empty((n_rows, n_out)) if pointwise else None
        ess = np.empty((n_rows, n_out)) if pointwise else None
        summary = np.zeros((n_out, 4))
        self._chk(self._lib.npbnn_predict_sets_convergence(self._ctx, capi.dptr(packed), capi.dptr(ap), n_sets, int(n_chains), which,
                                                           1 if apply_out_fn else 0, float(rhat_threshold), capi.dptr(rhat), capi.dptr(ess),
                                                           capi.dptr(summary)))
        return result_dict(rhat, ess, summary, n_rows, n_chains, n_draws)

    def predict_sets_predictive(self, weight_sets, probs=(0.025, 0.5, 0.975), sigma_sets=None, targets=None, act_prm_sets=None, which=capi.TRAIN,
                                want_mean=True, want_crps_i=True):
        """The posterior predictive distribution of several weight sets on the resident matrix, per (row, target)
        (npbnn_predict_sets_predictive); the kind follows the architecture's output function: OUT_IDENTITY (T = n_out targets, with
        ``sigma_sets`` [n_sets, T] or [n_sets]) or OUT_SOFTPLUS_HALF (T = n_out / 2, the sigma predicted per row).  A dict with
        ``quantiles`` [len(probs), n_rows, T] (None without probs), ``mean`` [n_rows, T] (None without ``want_mean``) and, with
        ``targets`` [n_rows, T] (float64, sent with the call), ``crps_i`` [n_rows, T] (None without ``want_crps_i``) and
        ``crps_total`` [T], its sum over the rows; both are None without targets.  ``npbnn_amd.predictive`` has the definitions.  The
        sets replay as in ``predict_sets_hpd`` into a float32 stack that stays on the device; the results are the definitions' on
        the float64 array ``predict_sets`` returns."""
        from .predictive import MAX_SAMPLES, check_probs
        who = "predict_sets_predictive"
        pr = check_probs(probs, who)
        packed, ap, n_sets = self._pack_sets(weight_sets, act_prm_sets, who)
        n_rows, n_out, kind = self.n_rows[which], self.n_out, self.arch.out_kind
        if n_sets > MAX_SAMPLES:
            raise ValueError("%s: %d samples, at most %d are supported" % (who, n_sets, MAX_SAMPLES))
        if n_rows < 1:
            raise ValueError("%s: the matrix has no rows" % who)
        if kind not in (capi.OUT_IDENTITY, capi.OUT_SOFTPLUS_HALF):
            raise ValueError("%s: the predictive distribution is that of a regression (OUT_IDENTITY or OUT_SOFTPLUS_HALF)" % who)
        if kind == capi.OUT_SOFTPLUS_HALF and n_out % 2:
            raise ValueError("%s: OUT_SOFTPLUS_HALF splits the outputs into means and sigmas, and %d is odd" % (who, n_out))
        t = n_out // 2 if kind == capi.OUT_SOFTPLUS_HALF else n_out
        sig = None
        if kind == capi.OUT_IDENTITY:
            sig = sigma_matrix(sigma_sets, n_sets, t, who)
        elif sigma_sets is not None:
            raise ValueError("%s: sigma_sets goes with OUT_IDENTITY only" % who)
        tg = None
        if targets is not None:
            from .stored import target_matrix
            tg = np.ascontiguousarray(target_matrix(targets, n_rows, t, who))
        if not len(pr) and not want_mean and tg is None:
            raise ValueError("%s: nothing asked for (no probs, no mean, no targets)" % who)
        quant = np.empty((len(pr), n_rows, t)) if len(pr) else None
        mean = np.empty((n_rows, t)) if want_mean else None
        crps_i = np.empty((n_rows, t)) if tg is not None and want_crps_i else None
        totals = np.zeros(t) if tg is not None else None
        self._chk(self._lib.npbnn_predict_sets_predictive(self._ctx, capi.dptr(packed), capi.dptr(ap), n_sets, which, capi.dptr(sig),
                                                          capi.dptr(pr) if len(pr) else None, len(pr), capi.dptr(tg), capi.dptr(quant),
                                                          capi.dptr(mean), capi.dptr(crps_i), capi.dptr(totals)))
        return dict(quantiles=quant, mean=mean, crps_i=crps_i, crps_total=totals)

    def predict_pdp(self, weight_sets, focal, grid, act_prm_sets=None, col_override=None, which=capi.TRAIN, apply_out_fn=True):
        """Partial dependence on the resident matrix (npbnn_predict_pdp): [n_grid, n_rows, n_out], per grid point and row the
        prediction averaged over the weight sets, the columns ``focal`` set to the grid point's values ``grid`` [n_grid, n_focal]
        and then the columns ``col_override`` gives (NaN = none) to its constants.  NPBNN_INFO_PDP_ROUTE: the route taken."""
        packed, ap, n_sets = self._pack_sets(weight_sets, act_prm_sets, "predict_pdp")
        cols = np.ascontiguousarray(focal, dtype=np.int32).ravel()
        g = np.asarray(grid, dtype=np.float64)
        # (no focal column: the grid has rows and no entries, so its first dimension alone says how many points there are)
        g = capi.as_f64(g.reshape(-1, len(cols)) if len(cols) else g.reshape(g.shape[0] if g.ndim else 1, 0))
        co = None if col_override is None else capi.as_f64(np.asarray(col_override, dtype=np.float64).ravel())
        out = np.empty((g.shape[0], self.n_rows[which], self.n_out), dtype=np.float64)
        self._chk(self._lib.npbnn_predict_pdp(self._ctx, capi.dptr(packed), capi.dptr(ap), n_sets,
                                              cols.ctypes.data_as(C.POINTER(C.c_int32)), len(cols), capi.dptr(g), g.shape[0],
                                              capi.dptr(co), which, 1 if apply_out_fn else 0, capi.dptr(out)))
        return out

    def predict_ale(self, weight_sets, focal, edges, act_prm_sets=None, col_override=None, which=capi.TRAIN, apply_out_fn=True):
        """Local effects of the column ``focal`` on the resident matrix (npbnn_predict_ale): ``(counts [K], effects [S, K, n_out])``
        for the K bins the K + 1 ``edges`` cut - the rows of each bin and, per weight set, the mean over them of the prediction at
        the bin's upper edge minus the one at its lower edge (0 for an empty bin).  ``col_override`` (NaN = none) applies after the
        edges.  NPBNN_INFO_ALE_ROUTE: the route taken."""
        packed, ap, n_sets = self._pack_sets(weight_sets, act_prm_sets, "predict_ale")
        z = capi.as_f64(np.asarray(edges, dtype=np.float64).ravel())
        n_bins = len(z) - 1
        co = None if col_override is None else capi.as_f64(np.asarray(col_override, dtype=np.float64).ravel())
        counts = np.zeros(max(n_bins, 0), dtype=np.int64)
        effects = np.zeros((n_sets, max(n_bins, 0), self.n_out), dtype=np.float64)
        self._chk(self._lib.npbnn_predict_ale(self._ctx, capi.dptr(packed), capi.dptr(ap), n_sets, int(focal), capi.dptr(z), n_bins,
                                              capi.dptr(co), which, 1 if apply_out_fn else 0,
                                              counts.ctypes.data_as(C.POINTER(C.c_int64)), capi.dptr(effects)))
        return counts, effects

    def predict_saliency(self, weight_sets, act_prm_sets=None, col_override=None, which=capi.TRAIN, apply_out_fn=True):
        """Input gradients on the resident matrix (npbnn_predict_saliency): ``(mean, abs, sq)``, each [S, n_out, F] - per weight
        set, output and feature the mean over the rows of the derivative of the output with respect to the feature, of its absolute
        value and of its square.  A column ``col_override`` gives a constant (NaN = none) has gradient 0.
        NPBNN_INFO_SALIENCY_ROUTE: the route taken."""
        packed, ap, n_sets = self._pack_sets(weight_sets, act_prm_sets, "predict_saliency")
        co = None if col_override is None else capi.as_f64(np.asarray(col_override, dtype=np.float64).ravel())
        out = [np.zeros((n_sets, self.n_out, int(self.arch.in_dim)), dtype=np.float64) for _ in range(3)]
        self._chk(self._lib.npbnn_predict_saliency(self._ctx, capi.dptr(packed), capi.dptr(ap), n_sets, capi.dptr(co), which,
                                                   1 if apply_out_fn else 0, capi.dptr(out[0]), capi.dptr(out[1]), capi.dptr(out[2])))
        return tuple(out)

    def predict_shapley(self, weight_sets, rows, bg_rows, perms, player_of=None, act_prm_sets=None, col_override=None, which=capi.TRAIN,
                        which_bg=None, apply_out_fn=True, want_phi=False):
        """Permutation-sampling Shapley attributions (npbnn_predict_shapley) of the rows ``rows`` of the resident matrix ``which``
        against the rows ``bg_rows`` of the resident matrix ``which_bg`` (default: the same), along the permutations ``perms``
        [n_perm, P] of the P players; ``player_of`` [F] names every column's player (None: a column is a player).  A dict:
        ``mean`` and ``sq`` [E, P, n_out], the means over the weight sets of phi and phi^2; ``abs`` [S, P, n_out], the mean over
        the rows of |phi|; ``fx`` [S, E, n_out]; ``base`` [S, n_out]; ``phi`` [S, E, P, n_out] with ``want_phi``, else None.
        NPBNN_INFO_SHAPLEY_ROUTE: the route taken."""
        packed, ap, n_sets = self._pack_sets(weight_sets, act_prm_sets, "predict_shapley")
        i64, i32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        rows = np.ascontiguousarray(rows, dtype=np.int64).ravel()
        bg = np.ascontiguousarray(bg_rows, dtype=np.int64).ravel()
        pm = np.ascontiguousarray(perms, dtype=np.int32)
        if pm.ndim != 2:
            raise ValueError("predict_shapley: perms must be [n_perm, n_players]")
        n_perm, n_players = pm.shape
        po = None if player_of is None else np.ascontiguousarray(player_of, dtype=np.int32).ravel()
        if po is not None and len(po) != int(self.arch.in_dim):
            raise ValueError("predict_shapley: player_of needs one entry per feature column")
        co = None if col_override is None else capi.as_f64(np.asarray(col_override, dtype=np.float64).ravel())
        e, n_out = len(rows), self.n_out
        res = dict(mean=np.zeros((e, n_players, n_out)), sq=np.zeros((e, n_players, n_out)), abs=np.zeros((n_sets, n_players, n_out)),
                   fx=np.zeros((n_sets, e, n_out)), base=np.zeros((n_sets, n_out)),
                   phi=np.zeros((n_sets, e, n_players, n_out)) if want_phi else None)
        self._chk(self._lib.npbnn_predict_shapley(
            self._ctx, capi.dptr(packed), capi.dptr(ap), n_sets, capi.dptr(co), which, rows.ctypes.data_as(i64), e,
            which if which_bg is None else which_bg, bg.ctypes.data_as(i64), len(bg), None if po is None else po.ctypes.data_as(i32), n_players,
            pm.ctypes.data_as(i32), n_perm, 1 if apply_out_fn else 0, capi.dptr(res["mean"]), capi.dptr(res["sq"]), capi.dptr(res["abs"]),
            capi.dptr(res["fx"]), capi.dptr(res["base"]), capi.dptr(res["phi"])))
        return res

    def time_eval(self, weights, iters=20):
        w = one_vector(weights)
        a, b = C.c_double(0), C.c_double(0)
        self._chk(self._lib.npbnn_time_eval(self._ctx, capi.dptr(w), int(iters), C.byref(a), C.byref(b)))
        return a.value, b.value

    def time_pass(self, weights, n_candidates=0, iters=20):
        """Mean duration (ms) of the evaluation kernel of a speculative chain pass and the candidates it evaluates."""
        w = one_vector(weights)
        ms, used = C.c_double(0), C.c_int(0)
        self._chk(self._lib.npbnn_time_pass(self._ctx, capi.dptr(w), int(n_candidates), int(iters), C.byref(ms), C.byref(used)))
        return ms.value, used.value

    def time_wide(self, weights, iters=20):
        """Weight-streamed path: mean duration (ms) of the first layer's product alone and of a whole pass, and the product's
        geometry (rows, outputs of a workgroup's block, K-slices, workgroups)."""
        w = one_vector(weights)
        ms0, ms = C.c_double(0), C.c_double(0)
        info = (C.c_int * 4)()
        self._chk(self._lib.npbnn_time_wide(self._ctx, capi.dptr(w), int(iters), C.byref(ms0), C.byref(ms), info))
        return ms0.value, ms.value, dict(block_rows=info[0], block_outputs=info[1], k_slices=info[2], workgroups=info[3])

    def _fill_chain_cfg(self, cfg, prior_kind, prior_scale, w_bound, temperature, lik_temp, cur_loglik, cur_logprior,
                        cur_sigma=None, sigma=None, n_candidates=0, schedule=0, sigma_mult=None, hastings=None, slopes=None,
                        fixed_slopes=None):
        # the settings of a plain batch rarely change between dispatches: when they are the ones this struct already holds, only the
        # chain's state goes in
        plain = (slopes is None and sigma_mult is None and type(prior_scale) is np.ndarray and prior_scale.ndim == 1
                 and prior_scale.dtype == np.float64)
        key = None
        if plain:
            key = (prior_kind, prior_scale.tobytes(), w_bound, temperature, lik_temp, n_candidates, schedule, sigma is None, cur_sigma is None,
                   None if fixed_slopes is None else np.asarray(fixed_slopes, dtype=np.float64).tobytes())
            if cfg.__dict__.get("_plain_key") == key:
                cfg.cur_loglik, cfg.cur_logprior = cur_loglik, cur_logprior
                cfg.force_f32 = 0
                if sigma is not None or cur_sigma is not None:
                    k = self.arch.n_targets
                    if sigma is not None:
                        for j, v in enumerate(np.broadcast_to(sigma, (k,))):
                            cfg.sigma[j] = float(v)
                    if cur_sigma is not None:
                        for j, v in enumerate(np.broadcast_to(cur_sigma, (k,))):
                            cfg.cur_sigma[j] = float(v)
                return
        cfg._plain_key = key
        cfg.slope_idx = cfg.slope_delta = None
        cfg.n_slopes = cfg.slope_term_in_prior = 0
        cfg._keep_slopes = None
        if fixed_slopes is not None and slopes is None:      # ActFun("genReLU", prm=...): the hidden layers' slopes, the same for every proposal
            fixed = np.asarray(fixed_slopes, dtype=np.float64).ravel()
            cfg.n_slopes = len(fixed)
            for i, v in enumerate(fixed):
                cfg.cur_slopes[i] = float(v)
        if slopes is not None:        # (slope_idx [K] int32, slope_delta [K], accepted slopes, does cur_logprior hold their term?)
            s_idx = np.ascontiguousarray(slopes[0], dtype=np.int32)
            s_delta = capi.as_f64(slopes[1])
            cur = np.asarray(slopes[2], dtype=np.float64).ravel()
            cfg._keep_slopes = (s_idx, s_delta)
            cfg.slope_idx = s_idx.ctypes.data_as(C.POINTER(C.c_int32))
            cfg.slope_delta = capi.dptr(s_delta)
            cfg.n_slopes = len(cur)
            for i, v in enumerate(cur):
                cfg.cur_slopes[i] = float(v)
            cfg.slope_term_in_prior = 1 if slopes[3] else 0
        cfg.prior_kind = int(prior_kind)
        cfg._keep_scale = None
        cfg.prior_scale_w = None
        if any(np.ndim(s) != 0 for s in prior_scale):
            # hyper_p = 2 / 3: a scale per input node (one row, broadcast over the nodes) or per weight -> one per packed weight
            rows = list(self.arch.out_dim[:self.arch.n_layers])
            cols = [self.arch.in_dim + self.arch.has_bias[0]] + [rows[l - 1] + self.arch.has_bias[l] for l in range(1, self.arch.n_layers)]
            per_w = np.concatenate([np.broadcast_to(np.asarray(s, dtype=np.float64), (r, c)).ravel()
                                    for s, r, c in zip(prior_scale, rows, cols)])
            cfg._keep_scale = capi.as_f64(per_w)
            cfg.prior_scale_w = capi.dptr(cfg._keep_scale)
        else:
            for i, s in enumerate(prior_scale):
                cfg.prior_scale[i] = float(s)
        cfg.w_bound = float(w_bound)
        cfg.temperature = float(temperature)
        cfg.lik_temp = float(lik_temp)
        cfg.sigma_given = 0 if sigma is None else 1
        k = self.arch.n_targets
        if sigma is not None:
            for j, v in enumerate(np.broadcast_to(sigma, (k,))):
                cfg.sigma[j] = float(v)
        if cur_sigma is not None:
            for j, v in enumerate(np.broadcast_to(cur_sigma, (k,))):
                cfg.cur_sigma[j] = float(v)
        cfg.cur_loglik, cfg.cur_logprior = float(cur_loglik), float(cur_logprior)
        cfg.n_candidates = int(n_candidates)
        cfg.schedule = int(schedule)
        cfg.force_f32 = 0
        if sigma_mult is not None:         # (the arrays are kept on the struct object: it only holds pointers)
            cfg._keep = (capi.as_f64(sigma_mult), capi.as_f64(hastings))
            cfg.sigma_mult, cfg.hastings = capi.dptr(cfg._keep[0]), capi.dptr(cfg._keep[1])
        else:
            cfg._keep = None
            cfg.sigma_mult = cfg.hastings = None

    def _result_dict(self, res):
        k = self.arch.n_targets
        return dict(loglik=res.loglik, logprior=res.logprior, sigma=np.array(res.sigma[:k]) if k else _NO_SIGMA,
                    n_accepted=res.n_accepted, n_passes=res.n_passes, n_candidates=res.n_candidates,
                    n_void_passes=res.n_void_passes, schedule=res.schedule, temperature=res.temperature,
                    iterations_done=res.iterations_done, overflow=res.overflow, slopes=res.slopes)

    def chain_run(self, weights, idx, delta, cnt, log_u, prior_kind, prior_scale, w_bound, temperature, lik_temp,
                  cur_loglik, cur_logprior, cur_sigma=None, sigma=None, mask=None, n_candidates=0, schedule=0, sigma_mult=None,
                  hastings=None, slopes=None, fixed_slopes=None):
        """K device-resident Metropolis-Hastings iterations (npbnn_chain_run).  Returns
        (new packed weights, accepted flags, proposed logLik, proposed logPrior, result dict)."""
        w = pack_weights(weights) if isinstance(weights, (list, tuple)) else capi.as_f64(weights).copy()
        K, M = idx.shape
        cfg = self.__dict__.get("_chain_cfg")
        if cfg is None:
            cfg = self._chain_cfg = capi.ChainCfg()
            self._chain_res = capi.ChainResult()
        self._fill_chain_cfg(cfg, prior_kind, prior_scale, w_bound, temperature, lik_temp, cur_loglik, cur_logprior,
                             cur_sigma, sigma, n_candidates, schedule, sigma_mult, hastings, slopes, fixed_slopes)
        m = None if mask is None else (pack_weights(mask) if isinstance(mask, (list, tuple)) else capi.as_f64(mask))
        if idx.dtype != np.int32 or not idx.flags.c_contiguous:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
        if cnt.dtype != np.int32 or not cnt.flags.c_contiguous:
            cnt = np.ascontiguousarray(cnt, dtype=np.int32)
        delta = capi.as_f64(delta)
        log_u = capi.as_f64(log_u)
        acc = np.empty(K, dtype=np.uint8)
        llp, lpp = np.empty(K), np.empty(K)
        res = self._chain_res
        run = capi.chain_run_by_address(self._lib)
        addr = (_addr(w), None if m is None else _addr(m), _addr(idx), _addr(delta), _addr(cnt), _addr(log_u), _addr(acc), _addr(llp),
                _addr(lpp))
        attempt, sync_retried = 0, False
        while True:
            cfg.force_f32 = attempt
            t_in = _now()
            rc = run(self._ctx, C.byref(cfg), addr[0], addr[1], K, M, addr[2], addr[3], addr[4], addr[5], addr[6], addr[7], addr[8],
                     C.byref(res))
            self.seconds_in_chain_run += _now() - t_in          # (what a dispatch spends inside the library: tools/profile_dispatch.py)
            # ('f16' asked for the fp16 pair and nothing else: there the error stands, as it does for eval and predict)
            if rc == capi.E_RANGE and attempt == 0 and self.l0_option() != "f16":
                attempt = 1
                continue        # a weight left the fp16 range: same batch again on the float32 path (state untouched)
            if rc == capi.E_SYNC and not sync_retried:
                sync_retried = True
                if cfg.schedule in (capi.SCHED_OVERLAP2, capi.SCHED_PERSIST, capi.SCHED_PERSIST_SERIAL):
                    cfg.schedule = capi.SCHED_OVERLAP
                    cfg._plain_key = None      # (the struct no longer holds what the caller asked for)
                self.sync_fallbacks += 1
                if self.sync_fallbacks == 1:
                    import warnings
                    warnings.warn("npbnn_amd: a device-side wait of the flag-ordered (two-stream / persistent) chain schedule timed out; the batch is repeated on "
                                  "one stream and this context stays on one stream from now on (HipContext.sync_fallbacks counts them)")
                continue        # (the state was left untouched)
            self._chk(rc)
            break
        return w, acc, llp, lpp, self._result_dict(res)


    def chain_run_general(self, weights, draws, log_u, mask=None, indicators=None, feature_indicators=None, feature_means=None,
                          prior_ind1=0.5, has_indicator_prior=False, **cfg_kw):
        """K iterations of the general device chain (npbnn_chain_run_general).  ``draws``: dict with ``kind`` (PROP_*), ``idx``,
        ``val`` [K, M], ``cnt`` [K], ``layer_mask`` [K] and, as the sampler's settings need them, ``h_idx`` / ``h_val`` / ``h_fac`` /
        ``h_cnt`` (every draw of the fixed-normal proposal), ``ind_ptr`` / ``ind_pos`` (weight-indicator flips), ``find_ptr`` /
        ``find_pos`` / ``find_use`` (feature-indicator flips).  Returns (weights, indicators, feature indicators, accepted flags,
        proposed logLik, proposed logPrior, result dict)."""
        i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)       # noqa: E731
        ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))        # noqa: E731
        w = one_vector(weights, copy=True)
        idx, cnt = i32(draws["idx"]), i32(draws["cnt"])
        val = capi.as_f64(draws["val"])
        K, M = idx.shape
        cfg, res, g = capi.ChainCfg(), capi.ChainResult(), capi.GeneralCfg()
        self._fill_chain_cfg(cfg, **cfg_kw)
        g.proposal_kind, g.M = int(draws["kind"]), int(M)
        keep = [idx, cnt, val]
        g.idx, g.val, g.cnt = ip(idx), capi.dptr(val), ip(cnt)
        lm = i32(draws.get("layer_mask") if draws.get("layer_mask") is not None else np.zeros(K))
        g.layer_mask = ip(lm)
        keep.append(lm)
        if draws.get("h_idx") is not None:
            h_idx, h_cnt = i32(draws["h_idx"]), i32(draws["h_cnt"])
            h_val, h_fac = capi.as_f64(draws["h_val"]), capi.as_f64(draws["h_fac"])
            g.h_idx, g.h_val, g.h_fac, g.h_cnt = ip(h_idx), capi.dptr(h_val), capi.dptr(h_fac), ip(h_cnt)
            keep += [h_idx, h_cnt, h_val, h_fac]
        ind = find = None
        if indicators is not None:
            ind = capi.as_f64(indicators).copy()
            iptr, ipos = i32(draws["ind_ptr"]), i32(draws["ind_pos"] if len(draws["ind_pos"]) else np.zeros(1))
            g.ind_inout, g.ind_ptr, g.ind_pos = capi.dptr(ind), ip(iptr), ip(ipos)
            g.prior_ind1, g.has_indicator_prior = float(prior_ind1), 1 if has_indicator_prior else 0
            keep += [iptr, ipos]
        if feature_indicators is not None:
            find = capi.as_f64(feature_indicators).copy()
            means = capi.as_f64(feature_means)
            fptr, fpos, fuse = i32(draws["find_ptr"]), i32(draws["find_pos"] if len(draws["find_pos"]) else np.zeros(1)), i32(draws["find_use"])
            g.find_inout, g.feature_means, g.find_ptr, g.find_pos, g.find_use = capi.dptr(find), capi.dptr(means), ip(fptr), ip(fpos), ip(fuse)
            keep += [means, fptr, fpos, fuse]
        m = None if mask is None else one_vector(mask)
        log_u = capi.as_f64(log_u)
        acc = np.empty(K, dtype=np.uint8)
        llp, lpp = np.empty(K), np.empty(K)
        self._chk(self._lib.npbnn_chain_run_general(self._ctx, C.byref(cfg), C.byref(g), capi.dptr(w), capi.dptr(m), K, capi.dptr(log_u),
                                                    acc.ctypes.data_as(C.POINTER(C.c_uint8)), capi.dptr(llp), capi.dptr(lpp), C.byref(res)))
        del keep
        return w, ind, find, acc, llp, lpp, self._result_dict(res)


class FastBatch:
    """A dispatch of the patch-list device chain whose settings are fixed: the settings struct filled once, the result struct, the
    accept flags and the packed mask kept, the C entry bound once - :meth:`run` only puts in the chain's state and the addresses of
    this batch's draws.  (What ``HipContext.chain_run`` does per call, minus everything that does not change between calls.)"""

    def __init__(self, ctx, K, M, mask, cfg_kwargs):
        self.ctx = ctx
        self.K, self.M = int(K), int(M)
        self.cfg = capi.ChainCfg()
        ctx._fill_chain_cfg(self.cfg, **cfg_kwargs)
        self.cfg_ref = C.byref(self.cfg)
        self.res = capi.ChainResult()
        self.res_ref = C.byref(self.res)
        self.acc = np.empty(self.K, dtype=np.uint8)
        self.acc_addr = _addr(self.acc)
        self.mask = None if mask is None else (pack_weights(mask) if isinstance(mask, (list, tuple)) else capi.as_f64(mask))
        self.mask_addr = None if self.mask is None else _addr(self.mask)
        self.n_targets = ctx.arch.n_targets
        self.entry = capi.chain_run_by_address(ctx._lib)

    def run(self, w, idx, delta, cnt, log_u, cur_loglik, cur_logprior, temperature, cur_sigma=None, just_before=None):
        """0 and the results in ``self.res`` / ``self.acc`` / ``w`` - or the C ABI's error code with the state untouched (a weight
        left the fp16 range, a device-side wait timed out ...: the caller repeats the batch through ``chain_run``, which knows the
        remedies).  ``just_before()`` is called as the last thing before the C entry: work for another thread is handed over there,
        so that the other thread finds the interpreter lock free (the C call releases it) instead of taking it from this one in
        the middle of its preparations (measured: copies of the weight vector that took 300 us instead of 4)."""
        cfg = self.cfg
        cfg.cur_loglik, cfg.cur_logprior = cur_loglik, cur_logprior
        cfg.temperature = temperature        # (state, not a setting: MC3 swaps it between two dispatches)
        if cur_sigma is not None:
            for j in range(self.n_targets):
                cfg.cur_sigma[j] = cur_sigma[j]
        ctx = self.ctx
        a_w, a_idx, a_delta, a_cnt, a_u = _addr(w), _addr(idx), _addr(delta), _addr(cnt), _addr(log_u)
        if just_before is not None:
            just_before()
        t_in = _now()
        rc = self.entry(ctx._ctx, self.cfg_ref, a_w, self.mask_addr, self.K, self.M, a_idx, a_delta, a_cnt, a_u, self.acc_addr, None, None,
                        self.res_ref)
        ctx.seconds_in_chain_run += _now() - t_in
        return rc


def fill_chain_job(J, q, job, K, span, chain_id, force_f32=0, n_seg=0, want_cold_w=False):
    """Fill ``J`` (a capi.ChainJob) from the job dict ``job`` (see :func:`chains_run_exchange`), number ``q`` of its group, for ``K``
    iterations - ``span`` says how the caller counts them, for the error about a wrong number of rows.  ``n_seg`` > 0 adds the
    per-exchange outputs ``state`` [n_seg, XSTATE_DOUBLES] and, with ``want_cold_w``, ``cold_w`` [n_seg, n_w].  Returns (the arrays
    and structs ``J`` points at - keep them until the call has returned -, the job's output dict)."""
    ctx = job["ctx"]
    w = one_vector(job["weights"], copy=True)
    idx, cnt = job["idx"], job["cnt"]
    if idx.shape[0] != K or len(cnt) != K:
        raise ValueError("job %d: %d rows of draws for %s iterations" % (q, idx.shape[0], span))
    if idx.dtype != np.int32 or not idx.flags.c_contiguous:
        idx = np.ascontiguousarray(idx, dtype=np.int32)
    if cnt.dtype != np.int32 or not cnt.flags.c_contiguous:
        cnt = np.ascontiguousarray(cnt, dtype=np.int32)
    delta, log_u = capi.as_f64(job["delta"]), capi.as_f64(job["log_u"])
    mask = job.get("mask")
    m = None if mask is None else one_vector(mask)
    cfg, res = capi.ChainCfg(), capi.ChainResult()
    ctx._fill_chain_cfg(cfg, **job["cfg"])
    cfg.force_f32 = force_f32
    acc = np.zeros(K, dtype=np.uint8)
    llp, lpp = np.zeros(K), np.zeros(K)
    i32p = C.POINTER(C.c_int32)
    J.ctx = ctx._ctx
    J.cfg = C.pointer(cfg)
    J.W_inout = capi.dptr(w)
    J.mask_packed = capi.dptr(m)
    J.M = idx.shape[1]
    J.chain_id = int(chain_id)
    J.idx = idx.ctypes.data_as(i32p)
    J.delta = capi.dptr(delta)
    J.cnt = cnt.ctypes.data_as(i32p)
    J.log_u = capi.dptr(log_u)
    J.out_accepted = acc.ctypes.data_as(C.POINTER(C.c_uint8))
    J.out_loglik_prop = capi.dptr(llp)
    J.out_logprior_prop = capi.dptr(lpp)
    J.result = C.pointer(res)
    out = dict(w=w, accepted=acc, loglik_prop=llp, logprior_prop=lpp, _res=res, _ctx=ctx)
    if n_seg:
        state = np.zeros((n_seg, capi.XSTATE_DOUBLES))
        cold = np.zeros((n_seg, w.size)) if want_cold_w else None
        J.out_state = capi.dptr(state)
        J.out_cold_w = capi.dptr(cold)
        out.update(state=state, cold_w=cold)
    return (w, idx, cnt, delta, log_u, m, cfg, res), out


def chains_run_exchange(jobs, n_chains, seg_len, n_seg, swap_j, swap_k, swap_logu, comm=None, launch_slack=1.25,
                        want_cold_w=True):
    """Several chains advance ``n_seg`` swap intervals of ``seg_len`` iterations with the temperature swaps done on the GPU
    (npbnn_chains_run_exchange; reference loop: np_bnn/BNN_mc3.py:94-112).

    ``jobs``: one dict per chain of this process - ``ctx`` (HipContext), ``chain_id``, ``weights``, ``idx``, ``delta``,
    ``cnt``, ``log_u`` (K = n_seg * seg_len rows), ``mask`` and the keyword arguments of :meth:`HipContext.chain_run`
    under ``cfg``.  ``comm``: the native communicator handle (``RcclComm._comm``) or None for the chains of this process.

    Returns ``(outs, records, segments_done)``: per job ``dict(w, accepted, loglik_prop, logprior_prop, state, cold_w,
    result)`` valid for the first ``result['iterations_done']`` iterations; ``records[s, i] = (logPost, temperature before
    swap s, finished flag, iterations done)`` of chain i; ``segments_done < n_seg`` when some chain fell short."""
    K = int(seg_len) * int(n_seg)
    lib = jobs[0]["ctx"]._lib
    arr = (capi.ChainJob * len(jobs))()
    keep, outs = [], []
    i32p = C.POINTER(C.c_int32)
    for q, job in enumerate(jobs):
        kept, out = fill_chain_job(arr[q], q, job, K, "%d x %d" % (n_seg, seg_len), job["chain_id"], n_seg=n_seg, want_cold_w=want_cold_w)
        keep.append(kept)
        outs.append(out)
    sj = np.ascontiguousarray(swap_j, dtype=np.int32)
    sk = np.ascontiguousarray(swap_k, dtype=np.int32)
    su = capi.as_f64(swap_logu)
    records = np.zeros((n_seg, n_chains, capi.REC_DOUBLES))
    done = C.c_int32(0)
    rc = lib.npbnn_chains_run_exchange(comm, arr, len(jobs), int(n_chains), int(seg_len), int(n_seg), sj.ctypes.data_as(i32p),
                                       sk.ctypes.data_as(i32p), capi.dptr(su), float(launch_slack), capi.dptr(records),
                                       C.byref(done))
    capi.check(lib, None, rc)
    for o in outs:
        o["result"] = o.pop("_ctx")._result_dict(o.pop("_res"))
    return outs, records, int(done.value)


def chains_run_batched(jobs, K):
    """2 or 3 chains of one model on one GPU advance ``K`` iterations each, one proposal per chain per streaming read of the
    feature matrix (npbnn_chains_run_batched).  ``jobs``: dicts as for :func:`chains_run_exchange` (``chain_id`` not needed).
    Returns per job ``dict(w, accepted, loglik_prop, logprior_prop, result)``.  A weight leaving the fp16 range sends the whole
    group through once more on the float32 layer-0 path."""
    K = int(K)
    lib = jobs[0]["ctx"]._lib
    for attempt in (0, 1):
        arr = (capi.ChainJob * len(jobs))()
        keep, outs = [], []
        for q, job in enumerate(jobs):
            kept, out = fill_chain_job(arr[q], q, job, K, "%d" % K, q, force_f32=attempt)
            keep.append(kept)
            outs.append(out)
        rc = lib.npbnn_chains_run_batched(arr, len(jobs), K)
        if rc == capi.E_RANGE and attempt == 0 and all(job["ctx"].l0_option() != "f16" for job in jobs):
            continue
        capi.check(lib, jobs[0]["ctx"]._ctx, rc)
        break
    for o in outs:
        o["result"] = o.pop("_ctx")._result_dict(o.pop("_res"))
    return outs
