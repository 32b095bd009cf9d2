"""Posterior prediction from stored weight samples: ``get_posterior_cat_prob``, ``sample_from_categorical``,
``predictBNN`` (reference: np_bnn/BNN_lib.py:352-501, 682-713).

The reference runs ``RunPredict`` once per stored sample - a fresh copy of the feature matrix and a full pass over
it every time.  Here the matrix is uploaded once and the samples go through ``npbnn_predict_sets``: up to three
weight sets per streaming read of X, all layers fused.  Shuffling of feature columns (feature importance) and the
posterior-predictive resampling draw from numpy's global stream exactly as the reference does.

``feature_importance`` keeps a permutation on the device when it can (summary modes 0 and 1, a built-in output function,
integer class labels): the shuffle is a gather of the block's columns inside the resident matrix
(``npbnn_permute_columns``, row indices drawn here), the summary over the samples and its confusion table against the labels
are accumulated there (``npbnn_predict_sets_summary``), and C x C integers come back per permutation.  ``NPBNN_FI_HOST=1``
keeps every permutation on the route through ``get_posterior_cat_prob`` (one upload and one stack of predictions each)."""
import os

import numpy as np

from . import _capi as capi
from .files import load_obj
from .layers import ActFun
from .likelihoods import CalcAccuracy
from .stored import Network, sigma_matrix


class _SamplePredictor:
    """One device context for a set of stored samples: the feature matrix can be replaced (column shuffles of
    feature_importance) while network description and packed weight sets stay."""

    def __init__(self, n_features, post_samples, actFun, output_act_fun):
        from .backend import HipContext, pack_weights
        self._weights = [s["weights"] for s in post_samples]
        self._packed = np.stack([pack_weights(w) for w in self._weights])
        self._net = Network(self._weights, [s["alphas"] for s in post_samples], actFun, output_act_fun)
        self._out_fn = output_act_fun
        self._n_features = n_features
        self._slopes, self._applied = self._net.slopes, self._net.apply_out_fn
        self._ctx = HipContext()
        self._arch_set = False

    def _load(self, features):
        ctx = self._ctx
        ctx.set_data(features)
        if not self._arch_set:
            self._net.describe_to(ctx, self._n_features)
            self._arch_set = True
        return ctx

    @property
    def custom_output(self):
        """A custom output callable: no device kind, applied on the host to every sample's stack."""
        return self._net.custom_output

    def _out_kind_for(self, kind, who):
        """The OUT_* constant the driver's ``kind`` stands for; ``ValueError`` in ``who``'s name when the model's output function is another."""
        want = {"classification": capi.OUT_SOFTMAX, "regression": capi.OUT_IDENTITY, "regression-error": capi.OUT_SOFTPLUS_HALF}[kind]
        if self._net.out_kind != want:
            raise ValueError("%s: kind %r does not go with the model's output function" % (who, kind))
        return want

    def predict(self, features):
        """[n_samples, n_rows, n_out] predictions of every stored sample on ``features``."""
        self.load(features)
        return self.predict_loaded()

    def predict_loaded(self):
        """``predict`` on the matrix ``load`` uploaded, without a second upload."""
        y = self._ctx.predict_sets(list(self._packed), act_prm_sets=self._slopes, apply_out_fn=self._applied)
        if self.custom_output:      # host side, sample by sample
            y = np.array([self._out_fn(yi) for yi in y])
        return y

    def predict_hpd(self, features, level):
        """(mean, lower, upper) [n_rows, n_out] over the stored samples' predictions on ``features``; the stack stays on the
        device (npbnn_predict_sets_hpd).  A custom output callable has no device kind: its stack is built on the host and goes
        through ``posterior_hpd``."""
        if self.custom_output:
            from .hpd import posterior_hpd
            y = self.predict(features)
            lo, hi = posterior_hpd(y, level)
            return np.mean(y, axis=0), lo, hi
        ctx = self._load(features)
        return ctx.predict_sets_hpd(list(self._packed), level, act_prm_sets=self._slopes, apply_out_fn=self._applied)

    def load(self, features):
        """Upload ``features`` (and describe the network on the first call): what ``permute`` and ``summary`` work on."""
        self._load(features)
        self._n_rows = len(features)

    def permute(self, columns, independently):
        """Shuffle ``columns`` of the loaded matrix between its rows on the device; columns an earlier call moved go back first.
        Draws what ``_shuffled_copy`` draws from numpy's global stream - ``np.random.permutation(n_rows)`` leaves the stream
        where ``np.random.permutation(values)`` does, and ``values[indices]`` is the array the latter returns: one permutation
        per column when ``independently`` and ``columns`` is a list, else one for the block (np_bnn/BNN_lib.py:366-371).
        Nothing to shuffle (``not columns``) only restores."""
        if not columns:
            self._ctx.permute_columns([], None)
            return
        if independently and type(columns) == list:
            perms = {}                                     # a column named again is shuffled again: x[p1][p2] = x[p1[p2]]
            for col in columns:
                idx = np.random.permutation(self._n_rows)
                col = _column_index(col, self._n_features)
                perms[col] = perms[col][idx] if col in perms else idx
            self._ctx.permute_columns(list(perms), np.stack(list(perms.values())))
        else:
            idx = np.random.permutation(self._n_rows)
            cols = list(dict.fromkeys(_column_index(c, self._n_features) for c in np.atleast_1d(columns).ravel()))
            self._ctx.permute_columns(cols, idx.reshape(1, -1))

    def summary(self, mode, labels=None, want_summary=True):
        """(summary [n_rows, n_out] or None, confusion table against ``labels`` or None) of the stored samples' predictions on
        the loaded matrix as it stands, mode 0 (votes) or 1 (mean): ``_summarise`` and CalcAccuracy's table, accumulated on
        the device."""
        if self.custom_output:
            raise ValueError("a custom output callable has no device summary")
        return self._ctx.predict_sets_summary(self._packed, mode, labels=labels, act_prm_sets=self._slopes,
                                              want_summary=want_summary, apply_out_fn=self._applied)

    def support(self, mode, labels, thresholds, **kw):
        """Threshold cube (and Bayes-factor table, NaN-masked summary, keep mask: ``HipContext.predict_sets_support``'s keywords) of
        the stored samples' summary on the loaded matrix, mode 0 or 1."""
        if self.custom_output:
            raise ValueError("a custom output callable has no device summary")
        return self._ctx.predict_sets_support(self._packed, mode, labels, thresholds, act_prm_sets=self._slopes,
                                              apply_out_fn=self._applied, **kw)

    def lppd(self, features, labels, lik_kind, sigma_sets=None, pointwise=False):
        """``HipContext.predict_sets_lppd``'s dict for the stored samples on ``features`` against ``labels`` (class indices,
        LIK_CATEGORICAL) or targets (LIK_GAUSS, ``sigma_sets`` per sample): the log-likelihood matrix stays on the device
        (npbnn_predict_sets_lppd).  A custom output callable has no device route: its stack is built on the host and goes through
        ``posterior_lppd``."""
        if self.custom_output:
            from .lppd import log_lik_of_stack, posterior_lppd
            res = posterior_lppd(log_lik_of_stack(self.predict(features), labels, lik_kind, sigma_sets))
            return res if pointwise else dict(res, lppd_i=None, mean_log_lik_i=None, p_waic_i=None)
        ctx = self._load(features)
        if lik_kind == capi.LIK_CATEGORICAL:
            ctx.set_labels(labels)
        else:
            ctx.set_targets(labels)
        return ctx.predict_sets_lppd(self._packed, lik_kind, sigma_sets=sigma_sets, act_prm_sets=self._slopes, pointwise=pointwise)

    def loo(self, features, labels, lik_kind, sigma_sets=None, log_lik=False, block_rows=None):
        """``posterior_loo``'s dict, with ``log_lik_sample`` [S] and (``log_lik``) the matrix ``log_lik`` [S, N] beside it, for the
        stored samples on ``features`` against ``labels`` (class indices, LIK_CATEGORICAL) or targets (LIK_GAUSS, ``sigma_sets`` per
        sample): the log-likelihood matrix stays on the device (npbnn_predict_sets_loo).  ``block_rows``: the most rows a device
        matrix may hold.  A table of more rows is uploaded whole - the scales of the first layer's half-precision split are the
        whole table's - and served block by block as the context's second table, labels or targets set per block; a row's
        results do not depend on the blocks, and the totals are formed from the concatenated arrays.  A custom output callable has
        no device route: its stack is built on the host and goes through ``posterior_loo``."""
        from .loo import check_samples, loo_totals, posterior_loo
        check_samples(len(self._packed), "loo")
        if self.custom_output:
            from .lppd import log_lik_of_stack
            ll = log_lik_of_stack(self.predict(features), labels, lik_kind, sigma_sets)
            return dict(posterior_loo(ll), log_lik_sample=np.sum(ll, axis=1), log_lik=ll if log_lik else None)
        ctx = self._load(features)
        kw = dict(sigma_sets=sigma_sets, act_prm_sets=self._slopes, log_lik=log_lik)
        set_y = ctx.set_labels if lik_kind == capi.LIK_CATEGORICAL else ctx.set_targets
        if block_rows is None or block_rows >= len(features):
            set_y(labels)
            parts = [ctx.predict_sets_loo(self._packed, lik_kind, **kw)]
        else:
            parts = []
            for r in range(0, len(features), block_rows):
                ctx.set_data(features[r:r + block_rows], capi.TEST)
                set_y(labels[r:r + block_rows], capi.TEST)
                parts.append(ctx.predict_sets_loo(self._packed, lik_kind, which=capi.TEST, **kw))
        res = loo_totals(*(np.concatenate([p[k] for p in parts]) for k in ("elpd_loo_i", "lppd_i", "pareto_k")), len(self._packed))
        res["log_lik_sample"] = np.sum([p["log_lik_sample"] for p in parts], axis=0)
        res["log_lik"] = np.concatenate([p["log_lik"] for p in parts], axis=1) if log_lik else None
        return res

    def uncertainty(self, features, kind, sigma_sets=None, pointwise=True):
        """``posterior_uncertainty``'s dict (without the counts) for the stored samples on ``features``, ``kind``
        ``"classification"``, ``"regression"`` (``sigma_sets`` per sample: the device returns mean and epistemic variance, and the
        mean of the squared sigmas, which does not depend on the row, is added here) or ``"regression-error"``; the stack stays on
        the device (npbnn_predict_sets_uncertainty), and without ``pointwise`` the [N, ...] arrays are None.  A custom output
        callable has no device kind: its stack is built on the host and goes through ``posterior_uncertainty``."""
        from .uncertainty import KINDS, posterior_uncertainty
        if kind not in KINDS:
            raise ValueError("uncertainty: kind %r; one of %s" % (kind, ", ".join(KINDS)))
        if self.custom_output:
            return posterior_uncertainty(self.predict(features), kind, sigma_sets)
        self._out_kind_for(kind, "uncertainty")
        sig = None
        if kind == "regression":
            sig = sigma_matrix(sigma_sets, len(self._packed), self._weights[0][-1].shape[0], "uncertainty", positive=False)
        ctx = self._load(features)
        res = ctx.predict_sets_uncertainty(self._packed, act_prm_sets=self._slopes, pointwise=pointwise)
        if kind == "regression":
            aleatoric = np.sum(sig * sig, axis=0) / len(sig)
            res["aleatoric_var_avg"] = aleatoric
            res["total_var_avg"] = res["epistemic_var_avg"] + aleatoric
            if pointwise:
                res["aleatoric_var"] = np.broadcast_to(aleatoric, res["epistemic_var"].shape).copy()
                res["total_var"] = res["epistemic_var"] + aleatoric
        return res

    def calibration(self, features, labels, kind, n_bins=15, levels=(0.5, 0.8, 0.9, 0.95), sigma_sets=None, pointwise=True):
        """``posterior_calibration``'s dict for the stored samples on ``features`` against ``labels`` - class indices
        (``"classification"``) or targets (``"regression"`` with ``sigma_sets`` per sample, ``"regression-error"``); the stack
        stays on the device (npbnn_predict_sets_calibration), and without ``pointwise`` the [N, ...] arrays are None.  A custom
        output callable has no device kind: its stack is built on the host and goes through ``posterior_calibration``."""
        from .calibration import CLASS_POINT_KEYS, KINDS, REGRESSION_POINT_KEYS, posterior_calibration
        if kind not in KINDS:
            raise ValueError("calibration: kind %r; one of %s" % (kind, ", ".join(KINDS)))
        if self.custom_output:
            res = posterior_calibration(self.predict(features), labels, kind, n_bins, levels, sigma_sets)
            return res if pointwise else {k: (None if k in CLASS_POINT_KEYS + REGRESSION_POINT_KEYS else v) for k, v in res.items()}
        self._out_kind_for(kind, "calibration")
        if kind == "regression" and sigma_sets is None:
            raise ValueError("calibration: kind \"regression\" needs sigma_sets (a sigma per sample and target)")
        ctx = self._load(features)
        if kind == "classification":
            ctx.set_labels(labels)
        else:
            ctx.set_targets(labels)
        return ctx.predict_sets_calibration(self._packed, n_bins=n_bins, levels=levels, sigma_sets=sigma_sets, act_prm_sets=self._slopes,
                                            pointwise=pointwise)

    def convergence(self, features, n_chains, rhat_threshold=1.01, pointwise=True):
        """``posterior_convergence``'s dict for the stored samples - ``n_chains`` chains of equal length, chain-major - on
        ``features``, predictions post-output; the stack stays on the device (npbnn_predict_sets_convergence), and without
        ``pointwise`` ``rhat`` and ``ess`` are None.  A custom output callable has no device kind: its stack is built on the host
        and goes through ``posterior_convergence``."""
        if self.custom_output:
            from .convergence import posterior_convergence
            res = posterior_convergence(self.predict(features), n_chains, rhat_threshold)
            return res if pointwise else dict(res, rhat=None, ess=None)
        ctx = self._load(features)
        return ctx.predict_sets_convergence(self._packed, n_chains, rhat_threshold, act_prm_sets=self._slopes,
                                            apply_out_fn=self._applied, pointwise=pointwise)

    def predictive(self, features, kind, probs=(0.025, 0.5, 0.975), sigma_sets=None, targets=None, block_rows=None, who="predictive"):
        """Quantiles, mean and CRPS of the posterior predictive distribution of the stored samples on ``features``, ``kind``
        ``"regression"`` (``sigma_sets`` per sample) or ``"regression-error"``: a dict with ``quantiles`` [len(probs), N, T], ``mean``
        [N, T] and, with ``targets`` [N, T], ``crps_i`` [N, T]; the stack stays on the device (npbnn_predict_sets_predictive).
        ``block_rows``: the most rows a device stack may hold.  A table of more rows is uploaded whole - the scales of the first
        layer's half-precision split are the whole table's - and served block by block as the context's second table, so a row's
        predictions do not depend on the blocks.  A custom output callable has no device kind: it is refused in ``who``'s name and no
        host stack is built."""
        from .predictive import KINDS
        if kind not in KINDS:
            raise ValueError("%s: kind %r; one of %s" % (who, kind, ", ".join(KINDS)))
        if self.custom_output:
            raise ValueError("%s: the model's output function is a custom callable, which has no device kind; build the stack "
                             "and call posterior_predictive" % who)
        self._out_kind_for(kind, who)
        if kind == "regression" and sigma_sets is None:
            raise ValueError("%s: kind \"regression\" needs sigma_sets (a sigma per sample and target)" % who)
        ctx = self._load(features)
        kw = dict(probs=probs, sigma_sets=sigma_sets, act_prm_sets=self._slopes)
        if block_rows is None or block_rows >= len(features):
            return ctx.predict_sets_predictive(self._packed, targets=targets, **kw)
        parts = []
        for r in range(0, len(features), block_rows):
            ctx.set_data(features[r:r + block_rows], capi.TEST)
            parts.append(ctx.predict_sets_predictive(self._packed, targets=None if targets is None else targets[r:r + block_rows], which=capi.TEST, **kw))
        return {k: (None if parts[0][k] is None else np.concatenate([p[k] for p in parts], axis=1 if k == "quantiles" else 0))
                for k in ("quantiles", "mean", "crps_i")}

    def close(self):
        self._ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _column_index(col, n_features):
    """A column as numpy indexes it: negative values count from the end."""
    c = int(col)
    if c != col or not -n_features <= c < n_features:
        raise IndexError("column %r outside a matrix of %d features" % (col, n_features))
    return c % n_features


def _predict_samples(features, post_samples, actFun, output_act_fun):
    with _SamplePredictor(features.shape[1], post_samples, actFun, output_act_fun) as pred:
        return pred.predict(features)


def sample_from_categorical(posterior_weights=None, post_prob_file=None, verbose=False):
    """Posterior-predictive resampling (np_bnn/BNN_lib.py:682-713): one class drawn per (instance, stored sample) from that
    sample's class probabilities; the point estimate of an instance is the class frequency among its draws.  The uniforms
    come from numpy's global stream in the upstream order (instance by instance, one per sample), so a seeded run
    reproduces upstream's draws; the arithmetic is done for all instances at once."""
    if posterior_weights is None:
        if not post_prob_file:
            raise ValueError("sample_from_categorical needs posterior_weights or post_prob_file")
        posterior_weights = np.load(post_prob_file)
    probs = np.asarray(posterior_weights)
    n_samples, n_instances, n_classes = probs.shape
    cdf = np.cumsum(np.transpose(probs, (1, 0, 2)), axis=2)               # [instance, sample, class]
    u = np.random.random((n_instances, n_samples))
    # the class drawn is the one whose cumulative probability exceeds u by the least (ties and a cdf that never gets there
    # fall to the first such class, as upstream's argmin over the masked differences does)
    excess = cdf - u[:, :, None]
    excess[excess < 0] = 1
    draws = np.argmin(excess, axis=2)                                      # [instance, sample]
    one_hot = draws[:, :, None] == np.arange(n_classes)[None, None, :]
    return {'predictions': one_hot.sum(axis=1) / n_samples,
            'class_counts': one_hot.sum(axis=0).astype(float),
            'post_predictions': draws.astype(float)}


def _shuffled_copy(features, columns, independently):
    """``features`` with the given column(s) permuted between the rows: every column on its own, or the block as a whole
    (rows stay intact inside the block).  Permutations from numpy's global stream (np_bnn/BNN_lib.py:366-372)."""
    out = np.array(features, dtype=np.float64, copy=True)
    if not columns:
        return out
    if independently and type(columns) == list:
        for col in columns:
            out[:, col] = np.random.permutation(out[:, col])
    else:
        out[:, columns] = np.random.permutation(out[:, columns])
    return out


def _summarise(probs, mode):
    """[sample, instance, class] probabilities -> [instance, class]: 0 share of samples voting for the class, 1 mean
    probability, 2 posterior-predictive resampling (np_bnn/BNN_lib.py:382-395)."""
    if mode == 0:
        votes = np.argmax(probs, axis=2)                                   # [sample, instance]
        return (votes[:, :, None] == np.arange(probs.shape[2])).mean(axis=0)
    if mode == 1:
        return np.mean(probs, axis=0)
    if mode == 2:
        return sample_from_categorical(posterior_weights=probs)['predictions']
    return None


def get_posterior_cat_prob(pred_features, post_samples=None, feature_index_to_shuffle=None, post_summary_mode=0,
                           unlink_features_within_block=False, actFun=None, output_act_fun=None, _predictor=None):
    """Predictions of every stored posterior sample and their summary (np_bnn/BNN_lib.py:352-397).  Returns
    ``(per-sample predictions [sample, instance, output], summary [instance, output])``."""
    if len(pred_features) == 0:
        print("Data not found.")
        return 0
    features = _shuffled_copy(pred_features, feature_index_to_shuffle, unlink_features_within_block)
    act = ActFun() if actFun is None else actFun
    if len(post_samples):
        act.reset_prm(post_samples[-1]['alphas'])          # (upstream leaves the last sample's slopes installed)
    probs = _predictor.predict(features) if _predictor is not None else _predict_samples(features, post_samples, act, output_act_fun)
    return probs, _summarise(probs, post_summary_mode)


def get_posterior_est(pkl_file):
    """Predictions of every stored posterior sample of a checkpoint on its own training and test matrices, and their means
    over the samples (np_bnn/BNN_lib.py:715-748; the regression drivers read the estimated parameters from it).  Keys as
    upstream: ``post_est`` / ``post_est_test`` [sample, row, output], ``prm_mean`` / ``prm_mean_test`` [row, output],
    ``error_prm`` (the samples' error parameters, or an empty list when the model has none)."""
    model, _, logger = load_obj(pkl_file)
    samples = logger._post_weight_samples
    act = model._act_fun
    if len(samples):
        act.reset_prm(samples[-1]['alphas'])          # (upstream leaves the last sample's slopes installed)

    def on(matrix):
        if len(matrix) == 0:
            return np.zeros((len(samples), 0, model._size_output))
        return _predict_samples(np.asarray(matrix, dtype=np.float64), samples, act, model._output_act_fun)

    est, est_test = on(model._data), on(model._test_data)
    return {'prm_mean': np.mean(est, axis=0), 'post_est': est,
            'prm_mean_test': np.mean(est_test, axis=0), 'post_est_test': est_test,
            'error_prm': [s['error_prm'] for s in samples] if (len(samples) and 'error_prm' in samples[0]) else []}


def _confusion_table(true_labels, predicted, n_classes):
    table = np.zeros((n_classes, n_classes), dtype=int)
    np.add.at(table, (np.asarray(true_labels, dtype=int), np.asarray(predicted, dtype=int)), 1)
    return table


def _write_predictions(stem, per_sample, summary, instance_id, verbose):
    """``<stem>_pred_mean_pr.txt`` (the summary, with the instance names in front when given) and ``<stem>_pred_pr.npy`` (every
    sample's predictions), as np_bnn/BNN_lib.py:489-500 writes them."""
    if len(instance_id):
        names = np.asarray(instance_id).reshape(-1, 1)
        np.savetxt(stem + '_pred_mean_pr.txt', np.hstack((names, np.round(summary, 4).astype(str))), fmt='%s', delimiter='\t')
    else:
        np.savetxt(stem + '_pred_mean_pr.txt', summary, fmt='%.3f')
    np.save(stem + '_pred_pr.npy', per_sample)
    if verbose:
        print("Predictions saved in files:\n    %s\n    %s\n" % (stem + '_pred_pr.npy', stem + '_pred_mean_pr.txt'))


def _output_stem(pickle_file, fname, wd):
    return os.path.join(wd if wd else os.path.dirname(pickle_file),
                        (fname + "_" if fname else "") + os.path.splitext(os.path.basename(pickle_file))[0])


def _accuracy_report(summary, test_labels, stem, threshold, verbose):
    """(mean accuracy, C x C confusion table) of a summary against its labels; ``<stem>_accuracy.txt`` with the true- and
    false-positive rates at ``threshold`` (np_bnn/BNN_lib.py:440-455)."""
    from .support import CalcFP, CalcTP
    accuracy = np.mean(CalcAccuracy(summary, test_labels))
    tp, fp = CalcTP(summary, test_labels, threshold=threshold), CalcFP(summary, test_labels, threshold=threshold)
    table = _confusion_table(test_labels, np.argmax(summary, axis=1), summary.shape[1])
    with open(stem + '_accuracy.txt', 'w') as fh:
        fh.write("Mean accuracy: %s (TP: %s; FP: %s)" % (accuracy, tp, fp))
    if verbose:
        print("Accuracy:", accuracy)
        print("True positive rate:", np.mean(tp))
        print("False positive rate:", np.mean(fp))
        print("Confusion matrix:\n", table)
    return accuracy, table


def _prior_mean_prediction(features, prior_samples, act, output_act_fun):
    """Mean over the prior samples of their predictions on ``features`` [row, class]: accumulated on the device
    (``npbnn_predict_sets_summary`` mode 1, no stack) when the output function has a device kind, else from the stack."""
    act.reset_prm(prior_samples[-1]['alphas'])            # (upstream installs every prior sample's slopes in turn: the last stays)
    with _SamplePredictor(features.shape[1], prior_samples, act, output_act_fun) as pred:
        if pred.custom_output:
            return np.mean(pred.predict(features), axis=0)
        pred.load(features)
        return pred.summary(1)[0]


def predictBNN(predict_features, pickle_file, test_labels=[], instance_id=[], pickle_file_prior=0, target_acc=None,
               post_cutoff=None, threshold=0.95, bf=150, post_summary_mode=0, fname="", wd="", verbose=1):
    """Posterior predictions for a feature matrix from a checkpoint ``[bnn, mcmc, logger]`` (np_bnn/BNN_lib.py:404-501), with
    upstream's keywords, defaults and order of effects.  Files, next to the checkpoint or in ``wd``:
    ``<fname_><checkpoint>_pred_pr.npy`` (every sample's predictions), ``..._pred_mean_pr.txt`` (the summary, with the
    instance names in front when given), ``..._accuracy.txt`` when labels are given (mean accuracy, and the true- / false-positive
    rates ``CalcTP`` / ``CalcFP`` at ``threshold``).

    ``pickle_file_prior``: a pickled list of prior samples (dicts with ``weights`` and ``alphas``); their mean prediction gives
    the Bayes factor of every instance's call, and the true- / false-positive rates at ``bf`` (``CalcTP_BF`` / ``CalcFP_BF``) are
    printed.  Upstream's branch cannot run as written: it calls ``RunPredict`` without an
    output function (:468).  What it means is built here - the prior samples go through the model's own output function.
    ``target_acc`` (a threshold from ``get_posterior_threshold`` on the checkpoint's test set; upstream compares against the whole
    selected row, :482-485, where the row's first entry, the threshold, is meant) or ``post_cutoff`` (a threshold given): the
    summary and every sample's slice of the stack are NaN in the instances whose largest summary value does not exceed it, in the
    returned summary and in both files (``turn_low_pp_instances_to_nan``).  ``confusion_matrix`` stays the plain C x C table."""
    from . import support
    model, _, logger = load_obj(pickle_file)
    per_sample, summary = get_posterior_cat_prob(predict_features, logger._post_weight_samples,
                                                 post_summary_mode=post_summary_mode, actFun=model._act_fun,
                                                 output_act_fun=model._output_act_fun)
    stem = _output_stem(pickle_file, fname, wd)
    result = {'post_prob_predictions': summary, 'mean_accuracy': np.nan, 'confusion_matrix': np.nan}
    if len(test_labels):
        result['mean_accuracy'], result['confusion_matrix'] = _accuracy_report(summary, test_labels, stem, threshold, verbose)
    if pickle_file_prior:
        prior_samples = load_obj(pickle_file_prior)
        prior = _prior_mean_prediction(np.asarray(predict_features, dtype=np.float64), prior_samples, model._act_fun,
                                       model._output_act_fun)
        if len(test_labels) and verbose:
            print("True positive rate (BF):", np.mean(support.CalcTP_BF(summary, prior, test_labels, threshold=bf)))
            print("False positive rate (BF):", np.mean(support.CalcFP_BF(summary, prior, test_labels, threshold=bf)))
    if target_acc or post_cutoff:
        cutoff = support.get_posterior_threshold(pickle_file, target_acc, post_summary_mode)[0] if target_acc else post_cutoff
        high_pp_indices = np.where(np.max(summary, axis=1) > cutoff)[0]
        summary = support.turn_low_pp_instances_to_nan(summary, high_pp_indices)
        per_sample = np.array([support.turn_low_pp_instances_to_nan(y, high_pp_indices) for y in per_sample])
        result['post_prob_predictions'] = summary
    _write_predictions(stem, per_sample, summary, instance_id, verbose)
    return result


def _feature_blocks(feature_blocks, names):
    """(column lists, block names): the caller's dict {name: columns} or list of column lists; one block per column when
    none is given (np_bnn/BNN_lib.py:521-533)."""
    if isinstance(feature_blocks, dict):
        if feature_blocks:
            return list(feature_blocks.values()), list(feature_blocks.keys())
        return [[i] for i in range(len(names))], list(names)
    return list(feature_blocks), ['block_%d' % i for i in range(len(feature_blocks))]


def _device_route(post_summary_mode, predictor, features, true_labels, weights_posterior):
    """Can a permutation of feature_importance stay on the device?  Summary modes 0 and 1 (mode 2 needs a uniform per instance
    and sample from the host stream), an output function with a device kind, one integer class label per instance, and
    NPBNN_FI_HOST not set."""
    if os.environ.get("NPBNN_FI_HOST", "") not in ("", "0"):
        return False
    if post_summary_mode not in (0, 1) or predictor.custom_output:
        return False
    if features.ndim != 2 or len(features) == 0 or len(weights_posterior) == 0:
        return False
    labels = np.asarray(true_labels)
    if labels.ndim != 1 or len(labels) != len(features) or labels.dtype.kind not in "iuf":
        return False
    n_classes = predictor._weights[0][-1].shape[0]
    return bool(np.all(labels == np.floor(labels)) and np.all(labels >= 0) and np.all(labels < n_classes))


def feature_importance(input_features, weights_pkl=None, weights_posterior=None, true_labels=[], fname_stem='',
                       feature_names=[], verbose=False, post_summary_mode=0, n_permutations=100, feature_blocks=dict(),
                       write_to_file=True, predictions_outdir='', unlink_features_within_block=True, actFun=None,
                       output_act_fun=None):
    """Permutation importance (np_bnn/BNN_lib.py:504-597): how much accuracy is lost when a block of feature columns is
    shuffled between the instances, ``n_permutations`` shuffles per block (numpy's global stream, upstream's order).  The
    stored samples stay packed on the device.  With ``post_summary_mode`` 0 or 1, a built-in output function and integer class
    labels the matrix is uploaded once and a shuffle is a column gather, the passes and one confusion table on the device
    (``_device_route``); otherwise (and with ``NPBNN_FI_HOST=1``) a shuffle costs one upload of the matrix and one
    ``npbnn_predict_sets``.
    Returns a data frame, most important block first, with upstream's column names; written to
    ``<fname_stem_>feature_importance.txt`` unless ``write_to_file`` is off."""
    import pandas as pd
    features = np.asarray(input_features)
    names = feature_names if len(feature_names) else np.arange(features.shape[1]).astype(str)
    blocks, block_names = _feature_blocks(feature_blocks, names)
    if weights_pkl:
        model, _, logger = load_obj(weights_pkl)
        weights_posterior, actFun, output_act_fun = logger._post_weight_samples, model._act_fun, model._output_act_fun
    act = ActFun() if actFun is None else actFun

    with _SamplePredictor(features.shape[1], weights_posterior, act, output_act_fun) as predictor:
        on_device = _device_route(post_summary_mode, predictor, features, true_labels, weights_posterior)
        if on_device:
            labels = np.asarray(true_labels).astype(np.int64).ravel()
            if len(weights_posterior):
                act.reset_prm(weights_posterior[-1]['alphas'])      # (as get_posterior_cat_prob leaves it)
            predictor.load(features)                                # the one upload

            def accuracy(shuffle=None):
                predictor.permute(shuffle, unlink_features_within_block)
                table = predictor.summary(post_summary_mode, labels, want_summary=False)[1]
                return np.trace(table) / len(labels)
        else:
            def accuracy(shuffle=None):
                summary = get_posterior_cat_prob(features, weights_posterior, feature_index_to_shuffle=shuffle,
                                                 post_summary_mode=post_summary_mode, actFun=act, output_act_fun=output_act_fun,
                                                 unlink_features_within_block=unlink_features_within_block, _predictor=predictor)[1]
                return CalcAccuracy(summary, true_labels)

        baseline = accuracy()
        if verbose:
            print("Reference accuracy (mean):", np.mean(baseline))
        shuffled = np.array([[accuracy(block) for _ in range(n_permutations)] for block in blocks])    # [block, permutation]
        if on_device:
            predictor.permute(None, False)                          # the columns go back

    loss = baseline - shuffled
    table = pd.DataFrame({'feature_block_index': np.arange(len(blocks)).astype(str), 'feature_name': [str(n) for n in block_names],
                          'delta_acc_mean': loss.mean(axis=1), 'delta_acc_std': loss.std(axis=1),
                          'acc_with_feature_randomized_mean': shuffled.mean(axis=1),
                          'acc_with_feature_randomized_std': shuffled.std(axis=1)})
    table = table.sort_values('delta_acc_mean', ascending=False)
    if write_to_file:
        out_dir = predictions_outdir if predictions_outdir else os.path.dirname(weights_pkl)
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, (fname_stem + "_" if fname_stem else "") + 'feature_importance.txt')
        table.to_csv(path, sep='\t', index=False, header=True, float_format='%.6f')
        print("Output saved in: %s" % path)
    return table
