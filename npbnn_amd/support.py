"""Confidence thresholds and Bayes-factor support of posterior predictions: ``CalcTP``, ``CalcFP``, ``CalcTP_BF``, ``CalcFP_BF``,
``CalcAccAboveThreshold``, ``CalcConfusionMatrix``, ``get_accuracy_threshold``, ``get_posterior_threshold``,
``turn_low_pp_instances_to_nan`` (reference: np_bnn/BNN_lib.py:221-226, 305-349, 627-679) - the "abstain below a confidence
threshold" workflow: which posterior probability must a call reach for the calls above it to be right ``target_acc`` of the time?

The array-in, number-out functions are host numpy and give the reference's values to the last bit.  ``get_posterior_threshold``
is the expensive one upstream: a ``predictBNN`` that materialises the [sample, row, class] stack, then 99 thresholds, each a pass over
all rows with a cross-tabulation.  Here (summary modes 0 and 1, a built-in output function, integer labels: ``posterior._device_route``)
the checkpoint's test matrix is uploaded once and one ``npbnn_predict_sets_support`` call returns an integer cube
[threshold bin, label, call]: every threshold's accuracy and retained share are suffix sums of it."""
import sys

import numpy as np

from .files import load_obj

small_number = 1e-10

THRESHOLD_GRID = (0.01, 0.99, 99)       # np.linspace arguments of the sweep (np_bnn/BNN_lib.py:653)


def _calls(y):
    """(the class called per row - the first among equal ones -, its value)"""
    prediction = np.argmax(y, axis=1)
    return prediction, y[np.arange(len(prediction)), prediction]


def CalcTP(y, lab, threshold=0.95):
    """Share of all rows called correctly with a value above ``threshold``."""
    prediction, max_p = _calls(y)
    z = (max_p > threshold).astype(float)
    return np.sum(z[prediction == lab]) / len(prediction)


def CalcFP(y, lab, threshold=0.95):
    """Share of all rows called wrongly with a value above ``threshold``."""
    prediction, max_p = _calls(y)
    z = (max_p > threshold).astype(float)
    return np.sum(z[prediction != lab]) / len(prediction)


def _bayes_factor(y, y_p):
    prediction, max_p = _calls(y)
    prior = y_p[np.arange(len(prediction)), prediction]
    return prediction, (max_p / (small_number + 1 - max_p)) / (prior / (small_number + 1 - prior))


def CalcTP_BF(y, y_p, lab, threshold=150):
    """Share of all rows called correctly with a Bayes factor (posterior odds of the call over its prior odds ``y_p``) above
    ``threshold``."""
    prediction, bf = _bayes_factor(y, y_p)
    z = (bf > threshold).astype(float)
    return np.sum(z[prediction == lab]) / len(prediction)


def CalcFP_BF(y, y_p, lab, threshold=150):
    """Share of all rows called wrongly with a Bayes factor above ``threshold``."""
    prediction, bf = _bayes_factor(y, y_p)
    z = (bf > threshold).astype(float)
    return np.sum(z[prediction != lab]) / len(prediction)


def CalcAccAboveThreshold(y, lab, threshold=0.95):
    """Prints (as upstream does) and returns upstream's figure: among the rows whose largest value exceeds ``threshold``, the share
    called correctly AND confirmed by a second look-up - which upstream makes in the first rows of ``y`` instead of the supported
    ones (np_bnn/BNN_lib.py:344); kept, since the value is the reference's."""
    supported = np.where(np.max(y, axis=1) > threshold)
    prediction = np.argmax(y, axis=1)[supported]
    max_p = y[np.arange(len(prediction)), prediction]
    z = (max_p > threshold).astype(float)
    res = np.sum(z[prediction == np.asarray(lab)[supported]]) / len(prediction)
    print(res)
    return res


def CalcConfusionMatrix(y, lab):
    """Cross-tabulation of labels against calls with margins, over the classes present among the labels (a pandas data frame)."""
    import pandas as pd
    classes = np.unique(lab)
    actual = pd.Categorical(lab, categories=classes)
    called = pd.Categorical(np.argmax(y, axis=1), categories=classes)
    return pd.crosstab(actual, called, margins=True, rownames=['True'], colnames=['Predicted'], dropna=False)


def turn_low_pp_instances_to_nan(pred, high_pp_indices):
    """``pred`` with every row outside ``high_pp_indices`` NaN."""
    out = np.full(np.shape(pred), np.nan)
    out[high_pp_indices] = pred[high_pp_indices]
    return out


def get_accuracy_threshold(probs, labels, threshold=0.75):
    """Calls, accuracy, retained share and confusion table of the rows whose largest value exceeds ``threshold``; no such row is a
    ZeroDivisionError, as upstream."""
    indx = np.where(np.max(probs, axis=1) > threshold)[0]
    supported, labels_supported = probs[indx, :], labels[indx]
    pred = np.argmax(supported, axis=1)
    accuracy = len(pred[pred == labels_supported]) / len(pred)
    return {'predictions': pred, 'accuracy': accuracy, 'retained_samples': len(pred) / len(labels),
            'confusion_matrix': CalcConfusionMatrix(supported, labels_supported)}


def table_from_cube(cube, thresholds):
    """Rows ``[threshold, accuracy, retained share]`` from ``npbnn_predict_sets_support``'s cube [bin, label, call]: the rows retained
    at ``thresholds[i]`` are the bins above ``i``, so both counts are suffix sums; accuracy and share are the integer ratios
    ``correct / kept`` and ``kept / n`` get_accuracy_threshold forms.  Thresholds that retain no row are left out."""
    cube = np.asarray(cube)
    per_bin = cube.sum(axis=(1, 2))
    correct_per_bin = np.trace(cube, axis1=1, axis2=2)
    kept = np.cumsum(per_bin[::-1])[::-1][1:]
    correct = np.cumsum(correct_per_bin[::-1])[::-1][1:]
    n = int(per_bin.sum())
    some = kept > 0
    return np.column_stack((np.asarray(thresholds, dtype=np.float64)[some], correct[some] / kept[some], kept[some] / n)).reshape(-1, 3)


def _select(table, target_acc, output_file):
    if output_file is not None:
        import pandas as pd
        df = np.round(pd.DataFrame(table, columns=['Threshold', 'Accuracy', 'Retained_data']), 3)
        df.to_csv(path_or_buf=output_file, sep='\t', index=False, header=True)
    reached = np.where(np.round(table[:, 1], 2) >= target_acc)[0]
    if len(reached) == 0:
        sys.exit('Target accuracy can not be reached. Please set threshold lower or try different post_summary_mode.')
    selected_row = table[np.min(reached), :]
    print("Selected threshold: PP =", np.round(selected_row[0], 3), "yielding test accuracy ~ %s" % (target_acc))
    print("Retained instances above threshold:", np.round(selected_row[2], 3))
    return selected_row


def get_posterior_threshold(pkl_file, target_acc=0.9, post_summary_mode=1, output_file=None, *, write_predictions=True):
    """The lowest of 99 posterior-probability thresholds (0.01 ... 0.99) at which the calls above it on the checkpoint's own test
    set reach ``target_acc`` (accuracy rounded to 2 decimals): ``[threshold, accuracy, retained share]``; ``sys.exit`` with upstream's
    message when none does.  ``output_file``: the whole table, tab-separated, rounded to 3.

    Summary modes 0 and 1 with a built-in output function and integer labels stay on the device: one upload of the test matrix, one
    ``npbnn_predict_sets_support`` with the 99 thresholds, the table from the cube (``table_from_cube``).  Mode 2, a custom output
    callable and ``NPBNN_FI_HOST=1`` go through ``predictBNN`` and ``get_accuracy_threshold`` per threshold, as upstream.  Upstream's
    call leaves ``predictBNN``'s three files of the test set beside the checkpoint; so does this one, unless ``write_predictions`` is
    off - the route on which the stack of per-sample predictions is never built."""
    from . import posterior
    model, _, logger = load_obj(pkl_file)
    features = np.asarray(model._test_data, dtype=np.float64)
    labels = np.asarray(model._test_labels)
    samples, act, out_fn = logger._post_weight_samples, model._act_fun, model._output_act_fun
    grid = np.linspace(*THRESHOLD_GRID)
    if len(samples):
        with posterior._SamplePredictor(features.shape[1] if features.ndim == 2 else 0, samples, act, out_fn) as predictor:
            if posterior._device_route(post_summary_mode, predictor, features, labels, samples):
                int_labels = labels.astype(np.int64).ravel()
                act.reset_prm(samples[-1]['alphas'])                        # (as get_posterior_cat_prob leaves it)
                predictor.load(features)                                    # the one upload
                if write_predictions:
                    stack = predictor.predict_loaded()
                    summary = posterior._summarise(stack, post_summary_mode)
                    stem = posterior._output_stem(pkl_file, "", "")
                    posterior._accuracy_report(summary, labels, stem, 0.95, 0)
                    posterior._write_predictions(stem, stack, summary, [], 0)
                table = table_from_cube(predictor.support(post_summary_mode, int_labels, grid)['cube'], grid)
                return _select(table, target_acc, output_file)
    if write_predictions:
        res = posterior.predictBNN(model._test_data, pickle_file=pkl_file, test_labels=model._test_labels,
                                   post_summary_mode=post_summary_mode, verbose=0)['post_prob_predictions']
    else:
        res = posterior.get_posterior_cat_prob(model._test_data, samples, post_summary_mode=post_summary_mode, actFun=act,
                                               output_act_fun=out_fn)[1]
    rows = []
    for t in grid:
        try:
            scores = get_accuracy_threshold(res, labels, threshold=t)
            rows.append([t, scores['accuracy'], scores['retained_samples']])
        except ZeroDivisionError:                                       # no row above this threshold
            pass
    return _select(np.array(rows, dtype=np.float64).reshape(-1, 3), target_acc, output_file)
