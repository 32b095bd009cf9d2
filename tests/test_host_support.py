"""Confidence thresholds and Bayes-factor support on the host (no GPU): the array functions of npbnn_amd/support.py against the
reference's values (tests/golden/support.npz), the routing of ``get_posterior_threshold`` and ``predictBNN``'s threshold / prior
keywords over a float64 stand-in of the device context, argument checks, and the new symbol of the C ABI."""
import contextlib
import ctypes
import importlib
import io
import os
import pickle
import types

import numpy as np
import pytest

import npbnn_amd as bn
import oracle as orc
import support_cases as sc
from npbnn_amd import _capi as capi
from test_host_importance import Float64Context, _bare_context

posterior = importlib.import_module("npbnn_amd.posterior")
backend = importlib.import_module("npbnn_amd.backend")
support = importlib.import_module("npbnn_amd.support")

INPUT_CASES = [(name, s) for name in sc.INPUTS for s in (9, 10)]


class SupportContext(Float64Context):
    """Float64Context with npbnn_predict_sets_support's contract, computed in float64 numpy."""

    def predict_sets_support(self, weight_sets, mode, labels, thresholds, prior_summary=None, bf_thresholds=(), cutoff=None,
                             act_prm_sets=None, which=capi.TRAIN, want_summary=False, want_keep=False, apply_out_fn=True):
        Float64Context.log.append("predict_sets_support")
        summary = posterior._summarise(self.predict_sets(list(weight_sets), act_prm_sets), mode)
        del Float64Context.log[-1]
        cube = sc.cube_of(summary, labels, np.asarray(thresholds))
        call = np.argmax(summary, axis=1)
        p = summary[np.arange(len(call)), call]
        bf = None
        if prior_summary is not None:
            r = prior_summary[np.arange(len(call)), call]
            with np.errstate(divide="ignore", invalid="ignore"):
                factor = (p / (1e-10 + 1 - p)) / (r / (1e-10 + 1 - r))
            bf = np.zeros((len(bf_thresholds) + 1, 2), dtype=np.int64)
            np.add.at(bf, (np.sum(factor[:, None] > np.asarray(bf_thresholds)[None, :], axis=1), (call == labels).astype(int)), 1)
        keep = np.ones(len(call), dtype=bool) if cutoff is None else p > cutoff
        masked = summary.copy()
        masked[~keep] = np.nan
        return dict(cube=cube, bf=bf, summary=masked if want_summary else None, keep=keep if want_keep else None)


@pytest.fixture
def seam(monkeypatch):
    Float64Context.log = []
    monkeypatch.setattr(backend, "HipContext", SupportContext)
    monkeypatch.setattr(posterior, "CalcAccuracy", lambda y, lab: orc.acc_classification(y, np.asarray(lab)))
    monkeypatch.delenv("NPBNN_FI_HOST", raising=False)
    return Float64Context


def write_checkpoint(directory, inp, name="run"):
    """A checkpoint-shaped pickle [model, mcmc, logger] with the case's test set and stored samples."""
    model = types.SimpleNamespace(_test_data=inp["x"], _test_labels=inp["labels"], _act_fun=sc.act_for(bn, inp["fun"]),
                                  _output_act_fun=bn.SoftMax, _data=inp["x"][:3], _labels=inp["labels"][:3])
    logger = types.SimpleNamespace(_post_weight_samples=inp["samples"])
    path = os.path.join(str(directory), name + ".pkl")
    with open(path, "wb") as fh:
        pickle.dump([model, None, logger], fh)
    return path


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = f(*a, **k)
    return res, out.getvalue()


# ---- the array functions against the reference ---------------------------------------------------------------------------------
def test_golden_file_is_complete():
    g = sc.load()
    want = [name + "/prior_mean" for name in sc.INPUTS] + [sc.key(n, s) + "/near_ties" for n, s in INPUT_CASES]
    want += [sc.key(*c) + "/" + part for c in sc.CASES for part in ("summary", "table", "target", "selected", "tp_fp", "tp_fp_bf", "cube")]
    assert sorted(g.files) == sorted(want)
    for c in sc.CASES:
        table = g[sc.key(*c) + "/table"]
        assert table[-1, 1] - table[0, 1] >= 0.15 and table[:, 2].min() < 0.5 and len(table) >= 60
        assert 0 < np.where(np.all(table == g[sc.key(*c) + "/selected"], axis=1))[0][0] < len(table) - 1


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_host_functions_give_the_references_values(case):
    name, n_samples, mode = case
    g, k = sc.load(), sc.key(*case)
    summary, labels = g[k + "/summary"], sc.inputs(name, n_samples)["labels"]
    prior = g[name + "/prior_mean"]
    np.testing.assert_array_equal([[bn.CalcTP(summary, labels, threshold=t), bn.CalcFP(summary, labels, threshold=t)] for t in (0.95, 0.6)],
                                  g[k + "/tp_fp"])
    with np.errstate(divide="ignore", invalid="ignore"):
        np.testing.assert_array_equal([[bn.CalcTP_BF(summary, prior, labels, threshold=t), bn.CalcFP_BF(summary, prior, labels, threshold=t)]
                                       for t in sc.BF_GRID], g[k + "/tp_fp_bf"])
    rows = []
    for t in sc.GRID:
        try:
            s = bn.get_accuracy_threshold(summary, labels, threshold=t)
            assert sorted(s) == ['accuracy', 'confusion_matrix', 'predictions', 'retained_samples']
            rows.append([t, s['accuracy'], s['retained_samples']])
        except ZeroDivisionError:
            pass
    np.testing.assert_array_equal(np.array(rows), g[k + "/table"])
    # the cube holds the whole sweep: integer suffix sums give the same table, bit for bit
    np.testing.assert_array_equal(sc.cube_of(summary, labels), g[k + "/cube"])
    np.testing.assert_array_equal(support.table_from_cube(g[k + "/cube"], sc.GRID), g[k + "/table"])
    # ... and the rates at a threshold of the grid
    i = 59
    above = g[k + "/cube"][i + 1:].sum(axis=0)
    assert np.trace(above) / len(labels) == bn.CalcTP(summary, labels, threshold=sc.GRID[i])
    assert (above.sum() - np.trace(above)) / len(labels) == bn.CalcFP(summary, labels, threshold=sc.GRID[i])


def test_small_helpers():
    rs = np.random.default_rng(4)
    y = rs.dirichlet(np.ones(3) * 0.3, 50)
    lab = rs.integers(0, 3, 50)
    masked = bn.turn_low_pp_instances_to_nan(y, np.array([1, 7, 20]))
    assert np.isnan(masked).all(axis=1).sum() == 47 and np.array_equal(masked[[1, 7, 20]], y[[1, 7, 20]])
    cm = bn.CalcConfusionMatrix(y, lab)
    assert cm.shape == (4, 4) and cm.values[-1, -1] == 50
    np.testing.assert_array_equal(cm.values[:3, :3], orc.confusion_counts(y, lab, 3))
    res, printed = quiet(bn.CalcAccAboveThreshold, y, lab, 0.8)
    sup = np.where(y.max(axis=1) > 0.8)[0]
    pred = np.argmax(y, axis=1)[sup]
    want = np.sum((y[np.arange(len(pred)), pred] > 0.8)[pred == lab[sup]]) / len(pred)      # (upstream's look-up in the first rows)
    assert res == want and printed.strip() == str(want)


# ---- get_posterior_threshold ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("write", [True, False], ids=["files", "no_files"])
@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_threshold_device_route_reproduces_the_reference(case, write, seam, tmp_path):
    name, n_samples, mode = case
    g, k = sc.load(), sc.key(*case)
    pkl = write_checkpoint(tmp_path, sc.inputs(name, n_samples))
    out_file = str(tmp_path / "table.txt")
    row, printed = quiet(bn.get_posterior_threshold, pkl, float(g[k + "/target"]), mode, out_file, write_predictions=write)
    np.testing.assert_array_equal(row, g[k + "/selected"])
    np.testing.assert_array_equal(np.loadtxt(out_file, skiprows=1), np.round(g[k + "/table"], 3))
    assert open(out_file).readline().split() == ['Threshold', 'Accuracy', 'Retained_data']
    assert printed.splitlines() == ["Selected threshold: PP = %s yielding test accuracy ~ %s" % (np.round(row[0], 3), float(g[k + "/target"])),
                                    "Retained instances above threshold: %s" % np.round(row[2], 3)]
    log = seam.log
    assert log.count("set_data") == 1 and log.count("predict_sets_support") == 1 and log.count("predict_sets") == (1 if write else 0)
    files = sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("run_"))
    assert files == (["run_accuracy.txt", "run_pred_mean_pr.txt", "run_pred_pr.npy"] if write else [])


@pytest.mark.parametrize("how", ["mode2", "callable", "env"])
def test_threshold_host_route(how, seam, tmp_path, monkeypatch):
    inp = sc.inputs("tanh", 9)
    g, k = sc.load(), sc.key("tanh", 9, 1)
    pkl = write_checkpoint(tmp_path, inp)
    mode = 1
    if how == "mode2":
        mode = 2
        np.random.seed(3)
    elif how == "env":
        monkeypatch.setenv("NPBNN_FI_HOST", "1")
    else:
        monkeypatch.setattr(SupportContext, "set_arch_from_weights",
                            lambda self, w, *a: (setattr(self, "shapes", [m.shape for m in w]), setattr(self, "fun", "tanh")))
        model, mcmc, logger = bn.load_obj(pkl)
        model._output_act_fun = _custom_output
        bn.SaveObject([model, mcmc, logger], pkl)
    row, _ = quiet(bn.get_posterior_threshold, pkl, 0.9, mode)
    assert "predict_sets_support" not in seam.log and seam.log.count("predict_sets") == 1
    assert os.path.exists(str(tmp_path / "run_pred_pr.npy"))
    if how != "mode2":
        table = g[k + "/table"]
        np.testing.assert_array_equal(row, table[np.min(np.where(np.round(table[:, 1], 2) >= 0.9))])


def _custom_output(z):
    return z                      # (the stand-in's predict_sets has applied the softmax already)


def test_unreachable_target_exits_with_the_references_message(seam, tmp_path, monkeypatch):
    pkl = write_checkpoint(tmp_path, sc.inputs("genrelu", 9))
    for host in (False, True):
        if host:
            monkeypatch.setenv("NPBNN_FI_HOST", "1")
        with pytest.raises(SystemExit) as e:
            quiet(bn.get_posterior_threshold, pkl, 1.01, 0)
        assert str(e.value) == 'Target accuracy can not be reached. Please set threshold lower or try different post_summary_mode.'


# ---- predictBNN's keywords -----------------------------------------------------------------------------------------------------
def test_predictbnn_signature_is_the_references():
    import inspect
    prm = inspect.signature(bn.predictBNN).parameters
    assert list(prm) == ['predict_features', 'pickle_file', 'test_labels', 'instance_id', 'pickle_file_prior', 'target_acc', 'post_cutoff',
                         'threshold', 'bf', 'post_summary_mode', 'fname', 'wd', 'verbose']
    assert [prm[n].default for n in ('pickle_file_prior', 'target_acc', 'post_cutoff', 'threshold', 'bf')] == [0, None, None, 0.95, 150]


@pytest.mark.parametrize("case", [("tanh", 10, 0), ("genrelu", 9, 1), ("swish_bias3", 10, 1)], ids=sc.case_id)
def test_predictbnn_cutoff_target_and_prior(case, seam, tmp_path):
    name, n_samples, mode = case
    g, k = sc.load(), sc.key(*case)
    inp = sc.inputs(name, n_samples)
    summary, labels = g[k + "/summary"], inp["labels"]
    pkl = write_checkpoint(tmp_path, inp)
    prior_pkl = str(tmp_path / "prior.pkl")
    bn.SaveObject(inp["prior"], prior_pkl)
    # a cutoff given, the prior samples, TP / FP at a threshold of the caller's
    res, printed = quiet(bn.predictBNN, inp["x"], pkl, test_labels=labels, post_cutoff=0.7, threshold=0.6, bf=20.0,
                         pickle_file_prior=prior_pkl, post_summary_mode=mode, fname="cut")
    assert sorted(res) == ['confusion_matrix', 'mean_accuracy', 'post_prob_predictions']
    low = ~(summary.max(axis=1) > 0.7)
    assert 0 < low.sum() < len(low)
    np.testing.assert_array_equal(np.isnan(res['post_prob_predictions']).all(axis=1), low)
    np.testing.assert_array_equal(res['post_prob_predictions'][~low], summary[~low])
    stack = np.load(str(tmp_path / "cut_run_pred_pr.npy"))
    assert stack.shape == (n_samples, len(labels), inp["n_classes"])
    assert np.isnan(stack[:, low]).all() and not np.isnan(stack[:, ~low]).any()
    assert np.isnan(np.loadtxt(str(tmp_path / "cut_run_pred_mean_pr.txt"))).all(axis=1).sum() == low.sum()
    assert res['confusion_matrix'].shape == (inp["n_classes"],) * 2 and res['confusion_matrix'].sum() == len(labels)
    tp, fp = g[k + "/tp_fp"][1]
    assert open(str(tmp_path / "cut_run_accuracy.txt")).read() == "Mean accuracy: %s (TP: %s; FP: %s)" % (res['mean_accuracy'], tp, fp)
    tp_bf, fp_bf = g[k + "/tp_fp_bf"][list(sc.BF_GRID).index(20.0)]
    assert "True positive rate: %s\n" % tp in printed and "False positive rate: %s\n" % fp in printed
    assert "True positive rate (BF): %s\n" % tp_bf in printed and "False positive rate (BF): %s\n" % fp_bf in printed
    assert "predict_sets_summary" in seam.log                     # the prior samples' mean: no stack
    # a target accuracy: the threshold get_posterior_threshold selects on the checkpoint's test set
    res, _ = quiet(bn.predictBNN, inp["x"], pkl, test_labels=labels, target_acc=float(g[k + "/target"]), post_summary_mode=mode, verbose=0)
    low = ~(summary.max(axis=1) > g[k + "/selected"][0])
    np.testing.assert_array_equal(np.isnan(res['post_prob_predictions']).all(axis=1), low)
    assert np.mean(~low) == g[k + "/selected"][2]


def test_predictbnn_default_arguments_only_add_the_rates_to_the_accuracy_file(seam, tmp_path):
    inp = sc.inputs("tanh", 9)
    pkl = write_checkpoint(tmp_path, inp)
    res, _ = quiet(bn.predictBNN, inp["x"], pkl, test_labels=inp["labels"], post_summary_mode=1, verbose=0)
    np.testing.assert_array_equal(res['post_prob_predictions'], sc.load()[sc.key("tanh", 9, 1) + "/summary"])
    assert not np.isnan(np.load(str(tmp_path / "run_pred_pr.npy"))).any()
    text = open(str(tmp_path / "run_accuracy.txt")).read()
    assert text.startswith("Mean accuracy: %s (TP: " % res['mean_accuracy']) and text.endswith(")")


# ---- argument checks raise before any device call ------------------------------------------------------------------------------
def test_argument_checks_in_python():
    ctx = _bare_context()
    sets, lab = [np.zeros(5)], np.zeros(10)
    for bad in (dict(mode=2), dict(labels=None), dict(labels=np.zeros(9)), dict(thresholds=[0.5, 0.4]), dict(thresholds=[0.1, np.nan]),
                dict(bf_thresholds=[1.0]), dict(prior_summary=np.zeros((10, 2))), dict(prior_summary=np.zeros((10, 3)), bf_thresholds=[3.0, 1.0]),
                dict(cutoff=np.nan)):
        kw = dict(mode=0, labels=lab, thresholds=[0.1, 0.2])
        kw.update(bad)
        with pytest.raises(ValueError):
            ctx.predict_sets_support(sets, kw.pop("mode"), kw.pop("labels"), kw.pop("thresholds"), **kw)
    ctx.close = lambda: None


def test_the_new_symbol_is_declared_bound_and_exported():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "npbnn_predict_sets_support(" in open(os.path.join(root, "include", "npbnn_hip.h")).read()
    assert len(capi.SIGNATURES["npbnn_predict_sets_support"][1]) == 18
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "npbnn_predict_sets_support")
    for name in ("get_posterior_threshold", "get_accuracy_threshold", "turn_low_pp_instances_to_nan", "CalcTP", "CalcFP", "CalcTP_BF",
                 "CalcFP_BF", "CalcAccAboveThreshold", "CalcConfusionMatrix"):
        assert callable(getattr(bn, name))
