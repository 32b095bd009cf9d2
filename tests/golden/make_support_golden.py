#!/usr/bin/env python3
"""Generate tests/golden/support.npz from the REFERENCE's confidence-threshold tools (np_bnn 0.1.23, np_bnn/BNN_lib.py:
get_posterior_cat_prob :352-397, CalcTP / CalcFP :305-317, CalcTP_BF / CalcFP_BF :320-337, get_accuracy_threshold :627-637,
get_posterior_threshold :640-671).  Runs only beside a checkout of the upstream repository (imported unmodified; only its numeric
outputs on seeded synthetic inputs are stored).  Usage:
    NPBNN_UPSTREAM_DIR=<np_bnn checkout> python tests/golden/make_support_golden.py

Inputs: ``support_cases.inputs`` (a teacher network, stored samples around it, the teacher's calls with 2 % flipped as labels; 2000
rows; the three activations of ``cases.POSTERIOR_CASES``, one with 6 classes; 9 and 10 stored samples; summary modes 0 and 1).
Per (activation, samples, mode): the reference's summary, the table of its sweep of 99 thresholds, a target accuracy and the row
get_posterior_threshold selects for it (from a checkpoint-shaped pickle), CalcTP / CalcFP at 0.95 and 0.6, CalcTP_BF / CalcFP_BF
against the mean prediction of prior samples at four Bayes factors, and the cube [threshold bin, label, call] of the summary.  Per
(activation, samples): the near-ties of the stack - [row, sample, runner-up] wherever a sample's two leading probabilities lie
within the project's float32 tolerance.  Per activation: the prior samples' mean prediction.
The conditions the tests rest on are asserted here, on the reference alone."""
import contextlib
import io
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
UPSTREAM = os.environ.get("NPBNN_UPSTREAM_DIR")
if not UPSTREAM:
    sys.exit("NPBNN_UPSTREAM_DIR: set it to a checkout of the upstream np_bnn repository (0.1.23)")
sys.path.insert(0, UPSTREAM)

import np_bnn as bn  # noqa: E402  (the reference)

import support_cases as sc  # noqa: E402


def sweep(summary, labels):
    """get_posterior_threshold's loop (:652-659) over the reference's get_accuracy_threshold."""
    rows = []
    for t in np.linspace(0.01, 0.99, 99):
        try:
            s = bn.get_accuracy_threshold(summary, labels, threshold=t)
            rows.append([t, s['accuracy'], s['retained_samples']])
        except ZeroDivisionError:
            pass
    return np.array(rows)


def main():
    out = {}
    report = []
    for name in sc.INPUTS:
        for n_samples in (9, 10):
            inp = sc.inputs(name, n_samples)
            x, labels, c = inp["x"], inp["labels"], inp["n_classes"]
            # the prior samples' mean prediction: what predictBNN's prior branch means (:460-472, RunPredict with the output function)
            act = sc.act_for(bn, inp["fun"])
            prior_stack = []
            for smp in inp["prior"]:
                act.reset_prm(smp["alphas"])
                prior_stack.append(bn.RunPredict(x, smp["weights"], actFun=act, output_act_fun=bn.SoftMax))
            prior_mean = np.mean(np.array(prior_stack), axis=0)
            out[name + "/prior_mean"] = prior_mean
            stack = None
            for mode in (0, 1):
                k = sc.key(name, n_samples, mode)
                act = sc.act_for(bn, inp["fun"])
                stack, summary = bn.get_posterior_cat_prob(x, inp["samples"], post_summary_mode=mode, actFun=act, output_act_fun=bn.SoftMax)
                table = sweep(summary, labels)
                # a target that selects a row strictly inside the table
                acc2 = np.round(table[:, 1], 2)
                target = float(acc2[len(table) // 2])
                idx = int(np.min(np.where(acc2 >= target)))
                assert 0 < idx < len(table) - 1, (k, idx, len(table))
                # ... and the reference's own get_posterior_threshold on a checkpoint-shaped pickle selects that row
                with tempfile.TemporaryDirectory() as tmp:
                    model = types.SimpleNamespace(_test_data=x, _test_labels=labels, _act_fun=sc.act_for(bn, inp["fun"]), _output_act_fun=bn.SoftMax)
                    logger = types.SimpleNamespace(_post_weight_samples=inp["samples"])
                    pkl = os.path.join(tmp, "run.pkl")
                    with open(pkl, "wb") as fh:
                        pickle.dump([model, None, logger], fh)
                    with contextlib.redirect_stdout(io.StringIO()):
                        selected = bn.get_posterior_threshold(pkl, target_acc=target, post_summary_mode=mode)
                np.testing.assert_array_equal(selected, table[idx])
                # the conditions the tests rest on
                assert table[:, 1].max() - table[0, 1] >= 0.15 and table[-1, 1] - table[0, 1] >= 0.15, (k, table[0], table[-1])
                assert table[:, 2].min() < 0.5, (k, table[:, 2].min())
                assert len(table) >= 60, (k, len(table))
                ties = sc.near_ties_of(stack)
                border = sc.candidate_cells(summary, labels, mode, n_samples, ties)
                assert len(border) <= 0.02 * len(labels), (k, len(border))
                cube = sc.cube_of(summary, labels)
                assert cube.sum() == len(labels)
                out[k + "/summary"] = summary
                out[k + "/table"] = table
                out[k + "/target"] = np.array(target)
                out[k + "/selected"] = np.asarray(selected, dtype=np.float64)
                out[k + "/tp_fp"] = np.array([[bn.CalcTP(summary, labels, threshold=t), bn.CalcFP(summary, labels, threshold=t)] for t in (0.95, 0.6)])
                with np.errstate(divide="ignore", invalid="ignore"):
                    out[k + "/tp_fp_bf"] = np.array([[bn.CalcTP_BF(summary, prior_mean, labels, threshold=t),
                                                      bn.CalcFP_BF(summary, prior_mean, labels, threshold=t)] for t in sc.BF_GRID])
                out[k + "/cube"] = cube
                report.append("%-22s rows %2d  acc %.3f -> %.3f  retained min %.3f  target %.2f -> row %2d  borderline %d"
                              % (k, len(table), table[0, 1], table[-1, 1], table[:, 2].min(), target, idx, len(border)))
            out[sc.key(name, n_samples) + "/near_ties"] = sc.near_ties_of(stack)
    np.savez_compressed(os.path.join(HERE, "support.npz"), **out)
    print("\n".join(report))
    print("wrote %d arrays to support.npz (%d bytes)" % (len(out), os.path.getsize(os.path.join(HERE, "support.npz"))))


if __name__ == "__main__":
    main()
