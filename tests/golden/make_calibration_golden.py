#!/usr/bin/env python3
"""Generate tests/golden/calibration.npz with the REFERENCE (np_bnn 0.1.23): per stored sample ``RunPredict`` (np_bnn/BNN_lib.py:245-256)
with ``SoftMax`` (:166), ``RegressTransform`` (:174) or ``RegressTransformError`` (:177), then, in float64, the definitions of
posterior calibration: the mean probabilities' confidence, predicted class, Brier score and negative log-likelihood per row with
the reliability table; the probability integral transform under the mixture of the samples' normal predictive distributions
(``scipy.stats.norm.cdf``), the mean and the squared error per (row, target) with the histogram of the transform and the coverage
counts.  Runs only beside a checkout of the upstream repository (imported unmodified; only numeric outputs on seeded synthetic
inputs are stored).
    NPBNN_UPSTREAM_DIR=<np_bnn checkout> python tests/golden/make_calibration_golden.py

Inputs: ``calibration_cases.inputs``, bins and levels ``calibration_cases.params``.  Only the pointwise arrays and the tables are
stored.  Conditions on the fixture, printed here and asserted in tests/test_host_calibration.py: no confidence or transform within
1e-9 of an edge, and at most 4 rows of a case within 1e-4 of one or with their two largest mean probabilities within 2e-4."""
import os
import sys

import numpy as np
import scipy.stats

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
UPSTREAM = os.environ.get("NPBNN_UPSTREAM_DIR")
if not UPSTREAM:
    sys.exit("NPBNN_UPSTREAM_DIR: set it to a checkout of the upstream np_bnn repository (0.1.23)")
sys.path.insert(0, UPSTREAM)

import np_bnn as bn  # noqa: E402  (the reference)

import calibration_cases as cc  # noqa: E402

OUT_FN = {"cat": bn.SoftMax, "reg": bn.RegressTransform, "err": bn.RegressTransformError}


def reference_stack(inp):
    act = cc.act_for(bn, inp["fun"], len(inp["nodes"]))
    stack = []
    for smp in inp["samples"]:
        act.reset_prm(smp["alphas"])
        stack.append(np.array(bn.RunPredict(inp["x"], smp["weights"], actFun=act, output_act_fun=OUT_FN[inp["kind"]]), dtype=np.float64))
    return np.array(stack)


def calibrate(inp, y, n_bins, levels):
    n_rows = y.shape[1]
    if inp["kind"] == "cat":
        lab = np.asarray(inp["labels"], dtype=np.int64)
        m = y.mean(axis=0)
        best = np.argmax(m, axis=1)
        conf = m.max(axis=1)
        top = np.sort(m, axis=1)
        onehot = np.eye(m.shape[1])[lab]
        bins = np.minimum(n_bins - 1, np.floor(conf * n_bins).astype(np.int64))
        hist = lambda w=None, sel=slice(None): np.bincount(bins[sel], weights=None if w is None else w[sel], minlength=n_bins)      # noqa: E731
        return dict(confidence=conf, predicted_class=best.astype(np.int64), brier_i=((m - onehot) ** 2).sum(axis=1),
                    nll_i=-np.log(m[np.arange(n_rows), lab]), count=hist().astype(np.int64), sum_confidence=hist(conf).astype(np.float64),
                    n_correct=hist(sel=best == lab).astype(np.int64), top_two_gap=top[:, -1] - top[:, -2])
    if inp["kind"] == "err":
        t = y.shape[2] // 2
        mu, sig = y[:, :, :t], y[:, :, t:]
    else:
        mu, sig = y, np.array([np.ones(y.shape[2]) * smp["error_prm"] for smp in inp["samples"]])[:, None, :]
    target = np.asarray(inp["labels"], dtype=np.float64).reshape(n_rows, -1)
    pit = scipy.stats.norm.cdf(target[None], mu, sig).mean(axis=0)
    mean = mu.mean(axis=0)
    bins = np.minimum(n_bins - 1, np.floor(pit * n_bins).astype(np.int64))
    pit_hist = np.array([np.bincount(bins[:, k], minlength=n_bins) for k in range(pit.shape[1])], dtype=np.int64)
    covered = np.array([[np.sum(np.abs(pit[:, k] - 0.5) <= lv / 2) for lv in levels] for k in range(pit.shape[1])], dtype=np.int64)
    return dict(pit=pit, mean=mean, sq_err=(target - mean) ** 2, pit_hist=pit_hist, covered=covered.reshape(pit.shape[1], len(levels)))


def main():
    out = {}
    for name in cc.CASES:
        inp = cc.inputs(name)
        n_bins, levels = cc.params(name)
        y = reference_stack(inp)
        assert y.shape[:2] == (cc.CASES[name]["s"], cc.N_ROWS)
        res = calibrate(inp, y, n_bins, levels)
        assert sorted(res) == sorted(cc.fields_of(name))
        for f, v in res.items():
            out[cc.key(name, f)] = np.asarray(v)
        cat = inp["kind"] == "cat"
        value = res["confidence" if cat else "pit"]
        gap = res["top_two_gap"] if cat else None
        print("%-22s B %2d levels %d  rows within 1e-9 of an edge %d, within 1e-4 (or top two within 2e-4) %d  %s"
              % (name, n_bins, len(levels), cc.rows_near_an_edge(name, value, 1e-9), cc.rows_near_an_edge(name, value, 1e-4, gap, 2e-4),
                 "accuracy %.3f mean confidence %.3f" % (np.mean(res["predicted_class"] == inp["labels"]), value.mean()) if cat
                 else "mean pit %s" % np.round(value.mean(axis=0), 3)))
    path = os.path.join(HERE, "calibration.npz")
    np.savez_compressed(path, **out)
    print("wrote %d arrays to calibration.npz (%d bytes)" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
