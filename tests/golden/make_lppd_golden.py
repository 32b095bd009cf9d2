#!/usr/bin/env python3
"""Generate tests/golden/lppd.npz with the REFERENCE (np_bnn 0.1.23): per stored sample ``RunPredict`` (np_bnn/BNN_lib.py:245-256) with the
model's output function, then the summands of its own likelihoods - ``np.log(prediction[sample_id, labels])`` (calc_likelihood, :121)
and ``scipy.stats.norm.logpdf(true_values, prediction, sig2)`` summed over the target columns (calc_likelihood_regression, :131) -
and, in float64, the definitions of lppd, mean log-likelihood, p_waic (variance with ddof 1) and the per-sample totals.  Runs only
beside a checkout of the upstream repository (imported unmodified; only numeric outputs on seeded synthetic inputs are stored).
    NPBNN_UPSTREAM_DIR=<np_bnn checkout> python tests/golden/make_lppd_golden.py

Inputs: ``lppd_cases.inputs``.  A condition on the fixture, asserted here: the reference's log(softmax) is finite on every row of
every sample, and no row's log-likelihoods are so spread that the weight scales would have to be called degenerate."""
import os
import sys

import numpy as np
import scipy.special
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

import lppd_cases as lc  # noqa: E402


def reference_log_lik(inp):
    rows = []
    act = lc.act_for(bn, inp["fun"], len(inp["nodes"]))
    for smp in inp["samples"]:
        act.reset_prm(smp["alphas"])
        if inp["kind"] == "cat":
            pred = bn.RunPredict(inp["x"], smp["weights"], actFun=act, output_act_fun=bn.SoftMax)
            rows.append(np.log(pred[np.arange(len(pred)), inp["labels"]]))
        else:
            pred = bn.RunPredict(inp["x"], smp["weights"], actFun=act, output_act_fun=bn.RegressTransform)
            rows.append(np.sum(scipy.stats.norm.logpdf(inp["labels"], pred, np.asarray(smp["error_prm"])), axis=1))
    return np.array(rows, dtype=np.float64)


def main():
    out = {}
    for name in lc.CASES:
        inp = lc.inputs(name)
        ll = reference_log_lik(inp)
        s, n = ll.shape
        assert (s, n) == (lc.CASES[name]["s"], lc.N_ROWS)
        assert np.all(np.isfinite(ll)), name                      # the condition on the fixture
        assert ll.min() > -200.0, (name, ll.min())
        out[lc.key(name, "lppd_i")] = scipy.special.logsumexp(ll, axis=0) - np.log(s)
        out[lc.key(name, "mean_log_lik_i")] = np.mean(ll, axis=0)
        out[lc.key(name, "p_waic_i")] = np.var(ll, axis=0, ddof=1) if s > 1 else np.zeros(n)
        out[lc.key(name, "log_lik_sample")] = np.sum(ll, axis=1)
        print("%-22s S %2d  ll in [%8.3f, %7.4f]  lppd %10.4f  p_waic %9.4f" % (name, s, ll.min(), ll.max(), out[lc.key(name, "lppd_i")].sum(),
                                                                              out[lc.key(name, "p_waic_i")].sum()))
    path = os.path.join(HERE, "lppd.npz")
    np.savez_compressed(path, **out)
    print("wrote %d arrays to lppd.npz (%d bytes)" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
