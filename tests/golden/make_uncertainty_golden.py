#!/usr/bin/env python3
"""Generate tests/golden/uncertainty.npz with the REFERENCE (np_bnn 0.1.23): per stored sample ``RunPredict`` (np_bnn/BNN_lib.py:245-256)
with ``SoftMax`` (:166), ``RegressTransform`` (:174) or ``RegressTransformError`` (:177), then, in float64, the definitions of the
uncertainty decomposition: the mean probabilities, the entropy of the mean (``scipy.special.entr``), the mean of the samples'
entropies and their difference; the mean, the variance over the samples (ddof 0) and the mean of the squared sigmas.  Runs only
beside a checkout of the upstream repository (imported unmodified; only numeric outputs on seeded synthetic inputs are stored).
    NPBNN_UPSTREAM_DIR=<np_bnn checkout> python tests/golden/make_uncertainty_golden.py

Inputs: ``uncertainty_cases.inputs``.  Conditions on the fixture, asserted here: every value is finite, and the mutual information
of every classification case with more than one sample has a maximum above 1e-2 (the cases are not degenerate)."""
import os
import sys

import numpy as np
import scipy.special

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
UPSTREAM = os.environ.get("NPBNN_UPSTREAM_DIR")
if not UPSTREAM:
    sys.exit("NPBNN_UPSTREAM_DIR: set it to a checkout of the upstream np_bnn repository (0.1.23)")
sys.path.insert(0, UPSTREAM)

import np_bnn as bn  # noqa: E402  (the reference)

import uncertainty_cases as uc  # noqa: E402

OUT_FN = {"cat": bn.SoftMax, "reg": bn.RegressTransform, "err": bn.RegressTransformError}


def reference_stack(inp):
    act = uc.act_for(bn, inp["fun"], len(inp["nodes"]))
    stack = []
    for smp in inp["samples"]:
        act.reset_prm(smp["alphas"])
        stack.append(np.array(bn.RunPredict(inp["x"], smp["weights"], actFun=act, output_act_fun=OUT_FN[inp["kind"]]), dtype=np.float64))
    return np.array(stack)


def decompose(inp, y):
    s = y.shape[0]
    if inp["kind"] == "cat":
        mean_prob = y.mean(axis=0)
        predictive = scipy.special.entr(mean_prob).sum(axis=1)
        expected = scipy.special.entr(y).sum(axis=2).mean(axis=0)
        mutual = np.maximum(0.0, predictive - expected) if s > 1 else np.zeros(y.shape[1])
        return dict(mean_prob=mean_prob, predictive_entropy_i=predictive, expected_entropy_i=expected, mutual_information_i=mutual)
    if inp["kind"] == "err":
        t = y.shape[2] // 2
        mu, aleatoric = y[:, :, :t], np.mean(y[:, :, t:] ** 2, axis=0)
    else:
        mu = y
        aleatoric = np.tile(np.mean(np.array([smp["error_prm"] for smp in inp["samples"]]) ** 2, axis=0), (y.shape[1], 1))
    return dict(mean=np.mean(mu, axis=0), epistemic_var=np.var(mu, axis=0), aleatoric_var=aleatoric)


def main():
    out = {}
    for name in uc.CASES:
        inp = uc.inputs(name)
        y = reference_stack(inp)
        assert y.shape[:2] == (uc.CASES[name]["s"], uc.N_ROWS)
        res = decompose(inp, y)
        assert sorted(res) == sorted(uc.fields_of(name))
        for f, v in res.items():
            assert np.all(np.isfinite(v)), (name, f)                  # the conditions on the fixture
            out[uc.key(name, f)] = np.asarray(v, dtype=np.float64)
        if inp["kind"] == "cat":
            if y.shape[0] > 1:
                assert res["mutual_information_i"].max() > 1e-2, (name, res["mutual_information_i"].max())
            print("%-22s S %2d  smallest probability %9.2e  predictive entropy in [%8.2e, %6.4f]  largest mutual information %6.4f"
                  % (name, y.shape[0], y.min(), res["predictive_entropy_i"].min(), res["predictive_entropy_i"].max(), res["mutual_information_i"].max()))
        else:
            print("%-22s S %2d  epistemic variance up to %9.3e  aleatoric variance in [%9.3e, %9.3e]"
                  % (name, y.shape[0], res["epistemic_var"].max(), res["aleatoric_var"].min(), res["aleatoric_var"].max()))
    path = os.path.join(HERE, "uncertainty.npz")
    np.savez_compressed(path, **out)
    print("wrote %d arrays to uncertainty.npz (%d bytes)" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
