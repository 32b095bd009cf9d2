#!/usr/bin/env python3
"""Generate tests/golden/importance.npz from the REFERENCE's permutation importance (np_bnn 0.1.23: feature_importance,
np_bnn/BNN_lib.py:504-597).  Runs only beside a checkout of the upstream repository (imported unmodified; only its numeric
outputs on seeded synthetic inputs are stored).  Usage:
    NPBNN_UPSTREAM_DIR=<np_bnn checkout> python tests/golden/make_importance_golden.py

Inputs: ``cases.importance_inputs`` of tests/importance_cases.py (``cases.posterior_inputs`` with 400 rows and 9 stored samples,
the three activations of ``cases.POSTERIOR_CASES``).  Per activation, summary mode (0 votes, 1 mean), linked / unlinked blocks and
block layout (one block per column, a dict of three blocks, a list of lists) the file keeps the ranking
(``feature_block_index``) and the four numeric columns of the data frame, seed 7, three permutations per block."""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
UPSTREAM = os.environ.get("NPBNN_UPSTREAM_DIR")
if not UPSTREAM:
    sys.exit("NPBNN_UPSTREAM_DIR: set it to a checkout of the upstream np_bnn repository (0.1.23)")
sys.path.insert(0, UPSTREAM)

import np_bnn as bn  # noqa: E402  (the reference)

import importance_cases as ic  # noqa: E402


def main():
    out = {}
    for case in ic.CASES:
        inp = ic.inputs(case)
        for mode, unlink, tag in ic.combinations():
            act = bn.ActFun(fun=inp["fun"], prm=np.zeros(2)) if inp["fun"] == "genReLU" else bn.ActFun(fun=inp["fun"])
            np.random.seed(ic.SEED)
            with contextlib.redirect_stdout(io.StringIO()):
                df = bn.feature_importance(inp["x"], weights_posterior=inp["samples"], true_labels=inp["labels"],
                                           n_permutations=ic.N_PERMUTATIONS, feature_blocks=ic.BLOCKS[tag], write_to_file=False,
                                           post_summary_mode=mode, unlink_features_within_block=unlink, actFun=act,
                                           output_act_fun=bn.SoftMax)
            key = ic.key(case, mode, unlink, tag)
            out[key + "/index"] = df["feature_block_index"].to_numpy().astype(np.int64)
            out[key + "/values"] = df.iloc[:, 2:].to_numpy().astype(np.float64)
    np.savez_compressed(os.path.join(HERE, "importance.npz"), **out)
    top = [v[0, 0] for k, v in out.items() if k.endswith("/values")]
    print("wrote %d tables to importance.npz; top-ranked losses between %.4f and %.4f" % (len(top), min(top), max(top)))


if __name__ == "__main__":
    main()
