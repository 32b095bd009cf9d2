#!/usr/bin/env python3
"""Generate tests/golden/pdp.npz from the REFERENCE's partial dependence (np_bnn 0.1.23: get_feature_summary, make_pdp_features,
get_pdp).  Runs only beside a checkout of the upstream repository (imported unmodified; only its numeric outputs on seeded
synthetic inputs are stored).  Usage:
    NPBNN_UPSTREAM_DIR=<np_bnn checkout> python tests/golden/make_pdp_golden.py

Every case stores its inputs (feature matrix, focal columns, per-sample weights, slopes, feature indicators and means) and the
reference's outputs under keys ``<case>/<name>``; tests/pdp_cases.py rebuilds the calls from them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
UPSTREAM = os.environ.get("NPBNN_UPSTREAM_DIR")
if not UPSTREAM:
    sys.exit("NPBNN_UPSTREAM_DIR: set it to a checkout of the upstream np_bnn repository (0.1.23)")
sys.path.insert(0, UPSTREAM)

import np_bnn as bn  # noqa: E402  (the reference)

N_ROWS = 83


def features(seed):
    """Columns: 0 continuous, 1 binary, 2 ordinal 1..4, 3 continuous, 4-6 one-hot block, 7 continuous."""
    rs = np.random.default_rng(seed)
    x = np.zeros((N_ROWS, 8))
    x[:, 0] = rs.normal(0.5, 1.3, N_ROWS)
    x[:, 1] = rs.integers(0, 2, N_ROWS)
    x[:, 2] = rs.integers(1, 5, N_ROWS)
    x[:, 3] = rs.uniform(-2, 3, N_ROWS)
    x[np.arange(N_ROWS), 4 + rs.integers(0, 3, N_ROWS)] = 1
    x[:, 7] = rs.standard_normal(N_ROWS)
    return x


def weight_sets(seed, n_features, n_nodes, n_out, n_samples):
    rs = np.random.default_rng(seed)
    dims = [n_features] + list(n_nodes) + [n_out]
    return [[rs.normal(0, 0.6, (dims[i + 1], dims[i] + 1)) for i in range(len(dims) - 1)] for _ in range(n_samples)]


# name: focal columns, activation, estimation mode, outputs, hidden layers, stored samples, indicators off (columns), seed
CASES = {
    "continuous": dict(focal=[0], fun="tanh", mode="classification", n_out=3, n_nodes=(6, 4), n_samples=5),
    "binary": dict(focal=[1], fun="tanh", mode="classification", n_out=3, n_nodes=(6, 4), n_samples=5),
    "ordinal_min1": dict(focal=[2], fun="swish", mode="classification", n_out=4, n_nodes=(5,), n_samples=4),
    "onehot": dict(focal=[4, 5, 6], fun="ReLU", mode="classification", n_out=3, n_nodes=(6, 4), n_samples=5),
    "two_continuous": dict(focal=[0, 3], fun="tanh", mode="classification", n_out=2, n_nodes=(5, 3), n_samples=3),
    "indicators": dict(focal=[0], fun="tanh", mode="classification", n_out=3, n_nodes=(6, 4), n_samples=4, off=[0, 7]),
    "indicators_ordinal": dict(focal=[2], fun="tanh", mode="regression", n_out=1, n_nodes=(6, 4), n_samples=4, off=[3]),
    "genrelu": dict(focal=[2], fun="genReLU", mode="classification", n_out=3, n_nodes=(6, 4), n_samples=6),
    "regression": dict(focal=[0], fun="tanh", mode="regression", n_out=1, n_nodes=(7, 3), n_samples=5),
    "regression_onehot": dict(focal=[4, 5, 6], fun="genReLU", mode="regression", n_out=2, n_nodes=(4, 4, 3), n_samples=3),
}


def main():
    out = {}
    for i, (name, c) in enumerate(CASES.items()):
        x = features(100 + i)
        weights = weight_sets(200 + i, x.shape[1], c["n_nodes"], c["n_out"], c["n_samples"])
        n_hidden = len(c["n_nodes"])
        rs = np.random.default_rng(300 + i)
        alphas = [rs.uniform(0.01, 0.4, n_hidden) if c["fun"] == "genReLU" else np.zeros(n_hidden) for _ in weights]
        act = bn.ActFun(fun=c["fun"])
        out_fn = bn.SoftMax if c["mode"] == "classification" else bn.RegressTransform
        indicators = np.ones(x.shape[1])
        for col in c.get("off", []):
            indicators[col] = 0
        means = np.mean(x, axis=0)
        transform = bn.BNN_env.data_transform_obj(indicators, means) if c.get("off") else None
        res = bn.get_pdp(x, c["focal"], c["mode"], c["n_out"], act, out_fn, weights, alphas, transform)
        key = name + "/"
        out[key + "x"] = x
        out[key + "focal"] = np.array(c["focal"])
        out[key + "fun"] = np.array(c["fun"])
        out[key + "mode"] = np.array(c["mode"])
        out[key + "n_out"] = np.array(c["n_out"])
        out[key + "n_layers"] = np.array(len(weights[0]))
        for s, w in enumerate(weights):
            for l, m in enumerate(w):
                out[key + "w_%d_%d" % (s, l)] = m
        out[key + "n_samples"] = np.array(len(weights))
        out[key + "alphas"] = np.array(alphas)
        out[key + "indicators"] = indicators
        out[key + "means"] = means
        out[key + "has_transform"] = np.array(transform is not None)
        out[key + "summary"] = bn.get_feature_summary(x, c["focal"])
        out[key + "grid"] = bn.make_pdp_features(x, c["focal"])
        out[key + "feature"] = res["feature"]
        out[key + "pdp"] = res["pdp"]
        out[key + "last_prm"] = np.asarray(act._prm, dtype=float)
    np.savez_compressed(os.path.join(HERE, "pdp.npz"), **out)
    print("wrote %d cases to %s" % (len(CASES), os.path.join(HERE, "pdp.npz")))


if __name__ == "__main__":
    main()
