#!/usr/bin/env python3
"""Wall time of the posterior predictive distribution (quantiles, mean and CRPS per row and target) of stored samples on its two
routes.

Both routes start from the feature matrix, the targets and the stored samples on the host and end with posterior_predictive's
arrays:
  device  one upload, one npbnn_predict_sets_predictive (what get_posterior_predictive does after it has read its checkpoint);
  host    one upload, npbnn_predict_sets (the [sample, row, output] stack comes back as float64), then posterior_predictive in
          numpy: vectorised bisection and the O(S^2) pair term, sample row by sample row.
Measured --repeats times each, interleaved pairs, in one process, after a discarded warm-up of each.  The times are measurements,
not acceptance criteria: neither the reference nor an earlier version has anything to compare against.  Run it under `timeout`.

    python tools/time_predictive.py [--rows 20000] [--features 64] [--targets 2] [--samples 100] [--repeats 3] [--no-crps]

Prints one line per measurement and a JSON summary line last."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import npbnn_amd as bn  # noqa: E402
from npbnn_amd import posterior, predictive  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--targets", type=int, default=2)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-crps", action="store_true")
    a = ap.parse_args()

    rs = np.random.default_rng(2)
    x = rs.standard_normal((a.rows, a.features))
    dims = [a.features, 16, 4, a.targets]
    teacher = [rs.normal(0, 0.25, (dims[i + 1], dims[i] + 1)) for i in range(3)]
    samples = [dict(weights=[t + rs.normal(0, 0.05, t.shape) for t in teacher], alphas=np.zeros(1), mcmc_it=i) for i in range(a.samples)]
    sigma = np.exp(rs.normal(-0.5, 0.2, (a.samples, a.targets)))
    y = None if a.no_crps else rs.standard_normal((a.rows, a.targets))
    act = bn.ActFun(fun="tanh")
    probs = predictive.DEFAULT_PROBS

    def device():
        pred = posterior._SamplePredictor(a.features, samples, act, bn.RegressTransform)
        try:
            t0 = time.perf_counter()
            res = pred.predictive(x, "regression", probs=probs, sigma_sets=sigma, targets=y)
            return time.perf_counter() - t0, res
        finally:
            pred.close()

    def host():
        pred = posterior._SamplePredictor(a.features, samples, act, bn.RegressTransform)
        try:
            t0 = time.perf_counter()
            res = predictive.posterior_predictive(pred.predict(x), "regression", sigma_sets=sigma, probs=probs, targets=y)
            return time.perf_counter() - t0, res
        finally:
            pred.close()

    device(), host()                                              # warm-up, discarded
    times = {"device": [], "host": []}
    res = {}
    for r in range(a.repeats):
        for name, f in (("host", host), ("device", device)):
            t, res[name] = f()
            times[name].append(t)
            print("repeat %d %-6s route: %9.1f ms" % (r, name, 1e3 * t), flush=True)
    diff = {"quantiles": float(np.max(np.abs(res["device"]["quantiles"] - res["host"]["quantiles"])))}
    if y is not None:
        diff["crps_i"] = float(np.max(np.abs(res["device"]["crps_i"] - res["host"]["crps_i"])))
    med = {k: float(np.median(v)) for k, v in times.items()}
    print("host %.1f ms, device %.1f ms (medians of %d); largest absolute difference %s"
          % (1e3 * med["host"], 1e3 * med["device"], a.repeats, {k: "%.1e" % v for k, v in diff.items()}))
    print(json.dumps(dict(rows=a.rows, features=a.features, targets=a.targets, samples=a.samples, crps=y is not None, repeats=a.repeats,
                          host_ms=[round(1e3 * t, 2) for t in times["host"]], device_ms=[round(1e3 * t, 2) for t in times["device"]],
                          host_median_ms=round(1e3 * med["host"], 2), device_median_ms=round(1e3 * med["device"], 2), absolute_difference=diff)))


if __name__ == "__main__":
    main()
