#!/usr/bin/env python3
"""Wall time of the convergence diagnostics (split R-hat and effective sample size per row and output) of stored samples on their
two routes, and what the device route's kernels cost.

Both routes start from the feature matrix and the stored samples on the host and end with posterior_convergence's dictionary (the
pointwise arrays and the summary):
  device  one upload, one npbnn_predict_sets_convergence (what get_posterior_convergence does after it has read its checkpoints);
  host    one upload, npbnn_predict_sets (the [sample, row, output] stack comes back as float64), then posterior_convergence in
          numpy - the route a custom output callable takes.
Measured --repeats times each, interleaved pairs, in one process, after a discarded warm-up of each; then one device-route call with
NPBNN_FI_TIMING=1 reads the HIP-event times of its passes and of its diagnostic and summary kernels.  Run it under `timeout`.

    python tools/time_convergence.py [--rows 100000] [--features 256] [--classes 10] [--samples 100] [--chains 2] [--repeats 5]

Prints one line per measurement and a JSON summary line last."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import npbnn_amd as bn  # noqa: E402
from npbnn_amd import _capi as capi, convergence, posterior  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--chains", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()

    rs = np.random.default_rng(2)
    x = rs.standard_normal((a.rows, a.features))
    dims = [a.features, 32, 8, a.classes]
    teacher = [rs.normal(0, 0.25, (dims[i + 1], dims[i] + 1)) for i in range(3)]
    # every chain an AR(1) walk around the teacher: a row's predictions are a correlated series
    samples, state = [], None
    for i in range(a.samples):
        if i % (a.samples // a.chains) == 0:
            state = [rs.normal(0, 0.08, t.shape) for t in teacher]
        state = [0.8 * w + rs.normal(0, 0.048, w.shape) for w in state]
        samples.append(dict(weights=[t + w for t, w in zip(teacher, state)], alphas=np.zeros(1), mcmc_it=i))
    act = bn.ActFun(fun="tanh")

    def device(info=None):
        pred = posterior._SamplePredictor(a.features, samples, act, bn.SoftMax)
        try:
            t0 = time.perf_counter()
            res = pred.convergence(x, a.chains, pointwise=True)
            t = time.perf_counter() - t0
            if info is not None:
                ctx = pred._ctx
                info.update(pass_ns=ctx.info(capi.INFO_SUMMARY_PASS_NS), final_ns=ctx.info(capi.INFO_CONVERGENCE_FINAL_NS))
            return t, res
        finally:
            pred.close()

    def host():
        pred = posterior._SamplePredictor(a.features, samples, act, bn.SoftMax)
        try:
            t0 = time.perf_counter()
            res = convergence.posterior_convergence(pred.predict(x), a.chains)
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
    rel = {k: float(np.nanmax(np.abs(res["device"][k] - res["host"][k]) / np.abs(res["host"][k]))) for k in ("rhat", "ess")}
    os.environ["NPBNN_FI_TIMING"] = "1"
    info = {}
    try:
        device(info)
    finally:
        os.environ.pop("NPBNN_FI_TIMING", None)
    med = {k: float(np.median(v)) for k, v in times.items()}
    lower = all(d < h for d, h in zip(times["device"], times["host"]))
    d = res["device"]
    print("host %.1f ms, device %.1f ms (medians of %d); device lower in every pair: %s; largest relative difference %s"
          % (1e3 * med["host"], 1e3 * med["device"], a.repeats, lower, {k: "%.1e" % v for k, v in rel.items()}))
    print("max rhat %.3f, min ess %.1f, share of columns above 1.01 %.3f, constant columns %d" % (d["max_rhat"], d["min_ess"], d["frac_rhat_above"], d["n_constant"]))
    print("passes %.1f us, diagnostic and summary kernels %.1f us" % (info["pass_ns"] / 1e3, info["final_ns"] / 1e3))
    print(json.dumps(dict(rows=a.rows, features=a.features, outputs=a.classes, samples=a.samples, chains=a.chains, repeats=a.repeats,
                          host_ms=[round(1e3 * t, 2) for t in times["host"]], device_ms=[round(1e3 * t, 2) for t in times["device"]],
                          host_median_ms=round(1e3 * med["host"], 2), device_median_ms=round(1e3 * med["device"], 2),
                          device_lower_in_every_pair=lower, relative_difference=rel, max_rhat=d["max_rhat"], min_ess=d["min_ess"],
                          **{k.replace("_ns", "_us"): round(v / 1e3, 1) for k, v in info.items()})))


if __name__ == "__main__":
    main()
