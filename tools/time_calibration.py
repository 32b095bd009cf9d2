#!/usr/bin/env python3
"""Wall time of the posterior calibration of stored samples on its two routes, and what the device route's kernels cost.

Both routes start from the feature matrix, its labels or targets and the stored samples on the host and end with
posterior_calibration's dictionary (the tables, the scores and the pointwise arrays):
  device  one upload, one npbnn_predict_sets_calibration (what get_posterior_calibration does after it has read its checkpoint);
  host    one upload, npbnn_predict_sets (the [sample, row, output] stack comes back as float64), then posterior_calibration in
          numpy - the only route there was before the entry.
Measured --repeats times each, interleaved pairs, in one process, after a discarded warm-up of each; then one device-route call with
NPBNN_FI_TIMING=1 reads the HIP-event times of its passes, accumulation launches and final kernel.  Run it under `timeout`.

    python tools/time_calibration.py [--rows 100000] [--features 256] [--classes 10] [--samples 100] [--repeats 5] [--bins 15]
    python tools/time_calibration.py --kind regression-error --targets 2

Prints one line per measurement and a JSON summary line last.  There is no pass or fail threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import npbnn_amd as bn  # noqa: E402
from npbnn_amd import _capi as capi, calibration, posterior  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--targets", type=int, default=1)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bins", type=int, default=15)
    ap.add_argument("--kind", choices=calibration.KINDS, default="classification")
    a = ap.parse_args()

    rs = np.random.default_rng(2)
    x = rs.standard_normal((a.rows, a.features))
    n_out = {"classification": a.classes, "regression": a.targets, "regression-error": 2 * a.targets}[a.kind]
    out_fn = {"classification": bn.SoftMax, "regression": bn.RegressTransform, "regression-error": bn.RegressTransformError}[a.kind]
    dims = [a.features, 32, 8, n_out]
    teacher = [rs.normal(0, 0.25, (dims[i + 1], dims[i] + 1)) for i in range(3)]
    samples = [dict(weights=[t + rs.normal(0, 0.08, t.shape) for t in teacher], alphas=np.zeros(1), mcmc_it=i,
                    error_prm=rs.uniform(0.8, 1.2, n_out)) for i in range(a.samples)]
    sigma = np.array([s["error_prm"] for s in samples]) if a.kind == "regression" else None
    labels = rs.integers(0, a.classes, a.rows) if a.kind == "classification" else rs.standard_normal((a.rows, a.targets))
    act = bn.ActFun(fun="tanh")

    def device(info=None):
        pred = posterior._SamplePredictor(a.features, samples, act, out_fn)
        try:
            t0 = time.perf_counter()
            res = pred.calibration(x, labels, a.kind, n_bins=a.bins, sigma_sets=sigma, pointwise=True)
            t = time.perf_counter() - t0
            if info is not None:
                ctx = pred._ctx
                info.update(pass_ns=ctx.info(capi.INFO_SUMMARY_PASS_NS), acc_ns=ctx.info(capi.INFO_SUMMARY_ACC_NS),
                            final_ns=ctx.info(capi.INFO_CALIBRATION_FINAL_NS))
            return t, res
        finally:
            pred.close()

    def host():
        pred = posterior._SamplePredictor(a.features, samples, act, out_fn)
        try:
            t0 = time.perf_counter()
            res = calibration.posterior_calibration(pred.predict(x), labels, a.kind, a.bins, sigma_sets=sigma)
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
    keys = ("accuracy", "brier", "nll", "ece") if a.kind == "classification" else ("rmse", "mean_pit", "coverage")
    rel = {k: float(np.max(np.abs(np.asarray(res["device"][k]) - res["host"][k]) / np.maximum(1e-300, np.abs(res["host"][k])))) for k in keys}
    os.environ["NPBNN_FI_TIMING"] = "1"
    info = {}
    try:
        device(info)
    finally:
        os.environ.pop("NPBNN_FI_TIMING", None)
    med = {k: float(np.median(v)) for k, v in times.items()}
    lower = all(d < h for d, h in zip(times["device"], times["host"]))
    print("host %.1f ms, device %.1f ms (medians of %d); device lower in every pair: %s; relative difference of the scores %s"
          % (1e3 * med["host"], 1e3 * med["device"], a.repeats, lower, {k: "%.1e" % v for k, v in rel.items()}))
    print("passes %.1f us, accumulation launches %.1f us, final kernel %.1f us" % (info["pass_ns"] / 1e3, info["acc_ns"] / 1e3, info["final_ns"] / 1e3))
    print(json.dumps(dict(rows=a.rows, features=a.features, outputs=n_out, kind=a.kind, samples=a.samples, bins=a.bins, repeats=a.repeats,
                          host_ms=[round(1e3 * t, 2) for t in times["host"]], device_ms=[round(1e3 * t, 2) for t in times["device"]],
                          host_median_ms=round(1e3 * med["host"], 2), device_median_ms=round(1e3 * med["device"], 2),
                          device_lower_in_every_pair=lower, scores_relative_difference=rel,
                          **{k.replace("_ns", "_us"): round(v / 1e3, 1) for k, v in info.items()})))


if __name__ == "__main__":
    main()
