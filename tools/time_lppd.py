#!/usr/bin/env python3
"""Wall time of the log pointwise predictive density of stored samples on its two routes, and what the device route's accumulation costs.

Both routes start from the feature matrix and the stored samples on the host and end with posterior_lppd's dictionary (totals, the
per-sample trace and the three pointwise arrays):
  device  one upload, one npbnn_predict_sets_lppd (what get_posterior_lppd does after it has read its checkpoint);
  host    one upload, npbnn_predict_sets (the [sample, row, output] stack comes back as float64), numpy's log of the label's
          probability (or the Gaussian log-density), then posterior_lppd - the only route there was before the entry.
Measured --repeats times each, interleaved pairs, in one process, after a discarded warm-up of each; then one device-route call and
one npbnn_predict_sets_summary (mode 1) with NPBNN_FI_TIMING=1 read the HIP-event times of the accumulation launches of the two.

    python tools/time_lppd.py [--rows 100000] [--features 256] [--classes 10] [--samples 100] [--repeats 5]
    python tools/time_lppd.py --regression --rows 1000000 --features 64 --targets 1 --samples 100

Prints one line per measurement and a JSON summary line last."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import npbnn_amd as bn  # noqa: E402
from npbnn_amd import _capi as capi, lppd, posterior  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--targets", type=int, default=1)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--regression", action="store_true")
    a = ap.parse_args()

    rs = np.random.default_rng(2)
    x = rs.standard_normal((a.rows, a.features))
    n_out = a.targets if a.regression else a.classes
    dims = [a.features, 32, 8, n_out]
    teacher = [rs.normal(0, 0.25, (dims[i + 1], dims[i] + 1)) for i in range(3)]
    samples = [dict(weights=[t + rs.normal(0, 0.08, t.shape) for t in teacher], alphas=np.zeros(1), mcmc_it=i,
                    error_prm=rs.uniform(0.8, 1.2, n_out)) for i in range(a.samples)]
    act = bn.ActFun(fun="tanh")
    out_fn = bn.RegressTransform if a.regression else bn.SoftMax
    base = posterior._predict_samples(x, [dict(weights=teacher, alphas=np.zeros(1))], act, out_fn)[0]
    if a.regression:
        kind, sigma = capi.LIK_GAUSS, np.array([s["error_prm"] for s in samples])
        labels = base + rs.standard_normal(base.shape)
    else:
        kind, sigma = capi.LIK_CATEGORICAL, None
        labels = np.argmax(base, axis=1)
        labels = np.where(rs.random(a.rows) < 0.05, (labels + rs.integers(1, a.classes, a.rows)) % a.classes, labels).astype(np.int64)
    del base

    def device(info=None):
        pred = posterior._SamplePredictor(a.features, samples, act, out_fn)
        try:
            t0 = time.perf_counter()
            res = pred.lppd(x, labels, kind, sigma_sets=sigma, pointwise=True)
            t = time.perf_counter() - t0
            if info is not None:
                ctx = pred._ctx
                info.update(lppd_pass_ns=ctx.info(capi.INFO_SUMMARY_PASS_NS), lppd_acc_ns=ctx.info(capi.INFO_SUMMARY_ACC_NS),
                            lppd_final_ns=ctx.info(capi.INFO_LPPD_FINAL_NS))
                pred.summary(1)
                info.update(summary_pass_ns=ctx.info(capi.INFO_SUMMARY_PASS_NS), summary_acc_ns=ctx.info(capi.INFO_SUMMARY_ACC_NS),
                            summary_final_ns=ctx.info(capi.INFO_SUMMARY_FINAL_NS))
            return t, res
        finally:
            pred.close()

    def host():
        pred = posterior._SamplePredictor(a.features, samples, act, out_fn)
        try:
            t0 = time.perf_counter()
            res = lppd.posterior_lppd(lppd.log_lik_of_stack(pred.predict(x), labels, kind, sigma))
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
    rel = {k: abs(res["device"][k] - res["host"][k]) / abs(res["host"][k]) for k in ("lppd", "mean_log_lik", "p_waic")}
    os.environ["NPBNN_FI_TIMING"] = "1"
    info = {}
    try:
        device(info)
    finally:
        os.environ.pop("NPBNN_FI_TIMING", None)
    med = {k: float(np.median(v)) for k, v in times.items()}
    lower = all(d < h for d, h in zip(times["device"], times["host"]))
    bound_ns = 1.5 * info["summary_acc_ns"]
    print("host %.1f ms, device %.1f ms (medians of %d); device lower in every pair: %s; relative difference of the totals %s"
          % (1e3 * med["host"], 1e3 * med["device"], a.repeats, lower, {k: "%.1e" % v for k, v in rel.items()}))
    print("accumulation launches: lppd %.1f us, summary mode 1 %.1f us (x 1.5 = %.1f us: %s); passes %.1f / %.1f us; final kernels %.1f / %.1f us"
          % (info["lppd_acc_ns"] / 1e3, info["summary_acc_ns"] / 1e3, bound_ns / 1e3, "held" if info["lppd_acc_ns"] <= bound_ns else "NOT held",
             info["lppd_pass_ns"] / 1e3, info["summary_pass_ns"] / 1e3, info["lppd_final_ns"] / 1e3, info["summary_final_ns"] / 1e3))
    print(json.dumps(dict(rows=a.rows, features=a.features, outputs=n_out, regression=a.regression, samples=a.samples, repeats=a.repeats,
                          host_ms=[round(1e3 * t, 2) for t in times["host"]], device_ms=[round(1e3 * t, 2) for t in times["device"]],
                          host_median_ms=round(1e3 * med["host"], 2), device_median_ms=round(1e3 * med["device"], 2),
                          device_lower_in_every_pair=lower, totals_relative_difference=rel,
                          **{k.replace("_ns", "_us"): round(v / 1e3, 1) for k, v in info.items()})))


if __name__ == "__main__":
    main()
