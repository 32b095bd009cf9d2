#!/usr/bin/env python3
"""Wall time of PSIS leave-one-out cross-validation of stored samples: the device entry against the definition on the host.

Both start from the feature matrix and the stored samples on the host, in a fresh process each time (--processes of them, one after
the other), with one discarded warm-up and --repeats calls:
  device  one upload and one npbnn_predict_sets_loo: the pointwise arrays come back (what get_posterior_loo does after it has read
          its checkpoint);
  host    one upload, one npbnn_predict_sets_loo that also returns the float64 matrix ll [samples, rows], then posterior_loo on that
          matrix in numpy: the upload, the download and the host arithmetic, which is printed on its own as well.
One more device call per process runs with NPBNN_FI_TIMING=1 and reads the HIP-event times of the evaluation passes, of the launches
that write ll, and of the final kernel.

    python tools/time_loo.py [--rows 100000] [--features 256] [--classes 10] [--samples 100] [--repeats 5] [--processes 2]

Prints one line per measurement and a JSON summary line last."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def child(a):
    import npbnn_amd as bn
    from npbnn_amd import _capi as capi, loo, posterior

    rs = np.random.default_rng(2)
    x = rs.standard_normal((a.rows, a.features))
    dims = [a.features, 32, 8, a.classes]
    teacher = [rs.normal(0, 0.25, (dims[i + 1], dims[i] + 1)) for i in range(3)]
    samples = [dict(weights=[t + rs.normal(0, 0.08, t.shape) for t in teacher], alphas=np.zeros(1), mcmc_it=i) for i in range(a.samples)]
    act = bn.ActFun(fun="tanh")
    base = posterior._predict_samples(x, [dict(weights=teacher, alphas=np.zeros(1))], act, bn.SoftMax)[0]
    labels = np.argmax(base, axis=1)
    labels = np.where(rs.random(a.rows) < 0.05, (labels + rs.integers(1, a.classes, a.rows)) % a.classes, labels).astype(np.int64)
    del base

    def device(info=None):
        pred = posterior._SamplePredictor(a.features, samples, act, bn.SoftMax)
        try:
            t0 = time.perf_counter()
            res = pred.loo(x, labels, capi.LIK_CATEGORICAL)
            t = time.perf_counter() - t0
            if info is not None:
                ctx = pred._ctx
                info.update(pass_ns=ctx.info(capi.INFO_SUMMARY_PASS_NS), log_lik_ns=ctx.info(capi.INFO_SUMMARY_ACC_NS), final_ns=ctx.info(capi.INFO_LOO_FINAL_NS))
            return t, 0.0, res
        finally:
            pred.close()

    def host():
        pred = posterior._SamplePredictor(a.features, samples, act, bn.SoftMax)
        try:
            t0 = time.perf_counter()
            matrix = pred.loo(x, labels, capi.LIK_CATEGORICAL, log_lik=True)["log_lik"]
            t1 = time.perf_counter()
            res = loo.posterior_loo(matrix)
            t2 = time.perf_counter()
            return t2 - t0, t2 - t1, res
        finally:
            pred.close()

    device(), host()                                              # warm-up, discarded
    out = {"device_ms": [], "host_ms": [], "host_numpy_ms": []}
    res = {}
    for _ in range(a.repeats):
        for name, f in (("host", host), ("device", device)):
            t, t_np, res[name] = f()
            out[name + "_ms"].append(round(1e3 * t, 2))
            if name == "host":
                out["host_numpy_ms"].append(round(1e3 * t_np, 2))
    os.environ["NPBNN_FI_TIMING"] = "1"
    info = {}
    device(info)
    out.update({k.replace("_ns", "_us"): round(v / 1e3, 1) for k, v in info.items()})
    out["elpd_loo"] = res["device"]["elpd_loo"]
    out["elpd_loo_relative_difference"] = abs(res["device"]["elpd_loo"] - res["host"]["elpd_loo"]) / abs(res["host"]["elpd_loo"])
    kd, kh = res["device"]["pareto_k"], res["host"]["pareto_k"]
    fitted = np.isfinite(kh)
    assert np.array_equal(kd[~fitted], kh[~fitted])
    out["pareto_k_largest_difference"] = float(np.max(np.abs(kd[fitted] - kh[fitted]))) if fitted.any() else 0.0
    out["n_bad_k"] = res["device"]["n_bad_k"]
    print("CHILD " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for p in range(a.processes):
        cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [w for k in ("rows", "features", "classes", "samples", "repeats")
                                                                         for w in ("--" + k, str(getattr(a, k)))]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
        run = json.loads([line for line in text.splitlines() if line.startswith("CHILD ")][-1][6:])
        runs.append(run)
        print("process %d: device %s ms, host %s ms (numpy %s ms); passes %.1f us, log-likelihood launches %.1f us, final kernel %.1f us"
              % (p, run["device_ms"], run["host_ms"], run["host_numpy_ms"], run["pass_us"], run["log_lik_us"], run["final_us"]), flush=True)
    every = {k: [t for r in runs for t in r[k]] for k in ("device_ms", "host_ms", "host_numpy_ms")}
    summary = dict(rows=a.rows, features=a.features, classes=a.classes, samples=a.samples, repeats=a.repeats, processes=a.processes)
    for k, v in every.items():
        summary[k.replace("_ms", "_median_ms")] = round(float(np.median(v)), 2)
        summary[k.replace("_ms", "_range_ms")] = [min(v), max(v)]
    for k in ("pass_us", "log_lik_us", "final_us"):
        summary[k] = [r[k] for r in runs]
    summary.update(elpd_loo=runs[0]["elpd_loo"], n_bad_k=runs[0]["n_bad_k"],
                   elpd_loo_relative_difference=max(r["elpd_loo_relative_difference"] for r in runs),
                   pareto_k_largest_difference=max(r["pareto_k_largest_difference"] for r in runs))
    print("device %.1f ms [%.1f, %.1f], host %.1f ms [%.1f, %.1f] of which numpy %.1f ms (medians and ranges of %d calls in %d processes)"
          % (summary["device_median_ms"], *summary["device_range_ms"], summary["host_median_ms"], *summary["host_range_ms"],
             summary["host_numpy_median_ms"], len(every["device_ms"]), a.processes))
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
