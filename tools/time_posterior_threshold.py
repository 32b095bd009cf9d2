#!/usr/bin/env python3
"""Wall time of get_posterior_threshold's sweep on its two routes, and what the device route's final kernel costs.

Config 2's shapes (a 100k x 256 test matrix, 10 classes), the network [32, 8], 100 synthetic stored samples around a teacher network.
Both routes start from the matrix on the host and end with the selected row of the sweep of 99 thresholds:
  device  one upload, one npbnn_predict_sets_support, the table from the cube's suffix sums;
  host    one upload, npbnn_predict_sets (the [sample, row, class] stack comes back), the numpy summary and
          get_accuracy_threshold per threshold - the building blocks this package had before the support entry.
Measured --repeats times each, interleaved, in one process, after a discarded warm-up of each; then one device-route run and one
npbnn_predict_sets_summary with NPBNN_FI_TIMING=1 read the HIP-event times of the two final kernels.

    python tools/time_posterior_threshold.py [--rows 100000] [--features 256] [--samples 100] [--repeats 5] [--modes 0 1]

Prints one line per measurement and a JSON summary line last."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import npbnn_amd as bn  # noqa: E402
from npbnn_amd import _capi as capi, posterior, support  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--modes", type=int, nargs="+", default=[0, 1], choices=(0, 1))
    ap.add_argument("--target", type=float, default=0.9)
    a = ap.parse_args()

    rs = np.random.default_rng(2)
    x = rs.standard_normal((a.rows, a.features))
    dims = [a.features, 32, 8, a.classes]
    teacher = [rs.normal(0, 0.25, (dims[i + 1], dims[i] + 1)) for i in range(3)]
    samples = [dict(weights=[t + rs.normal(0, 0.08, t.shape) for t in teacher], alphas=np.zeros(1), mcmc_it=i) for i in range(a.samples)]
    act = bn.ActFun(fun="tanh")
    labels = np.argmax(posterior._predict_samples(x, [dict(weights=teacher, alphas=np.zeros(1))], act, bn.SoftMax)[0], axis=1)
    labels = np.where(rs.random(a.rows) < 0.05, (labels + rs.integers(1, a.classes, a.rows)) % a.classes, labels).astype(np.int64)
    grid = np.linspace(*support.THRESHOLD_GRID)

    def select(table):
        with contextlib.redirect_stdout(io.StringIO()):
            return support._select(table, a.target, None)

    def device(mode, info=None):
        pred = posterior._SamplePredictor(a.features, samples, act, bn.SoftMax)
        try:
            t0 = time.perf_counter()
            pred.load(x)
            cube = pred.support(mode, labels, grid)["cube"]
            row = select(support.table_from_cube(cube, grid))
            t = time.perf_counter() - t0
            if info is not None:
                info["support_final_ns"] = pred._ctx.info(capi.INFO_SUPPORT_FINAL_NS)
                pred.summary(mode, labels, want_summary=False)
                info["summary_final_ns"] = pred._ctx.info(capi.INFO_SUMMARY_FINAL_NS)
            return t, row
        finally:
            pred.close()

    def host(mode):
        pred = posterior._SamplePredictor(a.features, samples, act, bn.SoftMax)
        try:
            t0 = time.perf_counter()
            summary = posterior._summarise(pred.predict(x), mode)
            rows = []
            for t in grid:
                try:
                    s = support.get_accuracy_threshold(summary, labels, threshold=t)
                    rows.append([t, s['accuracy'], s['retained_samples']])
                except ZeroDivisionError:
                    pass
            row = select(np.array(rows).reshape(-1, 3))
            return time.perf_counter() - t0, row
        finally:
            pred.close()

    out = dict(rows=a.rows, features=a.features, classes=a.classes, samples=a.samples, repeats=a.repeats, modes={})
    for mode in a.modes:
        device(mode), host(mode)                                  # warm-up, discarded
        times = {"device": [], "host": []}
        rows = {}
        for r in range(a.repeats):
            for name, f in (("host", host), ("device", device)):
                t, rows[name] = f(mode)
                times[name].append(t)
                print("mode %d repeat %d %-6s route: %9.1f ms" % (mode, r, name, 1e3 * t), flush=True)
        same = bool(np.array_equal(rows["host"], rows["device"]))
        os.environ["NPBNN_FI_TIMING"] = "1"
        info = {}
        try:
            device(mode, info)
        finally:
            os.environ.pop("NPBNN_FI_TIMING", None)
        # what the final kernel moves: the accumulators and the labels in; the cube is a few KB
        final_bytes = a.rows * a.classes * (4 if mode == 0 else 8) + a.rows * 8
        final_us = info["support_final_ns"] / 1e3
        med = {k: float(np.median(v)) for k, v in times.items()}
        print("mode %d: host %.1f ms, device %.1f ms (medians of %d), same selected row: %s" % (mode, 1e3 * med["host"], 1e3 * med["device"], a.repeats, same))
        print("mode %d: support_final_kernel %.1f us (%.2f MB: %.2f TB/s, %.0f %% of 8 TB/s); summary_final_kernel on the same accumulators %.1f us"
              % (mode, final_us, final_bytes / 1e6, final_bytes / (final_us * 1e-6) / 1e12 if final_us else 0,
                 100 * final_bytes / (final_us * 1e-6) / HBM_BYTES_PER_S if final_us else 0, info["summary_final_ns"] / 1e3))
        out["modes"][str(mode)] = dict(host_ms=[round(1e3 * t, 2) for t in times["host"]], device_ms=[round(1e3 * t, 2) for t in times["device"]],
                                       host_median_ms=round(1e3 * med["host"], 2), device_median_ms=round(1e3 * med["device"], 2),
                                       same_selected_row=same, selected_row=[float(v) for v in rows["device"]],
                                       support_final_us=round(final_us, 1), summary_final_us=round(info["summary_final_ns"] / 1e3, 1),
                                       final_bytes=final_bytes)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
