#!/usr/bin/env python3
"""Wall time per permutation of feature_importance on its two routes, and where the device route's time goes.

Config 2's shapes (100k x 256, 10 classes), the network [32, 8], 100 synthetic stored samples, summary mode 1; 5 permutations on
each of 4 single-column blocks.  The host route (NPBNN_FI_HOST=1: one upload, one stack of predictions and one numpy summary per
permutation) and the device route (npbnn_permute_columns + npbnn_predict_sets_summary) are measured 5 times each, interleaved,
in one process, after a warm-up permutation of each; then one more device-route run with NPBNN_FI_TIMING=1 reads the HIP-event
times of the gather and patch of the split copies / the passes / the accumulation / the final kernel.

    python tools/time_feature_importance.py [--rows 100000] [--features 256] [--samples 100] [--repeats 5] [--mode 1]

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
from npbnn_amd import HipContext, _capi as capi  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--permutations", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mode", type=int, default=1, choices=(0, 1))
    a = ap.parse_args()

    rs = np.random.default_rng(2)
    x = rs.standard_normal((a.rows, a.features))
    labels = rs.integers(0, a.classes, a.rows)
    dims = [a.features, 32, 8, a.classes]
    samples = [dict(weights=[rs.normal(0, 0.3, (dims[i + 1], dims[i] + 1)) for i in range(3)], alphas=np.zeros(1), mcmc_it=i)
               for i in range(a.samples)]
    blocks = [[i] for i in range(a.blocks)]
    act = bn.ActFun(fun="tanh")

    def run(host, n_permutations, n_blocks):
        """(seconds per summary evaluated - the baseline and every permutation -, the data frame)"""
        if host:
            os.environ["NPBNN_FI_HOST"] = "1"
        else:
            os.environ.pop("NPBNN_FI_HOST", None)
        np.random.seed(7)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            df = bn.feature_importance(x, weights_posterior=samples, true_labels=labels, n_permutations=n_permutations,
                                       feature_blocks=blocks[:n_blocks], write_to_file=False, post_summary_mode=a.mode, actFun=act,
                                       output_act_fun=bn.SoftMax)
        return (time.perf_counter() - t0) / (1 + n_permutations * n_blocks), df

    for host in (True, False):               # warm-up: one permutation of each route
        run(host, 1, 1)
    times = {True: [], False: []}
    frames = {}
    for r in range(a.repeats):
        for host in (True, False):
            t, frames[host] = run(host, a.permutations, a.blocks)
            times[host].append(t)
            print("repeat %d %-6s route: %9.3f ms per permutation" % (r, "host" if host else "device", 1e3 * t), flush=True)
    same = bool(frames[True].equals(frames[False]))
    print("both routes give the same table: %s" % same)

    # the device route's split, from HIP events (a run of its own: the events add a wait per group of sets)
    split = {"permute": 0, "passes": 0, "accumulate": 0, "final": 0}
    counts = {"permute": 0, "summary": 0}
    real_permute, real_summary = HipContext.permute_columns, HipContext.predict_sets_summary

    def permute(self, *args, **kw):
        out = real_permute(self, *args, **kw)
        split["permute"] += self.info(capi.INFO_PERMUTE_NS)
        counts["permute"] += 1
        return out

    def summary(self, *args, **kw):
        out = real_summary(self, *args, **kw)
        split["passes"] += self.info(capi.INFO_SUMMARY_PASS_NS)
        split["accumulate"] += self.info(capi.INFO_SUMMARY_ACC_NS)
        split["final"] += self.info(capi.INFO_SUMMARY_FINAL_NS)
        counts["summary"] += 1
        return out

    os.environ["NPBNN_FI_TIMING"] = "1"
    HipContext.permute_columns, HipContext.predict_sets_summary = permute, summary
    try:
        t_timed, _ = run(False, a.permutations, a.blocks)
    finally:
        HipContext.permute_columns, HipContext.predict_sets_summary = real_permute, real_summary
        os.environ.pop("NPBNN_FI_TIMING", None)
    n = counts["summary"]
    per = {k: v / n / 1e3 for k, v in split.items()}            # microseconds per permutation
    # what the accumulation moves per permutation: every set's float32 predictions in, the accumulators in and out once per group
    per_set = a.rows * a.classes
    groups = -(-a.samples // 3)
    acc_bytes = a.samples * per_set * 4 + groups * 2 * per_set * (4 if a.mode == 0 else 8)
    acc_floor_us = acc_bytes / HBM_BYTES_PER_S * 1e6
    print("device route, HIP events, microseconds per permutation (%d summaries, %d permute calls):" % (n, counts["permute"]))
    print("  gather + patch of the split copies %10.1f" % per["permute"])
    print("  passes (weight upload and packing) %10.1f" % per["passes"])
    print("  accumulate                         %10.1f   (%.1f MB: %.1f us at 8 TB/s, %.0f %% of it)"
          % (per["accumulate"], acc_bytes / 1e6, acc_floor_us, 100 * acc_floor_us / per["accumulate"] if per["accumulate"] else 0))
    print("  final kernel                       %10.1f" % per["final"])
    print("  wall time per permutation of this run (events on) %8.3f ms" % (1e3 * t_timed))
    print(json.dumps(dict(rows=a.rows, features=a.features, classes=a.classes, samples=a.samples, mode=a.mode,
                          host_ms=[round(1e3 * t, 3) for t in times[True]], device_ms=[round(1e3 * t, 3) for t in times[False]],
                          device_faster_in_every_pair=bool(all(d < h for d, h in zip(times[False], times[True]))),
                          same_table=same, split_us={k: round(v, 1) for k, v in per.items()}, accumulate_bytes=acc_bytes,
                          accumulate_floor_us=round(acc_floor_us, 2))))


if __name__ == "__main__":
    main()
