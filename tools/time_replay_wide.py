#!/usr/bin/env python3
"""The replay of stored weight sets on the weight-streamed path: device time of the passes of one npbnn_predict_sets_summary (weight
packing included, HIP events: NPBNN_FI_TIMING) and what the replay launched (NPBNN_INFO_REPLAY_PASSES / _MAX_GROUP), on the shape the
path exists for - the default [50, 5] network on 100k x 1024, a posterior of 99 sets.  --alone gives every set a slope vector of its
own (tanh ignores them): groups of one, the replay as it was before its passes carried several sets.

    python tools/time_replay_wide.py [--rows 100000] [--features 1024] [--nodes 50-5] [--classes 10] [--sets 99] [--repeats 5] [--alone]

A library without the two info values (NPBNN_HIP_LIB pointing at an older build) reports them as null.  Prints one line per repeat
and a JSON summary line last.  Run it under `timeout`."""
import argparse
import json
import os
import sys

import numpy as np

os.environ["NPBNN_FI_TIMING"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from npbnn_amd import HipContext, _capi as capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--nodes", default="50-5")
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--sets", type=int, default=99)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--alone", action="store_true")
    a = ap.parse_args()

    rs = np.random.default_rng(3)
    x = rs.standard_normal((a.rows, a.features), dtype=np.float32)
    dims = [a.features] + [int(v) for v in a.nodes.split("-")] + [a.classes]
    sets = [[rs.normal(0, 1.0 / np.sqrt(dims[i] + 1), (dims[i + 1], dims[i] + 1)) for i in range(len(dims) - 1)] for _ in range(a.sets)]
    slopes = [np.full(len(dims) - 2, 0.001 * (i + 1)) for i in range(a.sets)] if a.alone else None
    ctx = HipContext(0)
    try:
        ctx.set_data(x)
        ctx.set_arch_from_weights(sets[0], a.features, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
        pass_us, info = [], None
        for r in range(a.repeats + 1):               # (the first call builds the fp16-split copy of X: discarded)
            ctx.predict_sets_summary(sets, 1, act_prm_sets=slopes)
            us = ctx.info(capi.INFO_SUMMARY_PASS_NS) / 1e3
            try:
                info = ctx.replay_info()
            except capi.NpbnnError:
                info = None
            if r:
                pass_us.append(us)
                print("repeat %d: passes %.1f us, accumulation %.1f us, replay_info %s" % (r, us, ctx.info(capi.INFO_SUMMARY_ACC_NS) / 1e3, info), flush=True)
        wide, mode = ctx.is_wide(), ctx.l0_mode()
    finally:
        ctx.close()
    print(json.dumps(dict(rows=a.rows, features=a.features, nodes=a.nodes, classes=a.classes, sets=a.sets, alone=a.alone, wide=wide, l0=mode,
                          replay_passes=None if info is None else info[0], replay_max_group=None if info is None else info[1],
                          pass_us=[round(v, 1) for v in pass_us], pass_us_median=round(float(np.median(pass_us)), 1),
                          pass_us_min=round(min(pass_us), 1), pass_us_max=round(max(pass_us), 1))))


if __name__ == "__main__":
    main()
