#!/usr/bin/env python3
"""What input-gradient saliency costs.  Config 2's shapes - 100 k x 256, [32, 8], 10 classes - with 100 stored samples:

  get_saliency                    the whole call: context, upload of the table, npbnn_predict_saliency, the summary on the host
  npbnn_predict_saliency alone    on a context that holds the table (route 1, and route 2 forced with NPBNN_SALIENCY_PLAIN=1)
  phase 2 alone                   the fold and reduce kernels of every launch (HIP events, NPBNN_FI_TIMING=1: that run waits for
                                  every launch pair, so the entry's own time is taken from a run without it), and its rate:
                                  2 x rows x H0P x F x outputs x samples flops over that time, as a share of the 157.3 TFLOP/s
                                  float32 matrix peak

Wall time of each, the best of two after a warm-up call.  For context only - it is another quantity, no bar to compare with -
feature_importance on the same table with one feature and two permutations: three replays of the stored samples, where a table
of all 256 features at its default 100 permutations takes 25 601.  Boxes differ in shader clock (tools/box_speed.py): compare
within one run.
    python tools/time_saliency.py [n_rows]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npbnn_amd as bn  # noqa: E402
from npbnn_amd import _capi as capi  # noqa: E402

N_ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
N_FEATURES, NODES, N_OUT, N_SETS = 256, (32, 8), 10, 100
PEAK_TF = 157.3


def best(f, runs=2, warm=True):
    if warm:
        f()
    t = float("inf")
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        t = min(t, time.perf_counter() - t0)
    return 1e3 * t


def main():
    rs = np.random.default_rng(3)
    x = rs.standard_normal((N_ROWS, N_FEATURES))
    dims = [N_FEATURES] + list(NODES) + [N_OUT]
    weights = [[rs.normal(0, 1.0 / np.sqrt(dims[i] + 1), (dims[i + 1], dims[i] + 1)) for i in range(len(dims) - 1)] for _ in range(N_SETS)]
    alphas = [np.zeros(len(NODES))] * N_SETS
    print("%d x %d, %s, %d classes, %d stored samples" % (N_ROWS, N_FEATURES, list(NODES), N_OUT, N_SETS), flush=True)

    def get_saliency():
        return bn.get_saliency(x, N_OUT, bn.ActFun(fun="tanh"), bn.SoftMax, weights, alphas, None)

    whole = best(get_saliency)
    print("get_saliency: %.1f ms" % whole, flush=True)

    flops = 2.0 * N_ROWS * 32 * N_FEATURES * N_OUT * N_SETS
    results = {}
    for label, force in (("route 1", None), ("route 2", "1")):
        if force:
            os.environ["NPBNN_SALIENCY_PLAIN"] = force
        ctx = bn.HipContext()
        ctx.set_data(x)
        ctx.set_arch_from_weights(weights[0], N_FEATURES, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
        entry = best(lambda: results.__setitem__(label, ctx.predict_saliency(weights)))
        route = ctx.info(capi.INFO_SALIENCY_ROUTE)
        os.environ["NPBNN_FI_TIMING"] = "1"
        ctx.predict_saliency(weights)
        fold_ms = 1e-6 * ctx.info(capi.INFO_SALIENCY_FOLD_NS)
        os.environ.pop("NPBNN_FI_TIMING", None)
        os.environ.pop("NPBNN_SALIENCY_PLAIN", None)
        ctx.close()
        print("npbnn_predict_saliency alone, route %d: %.1f ms   (phase 2 alone: %.1f ms, %.2f TFLOP, %.1f TFLOP/s = %.1f %% of %.1f)"
              % (route, entry, fold_ms, 1e-12 * flops, 1e-9 * flops / fold_ms, 100 * 1e-9 * flops / fold_ms / PEAK_TF, PEAK_TF), flush=True)
    print("routes differ by at most %.2e" % max(np.abs(a - b).max() for a, b in zip(results["route 1"], results["route 2"])), flush=True)

    labels = rs.integers(0, N_OUT, N_ROWS)
    samples = [{"weights": w, "alphas": a} for w, a in zip(weights, alphas)]
    fi_ms = best(lambda: bn.feature_importance(x, weights_posterior=samples, true_labels=labels, feature_blocks={"first": [0]}, n_permutations=2,
                                               write_to_file=False, actFun=bn.ActFun(fun="tanh"), output_act_fun=bn.SoftMax), runs=1)
    print("feature_importance, one feature x 2 permutations (3 replays of the samples): %.1f ms" % fi_ms, flush=True)


main()
