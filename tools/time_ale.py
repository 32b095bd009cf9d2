#!/usr/bin/env python3
"""What accumulated local effects cost next to the ways around them.  Config 2's shapes - 100 k x 256, [32, 8], 10 classes - with
100 stored samples and one continuous focal feature in K = 40 quantile bins:

  get_ale, route 1          both edges of a row's bin from one read of X per group of sets (NPBNN_INFO_ALE_ROUTE 1)
  get_ale, route 2          one pass per (edge, set group), forced with NPBNN_ALE_PER_EDGE=1
  get_pdp                   partial dependence on its 100 grid points
  host loop                 K + 1 times: the column set to an edge on the host, set_data, predict_sets, the rows of two bins picked

Wall time of the whole call each - context, upload of the table, result and host arithmetic included; the best of two after a
warm-up call (the host loop runs once) - and, for the two ALE routes, of npbnn_predict_ale alone on a context that holds the table,
next to npbnn_predict_pdp with two grid points there: the same layer-0 work and the same two later-layer evaluations per row and set.
Boxes differ in shader clock (tools/box_speed.py): compare within one run.
    python tools/time_ale.py [n_rows]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npbnn_amd as bn  # noqa: E402
from npbnn_amd import _capi as capi  # noqa: E402

N_ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
N_FEATURES, NODES, N_OUT, N_SETS, K, FOCAL = 256, (32, 8), 10, 100, 40, 0


def best(f, runs=2, warm=True):
    if warm:
        f()
    t = float("inf")
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        t = min(t, time.perf_counter() - t0)
    return 1e3 * t


def host_loop(x, weights, edges):
    """local effects from K + 1 predict_sets calls, the column moved on the host"""
    col = x[:, FOCAL].astype(np.float32)
    k_of_row = np.minimum(np.searchsorted(edges.astype(np.float32)[1:], col, side="left"), len(edges) - 2)
    effects = np.zeros((len(weights), len(edges) - 1, N_OUT))
    ctx = bn.HipContext()
    moved = x.copy()
    lower = None
    for k, z in enumerate(edges):
        moved[:, FOCAL] = z
        ctx.set_data(moved)
        ctx.set_arch_from_weights(weights[0], N_FEATURES, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
        upper = ctx.predict_sets(weights)
        if k > 0:
            rows = k_of_row == k - 1
            if rows.any():
                effects[:, k - 1] = (upper[:, rows] - lower[:, rows]).mean(axis=1)
        lower = upper
    ctx.close()
    return effects


def main():
    rs = np.random.default_rng(3)
    x = rs.standard_normal((N_ROWS, N_FEATURES))
    dims = [N_FEATURES] + list(NODES) + [N_OUT]
    weights = [[rs.normal(0, 1.0 / np.sqrt(dims[i] + 1), (dims[i + 1], dims[i] + 1)) for i in range(len(dims) - 1)] for _ in range(N_SETS)]
    alphas = [np.zeros(len(NODES))] * N_SETS
    edges = bn.make_ale_edges(x, FOCAL, n_bins=K)
    print("%d x %d, %s, %d classes, %d stored samples, K = %d" % (N_ROWS, N_FEATURES, list(NODES), N_OUT, N_SETS, len(edges) - 1), flush=True)

    def get_ale():
        return bn.get_ale(x, FOCAL, "classification", N_OUT, bn.ActFun(fun="tanh"), bn.SoftMax, weights, alphas, None, n_bins=K)

    ctx = bn.HipContext()
    ctx.set_data(x)
    ctx.set_arch_from_weights(weights[0], N_FEATURES, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
    results = {}
    for label, force in (("route 1", None), ("route 2", "1")):
        if force:
            os.environ["NPBNN_ALE_PER_EDGE"] = force
        results[label] = get_ale()
        whole = best(get_ale, warm=False)
        entry = best(lambda: ctx.predict_ale(weights, FOCAL, edges))
        print("get_ale, %s: %.1f ms   (npbnn_predict_ale alone, route %d: %.1f ms)" % (label, whole, ctx.info(capi.INFO_ALE_ROUTE), entry),
              flush=True)
        os.environ.pop("NPBNN_ALE_PER_EDGE", None)
    two = best(lambda: ctx.predict_pdp(weights, [FOCAL], edges[[0, -1]].reshape(2, 1)))
    print("npbnn_predict_pdp alone, 2 grid points (route %d; its [2, rows, classes] result copied back): %.1f ms" % (ctx.info(capi.INFO_PDP_ROUTE), two),
          flush=True)
    ctx.close()
    print("routes differ by at most %.2e" % np.abs(results["route 1"]["local_effects"] - results["route 2"]["local_effects"]).max(), flush=True)

    pdp_ms = best(lambda: bn.get_pdp(x, [FOCAL], "classification", N_OUT, bn.ActFun(fun="tanh"), bn.SoftMax, weights, alphas, None), runs=1)
    print("get_pdp, 100 grid points: %.1f ms" % pdp_ms, flush=True)

    t0 = time.perf_counter()
    looped = host_loop(x, weights, edges)
    print("host loop of %d predict_sets calls: %.1f ms   (differs from route 1 by at most %.2e)"
          % (len(edges), 1e3 * (time.perf_counter() - t0), np.abs(looped - results["route 1"]["local_effects"]).max()), flush=True)


main()
