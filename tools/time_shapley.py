#!/usr/bin/env python3
"""What Shapley attributions cost.  Config 2's shapes - 100 k x 256, [32, 8], 10 classes - with 100 stored samples.

At the working size (256 explained rows, 20 background rows, 8 permutations unless given):

  get_shapley                     the whole call on route 1 and on route 2 (NPBNN_SHAPLEY_PLAIN=1): context, upload of the table,
                                  npbnn_predict_shapley, the summary on the host
  npbnn_predict_shapley alone     on a context that holds the table, and the device time of its walk kernels (HIP events,
                                  NPBNN_FI_TIMING=1: that run waits for every launch, so the entry's own time is taken from a run
                                  without it), as steps per second: sets x rows x walks x players steps

At a size the other way round can run (64 explained rows, 4 backgrounds, 2 permutations): the same two, and the way round that
existed before: every hybrid row of every walk - rows x walks x (players + 1) of them - built with numpy, uploaded as a table, and
replayed with npbnn_predict_sets; the differences of consecutive rows are then phi's walks.  Its parts are timed one by one.

Wall time of each, the best of two after a warm-up call (the way round: one run after none; its parts add up to seconds).  Boxes
differ in shader clock (tools/box_speed.py): compare within one run.
    python tools/time_shapley.py [n_explain [n_background [n_perm]]]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npbnn_amd as bn  # noqa: E402
from npbnn_amd import _capi as capi  # noqa: E402

N_ROWS, N_FEATURES, NODES, N_OUT, N_SETS = 100000, 256, (32, 8), 10, 100
N_EXPLAIN = int(sys.argv[1]) if len(sys.argv) > 1 else 256
N_BG = int(sys.argv[2]) if len(sys.argv) > 2 else 20
N_PERM = int(sys.argv[3]) if len(sys.argv) > 3 else 8
SMALL = (64, 4, 2)


def best(f, runs=2, warm=True):
    if warm:
        f()
    t = float("inf")
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        t = min(t, time.perf_counter() - t0)
    return 1e3 * t


def timed(f):
    t0 = time.perf_counter()
    res = f()
    return res, 1e3 * (time.perf_counter() - t0)


def main():
    rs = np.random.default_rng(3)
    x = rs.standard_normal((N_ROWS, N_FEATURES))
    dims = [N_FEATURES] + list(NODES) + [N_OUT]
    weights = [[rs.normal(0, 1.0 / np.sqrt(dims[i] + 1), (dims[i + 1], dims[i] + 1)) for i in range(len(dims) - 1)] for _ in range(N_SETS)]
    alphas = [np.zeros(len(NODES))] * N_SETS
    print("%d x %d, %s, %d classes, %d stored samples" % (N_ROWS, N_FEATURES, list(NODES), N_OUT, N_SETS), flush=True)

    results = {}
    for n_e, n_bg, n_perm in ((N_EXPLAIN, N_BG, N_PERM), SMALL):
        rows = rs.choice(N_ROWS, n_e, replace=False)
        bg_rows = rs.choice(N_ROWS, n_bg, replace=False)
        perms = np.array([rs.permutation(N_FEATURES) for _ in range(n_perm)], dtype=np.int32)
        steps = float(N_SETS) * n_e * n_bg * n_perm * N_FEATURES
        print("\n%d explained rows, %d background rows, %d permutations: %.3g steps" % (n_e, n_bg, n_perm, steps), flush=True)
        for label, force in (("route 1", None), ("route 2", "1")):
            if force:
                os.environ["NPBNN_SHAPLEY_PLAIN"] = force
            whole = best(lambda: bn.get_shapley(x, N_OUT, bn.ActFun(fun="tanh"), bn.SoftMax, weights, alphas, None, rows=rows, background=bg_rows,
                                                n_perm=n_perm, antithetic=False))
            ctx = bn.HipContext()
            ctx.set_data(x)
            ctx.set_arch_from_weights(weights[0], N_FEATURES, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
            key = (label, n_e)
            entry = best(lambda: results.__setitem__(key, ctx.predict_shapley(weights, rows, bg_rows, perms)))
            route = ctx.info(capi.INFO_SHAPLEY_ROUTE)
            os.environ["NPBNN_FI_TIMING"] = "1"
            ctx.predict_shapley(weights, rows, bg_rows, perms)
            walk_ns = ctx.info(capi.INFO_SHAPLEY_WALK_NS)
            if walk_ns == 2 ** 31 - 1:
                print("(the walk kernels' time is at the counter's end, 2147 ms: it is a lower bound)", flush=True)
            walk_ms = 1e-6 * walk_ns
            os.environ.pop("NPBNN_FI_TIMING", None)
            os.environ.pop("NPBNN_SHAPLEY_PLAIN", None)
            ctx.close()
            print("%s: get_shapley %.1f ms; npbnn_predict_shapley alone, route %d: %.1f ms (walk kernels alone: %.1f ms, %.3g steps/s)"
                  % (label, whole, route, entry, walk_ms, steps / (1e-3 * walk_ms)), flush=True)
            results[(label, n_e, "entry_ms")] = entry
        a, b = results[("route 1", n_e)], results[("route 2", n_e)]
        print("routes differ by at most %.2e" % max(np.abs(a[k] - b[k]).max() for k in ("mean", "sq", "abs", "fx", "base")), flush=True)

    # the way round at the small size: the last rows, bg_rows and perms drawn above
    n_e, n_bg, n_perm = SMALL
    p = N_FEATURES

    def build():
        hybrid = np.empty((n_e, n_bg, n_perm, p + 1, N_FEATURES))
        hybrid[...] = x[bg_rows][None, :, None, None, :]
        for r, pi in enumerate(perms):
            for k in range(p):
                hybrid[:, :, r, k + 1:, pi[k]] = x[rows][:, None, None, pi[k]]
        return hybrid.reshape(-1, N_FEATURES)

    table, build_ms = timed(build)
    ctx = bn.HipContext()
    _, upload_ms = timed(lambda: ctx.set_data(table))
    ctx.set_arch_from_weights(weights[0], N_FEATURES, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
    y, replay_ms = timed(lambda: ctx.predict_sets(weights))
    ctx.close()

    def fold():
        y5 = y.reshape(N_SETS, n_e, n_bg, n_perm, p + 1, N_OUT)
        diff = y5[:, :, :, :, 1:] - y5[:, :, :, :, :-1]
        phi = np.zeros((N_SETS, n_e, p, N_OUT))
        for r, pi in enumerate(perms):
            phi[:, :, pi] += diff[:, :, :, r].sum(axis=2)
        return phi / (n_bg * n_perm)

    phi, fold_ms = timed(fold)
    total = build_ms + upload_ms + replay_ms + fold_ms
    mean = results[("route 1", n_e)]["mean"]
    print("\nthe way round, %d hybrid rows: build %.1f ms, upload %.1f ms, npbnn_predict_sets %.1f ms, differences %.1f ms: %.1f ms in all"
          % (table.shape[0], build_ms, upload_ms, replay_ms, fold_ms, total), flush=True)
    print("it differs from route 1 by at most %.2e" % np.abs(phi.mean(axis=0) - mean).max(), flush=True)
    entry = results[("route 1", n_e, "entry_ms")]
    print("npbnn_predict_shapley alone on route 1 takes %.1f ms: the way round takes %.0f times as long, its replay alone %.1f times"
          % (entry, total / entry, replay_ms / entry), flush=True)


main()
