#!/usr/bin/env python3
"""What a partial-dependence call (npbnn_predict_pdp) costs on each route: the grid-batched kernel (NPBNN_INFO_PDP_ROUTE 1) and one
pass per (grid point, set group) (2, forced with NPBNN_PDP_PER_GRID=1).  Config 2's shapes - 100 k x 256, [32, 8], 10 classes - with
100 stored samples and one continuous focal feature (100 grid points), and the default network [50, 5] on 1024 features, which runs
on the weight-streamed path (route 2 only).  Wall time of the whole call, copy of the [grid, rows, classes] result included; the best
of two after a warm-up call.  Boxes differ in shader clock (tools/box_speed.py): compare routes within one run.
    python tools/time_pdp.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npbnn_amd as bn  # noqa: E402
from npbnn_amd import _capi as capi  # noqa: E402


def case(name, n_rows, n_features, n_nodes, n_out, n_sets, seed=3):
    rs = np.random.default_rng(seed)
    x = rs.standard_normal((n_rows, n_features))
    dims = [n_features] + list(n_nodes) + [n_out]
    weights = [[rs.normal(0, 1.0 / np.sqrt(dims[i] + 1), (dims[i + 1], dims[i] + 1)) for i in range(len(dims) - 1)]
               for _ in range(n_sets)]
    grid = bn.make_pdp_features(x, [0])
    ctx = bn.HipContext()
    ctx.set_data(x)
    ctx.set_arch_from_weights(weights[0], n_features, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_NONE)
    routes = (("grid-batched", None), ("per grid point", "1")) if not ctx.info(capi.INFO_WIDE) else (("per grid point", None),)
    for label, force in routes:
        if force:
            os.environ["NPBNN_PDP_PER_GRID"] = force
        else:
            os.environ.pop("NPBNN_PDP_PER_GRID", None)
        ctx.predict_pdp(weights, [0], grid)
        best = float("inf")
        for _ in range(2):
            t0 = time.perf_counter()
            ctx.predict_pdp(weights, [0], grid)
            best = min(best, time.perf_counter() - t0)
        print("%s: route %d (%s), %d grid points x %d samples: %.1f ms" % (name, ctx.info(capi.INFO_PDP_ROUTE), label, len(grid), n_sets,
                                                                           1e3 * best), flush=True)
    os.environ.pop("NPBNN_PDP_PER_GRID", None)
    ctx.close()


case("config 2 (100k x 256, [32, 8], 10 classes)", 100000, 256, (32, 8), 10, 100)
case("default network (20k x 1024, [50, 5], 10 classes)", 20000, 1024, (50, 5), 10, 100)
