#!/usr/bin/env python3
"""Wall time of get_posterior_hpd (replay into a device stack, one HPD launch, mean and bounds back) against get_posterior_est (every
sample's predictions back to the host) followed by numpy's HPD of every (row, output) column.  A regression checkpoint with S stored
samples of a [32 features, 16, 8, 1 output] network on R rows; the numpy HPD is the vectorised restatement of calcHPD
(tests/hpd_cases.py), not upstream's per-row Python loop, which is slower still.
    python tools/time_hpd.py [--samples 1000] [--rows 100000] [--reps 3]
Run under `rocprofv3 --kernel-trace --stats -- python tools/time_hpd.py` to split the device time between the replay and hpd_kernel."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import npbnn_amd as bn  # noqa: E402
import hpd_cases  # noqa: E402


def checkpoint(path, n_samples, n_rows, n_features=32):
    rs = np.random.default_rng(0)
    x = rs.standard_normal((n_rows, n_features))
    y = np.tanh(x[:, :4].sum(axis=1, keepdims=True)) + 0.1 * rs.standard_normal((n_rows, 1))
    dat = dict(data=x, labels=y, test_data=np.zeros((0, n_features)), test_labels=np.zeros((0, 1)))
    bnn = bn.npBNN(dat, n_nodes=[16, 8], actFun=bn.ActFun(fun="tanh"), use_bias_node=2, estimation_mode="regression")
    mcmc = bn.MCMC(bnn, n_iteration=10, sampling_f=10, print_f=1000, n_post_samples=n_samples)
    logger = bn.postLogger(bnn, wdir=os.path.dirname(path), filename="t", log_all_weights=0)
    logger._post_weight_samples = [dict(weights=[w + rs.normal(0, 0.05, w.shape) for w in bnn._w_layers], alphas=np.zeros(3),
                                        mcmc_it=i, error_prm=np.array([1.0])) for i in range(n_samples)]
    bn.SaveObject([bnn, mcmc, logger], path)


def best_of(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return min(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--level", type=float, default=0.95)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        pkl = os.path.join(d, "t.pkl")
        checkpoint(pkl, a.samples, a.rows)
        bn.get_posterior_hpd(pkl, a.level)                  # warm-up: context, kernels, allocations
        t_hpd, res = best_of(lambda: bn.get_posterior_hpd(pkl, a.level), a.reps)

        def est_then_numpy():
            est = bn.get_posterior_est(pkl)
            return est, hpd_cases.hpd_columns(est['post_est'], a.level)
        t_est, (est, (lo, hi)) = best_of(est_then_numpy, a.reps)
        t_est_only, _ = best_of(lambda: bn.get_posterior_est(pkl), a.reps)
    same = bool(np.array_equal(res['lower'], lo) and np.array_equal(res['upper'], hi))
    print(json.dumps(dict(samples=a.samples, rows=a.rows, outputs=1, level=a.level, get_posterior_hpd_s=round(t_hpd, 4),
                          get_posterior_est_plus_numpy_hpd_s=round(t_est, 4), get_posterior_est_s=round(t_est_only, 4),
                          speedup=round(t_est / t_hpd, 2), bounds_equal=same)))


if __name__ == "__main__":
    main()
