#!/usr/bin/env python3
"""What the weight gradient of the log-likelihood costs (npbnn_loglik_grad), on config 2's shapes - 100 k x 256, [32, 8], 10 classes -
and config 4's - 1 M x 64, [16, 4], 2 Gaussian targets:

  npbnn_loglik_grad               one call on a context that holds the table: the median wall time of 200 calls after 20 warm ones
  phase 1, phase 2                their device time from NPBNN_INFO_GRAD_ROWS_NS / _FOLD_NS (HIP events, NPBNN_FI_TIMING=1: that run waits
                                  for every chunk, so the entry's own time is taken from the run without it), the medians of 200 calls;
                                  what is left of the entry is the upload of the weights, the preparation of the float32 blocks, the
                                  download of the totals and the host's work
  X bytes over time               phase 1 reads X once, phase 2 once per 32 hidden units: those bytes over the phase's time, as a share
                                  of 8 TB/s
  npbnn_eval                      the same weights through the evaluation entry, for scale: another quantity, no bar
  numpy float64                   bn.loglik_grad, the host definition, on the host arrays (the best of 3)

and, on config 2's shapes, bn.map_estimate's 200-step wall time with the log posterior it reaches beside the log posterior a default
MCMC reaches from the same start after 20 000 iterations.  Everything runs in two fresh processes, one after the other; boxes differ
in shader clock (tools/box_speed.py): compare within one run.
    python tools/time_grad.py [rows of config 2] [rows of config 4]"""
import contextlib
import io
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, TIMED, HBM_TBS = 20, 200, 8.0
SHAPES = {"config 2": dict(rows=100000, features=256, nodes=(32, 8), lik="cat", n_out=10),
          "config 4": dict(rows=1000000, features=64, nodes=(16, 4), lik="gauss", n_out=2)}


def median_ms(f, warm, timed):
    for _ in range(warm):
        f()
    t = []
    for _ in range(timed):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **k)


def one_shape(name, s):
    import npbnn_amd as bn
    from npbnn_amd import _capi as capi
    rs = np.random.default_rng(3)
    n, f = s["rows"], s["features"]
    x = rs.standard_normal((n, f)).astype(np.float32)
    dims = [f] + list(s["nodes"]) + [s["n_out"]]
    w = [rs.normal(0, 1.0 / np.sqrt(dims[i] + 1), (dims[i + 1], dims[i] + 1)) for i in range(len(dims) - 1)]
    cat = s["lik"] == "cat"
    y = rs.integers(0, s["n_out"], n) if cat else rs.standard_normal((n, s["n_out"]))
    sigma = None if cat else np.ones(s["n_out"])
    ctx = bn.HipContext()
    ctx.set_data(x)
    (ctx.set_labels if cat else ctx.set_targets)(y)
    ctx.set_arch_from_weights(w, f, capi.ACT_TANH, capi.OUT_SOFTMAX if cat else capi.OUT_IDENTITY, capi.LIK_CATEGORICAL if cat else capi.LIK_GAUSS,
                              n_targets=0 if cat else s["n_out"])
    entry = median_ms(lambda: ctx.loglik_grad(w, sigma=sigma), WARM, TIMED)
    ev = median_ms(lambda: ctx.eval(w, sigma=sigma), WARM, TIMED)
    os.environ["NPBNN_FI_TIMING"] = "1"
    ph = []
    for _ in range(TIMED):
        ctx.loglik_grad(w, sigma=sigma)
        ph.append((ctx.info(capi.INFO_GRAD_ROWS_NS), ctx.info(capi.INFO_GRAD_FOLD_NS)))
    os.environ.pop("NPBNN_FI_TIMING", None)
    p1, p2 = (1e-6 * float(np.median([p[i] for p in ph])) for i in (0, 1))
    ctx.close()
    fp = -(-f // 16) * 16
    b1, b2 = 4.0 * n * fp, 4.0 * n * fp * (-(-s["nodes"][0] // 32))
    act = bn.ActFun(fun="tanh")
    lik = bn.calc_likelihood if cat else bn.calc_likelihood_regression
    host = min(median_ms(lambda: bn.loglik_grad(x, y, w, act, lik, sigma=sigma), 0, 1) for _ in range(3))
    print("%s: %d x %d, %s, %s" % (name, n, f, list(s["nodes"]), "%d classes" % s["n_out"] if cat else "%d Gaussian targets" % s["n_out"]))
    print("  npbnn_loglik_grad %.3f ms   phase 1 %.3f ms (X at %.2f TB/s = %.1f %% of %.0f)   phase 2 %.3f ms (X at %.2f TB/s = %.1f %%)   "
          "upload, preparation, download and host %.3f ms" % (entry, p1, 1e-9 * b1 / p1, 100e-9 * b1 / p1 / HBM_TBS, HBM_TBS, p2, 1e-9 * b2 / p2,
                                                             100e-9 * b2 / p2 / HBM_TBS, entry - p1 - p2))
    print("  npbnn_eval of the same weights %.3f ms   numpy float64 host definition %.1f ms" % (ev, host), flush=True)


def warm_start(s):
    import npbnn_amd as bn
    rs = np.random.default_rng(5)
    n, f = s["rows"], s["features"]
    x = rs.standard_normal((n, f)).astype(np.float32)
    teacher = [rs.normal(0, 1.0 / np.sqrt(f + 1), (16, f + 1)), rs.normal(0, 1.0, (s["n_out"], 17))]
    h = np.tanh(x @ teacher[0][:, 1:].T + teacher[0][:, 0])
    labels = np.argmax(h @ teacher[1][:, 1:].T + teacher[1][:, 0] + rs.gumbel(size=(n, s["n_out"])), axis=1)
    dat = dict(data=x, labels=labels, test_data=np.zeros((0, f)), test_labels=np.zeros(0))

    def model():
        np.random.seed(1234)
        return quiet(bn.npBNN, dat, n_nodes=list(s["nodes"]), actFun=bn.ActFun(fun="tanh"), use_bias_node=2)

    bnn = model()
    bn.map_estimate(bnn, n_iter=2, apply=False)                     # (context, upload and first launches)
    t0 = time.perf_counter()
    res = bn.map_estimate(bnn, n_iter=200)
    t_map = time.perf_counter() - t0
    chain = model()
    mcmc = quiet(bn.MCMC, chain, n_iteration=20000)
    start = mcmc._logPost
    t0 = time.perf_counter()
    quiet(mcmc.run_steps, chain, 20000)
    t_mcmc = time.perf_counter() - t0
    print("warm start on %d x %d, %s: log posterior %.1f at the start; map_estimate, 200 steps: %.1f in %.2f s; default MCMC, 20 000 iterations: "
          "%.1f in %.2f s" % (n, f, list(s["nodes"]), start, res["log_posterior"].max(), t_map, mcmc._logPost, t_mcmc), flush=True)


def child(rows2, rows4):
    shapes = {k: dict(v) for k, v in SHAPES.items()}
    shapes["config 2"]["rows"], shapes["config 4"]["rows"] = rows2, rows4
    for name, s in shapes.items():
        one_shape(name, s)
    warm_start(shapes["config 2"])


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
    else:
        rows = [str(int(a)) for a in sys.argv[1:3]] + [str(SHAPES["config 2"]["rows"]), str(SHAPES["config 4"]["rows"])][len(sys.argv[1:3]):]
        for i in range(2):
            print("---- process %d" % (i + 1), flush=True)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child"] + rows)
