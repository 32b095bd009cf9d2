"""One rank of a multi-process test (started by npbnn_amd.launch.spawn_ranks; RANK / WORLD_SIZE / MASTER_* in the environment).

    python tests/rank_worker.py mc3 <tmpdir> <backend: oracle|hip> <comm: socket|rccl> <device_exchange: 0|1|none> [fail=<rank>:<mode>]
    python tests/rank_worker.py idle <seconds> [fail=<rank>:<mode>]
    python tests/rank_worker.py rowshard <backend: oracle|hip> <comm: socket|rccl> <case: cls|clsw|reg|regsig>
    python tests/rank_worker.py rowshard64 <backend: oracle|hip> <comm: socket|rccl> <case,case,...: names of rowshard_cases.CASES>
    python tests/rank_worker.py rowshard_range <backend: oracle|hip> <comm: socket|rccl>

``mc3``: the reference's golden MC3 run (tests/golden/mc3.npz: 4 chains, swaps every 20 iterations) with chain i on rank
i % world.  oracle backend (CPU stand-in, float64): the golden swap sequence, final states and log rows exactly; hip backend
(float32 rows on the GPU): the golden swap sequence for at least its first five accepted swaps, every rank agreeing on the
whole swap log.  Every rank prints ``RANK <r> OK`` at the end.

``fail=<rank>:<mode>`` plants a failure on that rank after the second swap interval: ``raise`` (exception, exit status 1),
``exit0`` (the rank leaves quietly with status 0 - its peers must notice by themselves).
"""
import contextlib
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def planted(argv):
    for a in argv:
        if a.startswith("fail="):
            r, mode = a[5:].split(":")
            return int(r), mode
    return None, None


def fail_now(mode, stamp_dir):
    if stamp_dir:
        with open(os.path.join(stamp_dir, "failed_at"), "w") as f:
            f.write(repr(time.time()))
    if mode == "exit0":
        os._exit(0)
    raise RuntimeError("planted failure")


def make_comm(kind, rank, world):
    from npbnn_amd import comm as cm
    if kind == "rccl":
        c = cm.RcclComm(rank=rank, world_size=world, device=int(os.environ.get("LOCAL_RANK", "0")))
        if rank == 0:
            print("comm:", c.describe(), flush=True)
        return c
    return cm.SocketComm(rank=rank, world_size=world, timeout=float(os.environ.get("NPBNN_SOCKET_TIMEOUT_S", "60")))


def run_mc3(argv):
    import numpy as np
    import cases
    import npbnn_amd as bn
    tmpdir, backend, comm_kind, dev_x = argv[:4]
    fail_rank, fail_mode = planted(argv)
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    comm = make_comm(comm_kind, rank, world)
    cfg = cases.MC3_TRACE
    g = np.load(os.path.join(ROOT, "tests", "golden", "mc3.npz"))
    dat = cases.classification_data(cfg["seed"], cfg["n_rows"], cfg["n_features"], cfg["n_classes"], cfg["n_test"])
    np.random.seed(1234)
    with contextlib.redirect_stdout(io.StringIO()):
        bnn = bn.npBNN(dat, n_nodes=cfg["n_nodes"], use_bias_node=cfg["bias"], seed=1, init_std=0.1)
        logger = bn.postLogger(bnn, filename="MC3", wdir=tmpdir, log_all_weights=0, continue_logfile=rank != 0)
        if backend == "oracle":
            from oracle_backend import OracleExchangeBackend, serve_from_oracle
            serve_from_oracle(lambda b: OracleExchangeBackend(b, 0))
        mc3 = bn.MC3(bnn, logger=logger, n_post_samples=10, sampling_f=cfg["swap_frequency"], n_iteration=cfg["n_iteration"],
                     n_chains=cfg["n_chains"], swap_frequency=cfg["swap_frequency"], verbose=0, comm=comm)
    mc3.device_exchange = None if dev_x == "none" else bool(int(dev_x))
    mc3.exchange_batch = 6
    assert mc3.local_ids == [i for i in range(cfg["n_chains"]) if i % world == rank]
    if fail_rank == rank:       # leave after the second swap interval
        from npbnn_amd import exchange as ex
        real = ex.host_swap
        seen = [0]

        def counting(*a, **k):
            out = real(*a, **k)
            seen[0] += 1
            if seen[0] == 2:
                fail_now(fail_mode, tmpdir)
            return out
        ex.host_swap = counting
    with contextlib.redirect_stdout(io.StringIO()):
        mc3.run_mcmc()
    accepted = [i for i, s in enumerate(mc3.swap_log) if s[4]]
    want = [int(r[0]) for r in g["swapped"]]
    if backend == "oracle":
        assert accepted == want, (accepted, want)
        for i, pair in enumerate(mc3.singleChainArgs):
            if pair is None:
                continue
            assert pair[1]._temperature == g["final_temperature"][i]
            np.testing.assert_allclose(pair[1]._logPost, g["final_logPost"][i], rtol=1e-9)
            for li, w in enumerate(pair[0]._w_layers):
                np.testing.assert_array_equal(w, g["w_c%d_l%d" % (i, li)])
    else:
        common = 0
        for a, b in zip(accepted, want):
            if a != b:
                break
            common += 1
        assert common >= 5, "swap sequences diverged immediately: %s vs %s" % (accepted, want)
    # every rank decided the same swaps
    mine = np.array([float(s[4]) for s in mc3.swap_log])
    allv = comm.allgather_f64(mine)
    assert np.all(allv == allv[0]), "ranks disagree on the swap log"
    temps = comm.allgather_f64(np.array([p[1]._temperature if p is not None else np.nan for p in mc3.singleChainArgs]))
    assert sorted(np.nanmax(temps, axis=0)) == sorted(g["temperatures0"]), "temperatures are a permutation of the ladder"
    comm.barrier()
    if rank == 0:
        rows = np.loadtxt(logger._logfile, skiprows=1)
        if backend == "oracle":
            np.testing.assert_allclose(rows, g["log_rows"], rtol=1e-8)
        else:
            assert rows.shape[0] >= 25
    comm.close()
    print("RANK %d OK" % rank, flush=True)


def run_rowshard(argv):
    """rowshard <backend: oracle|hip> <comm: socket|rccl> <case: cls|clsw|reg|regsig>: ONE chain whose rows are split over the ranks
    (MCMC(row_comm=...)) against the same chain on all rows in this very process: the same accept decisions, the same weights, the
    same statistics."""
    import numpy as np
    import cases
    import npbnn_amd as bn
    from npbnn_amd.rowshard import shard_rows
    backend, comm_kind, case = argv[:3]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    comm = make_comm(comm_kind, rank, world)
    if backend == "oracle":
        from oracle_backend import OracleChainBackend, serve_from_oracle
        serve_from_oracle(lambda b: OracleChainBackend(b, 0 if b._estimation_mode == "classification" else 1))
    if case in ("cls", "clsw"):
        dat = cases.classification_data(5, 403, 12, 4, n_test=61)
        model = dict(n_nodes=[8, 5], use_bias_node=2, seed=3, use_class_weights=int(case == "clsw"))
        sampler = dict(update_f=[0.05, 0.1, 0.2], update_ws=[0.05, 0.05, 0.05], n_iteration=2000, sampling_f=10, adapt_f=0.3, adapt_freq=25)
    else:
        dat = cases.regression_data(7, 389, 10, 2, n_test=50)
        model = dict(n_nodes=[6, 4], use_bias_node=2, seed=3, estimation_mode="regression", empirical_error=(case == "reg"),
                     actFun=bn.ActFun(fun="tanh"))
        sampler = dict(update_f=[0.05, 0.1, 0.2], update_ws=[0.03, 0.03, 0.03], n_iteration=200, sampling_f=10, estimate_error=(case == "regsig"))

    def run(data, **extra):
        np.random.seed(1234)
        with contextlib.redirect_stdout(io.StringIO()):
            bnn = bn.npBNN(data, **model)
            mcmc = bn.MCMC(bnn, **sampler, **extra)
            trail = [float(mcmc._logLik)]
            mcmc.run_steps(bnn, 30)
            trail.append(float(mcmc._logLik))
            for _ in range(4):
                mcmc.mh_step(bnn)
            trail.append(float(mcmc._logLik))
            mcmc.run_steps(bnn, 45)
            trail.append(float(mcmc._logLik))
            stats = [float(mcmc._accuracy), float(mcmc._test_accuracy)]
        return bnn, mcmc, trail, stats

    bnn0, mcmc0, trail0, stats0 = run(dat)
    bnn1, mcmc1, trail1, stats1 = run(shard_rows(dat, rank, world), row_comm=comm)
    assert mcmc1._backend.row_sharded and mcmc1._backend.n_rows_total == len(dat["data"])
    assert len(bnn1._data) < len(dat["data"])
    assert mcmc0._current_iteration == mcmc1._current_iteration == 79
    tol = 1e-10 if backend == "oracle" else 2e-6
    np.testing.assert_allclose(trail1, trail0, rtol=tol)
    assert mcmc1._last_accepted_mem == mcmc0._last_accepted_mem, "the sharded chain took other decisions"
    assert sum(mcmc0._last_accepted_mem) >= 5, "a chain that never moves proves nothing"
    for a, b in zip(bnn1._w_layers, bnn0._w_layers):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_allclose(stats1, stats0, rtol=1e-9 if backend == "oracle" else 1e-5)
    if case == "clsw":
        np.testing.assert_allclose(bnn1._class_w, bnn0._class_w, rtol=1e-14)
    if np.size(bnn0._error_prm):
        np.testing.assert_allclose(bnn1._error_prm, bnn0._error_prm, rtol=tol * 100)
    # every rank holds the same chain
    mine = np.concatenate([w.ravel() for w in bnn1._w_layers])
    allw = comm.allgather_f64(mine)
    assert np.all(allw == allw[0]), "ranks disagree on the chain"
    if backend == "hip":
        used = getattr(mcmc1, "_device_schedule_used", None)
        assert used == 1, "a row-sharded batch runs on kernel boundaries (schedule %r)" % used
    comm.barrier()
    comm.close()
    print("RANK %d OK" % rank, flush=True)


def run_rowshard64(argv):
    """rowshard64 <backend: oracle|hip> <comm: socket|rccl> <case,case,...>: for every named case of rowshard_cases.CASES, ONE chain
    whose rows are split over the ranks, advanced in short dispatches and held after every one of them to float64 ON ALL ROWS with
    the chain's own weights (test_hip_chain_oracle.check_state_on, its bars; 1e-10 on the float64 stand-in) - log-likelihood, prior,
    accuracies, sigma.  Rank 0 also runs the unsharded float64 twin on all rows and compares the accept / reject sequences; then
    all ranks must hold the same weights.  Every case prints its worst relative log-likelihood error."""
    import numpy as np
    import oracle as orc
    import npbnn_amd as bn
    import rowshard_cases as rc
    import test_hip_chain_oracle as tco
    from npbnn_amd.rowshard import shard_rows
    backend, comm_kind, names = argv[0], argv[1], argv[2].split(",")
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    comm = make_comm(comm_kind, rank, world)
    hip = backend == "hip"
    if not hip:
        from oracle_backend import OracleChainBackend, serve_from_oracle
        serve_from_oracle(lambda b: OracleChainBackend(b, {"classification": 0, "regression-error": 2}.get(b._estimation_mode, 1)))
    bars = {} if hip else dict(ll_rtol=1e-10, lp_rtol=1e-12, acc_tol=1e-10)
    sigma_tol = tco.ACC_TOL if hip else 1e-10         # (sigma^2 is the mean squared residual less the squared mean: the accuracy's bar)
    for name in names:
        case = rc.CASES[name]
        assert comm_kind == "rccl" or case["world"] == world, (name, world)       # (over RCCL: one rank per GPU, however many there are)
        lik, extra, rows = case["lik"], case["extra"], case["rows"]
        if case["l0"]:
            os.environ["NPBNN_L0"] = case["l0"]
        else:
            os.environ.pop("NPBNN_L0", None)
        dat = rc.case_data(case, world)
        x, lab, x_t, lab_t = dat["data"], dat["labels"], dat["test_data"], dat["test_labels"]
        slopes = extra.get("slopes")

        def build(data, **kw):
            model = dict(extra.get("model", {}))
            if slopes:
                model["actFun"] = bn.ActFun(fun="genReLU", prm=np.array(slopes, dtype=float), trainable=True)
            bnn, mcmc = tco.make_chain(bn, lik, data, case["widths"], model_kw=model, **dict(extra.get("mcmc", {}), **kw))
            mcmc.n_candidates, mcmc.SUB_BATCH = case["d"], 16
            return bnn, mcmc
        bnn, mcmc = build(shard_rows(dat, rank, world), row_comm=comm)
        assert mcmc._backend.row_sharded and mcmc._backend.n_rows_total == rows and len(bnn._data) < rows
        class_w = ()
        if extra.get("model", {}).get("use_class_weights"):          # balanced weights from the labels of ALL rows (BNN_env.py:98-102)
            counts = np.bincount(lab, minlength=rc.N_CLASSES).astype(float)
            class_w = (counts.max() / counts) / np.mean(counts.max() / counts)
            np.testing.assert_allclose(bnn._class_w, class_w, rtol=1e-14)
        moved = [False]

        def check(accuracy):
            act = orc.Act("genReLU", prm=np.array(bnn._act_fun._acc_prm, dtype=float), trainable=True) if slopes else None
            prior_extra = np.log(10.0) * -np.sum(bnn._act_fun._acc_prm) * 10.0 if slopes and mcmc._slope_term_in_prior else 0.0
            sig2 = None
            if extra.get("sigma") == "estimated":
                sig2 = np.ones(case["k"]) * bnn._error_prm             # the chain's own values
            elif extra.get("sigma") == "empirical" and moved[0]:       # (until the first accepted proposal sigma is the initial 1)
                y = orc.forward(x, bnn._w_layers, orc.Act("tanh"), orc.out_identity)
                sig2 = np.std(y - lab, axis=0)
                np.testing.assert_allclose(bnn._error_prm, sig2, rtol=sigma_tol)
            tco.check_state_on(lik, bnn, mcmc, x, lab, x_t, lab_t, worst=errs, accuracy=accuracy, act=act, sig2=sig2, class_w=class_w,
                               prior_extra=prior_extra, rowwise_accuracy=hip, min_abs=0.1 * rows, **bars)
            if accuracy and (hip or lik in ("cat", "gauss")):
                stats = np.array([float(mcmc._accuracy), float(mcmc._test_accuracy)])
                allv = np.asarray(comm.allgather_f64(stats)).reshape(world, 2)
                assert np.all(allv == allv[0]), ("ranks disagree on the accuracies", allv.tolist())
                if lik != "cat":              # (check_state_on holds the test accuracy of a classification only)
                    y_t = orc.forward(x_t, bnn._w_layers, orc.Act("tanh"), tco._out_fn(lik))
                    kk = lab_t.shape[1] if lik in ("gauss", "err", "nb2d") else 1
                    mean = y_t[:, :kk] if lik in ("gauss", "err") else (10.0 ** y_t[:, :kk] if lik == "nb10" else np.exp(y_t[:, :kk]))
                    want = float(np.mean((mean - lab_t[:, :kk]) ** 2))
                    tol = bars.get("acc_tol", tco.ACC_TOL)
                    assert abs(stats[1] - want) <= tol * max(1.0, want), ("test mse", stats[1], want)
                    if lik == "pois":         # (poi_acc: check_state_on leaves it out)
                        want = float(np.mean((np.exp(orc.forward(x, bnn._w_layers, orc.Act("tanh"), orc.out_identity)[:, 0]) - lab[:, 0]) ** 2))
                        assert abs(stats[0] - want) <= tol * max(1.0, want), ("poisson mse", stats[0], want)

        errs, decisions = [], []
        check(True)
        sizes = tco.dispatch_sizes(rc.N_ITER)
        for j, k in enumerate(sizes):
            mcmc.run_steps(bnn, k)
            decisions += list(mcmc._last_accepted_mem[-k:])
            moved[0] = moved[0] or sum(decisions) > 0
            check(j % 2 == 1 or j + 1 == len(sizes))
        assert mcmc._current_iteration == rc.N_ITER
        if extra.get("sigma") == "estimated":
            assert mcmc._current_iteration > mcmc._estimate_error and not np.all(bnn._error_prm == 1), "no sigma proposal was accepted"
        if hip:
            ctx = mcmc._backend.ctx
            assert mcmc._device_iterations == rc.N_ITER, "the batches did not run on the device (%d iterations did)" % mcmc._device_iterations
            assert mcmc._device_schedule_used == 1, "a row-sharded batch runs on kernel boundaries (schedule %r)" % mcmc._device_schedule_used
            if case["d"] > 1:
                assert mcmc._device_passes < rc.N_ITER, "the extra candidate slots were launched and thrown away"
            assert bool(ctx.is_wide()) == bool(extra.get("wide")), "the case did not take the path it names"
            if case["l0"]:
                from npbnn_amd import _capi
                assert ctx.info(_capi.INFO_L0_F16) == (0 if case["l0"] == "f32" else 1)
        if rank == 0:
            rb, rm = tco.oracle_twin(lik, lambda: build(dat))
            ref = []
            for k in sizes:
                rm.run_steps(rb, k)
                ref += list(rm._last_accepted_mem[-k:])
            prefix = tco.assert_trajectory(decisions, ref)
            assert hip or decisions == ref, "the sharded float64 chain left the float64 chain on all rows"
            assert sum(decisions) >= 5, "a chain that hardly moves proves nothing (%d accepted)" % sum(decisions)
            print("[rowshard64] %-10s %-11s world %d  worst logLik rel err %.3e  common prefix %d of %d  accepted %d"
                  % (extra["family"], name, world, max(errs), prefix, len(ref), sum(decisions)), flush=True)
        mine = np.concatenate([w.ravel() for w in bnn._w_layers])
        allw = comm.allgather_f64(mine)
        assert np.all(allw == allw[0]), "ranks disagree on the chain"
        if hip:
            mcmc._backend.ctx.close()
    comm.barrier()
    comm.close()
    print("RANK %d OK" % rank, flush=True)


def run_rowshard_range(argv):
    """rowshard_range <backend: oracle|hip> <comm: socket|rccl>: rowshard_cases.RANGE_CASE - ONE chain whose rows are split over
    the ranks takes planted draws (range_cases.serve_draws; planned in float64 on ALL rows, the same on every rank) whose
    iteration RANGE_T_STAR puts a layer-0 weight outside fp16: every rank abandons that batch and repeats it on float32
    (``l0_mode()``), the flags and weights are the float64 stand-in's on every rank, the state is float64's on all rows."""
    import numpy as np
    import npbnn_amd as bn
    import range_cases as rg
    import rowshard_cases as rc
    import test_hip_chain_oracle as tco
    from npbnn_amd.rowshard import shard_rows
    backend, comm_kind = argv[:2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    comm = make_comm(comm_kind, rank, world)
    hip = backend == "hip"
    if not hip:
        from oracle_backend import OracleChainBackend, serve_from_oracle
        serve_from_oracle(lambda b: OracleChainBackend(b, 0))
    os.environ["NPBNN_NO_FAST_DISPATCH"] = "1"           # (the kept dispatch draws for itself)
    os.environ.pop("NPBNN_L0", None)
    case = rc.RANGE_CASE
    assert case["world"] == world
    dat = rc.case_data(case, world)
    bnn, mcmc = tco.make_chain(bn, "cat", shard_rows(dat, rank, world), case["widths"], row_comm=comm)
    mcmc.n_candidates, mcmc.SUB_BATCH = case["d"], 64
    assert mcmc._backend.row_sharded and len(bnn._data) < case["rows"]
    assert bnn._prior_kind() == rg.PRIOR_NORMAL and bnn._w_bound == np.inf
    p = dict(rg.problem_of(bnn), x=np.asarray(dat["data"], dtype=np.float64), labels=np.asarray(dat["labels"]))
    K = sum(rc.RANGE_DISPATCHES)
    plant = rg.plant_index(p, np.random.default_rng(9))
    with np.errstate(over="ignore"):
        plan = rg.build_batches(p, 97, [(K, rc.RANGE_T_STAR, plant, False, 0, "mid")])[0]
    rg.serve_draws(mcmc, plan)
    bars = {} if hip else dict(ll_rtol=1e-10, lp_rtol=1e-12, acc_tol=1e-10)
    modes, done = [], 0
    if hip:            # the layer-0 path of every device batch, read before the dispatch's own evaluations (accuracies) follow it
        ctx = mcmc._backend.ctx
        real_chain_run = ctx.chain_run

        def chain_run(*a, **kw):
            out = real_chain_run(*a, **kw)
            modes.append(ctx.l0_mode())
            return out
        ctx.chain_run = chain_run
    with np.errstate(over="ignore"):
        for k in rc.RANGE_DISPATCHES:
            mcmc.run_steps(bnn, k)
            done += k
            assert list(mcmc._last_accepted_mem[-k:]) == [int(a) for a in plan["want"]["acc"][done - k:done]], "left the stand-in's decisions"
            tco.check_state_on("cat", bnn, mcmc, dat["data"], dat["labels"], dat["test_data"], dat["test_labels"], min_abs=0.1 * case["rows"], **bars)
    assert done - rc.RANGE_DISPATCHES[-1] > rc.RANGE_T_STAR >= rc.RANGE_DISPATCHES[0]
    assert rg.pack(bnn._w_layers).tobytes() == plan["want"]["w"].tobytes(), "the weights are not the stand-in's"
    if hip:
        assert modes == ["f16-split", "f32", "f16-split"], modes
        assert mcmc._device_iterations == K and mcmc._device_schedule_used == 1
    allw = comm.allgather_f64(rg.pack(bnn._w_layers))
    assert np.all(allw == allw[0]), "ranks disagree on the chain"
    flags = comm.allgather_f64(np.array(mcmc._last_accepted_mem[-K:], dtype=float))
    assert np.all(flags == flags[0]), "ranks disagree on the decisions"
    if hip:
        mcmc._backend.ctx.close()
    comm.barrier()
    comm.close()
    print("RANK %d OK" % rank, flush=True)


def run_idle(argv):
    fail_rank, fail_mode = planted(argv)
    rank = int(os.environ["RANK"])
    if fail_rank == rank:
        time.sleep(0.3)
        fail_now(fail_mode, None)
    time.sleep(float(argv[0]))
    print("RANK %d OK" % rank, flush=True)


if __name__ == "__main__":
    {"mc3": run_mc3, "idle": run_idle, "rowshard": run_rowshard, "rowshard64": run_rowshard64, "rowshard_range": run_rowshard_range}[sys.argv[1]](sys.argv[2:])
