"""GPU: the device chains held to float64 through the fp16-range repeat.

The fp16-split first layer is the default on every path; when a scaled layer-0 weight leaves the fp16 range the work is repeated
on the exact float32 path.  For the device chains that repeat is the most stateful one - the step kernel raises the flag while it
prepares candidates (also candidates that are dropped because an earlier one of their pass was accepted), the batch is thrown
away after the weight image already took the entries accepted before the flag, and the caller repeats it - and no chain of the
rest of the suite ever raises the flag.  Here the overflow is planted (tests/range_cases.py): explicit draws, one iteration adds
3e5 to a layer-0 weight, and ``log_u`` is built so that every decision has a float64 margin of 100 float32 log-likelihood bars.

    repeat path                                                          reached by                                        asserted from
    1  npbnn_chain_run returns NPBNN_E_RANGE, HipContext.chain_run       test_direct_entry_through_the_repeat              l0_mode(), the result's
       repeats with force_f32 (resident step on schedules 1-5, the       test_fp16_asked_for_by_name_raises_and_leaves_    schedule and candidates;
       outcome-speculative builds: schedule 5; weight-streamed step)     nothing_behind                                    NpbnnError.code
    2  FastBatch.run returns the code, the sampler hands the draws       test_sampler_walks_across_the_threshold           the codes FastBatch.run
       to the general path as "made ahead"                                                                                 returned, l0_mode()
    3  npbnn_chain_run_general repeats inside the C call                 test_general_chain_through_the_repeat             l0_mode()
    4  npbnn_chains_run_batched refuses the group, the wrapper builds    test_group_pass_through_the_repeat                l0_mode() of every chain
       every job again with force_f32
    5  npbnn_chains_run_exchange stops the chain before the proposal,    test_exchange_run_stops_before_the_planted_       segments_done, overflow,
       the driver finishes the interval through run_steps                proposal_and_the_driver_finishes                  on_interval's ``cold``
    6  the row-sharded chain: every rank abandons and repeats            test_row_sharded_chain_through_the_repeat         l0_mode() on every rank

What the planted batches found: ``HipContext.chain_run`` and ``chains_run_batched`` repeated on float32 even under
``set_l0_precision("f16")``, where every other entry raises NPBNN_E_RANGE (they raise now); the flag is raised when a candidate
is PREPARED, so a candidate that is out of range only beside an accepted earlier slot of its pass - and is dropped - repeats
the whole batch on float32 on schedules 1, 2, 4 and 5 alike (test_candidate_out_of_range_only_while_dropped asserts it: right
results, one batch slower); an exchange run, on the overlapped schedule, stops up to 2 D - 1 iterations before the proposal.

Every run is held to the float64 stand-in (``OracleChainBackend``) with the bars of test_hip_chain_oracle - accepted flags equal
at every iteration, proposed log-likelihoods to LL_RTOL, proposed log-priors to LP_RTOL, returned weights bit for bit (they are
float64 functions of the decisions) - and, where the repeat ran, to a second context with ``set_l0_precision("f32")`` byte for
byte: ``plan_launch`` with ``force_f32`` and with the ``f32`` option rebuild the same float32 network and plan the same launch
(wave count and kernel are functions of the network, the table and the candidate count; the schedule is given by number)."""
import numpy as np
import pytest

import range_cases as rc
from test_hip_chain_oracle import LL_RTOL, LP_RTOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bn():
    import npbnn_amd
    from npbnn_amd import _capi
    _capi.load_library()
    return npbnn_amd


def make_ctx(bn, p, l0="auto", share=None, weights=None):
    from npbnn_amd import _capi as capi
    ctx = bn.HipContext(0)
    if l0 != "auto":
        ctx.set_l0_precision(l0)
    if share is not None:
        ctx.share_data(share)
    else:
        ctx.set_data(p["x"])
    if p["lik"] == "cat":
        ctx.set_labels(p["labels"])
        ctx.set_arch_from_weights(weights or p["w"], rc.N_FEATURES, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_CATEGORICAL)
    else:
        ctx.set_targets(p["labels"])
        ctx.set_arch_from_weights(weights or p["w"], rc.N_FEATURES, capi.ACT_TANH, capi.OUT_IDENTITY, capi.LIK_GAUSS, p["n_out"])
    if p["mask"] is not None:
        ctx.set_layer_mask(p["mask"])
    return ctx


def run_batch(ctx, p, b, d, schedule):
    w, acc, llp, lpp, res = ctx.chain_run(b["start"]["w"], n_candidates=d, schedule=schedule, **rc.chain_kwargs(p, b))
    return dict(w=w, acc=acc.copy(), llp=llp, lpp=lpp, ll=res["loglik"], lp=res["logprior"],
                sigma=np.array(res["sigma"]) if p["lik"] == "gauss" else None, res=res)


def ran_as_named(ctx, got, name, d, schedule, path, what):
    """The launch carried the candidates and ran on the schedule the run names (range_cases.effective_schedule: what
    npbnn_sched_choose, npbnn_sched_plan.h, makes of the number).  The two-stream schedule 3 is the one form whose device-side waits may time out by
    design; the wrapper then repeats the batch on schedule 2, counts it in ``sync_fallbacks``, and that is what must be seen."""
    assert got["res"]["n_candidates"] == d, (what, "the launch did not carry the candidates the run names", got["res"]["n_candidates"])
    want = rc.effective_schedule(name, d, schedule, path)
    if schedule == 3 and ctx.sync_fallbacks:
        want = 2
    assert got["res"]["schedule"] == want, (what, "the batch did not run on the schedule the run names", got["res"]["schedule"], want)


def hold_to_float64(got, want, what):
    """The bars of test_hip_chain_oracle on one batch's outputs; no iteration is excused."""
    assert np.array_equal(got["acc"], want["acc"]), (what, "accepted flags", np.flatnonzero(got["acc"] != want["acc"]))
    err = np.abs(got["llp"] - want["llp"]) / np.abs(want["llp"])
    assert np.all(err <= LL_RTOL), (what, "proposed logLik", int(np.argmax(err)), float(np.max(err)))
    perr = np.abs(got["lpp"] - want["lpp"]) / np.maximum(1.0, np.abs(want["lpp"]))
    assert np.all(perr <= LP_RTOL), (what, "proposed logPrior", int(np.argmax(perr)), float(np.max(perr)))
    assert got["w"].tobytes() == np.asarray(want["w"], dtype=np.float64).tobytes(), (what, "weights")
    assert abs(got["ll"] - want["ll"]) <= LL_RTOL * abs(want["ll"]), (what, "logLik", got["ll"], want["ll"])
    assert abs(got["lp"] - want["lp"]) <= LP_RTOL * max(1.0, abs(want["lp"])), (what, "logPrior", got["lp"], want["lp"])
    if want.get("sigma") is not None:
        ws = np.asarray(want["sigma"], dtype=float)
        assert np.all(np.abs(got["sigma"] - ws) <= LP_RTOL * np.maximum(1.0, np.abs(ws))), (what, "sigma", got["sigma"], ws)
    return float(np.max(err))


def same_bytes(a, b, what):
    for key in ("acc", "llp", "lpp", "w"):
        assert a[key].tobytes() == b[key].tobytes(), (what, key)
    assert a["ll"] == b["ll"] and a["lp"] == b["lp"], (what, "result", a["ll"], b["ll"], a["lp"], b["lp"])
    if a["sigma"] is not None:
        assert a["sigma"].tobytes() == b["sigma"].tobytes(), (what, "sigma")


def _run_id(r):
    return "%s-d%d-s%d-%s" % r


# ---- 1: HipContext.chain_run ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", rc.direct_runs(), ids=_run_id)
def test_direct_entry_through_the_repeat(run, bn, monkeypatch):
    """Clean batch, planted batch, two clean batches on one context, 1 to 3 candidates: on the resident path on schedules 1, 2,
    4, 5 - each at every position of t*, schedule 5 with one or three candidates, for which there are builds with the speculative
    step - and once 3; on the weight-streamed path, which runs on kernel boundaries whatever is asked, on schedule 1.  Every
    batch, the float32 repeat included, reports the candidates and the schedule the run names (``ran_as_named``).  All four
    batches are the stand-in's; the planted batch - and, when its proposal was accepted, every batch after
    it, which starts with a weight already out of range - ran on float32 and is the ``f32`` context's byte for byte; after a
    rejected plant the next clean batch is back on the fp16 pair and is a fresh context's byte for byte."""
    name, d, schedule, path = run
    if path == "streamed":
        monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    sc = rc.scenario(name)
    p, accepted = sc["p"], sc["variant"]["accept"]
    main, f32c = make_ctx(bn, p), make_ctx(bn, p, "f32")
    assert main.is_wide() == f32c.is_wide() == (path == "streamed")
    modes, outs = [], []
    for j, b in enumerate(sc["batches"]):
        what = (name, "batch %d" % j)
        got = run_batch(main, p, b, d, schedule)
        modes.append(main.l0_mode())
        ran_as_named(main, got, name, d, schedule, path, what)
        hold_to_float64(got, b["want"], what)
        ref = run_batch(f32c, p, b, d, schedule)
        assert f32c.l0_mode() == "f32"
        ran_as_named(f32c, ref, name, d, schedule, path, what + ("f32 context",))
        hold_to_float64(ref, b["want"], what + ("f32 context",))
        if modes[-1] == "f32":
            same_bytes(got, ref, what + ("against the f32 context",))
        outs.append(got)
    assert modes == (["f16-split", "f32", "f32", "f32"] if accepted else ["f16-split", "f32", "f16-split", "f16-split"]), modes
    if not accepted:       # nothing of the abandoned attempt or of the float32 repeat is left in the context
        fresh = make_ctx(bn, p)
        got = run_batch(fresh, p, sc["batches"][2], d, schedule)
        assert fresh.l0_mode() == "f16-split"
        same_bytes(outs[2], got, (name, "the clean batch after the planted one against a fresh context"))
        fresh.close()
    main.close()
    f32c.close()


@pytest.mark.parametrize("path", ["resident", "streamed"])
@pytest.mark.parametrize("name,d,schedule", [("mid_rejected", 3, 2), ("slot1_rejected", 3, 4), ("last_rejected", 1, 5), ("first_rejected", 2, 1),
                                             ("gauss_rejected", 3, 1), ("masked_rejected", 2, 2)])
def test_fp16_asked_for_by_name_raises_and_leaves_nothing_behind(name, d, schedule, path, bn, monkeypatch):
    """``set_l0_precision("f16")``: the planted batch raises NPBNN_E_RANGE (no float32 repeat was asked for); the abandoned batch
    had committed the entries accepted before the flag to the device's weight image, moved its current weights and its state -
    the next clean batch on that context is a fresh context's byte for byte, and float64's."""
    from npbnn_amd import _capi as capi
    if path == "streamed":
        monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    sc = rc.scenario(name)
    p = sc["p"]
    clean0, planted, clean1, _ = sc["batches"]
    ctx, fresh = make_ctx(bn, p, "f16"), make_ctx(bn, p)
    got = run_batch(ctx, p, clean0, d, schedule)
    ran_as_named(ctx, got, name, d, schedule, path, (name, "clean"))
    hold_to_float64(got, clean0["want"], (name, "clean"))
    assert ctx.l0_mode() == "f16-split" and ctx.l0_option() == "f16"
    with pytest.raises(capi.NpbnnError) as e:
        run_batch(ctx, p, planted, d, schedule)
    assert e.value.code == capi.E_RANGE
    assert ctx.l0_mode() == "f16-split"
    got = run_batch(ctx, p, clean1, d, schedule)
    hold_to_float64(got, clean1["want"], (name, "clean batch after the refused one"))
    same_bytes(got, run_batch(fresh, p, clean1, d, schedule), (name, "after the refused batch against a fresh context"))
    assert ctx.l0_mode() == fresh.l0_mode() == "f16-split"
    ctx.close()
    fresh.close()


def _fp16_threshold(ctx, p, plant):
    """The least |value| of weight ``plant`` at which an evaluation leaves the fp16 pair, by bisection."""
    def leaves(v):
        w = rc.pack(p["w"])
        w[plant] = v
        ctx.eval(rc.unpack(w, p["shapes"]))
        return ctx.l0_mode() == "f32"
    lo, hi = 1.0, 1e6
    assert not leaves(lo) and leaves(hi)
    while hi - lo > 1e-6 * hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if leaves(mid) else (mid, hi)
    return hi


@pytest.mark.parametrize("d,schedule", [(1, 1), (3, 1), (3, 2), (3, 4), (3, 5)])
def test_candidate_out_of_range_only_while_dropped(d, schedule, bn):
    """range_cases.dropped_only_batch: the float64 chain never proposes a weight outside the range; with three candidates per
    pass the step prepares one that is (slot 1, beside an accepted slot 0, from the state before it) and drops it.  The flag is
    raised when a candidate is prepared, so that batch is repeated on float32 on schedules 1, 2, 4 and 5 alike;
    it is the stand-in's, and so is the clean batch after it, back on the fp16 pair.  One candidate per pass prepares no such
    candidate and stays on the fp16 pair."""
    p = rc.make_problem("cat", 300, (16, 5), 33)
    plant = rc.plant_index(p, np.random.default_rng(2))
    ctx = make_ctx(bn, p)
    threshold = _fp16_threshold(ctx, p, plant)
    b = rc.dropped_only_batch(p, plant, threshold)
    assert np.max(np.abs(b["watch_prop"])) < 0.6 * threshold
    got = run_batch(ctx, p, b, d, schedule)
    mode = ctx.l0_mode()
    assert got["res"]["n_candidates"] == d and got["res"]["schedule"] == schedule
    hold_to_float64(got, b["want"], ("dropped only", d, schedule))
    assert mode == ("f16-split" if d == 1 else "f32")
    after = rc.build_batches(p, 5, [(20, None, None, False, 0, None)],
                             state=dict(w=rc.unpack(b["want"]["w"], p["shapes"]), ll=b["want"]["ll"], lp=b["want"]["lp"], sigma=None))[0]
    hold_to_float64(run_batch(ctx, p, after, d, schedule), after["want"], ("after dropped only", d, schedule))
    assert ctx.l0_mode() == "f16-split"
    ctx.close()


# ---- 3: npbnn_chain_run_general ---------------------------------------------------------------------------------------------------

def run_general(ctx, p, b):
    w, ind, _, acc, llp, lpp, res = ctx.chain_run_general(b["start"]["w"], **rc.general_kwargs(p, b))
    return dict(w=w, ind=ind, acc=acc.copy(), llp=llp, lpp=lpp, ll=res["loglik"], lp=res["logprior"], sigma=None, res=res)


@pytest.mark.parametrize("path", ["resident", "streamed"])
@pytest.mark.parametrize("name", list(rc.GENERAL))
def test_general_chain_through_the_repeat(name, path, bn, monkeypatch):
    """The fixed-normal proposal, and UpdateNormal with weight indicators on four matrices (the plant on a weight whose
    indicator is 1): the C call repeats the planted batch by itself; float64's bars, the indicators exactly, the ``f32``
    context's bytes where float32 ran."""
    if path == "streamed":
        monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    sc = rc.general_scenario(name)
    p, accepted = sc["p"], sc["variant"]["accept"]
    main, f32c = make_ctx(bn, p), make_ctx(bn, p, "f32")
    assert main.is_wide() == f32c.is_wide() == (path == "streamed")
    modes = []
    for j, b in enumerate(sc["batches"]):
        what = (name, "batch %d" % j)
        got, ref = run_general(main, p, b), run_general(f32c, p, b)
        modes.append(main.l0_mode())
        assert f32c.l0_mode() == "f32"
        for out in (got, ref):
            hold_to_float64(out, b["want"], what)
            if b["want"]["ind"] is not None:
                assert np.array_equal(out["ind"], b["want"]["ind"]), (what, "indicators")
        if modes[-1] == "f32":
            same_bytes(got, ref, what + ("against the f32 context",))
            if got["ind"] is not None:
                assert got["ind"].tobytes() == ref["ind"].tobytes()
    assert modes == (["f16-split", "f32", "f32"] if accepted else ["f16-split", "f32", "f16-split"]), modes
    if not accepted:
        fresh = make_ctx(bn, p)
        same_bytes(got, run_general(fresh, p, sc["batches"][2]), (name, "the clean batch after the planted one against a fresh context"))
        fresh.close()
    main.close()
    f32c.close()


# ---- 4: npbnn_chains_run_batched --------------------------------------------------------------------------------------------------

def _group_jobs(ctxs, p, batches):
    jobs = []
    for ctx, b in zip(ctxs, batches):
        kw = rc.chain_kwargs(p, b)
        draws = {k: kw.pop(k) for k in ("idx", "delta", "cnt", "log_u", "mask")}
        jobs.append(dict(ctx=ctx, weights=b["start"]["w"], cfg=dict(kw, n_candidates=1, schedule=0), **draws))
    return jobs


def _group_contexts(bn, p, l0):
    owner = make_ctx(bn, p, l0)
    return [owner] + [make_ctx(bn, p, l0, share=owner) for _ in range(2)]


@pytest.mark.parametrize("lik", ["cat", "gauss"])
def test_group_pass_through_the_repeat(lik, bn):
    """Three chains of one model, the plant in chain 1 only: the whole group is refused and built again with force_f32 - all
    three are the stand-in's chains and the ``f32`` contexts' byte for byte; the next, clean group is back on the fp16 pair."""
    from npbnn_amd import backend
    p = rc.make_problem(lik, 641, (16, 5), 61)
    plant = rc.plant_index(p, np.random.default_rng(3))
    K = 30
    chains = [rc.build_batches(p, 70 + q, [(K, 15 if q == 1 else None, plant if q == 1 else None, False, 0, "mid"), (20, None, None, False, 0, None)])
              for q in range(3)]
    auto, f32c = _group_contexts(bn, p, "auto"), _group_contexts(bn, p, "f32")
    for j, (k, mode) in enumerate(((K, "f32"), (20, "f16-split"))):
        outs = backend.chains_run_batched(_group_jobs(auto, p, [c[j] for c in chains]), k)
        refs = backend.chains_run_batched(_group_jobs(f32c, p, [c[j] for c in chains]), k)
        for q in range(3):
            assert auto[q].l0_mode() == mode, (j, q)
            assert f32c[q].l0_mode() == "f32"
            got, ref = (dict(w=o["w"], acc=o["accepted"], llp=o["loglik_prop"], lpp=o["logprior_prop"], ll=o["result"]["loglik"],
                             lp=o["result"]["logprior"], sigma=np.array(o["result"]["sigma"]) if lik == "gauss" else None)
                        for o in (outs[q], refs[q]))
            hold_to_float64(got, chains[q][j]["want"], (lik, "group", j, "chain", q))
            hold_to_float64(ref, chains[q][j]["want"], (lik, "group", j, "chain", q, "f32 contexts"))
            if mode == "f32":
                same_bytes(got, ref, (lik, "group", j, "chain", q))
    for c in auto[::-1] + f32c[::-1]:
        c.close()


# ---- 5: npbnn_chains_run_exchange ---------------------------------------------------------------------------------------------------

class _NoSwaps:
    """Swap proposals between chain 0 and itself (test_hip_exchange._NoSwaps): the temperatures stay where they are, so that
    every chain's batch can be walked in float64 ahead of the run."""

    def get(self, first, n=1):
        return np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n)

    def release(self, upto):
        pass


def _state_of(chains):
    return [dict(w=[w.copy() for w in bnn._w_layers], ll=m._logLik, lp=m._logPrior, post=m._logPost, temp=m._temperature,
                 it=m._current_iteration, rate=m._acceptance_rate, mem=list(m._last_accepted_mem), err=np.array(bnn._error_prm))
            for bnn, m in chains]


def test_exchange_run_stops_before_the_planted_proposal_and_the_driver_finishes(bn, monkeypatch):
    """Two chains (temperatures 0.85 and 1), 4 intervals of 20, the plant in interval 1 of the cold chain; the chains take the
    planted draws where they would draw (range_cases.serve_draws).  The exchange run comes back after one interval with
    ``overflow`` set for the cold chain only, which stands before the pass that holds the planted proposal; the driver finishes
    interval 1 through run_steps (which repeats on float32) and the rest on the device again: the end state is the
    interval-by-interval path's, the flags and weights are the stand-in's, the state is float64's."""
    from npbnn_amd import exchange as ex
    from npbnn_amd.hip_backend import HipBackend
    from test_hip_chain_oracle import _exchange_chains, check_state, make_data
    from test_hip_exchange import assert_same
    monkeypatch.setenv("NPBNN_NO_FAST_DISPATCH", "1")       # (the kept dispatch draws for itself)
    temps, n_seg, seg_len, t_star = [0.85, 1.0], 4, 20, 27
    K = n_seg * seg_len
    dat = make_data("cat", 641, rc.N_FEATURES, seed=12)
    plans = []

    def build():
        chains = _exchange_chains(bn, "cat", dat, temps)
        for i, (bnn, m) in enumerate(chains):
            assert bnn._prior_kind() == rc.PRIOR_NORMAL and bnn._w_bound == np.inf and bnn._mask is None
            if len(plans) < len(chains):
                p = rc.problem_of(bnn)
                plant = rc.plant_index(p, np.random.default_rng(5))
                plans.append((p, rc.build_batches(p, 80 + i, [(K, t_star if i == 1 else None, plant if i == 1 else None, False, 0, "mid")],
                                                  temperature=temps[i])[0]))
            rc.serve_draws(m, plans[i][1])
        return chains
    ids = [0, 1]
    slack = HipBackend.exchange_slack
    try:
        a = build()
        assert ex.advance_intervals(a, ids, 2, n_seg, seg_len, _NoSwaps(), 0, device=False) == n_seg
        # the exchange run by itself: it stops inside interval 1
        b = build()
        done, records, outs = ex.run_exchange(b, ids, 2, n_seg, seg_len, _NoSwaps(), 0)
        assert done == 1
        assert [int(o["result"]["overflow"]) for o in outs] == [0, 1]
        for bnn, m in b:
            assert seg_len <= m._current_iteration <= 2 * seg_len
        d = int(outs[1]["result"]["n_candidates"])
        # (the exchange run is on the overlapped schedule: the step that prepares - and flags - the pass of the planted proposal
        # runs while the pass before it is still being evaluated, and nothing is decided after the flag)
        assert t_star - 2 * d < b[1][1]._current_iteration <= t_star, "the cold chain did not stop at the planted proposal"
        for (bnn, m), (p, plan) in zip(b, plans):
            k = m._current_iteration
            assert m._last_accepted_mem[-k:] == [int(x) for x in plan["want"]["acc"][:k]]
            check_state("cat", bnn, m, accuracy=False)
        # the driver: interval 0 on the device, interval 1 finished the slow way, intervals 2 and 3 on the device
        c = build()
        on_device = []
        assert ex.advance_intervals(c, ids, 2, n_seg, seg_len, _NoSwaps(), 0, batch=n_seg,
                                    on_interval=lambda s, info: on_device.append(info["cold"] is not None)) == n_seg
        assert on_device == [True, False, True, True]
    finally:
        HipBackend.exchange_slack = slack
    assert_same(_state_of(a), _state_of(c), exact=False)
    for chains in (a, c):
        for (bnn, m), (p, plan) in zip(chains, plans):
            assert m._current_iteration == K and m._device_iterations == K
            assert m._last_accepted_mem[-K:] == [int(x) for x in plan["want"]["acc"]]
            assert rc.pack(bnn._w_layers).tobytes() == plan["want"]["w"].tobytes()
            check_state("cat", bnn, m)
            assert m._backend.ctx.l0_mode() == "f16-split"          # (the planted proposal was rejected: back on the fp16 pair)


# ---- 2: FastBatch.run hands the batch back to the sampler ---------------------------------------------------------------------------

def test_sampler_walks_across_the_threshold(bn, monkeypatch):
    """MCMC.run_steps against the mh_step loop and the float64 stand-in on a table with an unstandardised column (times 2^12: the
    fp16 threshold T of its weights is a few units, found here by bisection on eval + l0_mode).  One such weight starts at
    0.98 T and layer 0 steps widely: candidates cross T again and again (range_cases / test_host_chain_f16_range: the first
    time in the third dispatch).  The kept dispatch is built after two equal calls, fails with NPBNN_E_RANGE in the third - its
    draws go to the general path as draws made ahead - and is built again 16 calls later; the chain is the mh_step loop's,
    the stand-in's over the first 150 decisions, float64's after every dispatch, and the random streams end where the mh_step
    loop leaves them."""
    from npbnn_amd import _capi as capi, backend
    from test_hip_chain_oracle import assert_trajectory, check_state, oracle_twin
    dat = rc.sampler_data()
    probe_bnn, probe = rc.sampler_chain(bn, dat, 1.0)
    ctx = probe._backend.ctx

    def leaves_fp16(v):
        ctx.eval(rc.sampler_weights(bn, v))
        return ctx.l0_mode() == "f32"
    lo, hi = 1.0, 16.0
    assert not leaves_fp16(lo) and leaves_fp16(hi)
    while hi - lo > 1e-4:
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if leaves_fp16(mid) else (mid, hi)
    threshold = min(rc.SAMPLER_THRESHOLDS, key=lambda t: abs(t - hi))
    assert abs(hi - threshold) <= 2e-4, ("the threshold is none of those the CPU test covers", hi)
    ctx.close()

    codes = []
    real_run = backend.FastBatch.run

    def spy(self, *a, **k):
        codes.append(real_run(self, *a, **k))
        return codes[-1]
    monkeypatch.setattr(backend.FastBatch, "run", spy)
    (ba, ma), (bb, mb) = rc.sampler_chain(bn, dat, threshold), rc.sampler_chain(bn, dat, threshold)
    n = sum(rc.SAMPLER_DISPATCHES)
    np.random.seed(77)
    for _ in range(n):
        ma.mh_step(ba)
    numpy_a, gen_a = np.random.get_state()[1].copy(), ma._rs.bit_generator.state
    np.random.seed(77)
    flags, modes = [], []
    for k in rc.SAMPLER_DISPATCHES:
        mb.run_steps(bb, k)
        modes.append(mb._backend.ctx.l0_mode())
        flags += list(mb._last_accepted_mem[-k:])
        with np.errstate(over="ignore"):        # (the oracle's tanh of the scaled column's pre-activations)
            check_state("cat", bb, mb)
    assert mb._current_iteration == n and mb._device_iterations == n
    assert mb._rs.bit_generator.state == gen_a
    np.testing.assert_array_equal(np.random.get_state()[1], numpy_a)
    # the path: the kept dispatch ran, failed on the range, and a rebuilt one ran again; batches were repeated on float32
    assert capi.E_RANGE in codes, codes
    assert len(codes) > codes.index(capi.E_RANGE) + 1, ("no kept dispatch was built again after the failed one", codes)
    assert "f32" in modes and "f16-split" in modes, modes
    with np.errstate(over="ignore"):
        br, mr = oracle_twin("cat", lambda: rc.sampler_chain(bn, dat, threshold))
        ref = []
        for k in rc.SAMPLER_DISPATCHES:
            mr.run_steps(br, k)
            ref += list(mr._last_accepted_mem[-k:])
    assert_trajectory(flags, ref)
    assert ma._last_accepted_mem == mb._last_accepted_mem and sum(flags) >= 2
    for wa, wb in zip(ba._w_layers, bb._w_layers):
        np.testing.assert_array_equal(wa, wb)


# ---- 6: the row-sharded chain -------------------------------------------------------------------------------------------------------

def test_row_sharded_chain_through_the_repeat():
    """rowshard_cases.RANGE_CASE (``rank_worker.py rowshard_range``): two ranks on GPU 0, the records over the TCP communicator,
    the planted draws served to both.  Each rank asserts that its planted dispatch ran on float32 and the ones around it on the
    fp16 pair, that its flags and weights are the stand-in's and its state float64's on all rows, and that the ranks agree."""
    import os
    import sys
    from npbnn_amd.launch import spawn_ranks
    import rowshard_cases
    worker = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "rank_worker.py")]
    world = rowshard_cases.RANGE_CASE["world"]
    status, out0, outs = spawn_ranks(worker + ["rowshard_range", "hip", "socket"], world, env=dict(os.environ), capture_all=True, timeout=300)
    assert status == 0, "\n".join(outs)
    assert all("RANK %d OK" % r in outs[r] for r in range(world)), "\n".join(outs)
