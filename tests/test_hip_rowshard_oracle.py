"""GPU: the row-sharded chain (npbnn_set_row_shard, MCMC(row_comm=...), npbnn_amd/rowshard.py) held to float64 on ALL rows.

The sharded chain was compared only with the same chain on all rows on the same kernels (rank_worker.py rowshard: four cases,
two ranks, one shape).  Here every case of tests/rowshard_cases.py - shares under a 16-row tile and either side of a tile
boundary, 2 to 5 ranks, all 33 values of the per-pass record, empirical and proposed sigma, class weights, an MTI 8 layer, every
float64 row-wise likelihood, trainable slopes, the streamed path fused and K-sliced - runs in short dispatches, and after every
dispatch each rank recomputes in float64, from its own weights and ALL rows, what the chain says it holds
(``rank_worker.py rowshard64``; the bars are test_hip_chain_oracle's: 2e-6, 1e-12, 1e-4, 150 common decisions with the float64
twin).  tests/test_host_rowshard.py rehearses the same cases on CPU.

  a. the host-callback route: the ranks of a case share GPU 0, the records travel over the TCP communicator;
  b. a world of one, in process: shard_sum_kernel and shard_spread_kernel with n_blocks below, at and above the 64-lane stride,
     against float64 and bit for bit against the unsharded chain on kernel boundaries;
  c. the RCCL route, where there are two or more GPUs."""
import os
import sys

import numpy as np
import pytest

import rowshard_cases as rc
import test_hip_chain_oracle as tco
from npbnn_amd.launch import spawn_ranks
from test_hip_chain_oracle import bn  # noqa: F401  (fixture)
from test_hip_multirank import needs_two, n_gpus, rank_counts  # noqa: F401  (n_gpus: the skip condition's name)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = [sys.executable, os.path.join(HERE, "rank_worker.py")]


def _run(names, world, env, comm):
    status, out0, outs = spawn_ranks(WORKER + ["rowshard64", "hip", comm, ",".join(names)], world, env=dict(os.environ, **env),
                                     capture_all=True, timeout=300)
    print(out0)                    # (the worst relative logLik error per case, with -s)
    assert status == 0, "\n".join(outs)
    assert all("RANK %d OK" % r in outs[r] for r in range(world)), "\n".join(outs)
    for n in names:
        assert " %s " % n in out0, "case %s did not report" % n


# ---- a. one GPU, the records through the host ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", rc.groups(), ids=rc.group_id)
def test_sharded_chain_against_float64_on_all_rows(group):
    """One spawn per (environment, world) of the table - two where the table has more than rowshard_cases.GROUP_MOST such cases -
    every rank on GPU 0 (at most five, six processes with this one)."""
    env, world, names = group
    assert world <= 5
    _run(names, world, env, "socket")


# ---- b. a world of one ----------------------------------------------------------------------------------------------------------------

class _Alone:
    rank, world_size = 0, 1

    def allgather_f64(self, v):
        return [np.asarray(v, dtype=np.float64)]


def _stride_rows(bn, lik, k):
    """Rows of 64 x INFO_WAVES_PER_BLOCK x n_cu: one workgroup's worth less and more put the count of per-wave records either
    side of the point where every compute unit holds a workgroup."""
    _, pm = tco.make_chain(bn, lik, tco.make_data(lik, 4096, 16, seed=8, k=k), (20, 5))
    wg = 64 * tco._info(pm, "INFO_WAVES_PER_BLOCK")
    n_cu = tco._info(pm, "INFO_N_CU")
    pm._backend.ctx.close()
    return wg, wg * n_cu


@pytest.mark.parametrize("n_rows", [5, 1025, 70001, "stride-wg", "stride+wg"])
@pytest.mark.parametrize("lik,k", [("cat", 0), ("gauss", 16)], ids=["cat", "gauss16"])
def test_world_of_one_against_float64_and_the_unsharded_chain(n_rows, lik, k, bn):
    """A communicator of one rank sends the chain through shard_sum_kernel and shard_spread_kernel with n_blocks = the pass's own
    record count: 1, a few, and below / above the 64-lane stride of the sum.  After every dispatch the state is float64's; and
    because shard_sum_kernel adds the records in the step kernel's own order, the chain is bit for bit the unsharded chain on
    kernel boundaries (device_schedule 1): the same decisions, weights and - from the first accepted proposal on, when the
    device's own sum has replaced the constructor's - log-likelihoods."""
    if isinstance(n_rows, str):
        wg, stride = _stride_rows(bn, lik, k)
        n_rows = stride - wg if n_rows == "stride-wg" else stride + wg
    dat = tco.make_data(lik, n_rows, 16, seed=8, k=max(k, 1))
    sizes = tco.dispatch_sizes(rc.N_ITER)

    def run(**kw):
        bnn, mcmc = tco.make_chain(bn, lik, dat, (20, 5), **kw)
        mcmc.n_candidates, mcmc.device_schedule, mcmc.SUB_BATCH = 3, 1, 16
        errs = [tco.check_state_on(lik, bnn, mcmc, dat["data"], dat["labels"], dat["test_data"], dat["test_labels"], min_abs=0.1 * n_rows)]
        trail, decisions = [], []
        for j, n in enumerate(sizes):
            mcmc.run_steps(bnn, n)
            decisions += list(mcmc._last_accepted_mem[-n:])
            tco.check_state_on(lik, bnn, mcmc, dat["data"], dat["labels"], dat["test_data"], dat["test_labels"], worst=errs,
                               accuracy=(j % 2 == 1), min_abs=0.1 * n_rows)
            trail.append((sum(decisions) > 0, float(mcmc._logLik)))
        assert mcmc._device_iterations == rc.N_ITER and mcmc._device_schedule_used == 1 and mcmc._device_passes < rc.N_ITER
        w = np.concatenate([x.ravel() for x in bnn._w_layers])
        mcmc._backend.ctx.close()
        return decisions, trail, w, max(errs)
    dec_s, trail_s, w_s, err_s = run(row_comm=_Alone())
    dec_u, trail_u, w_u, err_u = run()
    print("\n[rowshard64] world-of-one %s rows %d  worst logLik rel err %.3e (unsharded %.3e)" % (lik, n_rows, err_s, err_u))
    assert sum(dec_s) >= 5
    assert dec_s == dec_u, "the sharded chain of one rank took other decisions"
    assert np.array_equal(w_s, w_u)
    assert any(m for m, _ in trail_s)
    assert [ll for m, ll in trail_s if m] == [ll for m, ll in trail_u if m], "shard_sum_kernel does not add in the step kernel's order"


# ---- c. RCCL ----------------------------------------------------------------------------------------------------------------------------

@needs_two
@pytest.mark.parametrize("name", ["g16_d3", "nb2d", "wcat_d3", "cat1300"])
def test_sharded_chain_over_rccl_against_float64(name):
    """One GPU per rank, the records all-gathered by RCCL on the chains' streams: all 33 values at three candidates, a float64
    row-wise build, the streamed path forced and by itself."""
    for world in rank_counts():
        _run([name], world, rc.CASES[name]["env"], "rccl")
