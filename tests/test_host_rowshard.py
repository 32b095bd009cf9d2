"""One chain, rows split over ranks (npbnn_amd/rowshard.py), on CPU: two and three torch-free ranks over the TCP communicator, the
device stood in for by the oracle - the sharded chain takes the decisions of the same chain on all rows (SURVEY 8(e) alternative;
reference shape np_bnn/BNN_env.py:467-491: one sum over all rows per proposal).  Every case of rowshard_cases.CASES runs here too
(``rowshard64``): the float64 stand-in on shares of the rows against float64 on all rows, to 1e-10 - the rehearsal of the harness
and of rowshard.py's host sums that tests/test_hip_rowshard_oracle.py then runs on the kernels."""
import os
import sys

import numpy as np
import pytest

import rowshard_cases as rc
from npbnn_amd.launch import spawn_ranks
from npbnn_amd.rowshard import shard_bounds, shard_rows

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = [sys.executable, os.path.join(HERE, "rank_worker.py")]


def test_shares_are_contiguous_and_cover_every_row():
    for n, world in ((10, 3), (7, 7), (100000, 8), (5, 2)):
        b = [shard_bounds(n, r, world) for r in range(world)]
        assert b[0][0] == 0 and b[-1][1] == n
        assert all(b[i][1] == b[i + 1][0] for i in range(world - 1))
        sizes = [hi - lo for lo, hi in b]
        assert max(sizes) - min(sizes) <= 1


def test_shard_rows_cuts_every_per_row_array_and_nothing_else():
    dat = dict(data=np.arange(22.).reshape(11, 2), labels=np.arange(11), test_data=np.zeros((4, 2)), test_labels=np.arange(4),
               id_data=np.arange(11).astype(str), feature_names=["a", "b"], file_name="x")
    parts = [shard_rows(dat, r, 3) for r in range(3)]
    np.testing.assert_array_equal(np.concatenate([p["data"] for p in parts]), dat["data"])
    np.testing.assert_array_equal(np.concatenate([p["labels"] for p in parts]), dat["labels"])
    np.testing.assert_array_equal(np.concatenate([p["test_labels"] for p in parts]), dat["test_labels"])
    np.testing.assert_array_equal(np.concatenate([p["id_data"] for p in parts]), dat["id_data"])
    assert parts[1]["feature_names"] == ["a", "b"] and parts[2]["file_name"] == "x"
    assert len(dat["data"]) == 11          # (the caller's dictionary is untouched)


@pytest.mark.parametrize("case,world", [("cls", 2), ("clsw", 3), ("reg", 2), ("regsig", 2)])
def test_a_row_sharded_chain_is_the_chain_on_all_rows(case, world):
    status, out0, outs = spawn_ranks(WORKER + ["rowshard", "oracle", "socket", case], world, capture_all=True, timeout=600)
    assert status == 0, "\n".join(outs)
    assert all("RANK %d OK" % r in outs[r] for r in range(world))


@pytest.mark.parametrize("group", rc.groups(), ids=rc.group_id)
def test_every_sharded_case_against_float64_on_all_rows(group):
    """(The accuracies of the row-wise likelihoods are left out here: their callables run on the device.)"""
    env, world, names = group
    status, out0, outs = spawn_ranks(WORKER + ["rowshard64", "oracle", "socket", ",".join(names)], world, capture_all=True, timeout=600)
    assert status == 0, "\n".join(outs)
    assert all("RANK %d OK" % r in outs[r] for r in range(world))
    for n in names:
        assert " %s " % n in out0, "case %s did not report" % n
    print(out0)


def test_the_table_holds_what_it_is_there_for():
    c = rc.CASES
    from npbnn_amd.rowshard import shard_bounds
    sizes = lambda n: sorted({hi - lo for lo, hi in (shard_bounds(c[n]["rows"], r, c[n]["world"]) for r in range(c[n]["world"]))})
    assert sizes("cat33_w2") == [16, 17] and sizes("cat33_w5") == [6, 7] and sizes("gauss7_w5") == [1, 2]
    assert {c[n]["d"] for n in ("g16_d1", "g16_d2", "g16_d3")} == {1, 2, 3} and all(c[n]["k"] == 16 for n in ("g16_d1", "g16_emp"))
    assert {c[n]["lik"] for n in c if c[n]["extra"]["family"] == "row-wise"} == {"pois", "nb", "nb10", "nb2d", "err"}
    assert {c[n]["l0"] for n in c} == {"auto", "f32", None} and max(v["world"] for v in c.values()) <= 5
    assert sorted(n for g in rc.groups() for n in g[2]) == sorted(c)


def test_squared_error_accuracies_of_a_sharded_chain_come_from_all_ranks(monkeypatch):
    """MCMC._statistic on a row-sharded backend: the package's squared-error statistics from the sums of every rank (here the
    device's sums are numpy's), any other callable - and every callable on an unsharded backend - from the local rows."""
    from types import SimpleNamespace
    from npbnn_amd import device_ops, likelihoods as lk
    from npbnn_amd.sampler import MCMC
    rs = np.random.default_rng(0)
    y, lab = rs.standard_normal((11, 3)), rs.standard_normal((11, 3))
    lo, hi = shard_bounds(11, 1, 3)

    def sums(kind, yy, ll):
        assert kind in ("mse", "label_mse")
        return np.concatenate([[float(len(yy))], ((yy - ll) ** 2).sum(axis=0)])
    monkeypatch.setattr(device_ops, "statistic_sums", sums)
    others = sum(sums("mse", y[a:b], lab[a:b]) for a, b in (shard_bounds(11, r, 3) for r in (0, 2)))
    sharded = SimpleNamespace(_backend=SimpleNamespace(row_sharded=True, sum_over_ranks=lambda v: v + others))
    got = MCMC._statistic(sharded, lk.CalcAccuracyRegression, y[lo:hi], lab[lo:hi])
    np.testing.assert_allclose(got, np.mean((y - lab) ** 2), rtol=1e-14)
    np.testing.assert_allclose(MCMC._statistic(sharded, lk.CalcLabelAccuracyRegression, y[lo:hi], lab[lo:hi]), np.mean((y - lab) ** 2, axis=0),
                               rtol=1e-14)
    mine = lambda yy, ll: float(len(yy))
    assert MCMC._statistic(sharded, mine, y[lo:hi], lab[lo:hi]) == hi - lo
    alone = SimpleNamespace(_backend=SimpleNamespace())
    assert MCMC._statistic(alone, mine, y, lab) == 11
    assert device_ops.statistic_of_sums("mse_exp_col0", np.array([4.0, 10.0])) == 2.5
