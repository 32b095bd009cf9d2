"""The row-sharded chain's cases against float64 (``rank_worker.py rowshard64``), shared by the CPU rehearsal
(test_host_rowshard.py: oracle stand-in over the TCP communicator) and the GPU tests (test_hip_rowshard_oracle.py).

``CASES``: name -> dict(lik, rows, features, widths, k, world, d, l0, env, extra)

  lik, rows, features, k    what test_hip_chain_oracle.make_data builds (k: target columns of a Gaussian)
  widths                    the hidden layers
  world                     ranks the rows are split over (shard_bounds: shares that differ by at most one row)
  d                         MCMC.n_candidates (0: the library's choice)
  l0                        NPBNN_L0 of the case ("auto" / "f32", alternating over the table; None: the streamed path, which has
                            no fp16-split first layer to report)
  env                       environment switches the library reads once per process: they go to spawn_ranks(env=...), and cases
                            of one (env, world) share a spawn (``groups``)
  extra                     family, n_test, model (npBNN arguments), mcmc (MCMC arguments), sigma ("empirical" / "estimated"),
                            slopes, wide

The shapes are the smallest at which the sharded code can go wrong: shares under one 16-row tile and either side of a tile
boundary, every one of the record's 33 values in use, every float64 row-wise likelihood, the streamed path fused and K-sliced."""
import numpy as np

from npbnn_amd.rowshard import shard_bounds

N_ITER = 120
N_CLASSES = 5

_WIDE = {"NPBNN_FORCE_WIDE": "1"}
_SLICES = {"NPBNN_WIDE_SLICES": "3"}
_FEW = dict(update_f=[0.001, 0.05, 0.05], update_ws=[0.03, 0.075, 0.075])


def _c(family, lik, rows, features, widths, world, k=0, d=0, env=None, n_test=25, **extra):
    return dict(lik=lik, rows=rows, features=features, widths=tuple(widths), k=k, world=world, d=d, l0=None, env=dict(env or {}),
                extra=dict(extra, family=family, n_test=n_test))


CASES = {
    # shares: 17 and 16 rows (two tiles and one), every share under a tile, shares of 2 and 1 rows, a few tiles at 2, 3 and 5 ranks
    "cat33_w2": _c("shares", "cat", 33, 6, (8, 5), 2),
    "cat33_w5": _c("shares", "cat", 33, 6, (8, 5), 5),
    "gauss7_w5": _c("shares", "gauss", 7, 6, (6, 4), 5, k=1, n_test=10),
    "cat403_w2": _c("shares", "cat", 403, 12, (8, 5), 2),
    "cat403_w3": _c("shares", "cat", 403, 12, (8, 5), 3),
    "cat403_w5": _c("shares", "cat", 403, 12, (8, 5), 5),
    # record: all 1 + 2 x 16 values at 1, 2 and 3 candidates; sigma from the totals over all rows; sigma proposals
    "g16_d1": _c("record", "gauss", 389, 10, (6, 4), 3, k=16, d=1),
    "g16_d2": _c("record", "gauss", 389, 10, (6, 4), 3, k=16, d=2),
    "g16_d3": _c("record", "gauss", 389, 10, (6, 4), 3, k=16, d=3),
    "g16_emp": _c("record", "gauss", 389, 10, (6, 4), 3, k=16, model=dict(empirical_error=True), sigma="empirical"),
    "g3_est": _c("record", "gauss", 389, 10, (6, 4), 2, k=3, mcmc=dict(estimate_error=True, n_iteration=200), sigma="estimated"),
    # builds: the general build with balanced class weights from all ranks' counts; two ragged layer-0 tiles with an MTI 8 layer
    "catw_w3": _c("builds", "cat", 403, 12, (8, 5), 3, model=dict(use_class_weights=1)),
    "cat29_w2": _c("builds", "cat", 403, 12, (29, 40), 2),
    # row-wise: the float64 builds
    "pois": _c("row-wise", "pois", 101, 16, (20, 6), 3),
    "nb": _c("row-wise", "nb", 101, 16, (20, 6), 3),
    "nb10": _c("row-wise", "nb10", 101, 16, (20, 6), 3),
    "nb2d": _c("row-wise", "nb2d", 101, 16, (20, 6), 3),
    "err": _c("row-wise", "err", 101, 16, (20, 6), 3),
    "nb2d_mti8": _c("row-wise", "nb2d", 101, 16, (20, 40), 3),
    # slopes: every iteration proposes new activation slopes; the batches must still run on the device
    "cat_slopes": _c("slopes", "cat", 403, 12, (8, 5), 2, slopes=(0.02, 0.02)),
    # streamed: the fused pass forced at 1, 2 and 3 candidates and on a Gaussian; by itself; K-sliced
    "wcat_d1": _c("streamed", "cat", 403, 32, (32, 8), 3, d=1, env=_WIDE, wide=True),
    "wcat_d2": _c("streamed", "cat", 403, 32, (32, 8), 3, d=2, env=_WIDE, wide=True),
    "wcat_d3": _c("streamed", "cat", 403, 32, (32, 8), 3, d=3, env=_WIDE, wide=True),
    "wg4": _c("streamed", "gauss", 403, 32, (32, 8), 3, k=4, env=_WIDE, wide=True),
    # (a twentieth of 40 000 and of 300 000 first-layer weights per proposal is never accepted: a thousandth, smaller steps)
    "cat1300": _c("streamed", "cat", 600, 1300, (32, 8), 3, wide=True, mcmc=_FEW),
    "gsl3": _c("streamed", "gauss", 600, 1500, (200, 8), 2, k=2, env=_SLICES, wide=True, mcmc=_FEW),
}

# the planted fp16-range batch (tests/range_cases.py) on two ranks: every rank has to abandon and repeat the same batch
# (``rank_worker.py rowshard_range``; not one of CASES: its draws are planted, not the chain's own)
RANGE_CASE = _c("range", "cat", 403, 40, (16, 5), 2, d=3, n_test=0)
RANGE_CASE["l0"] = "auto"
RANGE_DISPATCHES = (20, 30, 20)          # clean, the planted one (t* = RANGE_T_STAR), clean
RANGE_T_STAR = 33

_resident = [n for n, c in CASES.items() if not c["extra"].get("wide")]
for _i, _n in enumerate(_resident):
    CASES[_n]["l0"] = "auto" if _i % 2 else "f32"


GROUP_MOST = 7          # cases per spawn: a group of the table's thirteen three-rank cases took twice the time of any other


def groups(names=None):
    """[(env, world, [case names])]: the cases that may share one spawn - one environment, one world, at most GROUP_MOST of
    them - in table order."""
    out = {}
    for n in (names or CASES):
        c = CASES[n]
        out.setdefault((tuple(sorted(c["env"].items())), c["world"]), []).append(n)
    res = []
    for (env, world), ns in out.items():
        n_parts = -(-len(ns) // GROUP_MOST)
        per = -(-len(ns) // n_parts)
        res += [(dict(env), world, ns[i:i + per]) for i in range(0, len(ns), per)]
    return res


def group_id(g):
    env, world, names = g
    return "_".join(["w%d" % world] + ["%s%s" % (k.replace("NPBNN_", "").lower(), v) for k, v in sorted(env.items())] + [names[0]])


def case_data(case, world=None):
    """The case's whole table.  A classification table is relabelled so that every share (of ``world`` ranks: the case's own unless
    given) starts with one row of every class (RowShardedBackend._agree_on_the_model refuses shares that miss one)."""
    world = world or case["world"]
    from test_hip_chain_oracle import make_data
    dat = make_data(case["lik"], case["rows"], case["features"], n_test=case["extra"]["n_test"], seed=5, k=max(case["k"], 1))
    if case["lik"] == "cat":
        lab = np.array(dat["labels"])
        for r in range(world):
            lo, hi = shard_bounds(case["rows"], r, world)
            assert hi - lo >= N_CLASSES
            lab[lo:lo + N_CLASSES] = np.arange(N_CLASSES)
        dat["labels"] = lab
    return dat
