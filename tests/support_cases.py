"""The confidence-threshold cases of tests/golden/support.npz (make_support_golden.py): inputs, keys, the cube of a summary and the
borderline rule the GPU tests hold the device's float32 forward pass to.

Inputs: a teacher network, the stored samples perturbations of it, the labels the teacher's calls with a share flipped - so that
confidence says something about correctness and the reference's sweep spans a useful range (``cases.posterior_inputs`` draws labels
and weights independently: accuracy at chance, no target reachable)."""
import os

import numpy as np

import cases

N_ROWS = 2000
N_FEATURES = 11
N_NODES = (6, 5)
N_PRIOR = 5
TOL = 2e-5                      # the project's bound on a class probability, float32 forward pass against float64 (test_hip_posterior.TOL)
GRID = np.linspace(0.01, 0.99, 99)
BF_GRID = np.array([1.0, 3.0, 20.0, 150.0])
# name -> activation, seed, bias mode, classes (one case with a class count that is not a multiple of 4)
INPUTS = {"tanh": dict(fun="tanh", seed=177, bias=2, n_classes=4), "genrelu": dict(fun="genReLU", seed=178, bias=2, n_classes=4),
          "swish_bias3": dict(fun="swish", seed=179, bias=3, n_classes=6)}
assert [c["name"] for c in cases.POSTERIOR_CASES] == list(INPUTS) and all(c["fun"] == INPUTS[c["name"]]["fun"] for c in cases.POSTERIOR_CASES)
CASES = [(name, s, mode) for name in INPUTS for s in (9, 10) for mode in (0, 1)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "support.npz")


def case_id(case):
    return "%s-S%d-m%d" % case


def key(name, n_samples, mode=None):
    return "%s/S%d" % (name, n_samples) + ("" if mode is None else "/m%d" % mode)


def inputs(name, n_samples=10, n_rows=N_ROWS):
    """x, the first ``n_samples`` of 10 stored samples, integer labels, prior samples.  The 9-sample case is the 10-sample case
    without its last sample."""
    spec = INPUTS[name]
    rs = np.random.default_rng(spec["seed"])
    x = rs.standard_normal((n_rows, N_FEATURES))
    shapes = cases.layer_shapes(N_FEATURES, list(N_NODES), spec["n_classes"], spec["bias"])
    teacher = [rs.normal(0, 0.9, s) for s in shapes]
    genrelu = spec["fun"] == "genReLU"
    samples = []
    for i in range(10):
        w = [t + rs.normal(0, 0.4, t.shape) for t in teacher]
        alphas = rs.uniform(0.0, 0.3, len(N_NODES)) if genrelu else np.zeros(1)
        samples.append(dict(weights=w, alphas=alphas, mcmc_it=100 * i))
    import oracle as orc                                  # (the float64 oracle's forward pass: the teacher's calls)
    labels = np.argmax(orc.forward(x, teacher, orc.Act(spec["fun"], np.full(len(N_NODES), 0.15)), orc.out_softmax), axis=1)
    flip = rs.random(n_rows) < 0.02
    labels = np.where(flip, (labels + rs.integers(1, spec["n_classes"], n_rows)) % spec["n_classes"], labels).astype(np.int64)
    prior = [dict(weights=[rs.normal(0, 0.6, s) for s in shapes], alphas=rs.uniform(0.0, 0.3, len(N_NODES)) if genrelu else np.zeros(1))
             for _ in range(N_PRIOR)]
    return dict(x=x, samples=samples[:n_samples], labels=labels, fun=spec["fun"], prior=prior, n_classes=spec["n_classes"],
                bias=spec["bias"])


def act_for(bn, fun):
    return bn.ActFun(fun=fun, prm=np.zeros(2)) if fun == "genReLU" else bn.ActFun(fun=fun)


def load():
    return np.load(GOLDEN)


# ---- what a summary implies ---------------------------------------------------------------------------------------------------
def cube_of(summary, labels, thresholds=GRID):
    """[bin, label, call] counts of a summary: bin = number of thresholds strictly below the row's largest value (plain numpy
    comparisons in float64, one threshold at a time - no search to share a mistake with the kernel's)."""
    call = np.argmax(summary, axis=1)
    p = summary[np.arange(len(call)), call]
    b = np.zeros(len(call), dtype=np.int64)
    for t in thresholds:
        b += p > t
    cube = np.zeros((len(thresholds) + 1, summary.shape[1], summary.shape[1]), dtype=np.int64)
    np.add.at(cube, (b, np.asarray(labels, dtype=np.int64), call), 1)
    return cube


def _cells(values, labels, row, thresholds):
    """The (bin, label, call) cell of one row's summary values."""
    call = int(np.argmax(values))
    return int(np.sum(values[call] > thresholds)), int(labels[row]), call


def candidate_cells(summary, labels, mode, n_samples, near_ties=None, thresholds=GRID, tol=TOL):
    """{row: set of cells} for the BORDERLINE rows of a float64 summary - the rows a forward pass within ``tol`` of float64 may
    count elsewhere; every other row must be counted in its own cell.
    mode 1: the row's largest value lies within ``tol`` of a threshold (either neighbouring bin) or of the second largest (either
    call).  mode 0: votes are integers, so only a sample whose two leading probabilities lie within ``tol`` of each other
    (``near_ties``: rows [row, sample, runner-up class]) can vote otherwise; each such sample's vote may go to its runner-up."""
    out = {}
    if mode == 1:
        top2 = np.sort(summary, axis=1)[:, -2:]
        p = top2[:, 1]
        near_thr = np.min(np.abs(p[:, None] - np.asarray(thresholds)[None, :]), axis=1) <= tol
        near_second = (p - top2[:, 0]) <= tol
        for r in np.where(near_thr | near_second)[0]:
            order = np.argsort(-summary[r], kind="stable")
            calls = [int(order[0])] + ([int(order[1])] if near_second[r] else [])
            cells = set()
            for c in calls:
                for v in (summary[r, c] - tol, summary[r, c], summary[r, c] + tol):
                    cells.add((int(np.sum(v > thresholds)), int(labels[r]), c))
            out[int(r)] = cells
        return out
    votes = np.rint(summary * n_samples).astype(np.int64)
    ties = {}
    for r, s, k2 in np.asarray(near_ties, dtype=np.int64).reshape(-1, 3):
        ties.setdefault(int(r), []).append((int(s), int(k2)))
    for r, lst in ties.items():
        cells = set()
        # each near-tied sample keeps its vote or gives it to its runner-up; its own vote is not stored, so every class holding a
        # vote is tried as the one that loses it
        options = [votes[r]]
        for _, k2 in lst:
            nxt = []
            for v in options:
                nxt.append(v)
                for k1 in np.where(v > 0)[0]:
                    if k1 != k2:
                        w = v.copy()
                        w[k1] -= 1
                        w[k2] += 1
                        nxt.append(w)
            options = nxt
        for v in options:
            cells.add(_cells(v / n_samples, labels, r, thresholds))
        out[r] = cells
    return out


def assert_cube_within_borderline(got, summary, labels, mode, n_samples, near_ties=None, thresholds=GRID, label=""):
    """Every cell of ``got`` lies between the count of the rows that must be there and that count plus the borderline rows that may
    be; the cube counts every row once.  Returns the number of borderline rows."""
    border = candidate_cells(summary, labels, mode, n_samples, near_ties, thresholds)
    sure = np.ones(len(labels), dtype=bool)
    sure[list(border)] = False
    low = cube_of(summary[sure], np.asarray(labels)[sure], thresholds)
    high = low.copy()
    for cells in border.values():
        for cell in cells:
            high[cell] += 1
    got = np.asarray(got)
    assert got.shape == low.shape and got.sum() == len(labels), label
    bad = np.argwhere((got < low) | (got > high))
    assert len(bad) == 0, "%s: %d cells outside the borderline rule, first %s: got %d, allowed [%d, %d]" % (
        label, len(bad), bad[0], got[tuple(bad[0])], low[tuple(bad[0])], high[tuple(bad[0])])
    return len(border)


def near_ties_of(stack, tol=TOL):
    """[row, sample, runner-up class] of every (sample, row) whose two leading probabilities lie within ``tol``."""
    order = np.argsort(-stack, axis=2, kind="stable")[:, :, :2]
    top = np.take_along_axis(stack, order, axis=2)
    s, r = np.where(top[:, :, 0] - top[:, :, 1] <= tol)
    return np.column_stack((r, s, order[s, r, 1])).astype(np.int64).reshape(-1, 3)
