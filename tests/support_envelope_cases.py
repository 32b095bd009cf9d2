"""The envelope of npbnn_predict_sets_support (npbnn_amd/csrc/npbnn_support.hip): the case table CASES, its seeded inputs and the plain
numpy restatement a case is held to.  tests/test_hip_support_envelope.py runs the cases on the device,
tests/test_host_support_envelope.py shows on the CPU that the restatement tells a wrong support_final_kernel from a right one on the
cases named there.  Nothing here needs a GPU.

A case is one or two axes away from the default: 300 rows x 5 features, one hidden layer of 6, tanh, 4 classes, 5 stored sets, the
99-point grid, no prior, no cutoff.  Every value of an axis is the smallest at which the code it names can go wrong:
  rows        wave and workgroup edges (64 lanes, 256 threads), one to four workgroups with a full and a ragged last one, one row;
  classes     the cell index (b * C + label) * C + call at small, odd and large C; with the grid's 100 bins, 10 classes are the last
              cube counted in LDS (10000 cells), 11 the first counted by global atomics (12100);
  edge        exactly 10240 cells (LDS) and the first count above it (global), at C = 32 and at C = 8;
  thresholds  none, one, two; 511, 512, 513 and 1024 (more than 512 are searched in global memory - with 4 classes 513 thresholds
              still leave the cube in LDS); equal neighbours; values at and outside [0, 1] with both infinities; every k / n_sets
              itself, so that in mode 0 ``p == t`` occurs by construction;
  bf          a prior with 0, 1, 4, 512 and 513 Bayes-factor thresholds (more than 512: searched and counted in global memory), the
              thresholds holding 1.0, a repeated value and +inf; and a prior the test builds from a first call's summary
              (``built_prior``): factors of exactly 1.0, +inf, and thresholds that ARE factors the rows attain;
  near full   all four LDS parts at once, about 50 KiB of dynamic LDS;
  sets        1, 2, 3, 4, 7, 64 (an even count gives real vote ties in mode 0); genReLU slope vectors a a b b b a: passes of 2, 3, 1;
  cutoff      0.0, 1.0, -inf, and 0.5 with 4 sets - a value mode 0 attains;
  outputs     the optional summary and keep mask in all four combinations;
  test        the statistic on the test table, 513 rows under 300 training rows, labels of its own draw;
  grid        2 classes, 3 features, 2 sets: 256 * 3 * n_cu + 300 rows with the cube in LDS (the cap of 3 workgroups per compute unit
              binds and 300 rows are reached in a second stride), and 2048 * 256 + 257 rows with the cube global (2560 thresholds: the
              2048 workgroups of grid_for take a second stride and search global memory);
  crossed     edges the one-axis cases do not reach together, so that every reachable combination of the three LDS switches has a case.

Inputs: a teacher network, the stored sets perturbations of it (the sets agree on most rows and disagree on some: unanimous votes,
split votes and ties all occur), labels the teacher's calls with a share redrawn and every class planted once.

Every comparison a case makes is an equality: the tables are integers, the quotients one float64 division of values the device and
the restatement share (the float32 predictions ``predict_sets`` returns from the same context)."""
import functools

import numpy as np

import cases
import oracle as orc
import support_cases as sc

MODES = (0, 1)
WORKGROUP = 256                                 # kFiThreads
FI_MAX_BLOCKS = 2048                            # kFiMaxBlocks: grid_for's cap
LDS_CELLS = 10240                               # kSupportLdsCells
LDS_THRESHOLDS = 512                            # kSupportLdsThresholds
WG_PER_CU = 3                                   # kSupportWgPerCu
ASSUMED_N_CU = 256                              # an MI355X; the GPU test asks the device (INFO_N_CU), the host model assumes
MAX_GROUP = 3                                   # kMaxCand, kWideMaxCand: sets a pass of the replay carries at most
SLOPES = "aabbba"

_DEFAULTS = dict(rows=300, features=5, nodes=(6,), n_out=4, sets=5, slopes=None, thresholds=("grid",), prior=None, n_bf=0, cutoff=None,
                 train_rows=None, outputs=False, edge=None)
CASES = {}


def _case(name, **kw):
    unknown = set(kw) - set(_DEFAULTS)
    assert not unknown and name not in CASES, (name, unknown)
    c = dict(_DEFAULTS, name=name, **kw)
    if c["slopes"]:
        c["sets"] = len(c["slopes"])
    CASES[name] = c


_case("default")
for _n in (1, 63, 64, 65, 255, 256, 257, 513, 769):
    _case("rows_%d" % _n, rows=_n)
for _c in (1, 2, 3, 5, 8, 10, 11, 31, 32, 33, 100):
    _case("classes_%d" % _c, n_out=_c)
# the cube's LDS edge exactly: (n + 1) * C * C = 10240, and the next count of thresholds
_case("edge_32_classes_lds", n_out=32, thresholds=("count", 9))
_case("edge_32_classes_global", n_out=32, thresholds=("count", 10))
_case("edge_8_classes_lds", n_out=8, thresholds=("count", 159))
_case("edge_8_classes_global", n_out=8, thresholds=("count", 160))
for _t in (0, 1, 2, 511, 512, 513, 1024):
    _case("thresholds_%d" % _t, thresholds=("count", _t))
_case("thresholds_equal_neighbours", thresholds=("equal",))
_case("thresholds_outside_0_1", thresholds=("outside",), edge="threshold")
_case("thresholds_are_the_votes", thresholds=("votes",), edge="threshold")
for _b in (0, 1, 4, 512, 513):
    _case("bf_%d" % _b, prior="drawn", n_bf=_b)
_case("prior_built", prior="built", edge="prior")
_case("near_full_lds", n_out=8, thresholds=("count", 159), prior="drawn", n_bf=512)
for _s in (1, 2, 3, 4, 7, 64):
    _case("sets_%d" % _s, sets=_s, edge="ties" if _s % 2 == 0 else None)
_case("slopes_aabbba", slopes=SLOPES)
_case("cutoff_0", cutoff=0.0)
_case("cutoff_1", cutoff=1.0)
_case("cutoff_minus_inf", cutoff=-np.inf)
_case("cutoff_attained", sets=4, cutoff=0.5, thresholds=("values", (0.25, 0.5, 0.75)), edge="cutoff")
_case("optional_outputs", outputs=True, cutoff=0.6)
_case("test_table", rows=513, train_rows=300)
_GRID = dict(n_out=2, features=3, sets=2)
_case("grid_capped", rows="cap+300", **_GRID)
_case("grid_max_blocks_global", rows=FI_MAX_BLOCKS * WORKGROUP + 257, thresholds=("count", 2560), **_GRID)
CROSSED = ("rows_257_classes_11_thr_513_bf_513_cutoff", "test_table_classes_32_thr_9", "thr_513_bf_4", "thr_513_bf_513", "classes_11_bf_4",
           "classes_11_bf_513", "classes_11_thr_513_bf_512", "rows_1_classes_8_bf_1")
_case(CROSSED[0], rows=257, n_out=11, thresholds=("count", 513), prior="drawn", n_bf=513, cutoff=0.3)
_case(CROSSED[1], rows=513, train_rows=300, n_out=32, thresholds=("count", 9))
_case(CROSSED[2], thresholds=("count", 513), prior="drawn", n_bf=4)
_case(CROSSED[3], thresholds=("count", 513), prior="drawn", n_bf=513)
_case(CROSSED[4], n_out=11, prior="drawn", n_bf=4)
_case(CROSSED[5], n_out=11, prior="drawn", n_bf=513)
_case(CROSSED[6], n_out=11, thresholds=("count", 513), prior="drawn", n_bf=512)
_case(CROSSED[7], rows=1, n_out=8, prior="drawn", n_bf=1)
ROUTED = CROSSED + ("test_table", "classes_31", "classes_32", "classes_33")
SAME_BYTES = ("grid_capped", "near_full_lds", "classes_11")


# ---- what the entry's launch does with a case ---------------------------------------------------------------------------------------
def rows_of(case, n_cu=ASSUMED_N_CU):
    return WORKGROUP * WG_PER_CU * n_cu + 300 if case["rows"] == "cap+300" else case["rows"]


def thresholds_of(case):
    kind = case["thresholds"][0]
    if kind == "grid":
        t = sc.GRID
    elif kind == "count":
        t = np.linspace(0.0, 1.0, case["thresholds"][1] + 2)[1:-1]
    elif kind == "values":
        t = np.array(case["thresholds"][1], dtype=np.float64)
    elif kind == "equal":
        t = np.array([0.2, 0.3, 0.3, 0.3, 0.5, 0.5, 0.9, 0.9])
    elif kind == "outside":
        t = np.array([-np.inf, -np.inf, -0.5, 0.0, 0.25, 0.5, 1.0, 1.0, 1.5, np.inf])
    else:
        assert kind == "votes"
        t = np.arange(case["sets"] + 1) / case["sets"]              # the quotient votes / n_sets itself
    return np.array(t, dtype=np.float64)


def drawn_bf_thresholds(n_bf):
    """Ascending; 4 and more hold 1.0, a repeated value and +inf."""
    if n_bf == 0:
        return np.zeros(0)
    if n_bf == 1:
        return np.array([1.0])
    if n_bf == 4:
        return np.array([1.0, 3.0, 3.0, np.inf])
    v = np.geomspace(1e-2, 1e4, n_bf - 3)
    return np.sort(np.concatenate([v, [1.0, v[len(v) // 2], np.inf]]))


def launch_plan(case, n_cu=ASSUMED_N_CU):
    """The switches, dynamic-LDS size and grid npbnn_predict_sets_support chooses for a case, restated from its host code."""
    c, n_thr = case["n_out"], len(thresholds_of(case))
    n_bf = None if case["prior"] is None else (case["n_bf"] if case["prior"] == "drawn" else -1)        # (-1: known once the test built them)
    cells = (n_thr + 1) * c * c
    lds_cube, lds_thr = cells <= LDS_CELLS, n_thr <= LDS_THRESHOLDS
    n_rows = rows_of(case, n_cu)
    grid = min(max(1, -(-n_rows // WORKGROUP)), FI_MAX_BLOCKS)
    if lds_cube:
        grid = min(grid, WG_PER_CU * n_cu)
    return dict(cells=cells, lds_cube=lds_cube, lds_thr=lds_thr, n_bf=n_bf, grid=grid, n_rows=n_rows, strides=-(-n_rows // (grid * WORKGROUP)))


def bf_side(n_bf):
    """"none" (no prior) | "lds" | "global": where the Bayes-factor thresholds and cells live."""
    return "none" if n_bf is None else ("lds" if n_bf <= LDS_THRESHOLDS else "global")


def lds_layout(c, n_thr, n_bf, lds_cube, lds_thr, lds_bf):
    """Byte offsets of [thresholds | bf thresholds | cube cells | bf cells] and the total: the launch's dynamic-LDS size."""
    cells, bf_cells = (n_thr + 1) * c * c, 0 if n_bf is None else (n_bf + 1) * 2
    thr = 0
    bft = thr + 8 * (n_thr if lds_thr else 0)
    cube = bft + 8 * (n_bf if lds_bf else 0)
    bf = cube + 4 * (cells if lds_cube else 0)
    return dict(thr=thr, bft=bft, cube=cube, bf=bf, total=bf + 4 * (bf_cells if lds_bf else 0))


def expected_groups(slopes, n_sets):
    """[(s0, g)]: the passes of the replay (fold_envelope_cases.expected_groups)."""
    out, s0 = [], 0
    while s0 < n_sets:
        g = 1
        while s0 + g < n_sets and g < MAX_GROUP and (slopes is None or np.array_equal(slopes[s0 + g], slopes[s0])):
            g += 1
        out.append((s0, g))
        s0 += g
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _seed(name):
    return cases.hash_name("support_envelope/" + name) % (2 ** 31)


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


def _labels(rs, calls, c):
    """The calls with three in ten redrawn, every class planted once where the rows allow."""
    n = len(calls)
    lab = np.where(rs.random(n) < 0.3, rs.integers(0, c, n), calls).astype(np.int64)
    at = rs.permutation(n)[:min(c, n)]
    lab[at] = np.arange(len(at))
    return lab


@functools.lru_cache(maxsize=4)
def inputs(name, n_cu=ASSUMED_N_CU):
    """What a case hands the device and the restatement: ``x`` and ``labels`` of the table the statistic is taken on, ``train_x`` and
    ``train_labels`` of the training slot above a test table (else None), the stored ``sets``, ``slopes`` per set (or None),
    ``thresholds``, ``prior`` / ``bf_thresholds`` (None where the case has no prior or builds it from a summary), ``cutoff``."""
    case = CASES[name]
    rs = np.random.default_rng(_seed(name))
    n, f, c, n_sets = rows_of(case, n_cu), case["features"], case["n_out"], case["sets"]
    x = rs.standard_normal((n, f))
    shapes = cases.layer_shapes(f, list(case["nodes"]), c, 2)
    teacher = [rs.normal(0, 2.0 / np.sqrt(s[1]), s) for s in shapes]
    sets = [[t + rs.normal(0, 1.4 / np.sqrt(t.shape[1]), t.shape) for t in teacher] for _ in range(n_sets)]
    slopes = None
    if case["slopes"]:
        vec = {"a": np.array([0.05]), "b": np.array([0.25])}
        slopes = [vec[ch] for ch in case["slopes"]]
    act = orc.Act("genReLU", np.array([0.15])) if slopes else orc.Act("tanh")
    labels = _labels(rs, np.argmax(orc.forward(x, teacher, act, orc.out_softmax), axis=1), c)
    out = dict(case=case, x=_frozen(x), labels=_frozen(labels), sets=sets, slopes=slopes, thresholds=_frozen(thresholds_of(case)), cutoff=case["cutoff"],
               train_x=None, train_labels=None, prior=None, bf_thresholds=None, groups=expected_groups(slopes, n_sets))
    if case["train_rows"]:
        out.update(train_x=_frozen(rs.standard_normal((case["train_rows"], f))), train_labels=_frozen(rs.integers(0, c, case["train_rows"])))
    if case["prior"] == "drawn":
        out.update(prior=_frozen(rs.dirichlet(np.ones(c), n)), bf_thresholds=_frozen(drawn_bf_thresholds(case["n_bf"])))
    return out


def oracle_stack(name, n_cu=ASSUMED_N_CU):
    """The float64 oracle's predictions of a case's sets [S, N, C], as a float32 holds them: what the host tests summarise."""
    inp = inputs(name, n_cu)
    out = []
    for s, w in enumerate(inp["sets"]):
        act = orc.Act("genReLU", inp["slopes"][s]) if inp["slopes"] else orc.Act("tanh")
        out.append(orc.forward(inp["x"], w, act, orc.out_softmax))
    return np.stack(out).astype(np.float32).astype(np.float64)


def built_prior(name, summary):
    """The prior of the "built" case, from a first call's summary: a third of the rows the summary itself (the factor is exactly 1.0),
    some rows 0.0 at the called class (+inf), some 1.0, the rest drawn; and Bayes-factor thresholds that hold 1.0, a repeated value,
    +inf and the factors 40 of the drawn rows attain (by the definition's order of operations)."""
    rs = np.random.default_rng(_seed(name + "/prior"))
    n, c = summary.shape
    rows, call = np.arange(n), np.argmax(summary, axis=1)
    prior = rs.dirichlet(np.ones(c), n)
    same, zero, one = rows % 3 == 0, rows % 12 == 1, rows % 12 == 2
    prior[same] = summary[same]
    prior[zero, call[zero]] = 0.0
    prior[one, call[one]] = 1.0
    factor = bayes_factor(summary[rows, call], prior[rows, call])
    attained = factor[~(same | zero | one)][:40]
    return prior, np.sort(np.concatenate([[1.0, 3.0, 3.0, np.inf], attained]))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def summarise(stack, mode):
    """mode 0: per-set argmax (the first of ties), integer votes, votes / n_sets; mode 1: the sets added in set order in float64, then
    / n_sets."""
    n_sets, n, c = stack.shape
    if mode == 0:
        votes = np.zeros((n, c), dtype=np.int64)
        rows = np.arange(n)
        for s in range(n_sets):
            votes[rows, np.argmax(stack[s], axis=1)] += 1
        return votes / n_sets
    total = np.zeros((n, c))
    for s in range(n_sets):
        total = total + stack[s]
    return total / n_sets


def bayes_factor(p, r):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return (p / (1e-10 + 1 - p)) / (r / (1e-10 + 1 - r))


def restatement(summary, labels, thresholds, prior=None, bf_thresholds=None, cutoff=None):
    """Everything the entry returns, from a summary by the definitions: ``cube`` (support_cases.cube_of), ``bf``, ``keep`` and the
    ``summary`` with NaN rows where keep is false; and the row values ``call``, ``p``, ``factor`` the edge conditions are read from."""
    labels = np.asarray(labels, dtype=np.int64)
    n = len(labels)
    rows, call = np.arange(n), np.argmax(summary, axis=1)
    p = summary[rows, call]
    out = dict(cube=sc.cube_of(summary, labels, thresholds), bf=None, call=call, p=p, factor=None)
    if prior is not None:
        factor = bayes_factor(p, prior[rows, call])
        b = np.zeros(n, dtype=np.int64)
        for t in bf_thresholds:
            b += factor > t
        bf = np.zeros((len(bf_thresholds) + 1, 2), dtype=np.int64)
        np.add.at(bf, (b, (call == labels).astype(np.int64)), 1)
        out.update(bf=bf, factor=factor)
    keep = p > cutoff if cutoff is not None else np.ones(n, dtype=bool)
    masked = summary.copy()
    masked[~keep] = np.nan
    out.update(keep=keep, summary=masked)
    return out


FIELDS = ("cube", "bf", "keep", "summary")


def same_bytes(got, want):
    """Byte equality of one returned field; a summary's NaNs by position, every other value by its bytes."""
    if got is None or want is None:
        return got is None and want is None
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        return bool(np.array_equal(np.isnan(got), nan)) and got[~nan].tobytes() == want[~nan].tobytes()
    return got.tobytes() == want.tobytes()


def differing_fields(got, want):
    return [k for k in FIELDS if not same_bytes(got[k], want[k])]


# ---- the edge a case says it exercises ------------------------------------------------------------------------------------------------
def rows_on_a_threshold(p, thresholds):
    return int(np.sum(np.isin(p, thresholds)))


def tied_rows(summary):
    """Rows whose largest value is held by two or more classes."""
    return int(np.sum(np.sum(summary == summary.max(axis=1, keepdims=True), axis=1) >= 2))


def must_tie(case, mode):
    """An even count of sets gives real vote ties in mode 0: every such case has to show one, whatever other edge it names."""
    return mode == 0 and case["sets"] % 2 == 0


def edge_count(case, mode, want, summary, thresholds, bf_thresholds, cutoff):
    """The number of rows on the edge the case names (None: the case names none for this mode).  Votes attain their quotients exactly,
    means do not: the threshold, cutoff and tie edges are mode 0's; the built prior's factor of exactly 1.0 is both modes'."""
    edge = case["edge"]
    if edge == "prior":
        return rows_on_a_threshold(want["factor"], bf_thresholds)
    if edge is None or mode != 0:
        return None
    if edge == "threshold":
        return rows_on_a_threshold(want["p"], thresholds)
    if edge == "cutoff":
        return int(np.sum(want["p"] == cutoff))
    assert edge == "ties"
    return tied_rows(summary)
