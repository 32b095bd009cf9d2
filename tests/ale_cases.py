"""Accumulated local effects restated in float64 on the oracle's forward pass: the definition as a plain loop over rows
(``loop_local_effects``), the vectorised form the tests use as their reference (``local_effects``), a stand-in for the device
seam of npbnn_amd.ale (``oracle_seam``), and the case table of npbnn_predict_ale's two routes (CASES) with its inputs and
reference.  Route 1's envelope is npbnn_predict_pdp's (tests/pdp_cases.py describes it); the inputs are drawn by its
``envelope_inputs``."""
import numpy as np

import oracle as orc
import pdp_cases
from attrib_common import _apply_override, seam_to_oracle

OUT_FNS = pdp_cases.OUT_FNS


def bins_of(column, edges):
    """0-based bin of every entry: the first k in 1..K with entry <= edges[k] (float32 against float32), K above the last
    edge - so entries at or below edges[0] land in the first bin."""
    e = np.asarray(edges, dtype=np.float64).astype(np.float32)
    return np.minimum(np.searchsorted(e[1:], np.asarray(column).astype(np.float32), side="left"), len(e) - 2)


def _predict(x, w, fun, slopes, trainable, out_fn):
    act = orc.Act(fun, prm=None if slopes is None else np.asarray(slopes, dtype=float), trainable=trainable)
    return out_fn(orc.forward_logits(x, w, act))


def local_effects(x, focal, edges, weights, fun="tanh", out_fn=orc.out_softmax, slopes=None, override=None, trainable=False):
    """(counts [K], effects [S, K, n_out]) in float64 on the table ``x`` as given: every row at the upper and at the lower edge
    of its own bin (two forward passes per set), ``override``'s columns (NaN = none) set after that, the differences averaged
    per bin; 0 for an empty bin."""
    x = np.asarray(x, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    n_bins = len(edges) - 1
    k = bins_of(x[:, focal], edges)
    counts = np.bincount(k, minlength=n_bins).astype(np.int64)
    hi, lo = np.array(x, copy=True), np.array(x, copy=True)
    hi[:, focal] = edges[k + 1]
    lo[:, focal] = edges[k]
    hi, lo = _apply_override(hi, override), _apply_override(lo, override)
    effects = None
    for s, w in enumerate(weights):
        sl = None if slopes is None else slopes[s]
        diff = _predict(hi, w, fun, sl, trainable, out_fn) - _predict(lo, w, fun, sl, trainable, out_fn)
        if effects is None:
            effects = np.zeros((len(weights), n_bins, diff.shape[1]))
        for b in range(n_bins):
            if counts[b]:
                effects[s, b] = diff[k == b].mean(axis=0)
    return counts, effects


def loop_local_effects(x, focal, edges, weights, fun="tanh", out_fn=orc.out_softmax, slopes=None, override=None, trainable=False):
    """The definition read out row by row: the row's bin by a scan over the edges, the row copied twice, two forward passes of
    one row each, sums per bin divided by the counts."""
    x = np.asarray(x, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    n_bins = len(edges) - 1
    e32 = edges.astype(np.float32)
    counts = np.zeros(n_bins, dtype=np.int64)
    sums = None
    for i in range(x.shape[0]):
        v = np.float32(x[i, focal])
        k = n_bins
        for m in range(1, n_bins + 1):
            if v <= e32[m]:
                k = m
                break
        counts[k - 1] += 1
        for s, w in enumerate(weights):
            pair = []
            for z in (edges[k], edges[k - 1]):
                row = np.array(x[i:i + 1], copy=True)
                row[0, focal] = z
                row = _apply_override(row, override)
                pair.append(_predict(row, w, fun, None if slopes is None else slopes[s], trainable, out_fn)[0])
            if sums is None:
                sums = np.zeros((len(weights), n_bins, len(pair[0])))
            sums[s, k - 1] += pair[0] - pair[1]
    return counts, sums / np.maximum(counts, 1)[None, :, None]


def curve(counts, effects):
    """[S, K + 1, n_out]: the centred accumulated curve of the definition, bin by bin."""
    counts = np.asarray(counts, dtype=np.float64)
    n_sets, n_bins, n_out = effects.shape
    acc = np.zeros((n_sets, n_bins + 1, n_out))
    for k in range(1, n_bins + 1):
        acc[:, k] = acc[:, k - 1] + effects[:, k - 1]
    centre = np.zeros((n_sets, n_out))
    for k in range(1, n_bins + 1):
        centre += counts[k - 1] * (acc[:, k - 1] + acc[:, k]) / (2.0 * counts.sum())
    return acc - centre[:, None, :]


def oracle_seam(data, focal, edges, weights, alphas, actFun, output_act_fun, data_transform):
    """float64 stand-in for npbnn_amd.ale._ale_local_effects: every sample with its own slopes, the feature indicators after
    the edges."""
    fun, out, slopes, override = seam_to_oracle(alphas, actFun, output_act_fun, data_transform)
    return local_effects(data, focal, edges, weights, fun=fun, out_fn=OUT_FNS[out], slopes=slopes, override=override)


# ---- the cases of npbnn_predict_ale (tests/test_hip_ale.py on the GPU, tests/test_host_ale.py's guard) -----------------------------
#
# A case is one of tests/pdp_cases.py's envelope cases (same keys, same draw) with one focal column and, instead of a grid:
#   bins   K of the quantile edges np.unique(np.quantile(training column, linspace(0, 1, K + 1))), or
#   edges  the edges themselves
#   ordinal  number of levels the focal column is replaced by (integers 0 .. levels - 1) in both tables; edges = the levels
# ``route`` is what NPBNN_INFO_ALE_ROUTE must say.  ``reroute``: a route-1 case that runs again on route 2, under
# NPBNN_ALE_PER_EDGE=1 and under NPBNN_FORCE_WIDE=1.
CASES = {}
_PER_EDGE = (("NPBNN_ALE_PER_EDGE", "1"),)
_WIDE = (("NPBNN_FORCE_WIDE", "1"),)
_LINEAR_7 = [-2.5, -1.2, -0.6, -0.1, 0.3, 0.8, 1.5, 2.5]


def _case(name, route, bins=7, edges=None, ordinal=0, **kw):
    assert name not in CASES, name
    unknown = set(kw) - set(pdp_cases._DEFAULTS)
    assert not unknown, (name, unknown)
    CASES[name] = dict(pdp_cases._DEFAULTS, name=name, route=route, seed=7000 + len(CASES), bins=bins, edges=edges, ordinal=ordinal,
                       reroute=route == 1 and not kw.get("env"), **kw)


# rows around a workgroup (edges given: one row has no quantiles), bins, sets around a launch
for _rows in (1, 255, 256, 257, 2111):
    _case("rows_%d" % _rows, 1, rows=_rows, edges=_LINEAR_7)
for _k in (1, 2, 7, 40):
    _case("bins_%d" % _k, 1, bins=_k)
for _sets in (1, 2, 3, 7):
    _case("sets_%d_two_a_launch" % _sets, 1, sets=_sets)                   # H0 = 20: two sets a launch
    _case("sets_%d_one_a_launch" % _sets, 1, sets=_sets, nodes=(40, 6))    # H0 = 40: one
# activations and slopes
_case("genrelu_per_set", 1, fun="genReLU", slopes="per_set", sets=5)
_case("genrelu_per_set_33", 1, fun="genReLU", slopes="per_set", sets=5, nodes=(33, 9))
for _fun in ("ReLU", "swish", "tanh"):
    _case("act_%s" % _fun.lower(), 1, fun=_fun, nodes=(16, 12, 6))
# outputs
for _tag, _kw in [("softmax", dict(out="softmax")), ("identity", dict(out="identity")), ("softplus_half_6", dict(out="softplus_half", n_out=6)),
                  ("softplus_half_5", dict(out="softplus_half", n_out=5))]:
    for _apply in (True, False):
        _case("out_%s_%s" % (_tag, "applied" if _apply else "raw"), 1, apply_out=_apply, **_kw)
_case("outputs_1", 1, n_out=1, out="identity")                       # (a softmax over one output is 1 whatever the kernel does)
_case("outputs_7", 1, n_out=7)
_case("outputs_32", 1, n_out=32)
_case("outputs_33", 2, n_out=33)
# widths at route 1's edges
for _h0, _route in [(32, 1), (33, 1), (64, 1), (65, 2)]:
    _case("h0_%d" % _h0, _route, nodes=(_h0, 6))
_case("later_32", 1, nodes=(20, 32))
_case("later_33", 2, nodes=(20, 33))
# depth and bias patterns
_case("one_matrix", 1, nodes=(), n_out=3)
_case("one_matrix_identity_no_bias", 1, nodes=(), n_out=7, out="identity", bias="none")
_case("one_matrix_33_outputs", 2, nodes=(), n_out=33)
_case("five_matrices_mixed01", 1, nodes=(20, 12, 9, 6), bias="mixed01")
_case("five_matrices_mixed10", 1, nodes=(20, 12, 9, 6), bias="mixed10")
# edges and rows
_case("ordinal_rows_on_edges", 1, ordinal=5, rows=600)
_case("test_table_beyond_the_edges", 1, which=1, test_rows=173, edges=[-1.0, -0.4, 0.0, 0.4, 1.0])
_case("test_table_empty_bin", 1, which=1, test_rows=173, edges=[-3.0, -0.5, -0.4999, 0.5, 3.0])
_case("test_table_per_edge", 2, which=1, test_rows=173, edges=[-1.0, -0.4, 0.0, 0.4, 1.0], env=_PER_EDGE)
# overrides
_case("override_beside_focal", 1, override={5: 1.25, 17: -0.75})
_case("override_on_the_focal", 1, override={3: 0.5}, pinned=True)
_case("override_on_the_focal_per_edge", 2, override={3: 0.5}, pinned=True, env=_PER_EDGE)
# 36 workgroups: the reduction's sixteen runs hold two or three workgroups each
_case("rows_9000", 1, rows=9000, sets=2)
# the workgroups' partials in chunks of one workgroup (two sets x 7 bins x 5 outputs x 8 bytes): nine launches per group of sets
_case("partials_in_chunks", 1, rows=2111, sets=3, env=(("NPBNN_ALE_PART_BYTES", str(2 * 7 * 5 * 8)),))
# route 2 on each path
_case("per_edge_l0_f32", 2, env=_PER_EDGE + (("NPBNN_L0", "f32"),), l0="f32")
_case("streamed_l0_f32", 2, env=_WIDE + (("NPBNN_L0", "f32"),), l0="f32")
# config 2's network
_case("config2_network", 1, rows=3000, features=256, nodes=(32, 8), n_out=10, bins=40)


def inputs(case):
    """pdp_cases.envelope_inputs' arrays for the case, plus ``edges`` and ``column``: the focal column."""
    inp = pdp_cases.envelope_inputs(case)
    j = case["focal"][0]
    if case["ordinal"]:
        rs = np.random.default_rng(case["seed"] + 1)
        for key in ("x", "x_test"):
            if inp[key] is not None:
                inp[key][:, j] = rs.integers(0, case["ordinal"], inp[key].shape[0])
        edges = np.arange(case["ordinal"], dtype=np.float64)
    elif case["edges"] is not None:
        edges = np.asarray(case["edges"], dtype=np.float64)
    else:
        edges = np.unique(np.quantile(inp["x"][:, j], np.linspace(0, 1, case["bins"] + 1)))
    inp["table"] = inp["x_test"] if case["which"] == 1 else inp["x"]
    inp["edges"] = edges
    inp["column"] = j
    return inp


def reference(case, inp, override=True):
    """(counts, effects) of the case in float64 on the table the device holds (float32 entries)."""
    table = inp["table"].astype(np.float32).astype(np.float64)
    out_fn = OUT_FNS[case["out"]] if case["apply_out"] else orc.out_identity
    return local_effects(table, inp["column"], inp["edges"], inp["weights"], fun=case["fun"], out_fn=out_fn, slopes=inp["slopes"],
                         override=inp["override"] if override else None, trainable=case["trainable"])
