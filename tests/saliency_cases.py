"""Input-gradient saliency restated in float64 on the oracle's layers: the analytic gradients of every row (``gradients``), their
three row means as npbnn_predict_saliency returns them (``means``, ``reference``), a stand-in for the device seam of
npbnn_amd.saliency (``oracle_seam``), and the case table of npbnn_predict_saliency's two routes (CASES) with its inputs.  Route 1's
envelope is npbnn_predict_pdp's (tests/pdp_cases.py describes it); the inputs are drawn by its ``envelope_inputs``.

Kinks: a ReLU or leaky unit whose pre-activation changes sign between float32 and float64 moves a row's gradient by a finite step,
not by a rounding error.  For the piecewise-linear activations ``inputs`` therefore redraws a row, from a generator of the case's
own, while any hidden pre-activation of any set on that row lies within MARGIN of zero in float64."""
import numpy as np

import oracle as orc
import pdp_cases
from attrib_common import _act, _apply_override, seam_to_oracle

MARGIN = 1e-4            # about 75 times the largest device - float64 difference measured on these draws (1.3e-6, NOTES 8)
MAX_REDRAWN = 0.03       # share of a case's rows that may be redrawn
PIECEWISE = ("ReLU", "genReLU")


def _matrix(w, n_in):
    """a layer's weights without its bias column (column 0, when there is one)"""
    return w[:, w.shape[1] - n_in:]


def _act_derivative(z, act, layer_n):
    """a'(z) on the branch orc.activate takes"""
    if act.kind == "relu":
        return (z > 0).astype(np.float64)
    if act.kind == "leaky":
        return np.where(z < 0, act.slope(layer_n), 1.0)
    if act.kind == "swish":
        s = (1 + np.exp(-z)) ** (-1)
        return s * (1 + z * (1 - s))
    t = orc.activate(np.array(z, copy=True), act, layer_n)
    return 1.0 - t * t


def hidden_preactivations(x, w, act):
    """the pre-activations of every hidden layer, [n, hidden units of all layers]"""
    tmp, res = x, []
    for i in range(len(w) - 1):
        z = orc.dense(tmp, w[i])
        res.append(np.array(z, copy=True))
        tmp = orc.activate(z, act, i)
    return np.concatenate(res, axis=1) if res else np.zeros((x.shape[0], 0))


def set_gradients(x, w, act, out="softmax", apply_out=True, wrong=None):
    """[n, C, F]: d f(x_i)_c / d x_ij of one weight set on the rows of x as given, by the chain rule over orc.dense and
    orc.activate.  ``wrong``: a deliberately wrong variant for the guard of tests/test_host_saliency.py - "no_factor" leaves out
    the first hidden layer's derivative factor, "softmax_diagonal" the -p_c p_k term of the softmax."""
    tmp, factors = np.asarray(x, dtype=np.float64), []
    for i in range(len(w) - 1):
        z = orc.dense(tmp, w[i])
        factors.append(_act_derivative(z, act, i))
        tmp = orc.activate(z, act, i)
    z = orc.dense(tmp, w[-1])
    n, c = z.shape
    kind = out if apply_out else "identity"
    if kind == "softmax":
        p = orc.out_softmax(z)
        g = p[:, :, None] * np.eye(c)[None]
        if wrong != "softmax_diagonal":
            g = g - p[:, :, None] * p[:, None, :]
    elif kind == "softplus_half":
        diag = np.ones((n, c))
        diag[:, int(c / 2):] = (1 + np.exp(-z[:, int(c / 2):])) ** (-1)
        g = diag[:, :, None] * np.eye(c)[None]
    else:
        g = np.broadcast_to(np.eye(c), (n, c, c))
    if wrong == "no_factor" and factors:
        factors[0] = np.ones_like(factors[0])
    for i in range(len(w) - 1, 0, -1):
        g = np.matmul(g, _matrix(w[i], w[i - 1].shape[0])) * factors[i - 1][:, None, :]
    return np.matmul(g, _matrix(w[0], x.shape[1]))


def gradients(x, weights, fun="tanh", out="softmax", slopes=None, override=None, apply_out=True, trainable=False, wrong=None):
    """[S, n, C, F]: the gradients of every weight set on the table ``x`` after ``override`` (NaN = none); 0 on its columns."""
    xo = _apply_override(x, override)
    res = []
    for s, w in enumerate(weights):
        g = set_gradients(xo, w, _act(fun, None if slopes is None else slopes[s], trainable), out, apply_out, wrong)
        if override is not None:
            g[:, :, ~np.isnan(override)] = 0.0
        res.append(g)
    return np.array(res)


def means(x, weights, **kw):
    """(mean, abs, sq), each [S, C, F]: the row means of G, |G| and G^2, reduced set by set"""
    res = ([], [], [])
    for s, w in enumerate(weights):
        sl = kw.get("slopes")
        g = gradients(x, [w], **dict(kw, slopes=None if sl is None else [sl[s]]))[0]
        for acc, v in zip(res, (g, np.abs(g), g * g)):
            acc.append(v.mean(axis=0))
    return tuple(np.array(a) for a in res)


def reference(case, inp, wrong=None):
    """(mean, abs, sq) of the case in float64 on the table the device holds (float32 entries)."""
    table = inp["table"].astype(np.float32).astype(np.float64)
    return means(table, inp["weights"], fun=case["fun"], out=case["out"], slopes=inp["slopes"], override=inp["override"],
                 apply_out=case["apply_out"], trainable=case["trainable"], wrong=wrong)


def oracle_seam(data, weights, alphas, actFun, output_act_fun, data_transform):
    """float64 stand-in for npbnn_amd.saliency._saliency_means: every sample with its own slopes, the feature indicators as
    an override."""
    fun, out, slopes, override = seam_to_oracle(alphas, actFun, output_act_fun, data_transform)
    return means(np.asarray(data, dtype=np.float64), weights, fun=fun, out=out, slopes=slopes, override=override)


# ---- the cases of npbnn_predict_saliency (tests/test_hip_saliency.py on the GPU, tests/test_host_saliency.py's guards) ---------------
#
# A case is one of tests/pdp_cases.py's envelope cases (same keys, same draw; its focal columns and grid are not used), one or two
# axes away from the defaults: the smallest shapes at which each part can go wrong.  ``route`` is what NPBNN_INFO_SALIENCY_ROUTE must
# say.  ``reroute``: a route-1 case that runs again on route 2, under NPBNN_SALIENCY_PLAIN=1 and under NPBNN_FORCE_WIDE=1.
CASES = {}


def _case(name, route, **kw):
    assert name not in CASES, name
    unknown = set(kw) - set(pdp_cases._DEFAULTS)
    assert not unknown, (name, unknown)
    CASES[name] = dict(pdp_cases._DEFAULTS, name=name, route=route, seed=9000 + len(CASES), reroute=route == 1 and not kw.get("env"), **kw)


# rows around a workgroup and a 32-row tile, features around phase 2's 32-feature tiles
for _rows in (1, 255, 256, 257, 2111):
    _case("rows_%d" % _rows, 1, rows=_rows)
for _f in (31, 32, 33, 64, 65):
    _case("features_%d" % _f, 1, features=_f)
# widths at route 1's edges
for _h0, _route in [(1, 1), (31, 1), (32, 1), (33, 1), (64, 1), (65, 2)]:
    _case("h0_%d" % _h0, _route, nodes=(_h0, 6))
_case("later_32", 1, nodes=(20, 32))
_case("later_33", 2, nodes=(20, 33))
_case("outputs_1", 1, n_out=1, out="identity")                       # (a softmax over one output is 1: its gradient is 0)
_case("outputs_7", 1, n_out=7)
_case("outputs_32", 1, n_out=32)
_case("outputs_33", 2, n_out=33)
_case("lds_tail_3300", 1, nodes=(32, 32, 32, 32), n_out=4)
# depth and bias patterns
_case("one_matrix", 1, nodes=(), n_out=3)
_case("one_matrix_no_bias", 1, nodes=(), n_out=3, bias="none")
_case("five_matrices_mixed01", 1, nodes=(20, 12, 9, 6), bias="mixed01")
_case("five_matrices_mixed10", 1, nodes=(20, 12, 9, 6), bias="mixed10")
# activations at real width ("leaky": the leaky kernel without slopes, what a trainable ReLU selects)
for _nodes in [(33, 9), (16, 12, 6)]:
    for _tag, _kw in [("relu", dict(fun="ReLU")), ("leaky", dict(fun="ReLU", trainable=True)),
                      ("genrelu_shared", dict(fun="genReLU", slopes="shared")), ("genrelu_per_set", dict(fun="genReLU", slopes="per_set")),
                      ("swish", dict(fun="swish")), ("tanh", dict(fun="tanh"))]:
        _case("act_%s_%s" % (_tag, "x".join(map(str, _nodes))), 1, nodes=_nodes, sets=5, **_kw)
# output side
for _tag, _kw in [("softmax", dict(out="softmax")), ("identity", dict(out="identity")), ("softplus_half_6", dict(out="softplus_half", n_out=6)),
                  ("softplus_half_5", dict(out="softplus_half", n_out=5))]:
    for _apply in (True, False):
        _case("out_%s_%s" % (_tag, "applied" if _apply else "raw"), 1, apply_out=_apply, **_kw)
# sets around a launch
for _sets in (1, 2, 3, 7):
    _case("sets_%d_two_a_launch" % _sets, 1, sets=_sets)                   # H0 = 20: two sets a launch
    _case("sets_%d_one_a_launch" % _sets, 1, sets=_sets, nodes=(40, 6))    # H0 = 40: one
# two overridden columns: their gradient must be exactly 0
_case("override_two_columns", 1, override={5: 1.25, 17: -0.75}, pinned=True)
_case("test_table", 1, which=1, test_rows=173)
# Scratch in chunks: chunks of 512 rows, five of them (tests/test_host_attrib_plan.py asserts the cut these bytes give).
_case("scratch_in_chunks", 1, rows=2111, env=(("NPBNN_SALIENCY_SCRATCH_BYTES", "900000"),))
# route 2 on real shapes: a wide first layer, and the reference's default network where the library streams its weights by itself
_case("wide_130x40", 2, nodes=(130, 40))
_case("streamed_257x700", 2, rows=257, features=700, nodes=(50, 5))
# config 2's network
_case("config2_network", 1, rows=3000, features=256, nodes=(32, 8), n_out=10)
# The turns of the plan's cut that nothing above takes; tests/test_host_attrib_plan.py asserts what each budget gives.  Route 2 with
# its outputs in launches of 2, 2 and 1 (the later launches read the activations the first left in the scratch) over chunks of 256
# and 44 rows; and the sets_7 cases with three sets' blocks prepared at a time: groups of 3, 3 and 1 sets.
_case("route2_outputs_in_chunks", 2, nodes=(65, 6), env=(("NPBNN_SALIENCY_SCRATCH_BYTES", "520000"),))
_case("sets_7_two_a_launch_in_groups", 1, sets=7, env=(("NPBNN_SALIENCY_PREP_BYTES", str(3 * 7104)),))
_case("sets_7_one_a_launch_in_groups", 1, sets=7, nodes=(40, 6), env=(("NPBNN_SALIENCY_PREP_BYTES", str(3 * 13760)),))


def inputs(case):
    """pdp_cases.envelope_inputs' arrays for the case; with a piecewise-linear activation the rows of both tables that come within
    MARGIN of a kink are drawn again.  ``redrawn``: the largest share of a table's rows that were; ``min_preactivation``: the
    smallest |hidden pre-activation| left on either table (inf without a hidden layer)."""
    inp = pdp_cases.envelope_inputs(case)
    inp["redrawn"], inp["min_preactivation"] = 0.0, np.inf
    if case["fun"] not in PIECEWISE or not case["nodes"]:
        return inp
    rs = np.random.default_rng(case["seed"] + 1)
    acts = [_act(case["fun"], None if inp["slopes"] is None else inp["slopes"][s], case["trainable"]) for s in range(case["sets"])]

    def closest(rows):
        held = _apply_override(rows.astype(np.float32).astype(np.float64), inp["override"])
        return np.min([np.abs(hidden_preactivations(held, w, a)).min(axis=1) for w, a in zip(inp["weights"], acts)], axis=0)

    for key in ("x", "x_test"):
        table = inp[key]
        if table is None:
            continue
        near = closest(table)
        first = np.flatnonzero(near < MARGIN)
        for i in first:
            while near[i] < MARGIN:
                table[i] = rs.standard_normal(table.shape[1])
                near[i] = closest(table[i:i + 1])[0]
        inp["redrawn"] = max(inp["redrawn"], len(first) / table.shape[0])
        inp["min_preactivation"] = min(inp["min_preactivation"], float(near.min()))
    inp["table"] = inp["x_test"] if case["which"] == 1 else inp["x"]
    return inp
