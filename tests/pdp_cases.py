"""The partial-dependence fixture (tests/golden/pdp.npz, written from the reference by tests/golden/make_pdp_golden.py) as calls of
this package, a float64 stand-in for the device seam of npbnn_amd.pdp built on the oracle's forward pass, and the case table of
npbnn_predict_pdp's envelope (ENVELOPE) with its float64 reference."""
import os

import numpy as np

import oracle as orc
from attrib_common import _apply_override, seam_to_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pdp.npz")


def load():
    """{case: dict of its inputs and the reference's outputs}"""
    z = np.load(GOLDEN)
    cases = {}
    for key in z.files:
        name, field = key.split("/", 1)
        cases.setdefault(name, {})[field] = z[key]
    for c in cases.values():
        c["weights"] = [[c["w_%d_%d" % (s, l)] for l in range(int(c["n_layers"]))] for s in range(int(c["n_samples"]))]
        c["focal"] = [int(v) for v in c["focal"]]
        c["fun"] = str(c["fun"])
        c["mode"] = str(c["mode"])
    return cases


def call_args(bn, case):
    """Arguments of ``get_pdp`` for a fixture case (a fresh activation object every time)."""
    act = bn.ActFun(fun=case["fun"])
    out_fn = bn.SoftMax if case["mode"] == "classification" else bn.RegressTransform
    transform = bn.data_transform_obj(case["indicators"], case["means"]) if bool(case["has_transform"]) else None
    return (case["x"], case["focal"], case["mode"], int(case["n_out"]), act, out_fn, case["weights"], list(case["alphas"]), transform)


def oracle_row_means(data, focal_features, grid, weights, alphas, actFun, output_act_fun, data_transform):
    """float64 stand-in for npbnn_amd.pdp._pdp_row_means: grid values, then the feature indicators, then every sample's forward pass
    with its own slopes."""
    fun, out, slopes, override = seam_to_oracle(alphas, actFun, output_act_fun, data_transform)
    res = []
    for point in grid:
        x = np.array(data, dtype=np.float64, copy=True)
        x[:, focal_features] = point
        x = _apply_override(x, override)
        preds = [OUT_FNS[out](orc.forward_logits(x, w, orc.Act(fun, prm=a))) for w, a in zip(weights, slopes)]
        res.append(np.mean(preds, axis=0))
    return np.array(res)


# ---- the envelope of npbnn_predict_pdp's two routes (tests/test_hip_pdp_envelope.py on the GPU, tests/test_host_pdp.py's guard) --------
#
# ``route`` is what NPBNN_INFO_PDP_ROUTE must say, written down by hand from route 1's limits (npbnn_pdp.hip, include/npbnn_hip.h):
# the LDS-resident path, a first layer of at most 64 nodes whose padded image round_up(F, 16) x (32 if H0 <= 32 else 64) floats takes at
# most 64 KiB, later layers and outputs of at most 32 nodes, and (2 if H0 <= 32 else 1) x tail floats x 4 bytes of at most 32 KiB,
# a later layer in -> out counting round_up(out, 4) + out x round_up(in, 8) tail floats.
_DEFAULTS = dict(rows=300, features=40, nodes=(20, 6), n_out=5, sets=3, bias="all", fun="tanh", trainable=False, slopes=None, out="softmax",
                 apply_out=True, focal=(3,), grid=(-2.0, 2.0, 4), override=None, which=0, test_rows=None, env=(), x="normal", l0=None,
                 pinned=False, both_routes=False, many_sets=False)
ENVELOPE = {}


def _case(name, route, **kw):
    unknown = set(kw) - set(_DEFAULTS)
    assert not unknown and name not in ENVELOPE, (name, unknown)
    ENVELOPE[name] = dict(_DEFAULTS, name=name, route=route, seed=1000 + len(ENVELOPE), **kw)


_PER_GRID = (("NPBNN_PDP_PER_GRID", "1"),)
_WIDE = (("NPBNN_FORCE_WIDE", "1"),)

# 1. depth and bias pattern: 1, 2, 3 and 5 weight matrices; every layer with a bias column, none, and the two alternating patterns
for _depth, _nodes, _out in [(1, (), 3), (2, (20,), 5), (3, (20, 6), 5), (5, (20, 12, 9, 6), 5)]:
    for _bias in ("all", "none") if _depth == 1 else ("all", "none", "mixed01", "mixed10"):
        _case("depth%d_bias_%s" % (_depth, _bias), 1, nodes=_nodes, n_out=_out, bias=_bias)
_case("one_matrix_32_outputs", 1, nodes=(), n_out=32)
_case("one_matrix_33_outputs", 2, nodes=(), n_out=33)               # (no later layer: the outputs are layer 0, held to 32)
_case("one_matrix_identity_no_bias", 1, nodes=(), n_out=7, out="identity", bias="none")

# 2. width edges of route 1
for _h0, _route in [(1, 1), (31, 1), (32, 1), (33, 1), (63, 1), (64, 1), (65, 2)]:
    _case("h0_%d" % _h0, _route, nodes=(_h0, 6), bias="mixed10" if _h0 in (31, 63) else "all")
for _w, _route in [(1, 1), (3, 1), (5, 1), (9, 1), (31, 1), (32, 1), (33, 2)]:
    _case("later_%d" % _w, _route, nodes=(20, _w), bias="mixed01" if _w in (3, 9) else "all")
_case("later_32_then_31", 1, nodes=(40, 32, 31), n_out=6, bias="none")
_case("outputs_1", 1, n_out=1, out="identity")                       # (a softmax over one output is 1 whatever the kernel does)
for _c in (2, 7, 32):
    _case("outputs_%d" % _c, 1, n_out=_c)
_case("outputs_33", 2, n_out=33)

# 3. LDS limits: 512 x 32 and 256 x 64 floats are 64 KiB; 513 and 257 features pad to 528 and 272
_case("lds_h0_32_f512", 1, features=512, nodes=(32, 8), focal=(3, 500), grid=(-3.0, 3.0, 3), rows=257)
_case("lds_h0_32_f513", 2, features=513, nodes=(32, 8), focal=(3, 512), grid=(-3.0, 3.0, 3), rows=257)
_case("lds_h0_48_f256", 1, features=256, nodes=(48, 8), focal=(3, 255), grid=(-3.0, 3.0, 3), rows=257)
_case("lds_h0_48_f257", 2, features=257, nodes=(48, 8), focal=(3, 256), grid=(-3.0, 3.0, 3), rows=257)
# tails after H0 = 32 (two sets a launch): 32 -> 32 is 32 + 32 x 32 = 1056 floats, 32 -> 4 is 4 + 4 x 32 = 132
_case("lds_tail_3300", 1, nodes=(32, 32, 32, 32), n_out=4)         # 3 x 1056 + 132 = 3300 floats, 26 400 bytes for two sets
_case("lds_tail_4356", 2, nodes=(32, 32, 32, 32, 32), n_out=4)     # 4 x 1056 + 132 = 4356 floats, 34 848 bytes for two sets

# 4. activations at real width ("leaky": the leaky kernel without slopes, what a trainable ReLU selects)
for _nodes in [(33, 9), (16, 12, 6)]:
    for _tag, _kw in [("relu", dict(fun="ReLU")), ("leaky", dict(fun="ReLU", trainable=True)),
                      ("genrelu_shared", dict(fun="genReLU", slopes="shared")), ("genrelu_per_set", dict(fun="genReLU", slopes="per_set")),
                      ("swish", dict(fun="swish")), ("tanh", dict(fun="tanh"))]:
        _case("act_%s_%s" % (_tag, "x".join(map(str, _nodes))), 1, nodes=_nodes, sets=5, **_kw)

# 5. output side
for _tag, _kw in [("softmax", dict(out="softmax")), ("identity", dict(out="identity")), ("softplus_half_6", dict(out="softplus_half", n_out=6)),
                  ("softplus_half_5", dict(out="softplus_half", n_out=5))]:
    for _apply in (True, False):
        _case("out_%s_%s" % (_tag, "applied" if _apply else "raw"), 1, apply_out=_apply, **_kw)
_case("out_softplus_half_5_per_grid", 2, out="softplus_half", n_out=5, env=_PER_GRID)
_case("out_softplus_half_5_one_matrix", 1, out="softplus_half", n_out=5, nodes=())

# 6. rows and sets
for _rows in (1, 255, 256, 257, 2111):
    _case("rows_%d" % _rows, 1, rows=_rows)
for _sets in (1, 2, 3, 7):
    _case("sets_%d_two_a_launch" % _sets, 1, sets=_sets)                   # H0 = 20: two sets a launch
    _case("sets_%d_one_a_launch" % _sets, 1, sets=_sets, nodes=(40, 6))    # H0 = 40: one
_case("one_grid_point", 1, grid=(1.5, 1.5, 1))
_case("one_grid_point_per_grid", 2, grid=(1.5, 1.5, 1), env=_PER_GRID)
# an accumulator of one grid point (300 rows x 5 outputs x 4 bytes): three chunks, each of three launches of two, two and one set
_case("chunks_of_one_grid_point", 1, sets=5, grid=(-2.0, 2.0, 3), env=(("NPBNN_PDP_ACC_BYTES", str(300 * 5 * 4)),))
_case("chunks_of_one_grid_point_per_grid", 2, sets=5, grid=(-2.0, 2.0, 3), env=(("NPBNN_PDP_ACC_BYTES", str(300 * 5 * 4)),) + _PER_GRID)
_case("no_focal_column", 1, focal=(), grid=(0.0, 0.0, 2), override={5: 1.25, 17: -0.75}, pinned=True)
_case("no_focal_column_per_grid", 2, focal=(), grid=(0.0, 0.0, 2), override={5: 1.25, 17: -0.75}, pinned=True, env=_PER_GRID)

# 7. overrides (col_override applies after the grid values: on a focal column it wins)
_case("override_beside_focal", 1, override={5: 1.25, 17: -0.75})
_case("override_on_one_of_two_focal", 1, focal=(3, 9), override={9: 0.5, 17: -0.75})
_case("override_on_the_focal", 1, override={3: 0.5}, pinned=True)
_case("override_on_the_focal_per_grid", 2, override={3: 0.5}, pinned=True, env=_PER_GRID)
_case("override_on_one_of_two_focal_per_grid", 2, focal=(3, 9), override={9: 0.5, 17: -0.75}, env=_PER_GRID)
_case("all_columns_focal", 1, features=24, focal=tuple(range(24)), grid=(-1.0, 1.0, 3))

# 8. the test table, with another row count than the training table's
_case("test_table", 1, which=1, test_rows=173)
_case("test_table_one_a_launch", 1, which=1, test_rows=517, nodes=(40, 6))
_case("test_table_per_grid", 2, which=1, test_rows=173, env=_PER_GRID)
_case("test_table_streamed", 2, which=1, test_rows=173, env=_WIDE)

# 9. grid values far outside the data: a saturated first layer, a peaked softmax; both routes
_case("far_grid_tanh", 1, fun="tanh", grid=[-1e3, 0.5, 1e3], both_routes=True)
_case("far_grid_swish", 1, fun="swish", grid=[-1e3, 0.5, 1e3], both_routes=True)

# 10. a posterior of realistic size through the float32 sum over the sets
_case("many_sets", 1, rows=500, features=64, nodes=(32, 8), n_out=10, sets=300, grid=(-2.0, 2.0, 5), many_sets=True)
_case("many_sets_per_grid", 2, rows=500, features=64, nodes=(32, 8), n_out=10, sets=60, grid=(-2.0, 2.0, 5), many_sets=True, env=_PER_GRID)

# 11. route 2 under each layer-0 path
_case("per_grid_l0_f32", 2, env=_PER_GRID + (("NPBNN_L0", "f32"),), l0="f32")
_case("per_grid_l0_auto_lognormal", 2, x="lognormal3", grid=(0.1, 2000.0, 4), env=_PER_GRID, l0="f16-split")
_case("streamed_l0_f32", 2, env=_WIDE + (("NPBNN_L0", "f32"),), l0="f32")


def _bias_flags(pattern, n):
    return {"all": [1] * n, "none": [0] * n, "mixed01": [l % 2 for l in range(n)], "mixed10": [(l + 1) % 2 for l in range(n)]}[pattern]


def envelope_inputs(case):
    """The arrays of an ENVELOPE case: data and weights drawn as tests/test_hip_pdp.py's ``_drawn`` draws them (N(0, 1) features,
    N(0, 1 / sqrt(fan_in + 1)) weights: outputs of order 1), a bias column where the case's pattern has one."""
    rs = np.random.default_rng(case["seed"])
    f = case["features"]

    def table(n):
        return np.exp(3.0 * rs.standard_normal((n, f))) if case["x"] == "lognormal3" else rs.standard_normal((n, f))

    x = table(case["rows"])
    x_test = table(case["test_rows"]) if case["test_rows"] else None
    dims = [f] + list(case["nodes"]) + [case["n_out"]]
    flags = _bias_flags(case["bias"], len(dims) - 1)
    scale = [1.0 / np.sqrt(dims[i] + 1) for i in range(len(dims) - 1)]
    if case["x"] == "lognormal3":
        # Features of mean e^4.5 = 90: the first layer's weights are drawn 90 times smaller, so that its sums are of order 1 as on the
        # N(0, 1) table.  Drawn for unit features, they would have terms of several thousand cancel into the few hidden nodes that
        # are not saturated, and float32's rounding of one such term (2^-24 x 5000 = 3e-4) is past the absolute bar by itself.
        scale[0] /= np.exp(4.5)
    weights = [[rs.normal(0, scale[i], (dims[i + 1], dims[i] + flags[i])) for i in range(len(dims) - 1)] for _ in range(case["sets"])]
    n_hidden = len(case["nodes"])
    slopes = None
    if case["slopes"] == "shared":
        slopes = [rs.uniform(0.01, 0.5, n_hidden)] * case["sets"]
    elif case["slopes"] == "per_set":
        slopes = [rs.uniform(0.01, 0.5, n_hidden) for _ in range(case["sets"])]
    focal = list(case["focal"])
    g = case["grid"]
    points = np.asarray(g, dtype=float) if isinstance(g, list) else np.linspace(g[0], g[1], g[2])
    grid = np.empty((len(points), len(focal)))
    for k in range(len(focal)):          # (another value per focal column)
        grid[:, k] = points * (1.0 - 0.25 * k / max(len(focal), 1))
    override = None
    if case["override"]:
        override = np.full(f, np.nan)
        for col, value in case["override"].items():
            override[col] = value
    return dict(x=x, x_test=x_test, table=x_test if case["which"] == 1 else x, weights=weights, slopes=slopes, focal=focal, grid=grid,
                override=override)


OUT_FNS = {"softmax": orc.out_softmax, "identity": orc.out_identity, "softplus_half": orc.out_regress_error}


def envelope_oracle(case, inp, per_set=False, grid=True, override=True):
    """float64 reference of npbnn_predict_pdp for an ENVELOPE case, as tests/test_hip_pdp.py's ``oracle_means``: on the table the
    device holds (float32 entries), grid point by grid point the focal columns at the grid values, then ``col_override``'s columns at
    theirs, the oracle's forward pass and the case's output function (none when the case asks for the last layer's values), the mean
    over the sets [n_grid, rows, outputs] - or every set's own predictions [n_grid, sets, rows, outputs].  ``grid`` / ``override``
    False: without that step, for the guard's counterfactuals."""
    x = inp["table"].astype(np.float32).astype(np.float64)
    out_fn = OUT_FNS[case["out"]] if case["apply_out"] else orc.out_identity
    res = []
    for point in inp["grid"]:
        xg = np.array(x, copy=True)
        if grid and inp["focal"]:
            xg[:, inp["focal"]] = point
        if override and inp["override"] is not None:
            cols = ~np.isnan(inp["override"])
            xg[:, cols] = inp["override"][cols]
        preds = []
        for i, w in enumerate(inp["weights"]):
            act = orc.Act(case["fun"], prm=None if inp["slopes"] is None else np.asarray(inp["slopes"][i]), trainable=case["trainable"])
            preds.append(out_fn(orc.forward_logits(xg, w, act)))
        res.append(np.array(preds) if per_set else np.mean(preds, axis=0))
    return np.array(res)
