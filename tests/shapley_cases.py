"""Permutation-sampling Shapley attributions restated in float64 on the oracle's layers: phi by the same permutations, naively, with
one full forward pass per step (``walks``), phi by enumeration of all 2^n_players coalitions (``exact``), the six outputs of
npbnn_predict_shapley from either (``outputs``, ``reference``), a stand-in for the device seam of npbnn_amd.shapley (``oracle_seam``),
and the case table of npbnn_predict_shapley's two routes (CASES) with its inputs.  Route 1's envelope is npbnn_predict_pdp's
(tests/pdp_cases.py describes it); the tables and weights are drawn by its ``envelope_inputs``.

The outputs are continuous in the inputs - a ReLU's kink moves a prediction by a rounding error, not by a step - so no row is drawn
again near a kink.

``wrong=`` gives deliberately wrong variants for the guards of tests/test_host_shapley.py: "inverse_perm" reads a permutation as its
inverse, "no_reset" starts a walk where the previous one ended, "bias_column" moves layer 0's pre-activation by the column one to the
left of the right one where the layer has a bias column."""
import itertools
import math

import numpy as np

import oracle as orc
import pdp_cases
from attrib_common import _act, _apply_override, seam_to_oracle

# The error of an output array is max|device - float64| / max|float64| over the case.  Largest values measured on an MI355X over the
# 143 runs of tests/test_hip_shapley.py's cases on both routes (NOTES 8.14):
#   mean 1.91e-06  sq 1.01e-06  abs 9.32e-07  phi 1.83e-06   all four on streamed_20x700, route 2 (700 players: the longest walks);
#                                                            without that case mean 6.85e-07 (explain_1, route 1)
#   fx 2.92e-07 (act_swish_33x9)  base 1.83e-07 (out_softplus_half_5_raw), the same on both routes
# The bar is 26 times the largest of them.
TOL = 5e-5
# The efficiency identity on the device's own outputs, max|sum_p phi - (f(x_e) - mean_b f(b))| / max|f(x_e)|: it carries the float32
# drift of z0 over the walk's n_players updates against the direct pass.  Measured: 3.77e-07 on streamed_20x700 (700 players),
# 3.08e-07 at most on the cases of 40 players or fewer (out_softmax_raw), 2.26e-07 on config2_network (256): on these draws the
# drift does not grow visibly with the players.  The bar is 53 times the largest.
TOL_EFFICIENCY = 2e-5


def _out_fn(out, apply_out):
    return pdp_cases.OUT_FNS[out] if apply_out else orc.out_identity


def _from_z0(z0, w, act, out_fn):
    """the prediction from layer 0's pre-activation, on the oracle's layers"""
    if len(w) == 1:
        return out_fn(z0)
    tmp = orc.activate(np.array(z0, copy=True), act, 0)
    for i in range(1, len(w) - 1):
        tmp = orc.activate(orc.dense(tmp, w[i]), act, i)
    return out_fn(orc.dense(tmp, w[-1]))


def players_of(n_features, groups=None):
    """the players' column lists: ``groups``, or one player per column"""
    return [[j] for j in range(n_features)] if groups is None else [list(g) for g in groups]


def set_walks(xe, xb, w, act, out_fn, perms, players, wrong=None):
    """phi [E, P, C] of one weight set: the mean over the walks (b, pi), b-major, of the step that sets player pi[k].  Every walk
    takes its step k in the same forward pass over the stacked hybrid rows [walk, E, F]."""
    n_e, n_f, n_p = xe.shape[0], xe.shape[1], len(players)
    order = [np.argsort(pi) if wrong == "inverse_perm" else np.asarray(pi) for _ in xb for pi in perms]
    cur = np.stack([np.tile(b, (n_e, 1)) for b in xb for _ in perms])
    if wrong == "no_reset":
        cur[1:] = xe                     # (a walk ends at the explained row)
    n_w = len(order)

    def predict():
        if wrong == "bias_column":
            return _from_z0(z0.reshape(n_w * n_e, -1), w, act, out_fn).reshape(n_w, n_e, -1)
        return orc.forward(cur.reshape(n_w * n_e, n_f), w, act, out_fn).reshape(n_w, n_e, -1)

    if wrong == "bias_column":
        z0 = orc.dense(cur.reshape(n_w * n_e, n_f), w[0]).reshape(n_w, n_e, -1)
    prev = predict()
    phi = np.zeros((n_e, n_p, prev.shape[2]))
    for k in range(n_p):
        for i, pi in enumerate(order):
            cols = players[pi[k]]
            if wrong == "bias_column":
                # (with a bias column feature j's weights are column j + 1 of the matrix: column j is one to the left)
                for j in cols:
                    z0[i] += np.outer(xe[:, j] - cur[i][:, j], w[0][:, j])
            cur[i][:, cols] = xe[:, cols]
        y = predict()
        for i, pi in enumerate(order):
            phi[:, pi[k]] += y[i] - prev[i]
        prev = y
    return phi / n_w


def set_exact(xe, xb, w, act, out_fn, players):
    """phi [E, P, C] of one weight set: the interventional Shapley value over the background rows, by all 2^P coalitions"""
    n_p = len(players)
    assert n_p <= 10
    weight = [math.factorial(k) * math.factorial(n_p - k - 1) / math.factorial(n_p) for k in range(n_p)]
    phi = None
    for b in xb:
        value = {}
        for mask in itertools.product((0, 1), repeat=n_p):
            x = np.tile(b, (xe.shape[0], 1))
            for p in range(n_p):
                if mask[p]:
                    x[:, players[p]] = xe[:, players[p]]
            value[mask] = orc.forward(x, w, act, out_fn)
        if phi is None:
            phi = np.zeros((xe.shape[0], n_p, value[mask].shape[1]))
        for mask, v in value.items():
            for p in range(n_p):
                if not mask[p]:
                    phi[:, p] += weight[sum(mask)] * (value[mask[:p] + (1,) + mask[p + 1:]] - v)
    return phi / len(xb)


def walks(xe, xb, weights, perms, players, fun="tanh", out="softmax", slopes=None, override=None, apply_out=True, trainable=False,
          wrong=None, enumerate_all=False):
    """(phi [S, E, P, C], fx [S, E, C], fb [S, B, C]) on the explained rows ``xe`` and background rows ``xb`` after ``override``
    (NaN = none); ``enumerate_all``: phi by ``set_exact`` instead of the permutations"""
    xe, xb = _apply_override(xe, override), _apply_override(xb, override)
    out_fn = _out_fn(out, apply_out)
    phi, fx, fb = [], [], []
    for s, w in enumerate(weights):
        act = _act(fun, None if slopes is None else slopes[s], trainable)
        phi.append(set_exact(xe, xb, w, act, out_fn, players) if enumerate_all else set_walks(xe, xb, w, act, out_fn, perms, players, wrong))
        fx.append(orc.forward(xe, w, act, out_fn))
        fb.append(orc.forward(xb, w, act, out_fn))
    return np.array(phi), np.array(fx), np.array(fb)


def exact(xe, xb, weights, players, **kw):
    return walks(xe, xb, weights, None, players, enumerate_all=True, **kw)


NAMES = ("mean", "sq", "abs", "fx", "base", "phi")


def outputs(phi, fx, fb):
    """npbnn_predict_shapley's six outputs from every set's phi, f(x_e) and f(b)"""
    return dict(mean=phi.mean(axis=0), sq=(phi * phi).mean(axis=0), abs=np.abs(phi).mean(axis=1), fx=fx, base=fb.mean(axis=1), phi=phi)


def efficiency_gap(res):
    """[S, E, C] from phi, or [E, C] from the means over the sets: sum_p phi - (f(x_e) - mean_b f(b))"""
    if res.get("phi") is not None:
        return res["phi"].sum(axis=2) - (res["fx"] - res["base"][:, None, :])
    return res["mean"].sum(axis=1) - (res["fx"].mean(axis=0) - res["base"].mean(axis=0)[None, :])


def oracle_seam(data, rows, background_data, bg_rows, player_of, perms, weights, alphas, actFun, output_act_fun, data_transform, want_phi):
    """float64 stand-in for npbnn_amd.shapley._shapley_device: every sample with its own slopes, the feature indicators as an
    override."""
    fun, out, slopes, override = seam_to_oracle(alphas, actFun, output_act_fun, data_transform)
    data = np.asarray(data, dtype=np.float64)
    bg = data if background_data is None else np.asarray(background_data, dtype=np.float64)
    n_players = int(np.max(player_of)) + 1
    players = [np.flatnonzero(np.asarray(player_of) == p).tolist() for p in range(n_players)]
    res = outputs(*walks(data[np.asarray(rows)], bg[np.asarray(bg_rows)], weights, np.asarray(perms), players, fun=fun, out=out,
                         slopes=slopes, override=override))
    if not want_phi:
        res["phi"] = None
    return res


# ---- the cases of npbnn_predict_shapley (tests/test_hip_shapley.py on the GPU, tests/test_host_shapley.py's guards) ---------------------
#
# A case is one of tests/pdp_cases.py's envelope cases (same keys, same draw; its focal columns and grid are not used) with the keys
# of _SHAPLEY on top, one or two axes away from the defaults: the smallest shapes at which each part can go wrong.  ``route`` is what
# NPBNN_INFO_SHAPLEY_ROUTE must say.  ``reroute``: a route-1 case; each runs again on route 2 under NPBNN_SHAPLEY_PLAIN=1, on top of the case's own environment.
#   n_explain, repeats   explained rows drawn from the table, with ``repeats`` from its first 20 rows with replacement
#   n_bg, n_perm         background rows (drawn without replacement) and permutations
#   n_groups             None: a column is a player; else the columns, shuffled, cut into that many groups of uneven size
#   all_perms            every permutation of the players instead of n_perm drawn ones
#   bg_table             0: the backgrounds come from the training table whatever table ``which`` names
_SHAPLEY = dict(n_explain=70, repeats=False, n_bg=3, n_perm=4, n_groups=None, all_perms=False, bg_table=None)
CASES = {}
FORCED_WIDE = ("sets_3_two_a_launch", "explain_257", "players_33", "act_swish_16x12x6", "two_tables")


def _case(name, route, **kw):
    assert name not in CASES, name
    unknown = set(kw) - set(pdp_cases._DEFAULTS) - set(_SHAPLEY)
    assert not unknown, (name, unknown)
    CASES[name] = dict(pdp_cases._DEFAULTS, **dict(_SHAPLEY, name=name, route=route, seed=11000 + len(CASES),
                                                    reroute=route == 1, **kw))


# explained rows around a wave and a workgroup, and a row list with repeats
for _e in (1, 63, 64, 65, 255, 256, 257):
    _case("explain_%d" % _e, 1, n_explain=_e)
_case("explain_repeats", 1, repeats=True)
for _b in (1, 2, 5):
    _case("backgrounds_%d" % _b, 1, n_bg=_b)
for _p in (1, 2, 7):
    _case("permutations_%d" % _p, 1, n_perm=_p)
# players through groups of uneven size, and a player per column around 32 and 64 columns
for _g in (1, 2, 31, 32, 33):
    _case("players_%d" % _g, 1, n_groups=_g)
for _f in (31, 32, 33, 64, 65):
    _case("features_%d" % _f, 1, features=_f)
for _sets in (1, 2, 3, 7):
    _case("sets_%d_two_a_launch" % _sets, 1, sets=_sets)                   # H0 = 20: H0P = 32 (partial dependence runs two sets a launch)
    _case("sets_%d_one_a_launch" % _sets, 1, sets=_sets, nodes=(40, 6))    # H0 = 40: H0P = 64
# widths at the envelope's edges
_case("h0_64", 1, nodes=(64, 6))
_case("h0_65", 2, nodes=(65, 6))
_case("later_32", 1, nodes=(20, 32))
_case("later_33", 2, nodes=(20, 33))
_case("outputs_32", 1, n_out=32)
_case("outputs_33", 2, n_out=33)
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
# two overridden columns: their players must be exactly 0 - as players of their own, and as a group of the two
_case("override_two_columns", 1, override={5: 1.25, 17: -0.75}, pinned=True)
_case("override_grouped", 1, override={5: 1.25, 17: -0.75}, pinned=True, n_groups=6)      # (inputs() makes the two columns the first group)
# explained rows from the test table against backgrounds from the training table, and both from the test table
_case("two_tables", 1, which=1, test_rows=173, bg_table=0)
_case("test_table_alone", 1, which=1, test_rows=173)
# Scratch in chunks: two splits of the walks, chunks of one block of 64 rows, one set a launch (tests/test_host_attrib_plan.py asserts
# the cut these bytes give).
_case("scratch_in_chunks", 1, n_explain=257, env=(("NPBNN_SHAPLEY_SCRATCH_BYTES", "250000"),))
# route 2 on real shapes: a wide first layer, and the reference's default network where the library streams its weights by itself
_case("wide_130x40", 2, nodes=(130, 40))
_case("streamed_20x700", 2, rows=60, features=700, nodes=(50, 5), n_explain=20, n_bg=2, n_perm=2)
# config 2's network
_case("config2_network", 1, features=256, nodes=(32, 8), n_out=10, n_explain=300, n_bg=4, n_perm=4)
# all 24 permutations of 4 players: the exact Shapley value
_case("exact_4_players", 1, n_groups=4, all_perms=True)
# The turns of the plan's cut that nothing above takes; tests/test_host_attrib_plan.py asserts what each budget gives.  Route 2 with
# room for two units of partials and scratch: two splits, two chunks, one set a launch; and the sets_7 cases with three sets' blocks
# prepared at a time: groups of 3, 3 and 1 sets.
_case("route2_scratch_in_chunks", 2, nodes=(130, 40), env=(("NPBNN_SHAPLEY_SCRATCH_BYTES", "450000"),))
_case("sets_7_two_a_launch_in_groups", 1, sets=7, env=(("NPBNN_SHAPLEY_PREP_BYTES", str(3 * 7104)),))
_case("sets_7_one_a_launch_in_groups", 1, sets=7, nodes=(40, 6), env=(("NPBNN_SHAPLEY_PREP_BYTES", str(3 * 13760)),))


def inputs(case):
    """pdp_cases.envelope_inputs' arrays for the case, and from a generator of the case's own: ``rows`` and ``bg_rows`` (indices),
    ``groups`` (column lists or None), ``players``, ``player_of`` and ``perms`` [n_perm, P]; ``xe`` and ``xb``: the explained and the
    background rows as the device holds them (float32 entries)."""
    inp = pdp_cases.envelope_inputs(case)
    rs = np.random.default_rng(case["seed"] + 1)
    f = case["features"]
    table = inp["table"]
    bg_which = case["which"] if case["bg_table"] is None else case["bg_table"]
    bg_table = inp["x_test"] if bg_which == 1 else inp["x"]
    n = table.shape[0]
    if case["repeats"]:
        rows = rs.integers(0, min(20, n), case["n_explain"])
    else:
        rows = rs.choice(n, case["n_explain"], replace=case["n_explain"] > n)
    bg_rows = rs.choice(bg_table.shape[0], case["n_bg"], replace=False)
    groups = None
    if case["n_groups"] is not None:
        g = case["n_groups"]
        cols = rs.permutation(f)
        cuts = np.sort(rs.choice(np.arange(1, f), g - 1, replace=False)) if g > 1 else np.zeros(0, dtype=int)
        groups = [sorted(int(j) for j in part) for part in np.split(cols, cuts)]
        if case["override"]:
            # (the overridden columns form the first group, so that a group of overridden columns alone is covered)
            off = sorted(case["override"])
            groups = [off] + [h for h in ([j for j in grp if j not in off] for grp in groups) if h]
    players = players_of(f, groups)
    player_of = np.empty(f, dtype=np.int32)
    for p, cols in enumerate(players):
        player_of[cols] = p
    n_p = len(players)
    if case["all_perms"]:
        perms = np.array(list(itertools.permutations(range(n_p))), dtype=np.int32)
    else:
        perms = np.array([rs.permutation(n_p) for _ in range(case["n_perm"])], dtype=np.int32)
    held = lambda a: a.astype(np.float32).astype(np.float64)      # noqa: E731
    inp.update(rows=rows.astype(np.int64), bg_rows=bg_rows.astype(np.int64), bg_which=bg_which, groups=groups, players=players,
               player_of=player_of, perms=perms, xe=held(table[rows]), xb=held(bg_table[bg_rows]))
    return inp


def _kw(case, inp):
    return dict(fun=case["fun"], out=case["out"], slopes=inp["slopes"], override=inp["override"], apply_out=case["apply_out"],
                trainable=case["trainable"])


def reference(case, inp, wrong=None):
    """the six outputs of the case in float64 on the rows the device holds, by ``walks``"""
    return outputs(*walks(inp["xe"], inp["xb"], inp["weights"], inp["perms"], inp["players"], wrong=wrong, **_kw(case, inp)))


def reference_exact(case, inp):
    return outputs(*exact(inp["xe"], inp["xb"], inp["weights"], inp["players"], **_kw(case, inp)))


def relative_error(got, want):
    """max|got - want| / max|want|"""
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(want).max())
