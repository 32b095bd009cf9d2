"""The general device chain's envelope (CPU side; tests/test_hip_general_oracle.py runs the table on the GPU,
tests/test_host_general_envelope.py rehearses it on the float64 stand-in alone).

``HipContext.chain_run_general`` and ``OracleChainBackend.run_chain_general`` take the same explicit draws.  A case is a model
(table, network, likelihood, prior, walls, tempering, mask, indicators) and one or two batches of draws; ``log_u`` is planted by
``range_cases.plan_general`` a margin of MARGIN_FACTOR * LL_BAR * max(1, |logLik|) away from every accept statistic, so no
decision is a near-tie and no iteration is excused.  The accept patterns take 40% of a batch's iterations.

Layer sizes are ``out x (in + bias)``; the name of a tree case lists the sizes of its network's layers."""
import contextlib
import functools
import io

import numpy as np

import cases
import range_cases as rc
from range_cases import LL_BAR, MARGIN_FACTOR, plan_general          # noqa: F401  (the planner and its margin, re-exported)
from test_hip_chain_oracle import GENERIC, make_data

PROP_NORMAL, PROP_FIXED_NORMAL, PROP_NORMAL_NORMALIZED = 0, 2, 3
PRIOR_UNIFORM, PRIOR_NORMAL, PRIOR_CAUCHY, PRIOR_LAPLACE = 0, 1, 2, 3
ASSUMED_WG = 512               # rows of a workgroup where no GPU says (the CPU rehearsal of the "wg-1" / "wg+1" cases)

DEFAULTS = dict(
    lik="cat", n_out=3, rows=300, F=10, widths=(6, 4), bias=2, act="tanh", slopes=None,
    kind=PROP_NORMAL, M=31, step=0.05, start="normal",
    prior=PRIOR_NORMAL, scales=1.0, w_bound=np.inf, temperature=1.0, lik_temp=1.0,
    mask_blocks=0, wind=False, prior_ind1=0.5, find=False, ind_flips=None,
    sigma=None, class_w=False, inst_w=False, path="resident", l0="auto", batches=(16, 12))


def _case(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def _tree(**kw):
    """UpdateNormalNormalized from all-positive start weights exp(U(-14, 0)), normalised per layer, without walls."""
    return _case(kind=PROP_NORMAL_NORMALIZED, start="positive", **kw)


_BIG = dict(n_out=5, F=256, widths=(17, 6), bias=2, rows=200)          # layers 17 x 257 = 4369, 6 x 18 = 108, 5 x 6 = 30
_GAUSS = dict(lik="gauss", n_out=2, sigma="given")

CASES = {
    # ---- a. the pairwise tree: the summed layers' sizes ---------------------------------------------------------------------------
    "tree_8_3_1":         _tree(lik="gauss", n_out=1, sigma="given", F=3, widths=(2, 1), bias=2, rows=120),      # 2x4, 1x3, 1x1: 12 weights
    "tree_6_48_17":       _tree(lik="gauss", n_out=1, sigma="given", F=2, widths=(3, 16), bias=-1, rows=120),    # 3x2, 16x3, 1x17
    "tree_15_9_9":        _tree(n_out=3, F=4, widths=(3, 3), bias=1),                                            # 3x5, 3x3, 3x3
    "tree_56_16":         _tree(n_out=2, F=7, widths=(8,), bias=0),                                              # 8x7, 2x8
    "tree_124_128_128":   _tree(n_out=4, F=31, widths=(4, 32), bias=0),                                          # 4x31, 32x4, 4x32
    "tree_136_172_129":   _tree(n_out=3, F=33, widths=(4, 43), bias=1),                                          # 4x34, 43x4, 3x43
    "tree_130_260_130":   _tree(n_out=5, F=12, widths=(10, 26), bias=1),     # 10x13, 26x10, 5x26 (130, not 137: a prime needs 137 nodes)
    "tree_256_264_165":   _tree(n_out=5, F=32, widths=(8, 33), bias=0),                                          # 8x32, 33x8, 5x33
    "tree_1230_240_40":   _tree(n_out=5, F=40, widths=(30, 8), bias=1),                                          # 30x41, 8x30, 5x8
    "tree_4369_108_30":   _tree(**_BIG),
    "tree_masked":        _tree(n_out=5, F=12, widths=(8, 4), bias=2, mask_blocks=4),                            # 8x13 with zeros, 4x9, 5x5
    # ---- b. entry lists longer than the block (1024 threads) ----------------------------------------------------------------------
    "entries_m1025":      _case(M=1025, step=0.01, **_BIG),
    "entries_m2500":      _case(M=2500, step=0.01, **_BIG),
    "fixed_dups_m1300":   _case(kind=PROP_FIXED_NORMAL, M=1300, step=0.1, **_BIG),                 # drawn with replacement: h_cnt > cnt
    "wind_flips_big":     _case(wind=True, ind_flips={3: 0, 4: 1, 5: 1500}, **_BIG),               # layer 0 has 4369 indicators
    "find_flips_f1100":   _case(find=True, n_out=3, F=1100, widths=(8, 4), rows=200),              # 0, 1100 and 1 feature flips
    # ---- c. walls -------------------------------------------------------------------------------------------------------------------
    "walls_normal":       _case(w_bound=0.2, start="inside", step=0.15),
    "walls_fixed":        _case(kind=PROP_FIXED_NORMAL, w_bound=0.2, start="inside", step=0.15),
    # ---- d. priors and tempering ---------------------------------------------------------------------------------------------------
    "prior_uniform":      _case(prior=PRIOR_UNIFORM, scales=0.3, w_bound=0.3, start="inside", step=0.1),
    "prior_normal_layers": _case(scales="layers"),
    "prior_normal_per_weight": _case(scales="per_weight"),
    "prior_cauchy_fixed": _case(prior=PRIOR_CAUCHY, scales=0.7, kind=PROP_FIXED_NORMAL, w_bound=0.4, start="inside", step=0.3),
    "prior_cauchy_layers": _case(prior=PRIOR_CAUCHY, scales="layers"),
    "prior_laplace_per_weight": _case(prior=PRIOR_LAPLACE, scales="per_weight"),
    "prior_laplace_tree_masked": _tree(prior=PRIOR_LAPLACE, scales=0.5, n_out=5, F=12, widths=(8, 4), mask_blocks=4),
    "temperature_07":     _case(temperature=0.7),
    "lik_temp_06":        _case(lik_temp=0.6),
    "temperature_07_lik_temp_06": _case(temperature=0.7, lik_temp=0.6, kind=PROP_FIXED_NORMAL, step=0.1),
    "wind_prior_03":      _case(wind=True, prior_ind1=0.3, widths=(6, 5, 4)),
    # ---- e. likelihoods --------------------------------------------------------------------------------------------------------------
    "cat_class_weights":  _case(class_w=True, wind=True, widths=(6, 5, 4)),
    "cat_instance_weights": _case(inst_w=True),
    "gauss_empirical":    _case(lik="gauss", n_out=2, sigma="empirical"),
    "gauss_given":        _case(lik="gauss", n_out=2, sigma="given", lik_temp=0.6),
    "gauss_multipliers":  _case(lik="gauss", n_out=2, sigma="mult", temperature=0.7),
    "err_mti1":           _case(lik="err", n_out=8, F=16, widths=(20, 6)),
    "err_mti8":           _case(lik="err", n_out=8, F=16, widths=(20, 40)),
    "pois_mti1":          _case(lik="pois", n_out=1, F=16, widths=(20, 6)),
    "pois_mti8":          _case(lik="pois", n_out=1, F=16, widths=(20, 40)),
    "nb_mti1":            _case(lik="nb", n_out=2, F=16, widths=(20, 6)),
    "nb_mti8":            _case(lik="nb", n_out=2, F=16, widths=(20, 40)),
    # ---- f. feature indicators -------------------------------------------------------------------------------------------------------
    "find_f1_bias":       _case(find=True, F=1, widths=(4, 3), bias=2),
    "find_f15_nobias":    _case(find=True, F=15, bias=0),
    "find_f17_bias":      _case(find=True, F=17, bias=2, kind=PROP_FIXED_NORMAL, step=0.1),
    "find_f40_nobias":    _case(find=True, F=40, bias=-1, n_out=5),
    "find_wind_four":     _case(find=True, wind=True, widths=(6, 5, 4), prior_ind1=0.4),
    "find_gauss_nobias":  _case(find=True, F=15, bias=0, lik="gauss", n_out=2, sigma="mult"),
    "find_streamed":      _case(find=True, F=40, bias=0, n_out=5, path="streamed"),
    "find_streamed_bias": _case(find=True, F=17, bias=2, path="streamed"),
    "find_f32":           _case(find=True, F=17, bias=0, l0="f32"),
    # ---- g. shapes ---------------------------------------------------------------------------------------------------------------------
    "rows_1":             _case(rows=1, F=16, widths=(20, 5), **_GAUSS),
    "rows_15":            _case(rows=15, F=16, widths=(20, 5)),
    "rows_17":            _case(rows=17, F=16, widths=(20, 5), lik="gauss", n_out=2, sigma="empirical"),
    "rows_wg_minus_1":    _case(rows="wg-1", F=16, widths=(20, 5)),
    "rows_wg_plus_1":     _case(rows="wg+1", F=16, widths=(20, 5), lik="gauss", n_out=2, sigma="empirical"),
    "eight_matrices":     _case(widths=(6, 5, 7, 4, 6, 5, 4), bias=3, kind=PROP_FIXED_NORMAL, step=0.1),
    "eight_matrices_tree": _tree(widths=(6, 5, 7, 4, 6, 5, 4), bias=3),
    "bias_last_only":     _case(bias=-1),
    "act_relu":           _case(act="ReLU"),
    "act_swish":          _case(act="swish", bias=1),
    "act_genrelu_fixed":  _case(act="genReLU", slopes=(0.1, 0.3)),
    "act_genrelu_fixed_gauss": _case(act="genReLU", slopes=(0.25, 0.05), lik="gauss", n_out=2, sigma="empirical"),
    # ---- h. the weight-streamed path (NPBNN_FORCE_WIDE) ----------------------------------------------------------------------------
    "streamed_normal":    _case(path="streamed", F=40, widths=(16, 5), n_out=5, w_bound=0.25, start="inside", step=0.15),
    "streamed_fixed":     _case(path="streamed", F=40, widths=(16, 5), n_out=5, kind=PROP_FIXED_NORMAL, step=0.1),
    "streamed_tree_656_85_25": _tree(path="streamed", F=40, widths=(16, 5), n_out=5),              # 16x41, 5x17, 5x5
    "streamed_wind":      _case(path="streamed", F=40, widths=(16, 5, 5), n_out=5, wind=True, prior_ind1=0.3),
}


def f32(x):
    return rc.f32(x)


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **k)


def seed_of(name):
    return 500 + 7 * sorted(CASES).index(name)


def layer_shapes(c):
    return cases.layer_shapes(c["F"], list(c["widths"]), c["n_out"], c["bias"])


def layer_sizes(c):
    return [int(np.prod(s)) for s in layer_shapes(c)]


def rows_of(c, wg=None):
    if c["rows"] == "wg-1":
        return (wg or ASSUMED_WG) - 1
    if c["rows"] == "wg+1":
        return (wg or ASSUMED_WG) + 1
    return c["rows"]


def _likelihood_f(lik):
    from npbnn_amd import likelihoods as L
    return {"cat": L.calc_likelihood, "gauss": L.calc_likelihood_regression, "err": L.calc_likelihood_regression_error,
            "pois": L.poi_likelihood, "nb": L.negbin_likelihood}[lik]


def _table(c, rows, seed):
    if c["lik"] == "cat":
        dat = cases.classification_data(seed, max(rows, c["n_out"]), c["F"], c["n_out"])
        dat["data"], dat["labels"] = f32(dat["data"][:rows]), dat["labels"][:rows]
        dat["test_data"] = f32(dat["test_data"])
        return dat
    k = {"gauss": c["n_out"], "err": GENERIC["err"]}.get(c["lik"], 2)
    return make_data(c["lik"], rows, c["F"], seed=seed, k=k)


def _start_weights(c, rs):
    shapes = layer_shapes(c)
    if c["start"] == "positive":
        w = [np.exp(rs.uniform(-14, 0, s)) for s in shapes]
        return [a / np.sum(a) for a in w]
    if c["start"] == "inside":                     # (no start weight outside the walls: the sampler keeps such chains on mh_step)
        return [rs.uniform(-0.9 * c["w_bound"], 0.9 * c["w_bound"], s) for s in shapes]
    return [rs.normal(0, 0.1, s) for s in shapes]


def _prior_scale(c, shapes, rs):
    n = len(shapes)
    if c["scales"] == "layers":
        return np.array([0.5, 1.0, 2.0, 0.8, 1.5, 0.6, 1.2, 0.9][:n])
    if c["scales"] == "per_weight":                # (hyper_p = 3: a scale per weight)
        return [rs.uniform(0.5, 2.0, s) for s in shapes]
    return np.full(n, float(c["scales"]))


def make_problem(name, wg=None):
    """Model of one case: the npBNN (what HipBackend and the stand-in are built from) and, in range_cases' form, its table,
    start weights, mask, prior scales and chain settings."""
    import npbnn_amd as bn
    c = CASES[name]
    seed = seed_of(name)
    rows = rows_of(c, wg)
    rs = np.random.default_rng(seed + 1000)
    dat = _table(c, rows, seed)
    w = _start_weights(c, rs)
    act = bn.ActFun(fun=c["act"]) if c["slopes"] is None else bn.ActFun(fun=c["act"], prm=np.array(c["slopes"], dtype=float))
    extra = {"cat": {}, "gauss": dict(estimation_mode="regression"),
             "err": dict(estimation_mode="regression-error", output_act_fun=bn.RegressTransformError),
             "pois": dict(estimation_mode="custom", size_output=1), "nb": dict(estimation_mode="custom", size_output=2)}[c["lik"]]
    if c["inst_w"]:
        extra["instance_weights"] = rs.uniform(0.2, 2.0, rows)
    bnn = quiet(bn.npBNN, dat, n_nodes=list(c["widths"]), use_bias_node=c["bias"], actFun=act, init_weights=w, prior_f=c["prior"],
                p_scale=1, w_bound=c["w_bound"], use_class_weights=1 if c["class_w"] else 0, seed=seed, **extra)
    assert [a.shape for a in bnn._w_layers] == [tuple(s) for s in layer_shapes(c)]
    if c["lik"] == "cat":
        assert bnn._size_output == c["n_out"]
    mask = None
    if c["mask_blocks"]:
        mask = rc.block_mask(w, c["F"], c["mask_blocks"])
        quiet(bnn.apply_mask, mask)
        w = bnn._w_layers
    shapes = [a.shape for a in w]
    chain = dict(prior_kind=c["prior"], w_bound=c["w_bound"], temperature=c["temperature"], lik_temp=c["lik_temp"], prior_ind1=c["prior_ind1"])
    if c["sigma"] == "given":
        chain["sigma"] = np.array([0.8, 1.3, 1.1, 0.9][:c["n_out"]])
    if c["slopes"] is not None:
        chain["fixed_slopes"] = act.device_slopes(len(c["widths"]), accepted=True)
    return dict(name=name, case=c, lik=c["lik"], x=dat["data"], labels=bnn._labels, w=w, shapes=shapes, mask=mask, n_out=c["n_out"],
                prior_scale=_prior_scale(c, shapes, rs), chain=chain, feature_means=np.mean(dat["data"], axis=0), bnn=bnn,
                lik_f=_likelihood_f(c["lik"]), out_kind={"cat": 0, "err": 2}.get(c["lik"], 1))


def standin(p, layer_sum=None):
    """The float64 stand-in of the device chain on this model (``layer_sum``: what the normalising proposal divides by, in place
    of np.sum)."""
    import oracle_backend
    be = oracle_backend.OracleChainBackend(p["bnn"], out_kind=p["out_kind"])
    be._lik_f = p["lik_f"]
    if layer_sum is not None:
        be._layer_sum = layer_sum
    return be


def start_state(p, be, rs):
    """Four in five weight indicators 1, two in three feature indicators 1 (at least one 0: while ``find_use`` is 0 the override
    must not apply to it); log-likelihood (without override), prior and sigma of that state in float64."""
    import oracle as orc
    c, ch = p["case"], p["chain"]
    ind = (rs.random(p["shapes"][0]) < 0.8).astype(float) if c["wind"] else None
    find = None
    if c["find"]:
        find = (rs.random(c["F"]) < 2.0 / 3.0).astype(float)
        find[int(rs.integers(c["F"]))] = 0.0
    fw = p["w"] if ind is None else [p["w"][0] * ind] + list(p["w"][1:])
    sigma = ch.get("sigma")
    if c["sigma"] == "mult":
        sigma = np.ones(c["n_out"])
    with np.errstate(over="ignore"):
        r = be.evaluate(fw, slopes=ch.get("fixed_slopes"), lik_temp=ch["lik_temp"], sigma=sigma)
    lp = orc.log_prior(p["w"], ch["prior_kind"], p["prior_scale"])
    if ind is not None:
        n_on = np.sum(ind)
        lp = lp + (n_on * np.log(ch["prior_ind1"]) + (ind.size - n_on) * np.log(1 - ch["prior_ind1"]))
    return dict(w=p["w"], ll=r["loglik"], lp=lp, ind=None if ind is None else ind.ravel(), find=find, sigma=r["sigma"])


def switch_of(K):
    """The first iteration of a first batch at which the feature indicators' override applies."""
    return K // 3


def draw_case(p, rs, K, first, find0=None):
    """The draws of one batch, independent of the chain's state, in the form MCMC._draw_general hands them over.  Iteration 1
    proposes in every layer, iteration 2 in none (cnt 0), iteration 0 fills its row of ``idx`` as far as the layers allow; the
    others propose in a random set of layers, 1 to M entries.  The fixed-normal proposal draws positions with replacement: every
    draw goes into the Hastings list, the last one of a position into ``idx``.  Weight indicators: three iterations in ten flip
    indicators and leave layer 0's weights alone (``ind_flips``: {iteration: how many positions}).  Feature indicators: in a first
    batch the override applies from ``switch_of(K)`` on - that iteration flips the zeros of the start state ``find0`` (every
    indicator 1: no column overridden; the pattern accepts it), the next flips every feature (every column overridden), the one
    after one feature - in a later batch from the start."""
    c = p["case"]
    sizes = [int(np.prod(s)) for s in p["shapes"]]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    L, kind, M = len(sizes), c["kind"], c["M"]
    fixed = kind == PROP_FIXED_NORMAL
    idx = np.full((K, M), -1, dtype=np.int32)
    val = np.zeros((K, M))
    cnt = np.zeros(K, dtype=np.int32)
    h_idx, h_val, h_fac, h_cnt = (np.full((K, M), -1, dtype=np.int32), np.zeros((K, M)), np.zeros((K, M)), np.zeros(K, dtype=np.int32)) \
        if fixed else (None, None, None, None)
    layer_mask = np.zeros(K, dtype=np.int32)
    ind_ptr, ind_pos = np.zeros(K + 1, dtype=np.int32), []
    find_ptr, find_pos, find_use = np.zeros(K + 1, dtype=np.int32), [], np.zeros(K, dtype=np.int32)
    forced_flips = (c["ind_flips"] or {}) if first else {}
    sw = switch_of(K) if first else 0
    for t in range(K):
        layers = [l for l in range(L) if rs.random() < 0.6] or [int(rs.integers(L))]
        if t in (0, 1):
            layers = list(range(L))
        if t == 2:
            layers = []
        if c["wind"] and t > 2 and (t in forced_flips or rs.random() < 0.3):
            layers = [l for l in layers if l > 0]
            n_flip = forced_flips.get(t, int(rs.integers(1, max(2, sizes[0] // 20))))
            ind_pos.extend(np.sort(rs.choice(sizes[0], n_flip, replace=False)).tolist())
        ind_ptr[t + 1] = len(ind_pos)
        if c["find"] and t >= sw:
            find_use[t] = 1
            n_flip = int(rs.integers(1, c["F"] // 2 + 2)) if rs.random() < 0.5 else 0
            if first and t == sw:
                find_pos.extend(np.flatnonzero(find0 == 0).tolist())
            else:
                n_flip = {sw + 1: c["F"], sw + 2: 1}.get(t, n_flip) if first else n_flip
                find_pos.extend(np.sort(rs.choice(c["F"], n_flip, replace=False)).tolist())
        find_ptr[t + 1] = len(find_pos)
        pool = np.concatenate([np.arange(offs[l], offs[l + 1]) for l in layers]) if layers else np.zeros(0, dtype=np.int64)
        if len(pool) == 0:
            continue
        for l in layers:
            layer_mask[t] |= 1 << l
        n = M if t == 0 else int(rs.integers(1, M + 1))
        layer_of = lambda pos: np.searchsorted(offs, pos, side="right") - 1          # noqa: E731
        if fixed:
            drawn = rs.choice(pool, n, replace=True)
            z = rs.normal(0, c["step"], n)
            h_idx[t, :n], h_val[t, :n], h_fac[t, :n], h_cnt[t] = drawn, z, 0.5 / c["step"] ** 2, n
            _, last = np.unique(drawn[::-1], return_index=True)          # (numpy's indexed assignment keeps the LAST draw)
            keep = np.sort(n - 1 - last)
            sel, v = drawn[keep], z[keep]
        else:
            n = min(n, len(pool))
            sel = np.sort(rs.choice(pool, n, replace=False))
            v = rs.normal(0, c["step"], n)
            if kind == PROP_NORMAL_NORMALIZED:        # (a layer's weights sum to 1: steps of a fifth of the mean weight)
                v = v / c["step"] * 0.2 / np.array(sizes)[layer_of(sel)]
        cnt[t] = len(sel)
        idx[t, :len(sel)], val[t, :len(sel)] = sel, v
    g = dict(kind=kind, idx=idx, val=val, cnt=cnt, layer_mask=layer_mask, h_idx=h_idx, h_val=h_val, h_fac=h_fac, h_cnt=h_cnt)
    if c["wind"]:
        g.update(ind_ptr=ind_ptr, ind_pos=np.array(ind_pos, dtype=np.int32))
    if c["find"]:
        g.update(find_ptr=find_ptr, find_pos=np.array(find_pos, dtype=np.int32), find_use=find_use)
    if c["sigma"] == "mult":                   # multiplier_proposal_vector(q, d=1.1, f=0.5) and its Hastings term
        chosen = rs.binomial(1, 0.5, (K, c["n_out"]))
        sm = np.exp(2 * np.log(1.1) * (rs.random((K, c["n_out"])) - .5))
        sm[chosen == 0] = 1.
        g.update(sigma_mult=sm, hastings=np.sum(np.log(sm), axis=1))
    return g


def pattern_for(rs, K):
    """Two iterations in five accepted, three in five rejected."""
    return rs.permutation(K) < int(np.ceil(0.4 * K))


class Watch:
    """What the planner's walk sees of a batch: how many proposed values passed the upper and the lower wall, and the feature
    indicators every iteration was proposed from."""

    def __init__(self, p, g):
        self.p, self.g, self.hi, self.lo, self.find = p, g, 0, 0, []

    def __call__(self, t, state):
        g, wb = self.g, self.p["chain"]["w_bound"]
        n = g["cnt"][t]
        if g["kind"] != PROP_NORMAL_NORMALIZED and n:
            v = g["val"][t, :n] if g["kind"] == PROP_FIXED_NORMAL else rc.pack(state["w"])[g["idx"][t, :n]] + g["val"][t, :n]
            self.hi += int(np.sum(v > wb))
            self.lo += int(np.sum(v < -wb))
        self.find.append(None if state.get("find") is None else np.array(state["find"]))


@functools.lru_cache(maxsize=None)
def scenario(name, wg=None):
    """Model and planned batches of one case; built once, shared, never changed.  ``wg``: a workgroup's rows (the GPU's answer,
    for the cases whose row count depends on it)."""
    c = CASES[name]
    p = make_problem(name, wg)
    rs = np.random.default_rng(seed_of(name) + 5)
    be = standin(p)
    state = start_state(p, be, rs)
    out = []
    for j, K in enumerate(c["batches"]):
        b = dict(K=K, draws=draw_case(p, rs, K, j == 0, state["find"]), pattern=pattern_for(rs, K), start=state)
        if c["find"] and j == 0 and not b["pattern"][switch_of(K)]:          # (the iteration that switches every feature on is accepted)
            other = int(np.flatnonzero(b["pattern"])[0])
            b["pattern"][[other, switch_of(K)]] = False, True
        watch = Watch(p, b["draws"])
        b["log_u"], b["stat"], b["margin"] = plan_general(p, be, state, b["draws"], b["pattern"], observe=watch)
        b["reflected"], b["find_seen"] = (watch.hi, watch.lo), watch.find
        b["want"] = rc.run_standin_general(p, b, be)
        w = b["want"]
        state = dict(w=rc.unpack(w["w"], p["shapes"]), ll=w["ll"], lp=w["lp"], ind=w["ind"], find=w["find"], sigma=w["sigma"])
        out.append(b)
    return dict(name=name, case=c, p=p, batches=out)


# ---- what the table covers, computed from the draws ------------------------------------------------------------------------------

def summed_sizes(sc):
    """Sizes of the layers some iteration's ``layer_mask`` selects (normalising cases)."""
    sizes = [int(np.prod(s)) for s in sc["p"]["shapes"]]
    out = set()
    if sc["case"]["kind"] == PROP_NORMAL_NORMALIZED:
        for b in sc["batches"]:
            for m in b["draws"]["layer_mask"]:
                out |= {sizes[l] for l in range(len(sizes)) if (m >> l) & 1}
    return out


# ---- wrong sums: what a kernel that got numpy's pairwise tree wrong would divide by ----------------------------------------------

def sum_left_to_right(a):
    return np.cumsum(np.ravel(a))[-1]


def sum_eight_accumulators(a):
    """numpy's unrolled block sum applied to the whole array: eight accumulators and the remainder, without the halving."""
    a = np.ravel(a)
    n = len(a)
    if n < 8:
        return np.cumsum(a)[-1]
    m = n - n % 8
    r = np.cumsum(a[:m].reshape(-1, 8), axis=0)[-1]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[m:]:
        res += v
    return res


def numpy_tree_sum(a):
    """A plain restatement of numpy's pairwise summation (what the kernel's numpy_sum restates)."""
    a = np.ravel(a)
    n = len(a)
    if n <= 128:
        return sum_eight_accumulators(a) if n >= 8 else (np.cumsum(a)[-1] if n else 0.0)
    n2 = n // 2
    n2 -= n2 % 8
    return numpy_tree_sum(a[:n2]) + numpy_tree_sum(a[n2:])
