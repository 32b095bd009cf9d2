"""Planted fp16-range batches for the device chains (CPU side; tests/test_hip_chain_f16_range.py runs them on the GPU and
tests/test_host_chain_f16_range.py checks this module without one).

``HipContext.chain_run`` and the float64 stand-in ``OracleChainBackend.run_chain`` take the same explicit draws
``(idx, delta, cnt, log_u)``.  A scenario is a short sequence of batches on one tanh network: a clean batch, the planted batch -
iteration ``t*`` adds PLANT to one layer-0 weight of a feature column, which puts the scaled weight far outside fp16 - and two
clean batches after it.  ``log_u`` is not drawn: the batch is walked in float64 (``plan_batch``), and at every iteration
``log_u[t]`` is put a margin ``m = MARGIN_FACTOR * LL_BAR * max(1, |logLik|)`` below the accept statistic where the pattern says
accept and the same margin above it where it says reject (|logLik|: the larger of the current and the proposed one).  Every
decision of a batch is then 100 of the project's float32 log-likelihood bars away from the threshold: no iteration is excused.

The accept patterns take roughly one iteration in six (a seeded Generator).  Over a scenario there are at least two accepts
before ``t*`` and one after it; where ``t*`` is the first or the last iteration of its batch those lie in the clean batches on
either side, else inside the planted batch itself."""
import functools
import types

import numpy as np

import cases
import oracle as orc
from test_hip_chain_oracle import LL_RTOL as LL_BAR          # the project's float32 log-likelihood bar (2e-6)

MARGIN_FACTOR = 100.0
PLANT = 3e5                    # what the evaluation and replay tests plant (fp16's largest finite number: 65504)
F16_MAX = 65504.0
N_FEATURES = 40
PRIOR_NORMAL = 1
ACT = orc.Act("tanh")

# name -> lik, hidden widths, rows, iterations of the planted batch, t* ("first" / "mid" / "last"), is the planted proposal
# accepted, slot (0: no placement; 1 / 2: with three candidates per pass the planted candidate sits in that slot of a pass whose
# slot 0 is accepted - prepared, flagged and dropped), blocks of a block-structured first layer
VARIANTS = {
    "first_rejected":  dict(lik="cat", widths=(16, 5), rows=37, K=24, pos="first", accept=False, slot=0, mask_blocks=0),
    "first_accepted":  dict(lik="cat", widths=(16, 5), rows=300, K=24, pos="first", accept=True, slot=0, mask_blocks=0),
    "mid_rejected":    dict(lik="cat", widths=(32, 8), rows=641, K=40, pos="mid", accept=False, slot=0, mask_blocks=0),
    "mid_accepted":    dict(lik="cat", widths=(32, 8), rows=1025, K=40, pos="mid", accept=True, slot=0, mask_blocks=0),
    "last_rejected":   dict(lik="cat", widths=(16, 5), rows=300, K=33, pos="last", accept=False, slot=0, mask_blocks=0),
    "last_accepted":   dict(lik="cat", widths=(32, 8), rows=37, K=40, pos="last", accept=True, slot=0, mask_blocks=0),
    "slot1_rejected":  dict(lik="cat", widths=(16, 5), rows=641, K=30, pos="mid", accept=False, slot=1, mask_blocks=0),
    "slot2_accepted":  dict(lik="cat", widths=(16, 5), rows=1025, K=30, pos="mid", accept=True, slot=2, mask_blocks=0),
    "masked_rejected": dict(lik="cat", widths=(16, 5), rows=300, K=36, pos="mid", accept=False, slot=0, mask_blocks=4),
    "gauss_rejected":  dict(lik="gauss", widths=(16, 5), rows=641, K=40, pos="mid", accept=False, slot=0, mask_blocks=0),
}
CLEAN_K = (20, 24, 16)         # the clean batch before the planted one, and the two after it


def f32(x):
    """Data the device holds exactly (test_hip_chain_oracle._f32)."""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def pack(layers):
    return np.concatenate([np.asarray(w, dtype=np.float64).ravel() for w in layers])


def unpack(v, shapes):
    out, off = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(v[off:off + n].reshape(s))
        off += n
    return out


def block_mask(layers, n_features, blocks):
    """The block-structured first layer test_hip_chain_oracle.make_chain builds: that many equal blocks of inputs, each feeding
    its own share of the first layer's nodes."""
    import npbnn_amd as bn
    w0 = layers[0].shape[0]
    per = [w0 // blocks] * blocks
    per[-1] += w0 - sum(per)
    return bn.create_mask(layers, indx_input_list=[list(np.repeat(np.arange(blocks), n_features // blocks))] + [[]] * (len(layers) - 1),
                          nodes_per_feature_list=[per] + [[]] * (len(layers) - 1))


def make_problem(lik, rows, widths, seed, mask_blocks=0, n_out=None, scale_column=None):
    """Table, labels and N(0, 0.1) start weights (bias in column 0 of every matrix) of a tanh network with hidden layers
    ``widths``.  ``scale_column``: (column, factor) - an unstandardised feature column."""
    if lik == "cat":
        n_out = n_out or 5
        dat = cases.classification_data(seed, max(rows, 5), N_FEATURES, n_out)
        x, labels = f32(dat["data"][:rows]), np.asarray(dat["labels"][:rows])
    else:
        n_out = n_out or 2
        dat = cases.regression_data(seed, rows, N_FEATURES, n_out)
        x, labels = f32(dat["data"]), f32(dat["labels"])
    if scale_column is not None:
        x[:, scale_column[0]] *= scale_column[1]
    rs = np.random.default_rng(seed + 1000)
    dims = [N_FEATURES] + list(widths) + [n_out]
    w = [rs.normal(0, 0.1, (dims[i + 1], dims[i] + 1)) for i in range(len(dims) - 1)]
    mask = None
    if mask_blocks:
        mask = block_mask(w, N_FEATURES, mask_blocks)
        w = [a * m for a, m in zip(w, mask)]
    return dict(lik=lik, x=x, labels=labels, w=w, shapes=[a.shape for a in w], mask=mask, n_out=n_out,
                prior_scale=np.ones(len(w)))


def standin(p, cls=None):
    """The float64 stand-in of the device chain on this problem's table."""
    import oracle_backend
    empty = np.zeros((0, N_FEATURES))
    bnn = types.SimpleNamespace(_data=p["x"], _labels=p["labels"], _test_data=empty, _test_labels=np.zeros(0),
                                _estimation_mode="classification" if p["lik"] == "cat" else "regression",
                                _act_fun=types.SimpleNamespace(_function="tanh", _trainable=False), _instance_weights=None,
                                _class_w=[])
    return (cls or oracle_backend.OracleChainBackend)(bnn, out_kind=0 if p["lik"] == "cat" else 1)


def loglik(p, layers, sigma=None):
    with np.errstate(over="ignore"):         # (the oracle's tanh of a planted pre-activation: exp overflows to inf, the result is 1)
        z = orc.forward_logits(p["x"], layers, ACT)
    if p["lik"] == "cat":
        return orc.lik_categorical(orc.out_softmax(z), p["labels"], np.arange(len(p["x"])))
    return orc.lik_gaussian(orc.out_identity(z), p["labels"], None, sig2=sigma)


def start_state(p):
    sigma = np.ones(p["n_out"]) if p["lik"] == "gauss" else None
    return dict(w=p["w"], ll=loglik(p, p["w"], sigma), lp=orc.log_prior(p["w"], PRIOR_NORMAL, p["prior_scale"]), sigma=sigma)


def plant_index(p, rs):
    """A layer-0 weight of a feature column (not the bias, column 0) that the mask keeps and whose column holds an |x| >= 1."""
    rows_, cols_ = p["shapes"][0]
    ok = np.ones((rows_, cols_), dtype=bool) if p["mask"] is None else p["mask"][0] != 0
    ok[:, 0] = False
    ok[:, 1:] &= (np.max(np.abs(p["x"]), axis=0) >= 1.0)[None, :]
    flat = np.flatnonzero(ok.ravel())
    return int(flat[rs.integers(len(flat))])


def draw_batch(p, rs, K, t_star=None, plant=None, plant_deltas=None):
    """Ordinary iterations: 5 to 30 weights moved by N(0, 0.05); ``t_star``: that iteration also adds PLANT to weight ``plant``
    (``plant_deltas``: {iteration: what it adds to that weight} instead)."""
    plant_deltas = plant_deltas if plant_deltas is not None else ({} if t_star is None else {t_star: PLANT})
    n_w = sum(int(np.prod(s)) for s in p["shapes"])
    M = 31
    idx = np.full((K, M), -1, dtype=np.int32)
    delta = np.zeros((K, M))
    cnt = rs.integers(5, 31, K).astype(np.int32)
    for t in range(K):
        pool = n_w if t not in plant_deltas else n_w - 1
        sel = np.sort(rs.choice(pool, cnt[t], replace=False))
        d = rs.normal(0, 0.05, cnt[t])
        if t in plant_deltas:
            sel = np.where(sel >= plant, sel + 1, sel)          # (never the planted weight itself)
            sel, d = np.append(sel, plant), np.append(d, plant_deltas[t])
            order = np.argsort(sel)
            sel, d = sel[order], d[order]
            cnt[t] += 1
        idx[t, :cnt[t]], delta[t, :cnt[t]] = sel, d
    sm = h = None
    if p["lik"] == "gauss":                                      # multiplier_proposal_vector(q, d=1.1, f=0.5) and its Hastings term
        chosen = rs.binomial(1, 0.5, (K, p["n_out"]))
        sm = np.exp(2 * np.log(1.1) * (rs.random((K, p["n_out"])) - .5))
        sm[chosen == 0] = 1.
        h = np.sum(np.log(sm), axis=1)
    return dict(idx=idx, delta=delta, cnt=cnt, sigma_mult=sm, hastings=h, K=K, t_star=t_star, plant=plant)


def t_star_of(v):
    return {"first": 0, "mid": v["K"] // 2, "last": v["K"] - 1}[v["pos"]]


def pattern_for(rs, K, t_star=None, accept=False, slot=0, pos="mid"):
    pat = rs.random(K) < 1.0 / 6.0
    if t_star is None:
        if pat.sum() < 2:              # (a clean batch: at least two accepts)
            pat[rs.choice(K, 2, replace=False)] = True
        return pat
    if pos == "mid":
        if pat[:t_star].sum() < 2:
            pat[rs.choice(t_star, 2, replace=False)] = True
        if not pat[t_star + 1:].any():
            pat[t_star + 1 + rs.integers(K - t_star - 1)] = True
    if slot:          # two accepts in a row: the second opens a pass and is its slot 0; the planted candidate follows in ``slot``
        pat[t_star - slot - 1:t_star] = False
        pat[t_star - slot - 1] = pat[t_star - slot] = True
    pat[t_star] = accept
    return pat


def pass_slots(pattern, d):
    """(first iteration of its pass, slot) of every iteration's deciding pass and, per pass, the candidates it prepared:
    a pass of ``d`` candidates, all proposed from the same state, ends at its first accepted one; the next begins behind that."""
    K = len(pattern)
    decided, prepared, t = {}, [], 0
    while t < K:
        cand = list(range(t, min(t + d, K)))
        prepared.append(cand)
        n = len(cand)
        for s, c in enumerate(cand):
            decided[c] = (t, s)
            if pattern[c]:
                n = s + 1
                break
        t += n
    return decided, prepared


def plan_batch(p, state, b, pattern):
    """Walk the batch in float64 and build ``log_u``; returns (log_u, accept statistics, margins, proposed logLik, state after)."""
    K = b["K"]
    temperature = b.get("temperature", 1.0)
    cur = pack(state["w"])
    m_flat = None if p["mask"] is None else pack(p["mask"])
    ll, lp, sig = state["ll"], state["lp"], state["sigma"]
    log_u, stat, margin, llp = np.zeros(K), np.zeros(K), np.zeros(K), np.zeros(K)
    b["watch_cur"], b["watch_prop"] = np.zeros(K), np.zeros(K)         # the planted weight before and in every proposal
    for t in range(K):
        prop = cur.copy()
        sel = b["idx"][t, :b["cnt"][t]]
        prop[sel] = cur[sel] + b["delta"][t, :b["cnt"][t]]
        if m_flat is not None:
            prop = prop * m_flat
        if b.get("plant") is not None:
            b["watch_cur"][t], b["watch_prop"][t] = cur[b["plant"]], prop[b["plant"]]
        wl = unpack(prop, p["shapes"])
        s_t = None if sig is None else sig * b["sigma_mult"][t]
        h = 0.0 if sig is None else b["hastings"][t]
        llp[t] = loglik(p, wl, s_t)
        lpp = orc.log_prior(wl, PRIOR_NORMAL, p["prior_scale"])
        stat[t] = ((llp[t] + lpp) - (ll + lp)) * temperature + h
        margin[t] = MARGIN_FACTOR * LL_BAR * max(1.0, abs(ll), abs(llp[t]))
        log_u[t] = stat[t] - margin[t] if pattern[t] else stat[t] + margin[t]
        if pattern[t]:
            cur, ll, lp, sig = prop, llp[t], lpp, s_t
    return log_u, stat, margin, llp, dict(w=unpack(cur, p["shapes"]), ll=ll, lp=lp, sigma=sig)


def chain_kwargs(p, b):
    """What HipContext.chain_run and OracleChainBackend.run_chain take for batch ``b`` beside the weights."""
    s = b["start"]
    return dict(idx=b["idx"], delta=b["delta"], cnt=b["cnt"], log_u=b["log_u"], prior_kind=PRIOR_NORMAL, prior_scale=p["prior_scale"],
                w_bound=np.inf, temperature=b.get("temperature", 1.0), lik_temp=1.0, cur_loglik=s["ll"], cur_logprior=s["lp"],
                cur_sigma=s["sigma"], sigma=None, mask=p["mask"], sigma_mult=b["sigma_mult"], hastings=b["hastings"])


def run_standin(p, b, be=None):
    """The batch on the float64 stand-in: dict(w, acc, llp, lpp, ll, lp, sigma)."""
    be = be or standin(p)
    with np.errstate(over="ignore"):
        w, acc, llp, lpp, res = be.run_chain(b["start"]["w"], **chain_kwargs(p, b))
    return dict(w=np.array(w), acc=acc, llp=llp, lpp=lpp, ll=res["loglik"], lp=res["logprior"], sigma=res["sigma"])


def build_batches(p, seed, specs, state=None, temperature=1.0):
    """``specs``: (K, t* or None, planted weight, accept, slot, pos) per batch, walked one after the other from ``state``; every
    batch carries its start state, its pattern, the walk's figures and what the stand-in returns (``want``)."""
    rs = np.random.default_rng(seed)
    state = state or start_state(p)
    be = standin(p)
    out = []
    for K, t_star, plant, accept, slot, pos in specs:
        b = draw_batch(p, rs, K, t_star, plant)
        b["temperature"] = temperature
        b["pattern"] = pattern_for(rs, K, t_star, accept, slot, pos)
        b["start"] = state
        b["log_u"], b["stat"], b["margin"], b["llp_walk"], after = plan_batch(p, state, b, b["pattern"])
        b["want"] = run_standin(p, b, be)
        state = dict(w=unpack(b["want"]["w"], p["shapes"]), ll=b["want"]["ll"], lp=b["want"]["lp"], sigma=b["want"]["sigma"])
        b["after_walk"] = after
        out.append(b)
    return out


@functools.lru_cache(maxsize=None)
def scenario(name):
    """Problem and batches (clean, planted, clean, clean) of one variant; built once, shared, never changed."""
    v = VARIANTS[name]
    seed = 40 + sorted(VARIANTS).index(name)
    p = make_problem(v["lik"], v["rows"], v["widths"], seed, v["mask_blocks"])
    plant = plant_index(p, np.random.default_rng(seed + 7))
    specs = [(CLEAN_K[0], None, None, False, 0, None), (v["K"], t_star_of(v), plant, v["accept"], v["slot"], v["pos"]),
             (CLEAN_K[1], None, None, False, 0, None), (CLEAN_K[2], None, None, False, 0, None)]
    return dict(name=name, variant=v, p=p, plant=plant, batches=build_batches(p, seed + 13, specs))


# ---- a candidate that is out of range only as long as it is dropped -------------------------------------------------------------

DROPPED_T = 10                 # iteration DROPPED_T - 1 and DROPPED_T are accepted: DROPPED_T opens a pass, DROPPED_T + 1 sits in its slot 1


def dropped_only_batch(p, plant, threshold, seed=123):
    """A batch whose float64 chain never proposes a weight outside the fp16 range ``threshold`` - and whose second candidate of
    one three-candidate pass does: iteration DROPPED_T (slot 0, accepted) takes the planted weight down by half the threshold,
    iteration DROPPED_T + 1 adds 1.05 of it.  Proposed beside slot 0, from the state before it, that candidate is out of range;
    proposed again from the state slot 0 left, it is at 0.55 of the threshold."""
    rs = np.random.default_rng(seed)
    K = 24
    b = draw_batch(p, rs, K, None, plant, {DROPPED_T: -0.5 * threshold, DROPPED_T + 1: 1.05 * threshold})
    pat = pattern_for(rs, K)
    pat[DROPPED_T - 1:DROPPED_T + 4] = [True, True, False, False, False]
    b["pattern"], b["start"], b["temperature"] = pat, start_state(p), 1.0
    b["log_u"], b["stat"], b["margin"], b["llp_walk"], b["after_walk"] = plan_batch(p, b["start"], b, pat)
    b["want"] = run_standin(p, b)
    return b


# ---- which launch runs which variant ------------------------------------------------------------------------------------------

SCHEDULES = (1, 2, 4, 5)       # serial, overlapped, persistent, persistent with the decision between the passes


def effective_schedule(name, d, schedule, path):
    """The schedule the library runs when ``schedule`` is asked for by number (npbnn_sched_choose, npbnn_sched_plan.h;
    tests/test_host_sched_plan.py holds the rule itself to this function for every run of ``direct_runs``): the
    weight-streamed path patches its candidate image between step and pass and runs on kernel boundaries (1) whatever is asked;
    schedule 5 needs a build with the speculative step - there are such builds for one and three candidates of a dense first
    layer - and falls back to the persistent overlapped form (4) elsewhere; 1, 2, 3 and 4 run as asked on a GPU the chain has to
    itself."""
    if path == "streamed":
        return 1
    if schedule == 5 and (d == 2 or VARIANTS[name]["mask_blocks"]):
        return 4
    return schedule


def direct_runs():
    """(variant, n_candidates, schedule, path) of every direct-entry run.  Resident: two per variant, the schedules 1, 2, 4, 5
    and the candidate counts round-robin - a run on schedule 5 with one or three candidates, so that it is schedule 5 that
    runs - the slot variants once with three candidates, the two-stream schedule 3 once.  Weight-streamed (kernel boundaries
    only): one per variant, candidate counts round-robin."""
    runs = []
    for i, name in enumerate(VARIANTS):
        for r in (0, 1):
            schedule = SCHEDULES[(2 * i + r) % 4]
            d = (i + r) % 3 + 1
            if (VARIANTS[name]["slot"] and r == 1) or (schedule == 5 and d == 2):
                d = 3
            runs.append((name, d, schedule, "resident"))
    runs.append(("mid_rejected", 2, 3, "resident"))
    for i, name in enumerate(VARIANTS):
        runs.append((name, i % 3 + 1, 1, "streamed"))
    return runs


# ---- planted draws behind a sampler (the exchange run takes its draws from the chains) -------------------------------------------

def problem_of(bnn, lik="cat"):
    """The problem of an npBNN (its table, labels, weights, prior scales) in this module's form."""
    w = [np.array(a, dtype=np.float64) for a in bnn._w_layers]
    return dict(lik=lik, x=np.asarray(bnn._data, dtype=np.float64), labels=np.asarray(bnn._labels), w=w, shapes=[a.shape for a in w],
                mask=None, n_out=w[-1].shape[0], prior_scale=bnn._prior_scale)


class _Served:
    saved = None
    queued = False

    def __init__(self, value):
        self.value = value

    def result(self):
        return self.value


def serve_draws(mcmc, b):
    """Make the chain take the draws of batch ``b`` (iterations 0 .. K-1 of the chain) wherever it asks for pre-drawn numbers -
    an exchange run, a device batch of run_steps - instead of drawing them: what MCMC._claim_draw / _submit_draw hand out.
    (A test seam on the sampler's private pre-draw pipeline, npbnn_amd/sampler.py: ``_claim_draw`` returns a job whose
    ``result()`` is (idx, delta, cnt, log u, sigma multipliers, Hastings terms); ``_submit_draw`` returns what
    ``MCMC._speculation`` holds - (key, job, may the draw be taken back, the step-size arrays it was made with) - and
    ``_cancel_speculation`` reads ``job.saved``.  A change of that layout has to be followed here.)"""
    def claim(bnn_obj, first_it, k):
        a, e = int(first_it), int(first_it) + int(k)
        assert e <= b["K"], "the planted draws end at iteration %d" % b["K"]
        return _Served((b["idx"][a:e], b["delta"][a:e], b["cnt"][a:e], b["log_u"][a:e].copy(), None, None))

    def submit(bnn_obj, first_it, k, rewindable=False):
        k = max(0, min(int(k), b["K"] - int(first_it)))
        return (("served", int(first_it), k), claim(bnn_obj, first_it, k), False, mcmc._update_ws)
    mcmc._claim_draw, mcmc._submit_draw = claim, submit


# ---- the sampler's walk to the threshold ----------------------------------------------------------------------------------------

SAMPLER_COLUMN, SAMPLER_FACTOR = 3, 2.0 ** 12
SAMPLER_ROWS, SAMPLER_WIDTHS = 300, [16, 5]
SAMPLER_WEIGHT = (0, SAMPLER_COLUMN + 1)          # layer-0 entry [node 0, feature column 3] (the bias is column 0)
SAMPLER_UPDATE_WS = [0.5, 0.075, 0.075]           # layer 0 steps wide enough to cross the threshold from 0.98 of it
# the kept dispatch (FastBatch) is built after two equal calls, runs the third, and - after it failed - is held back for 16 calls:
# built after calls 1-2, fails in call 3 (iterations 40-59), built again after call 19, runs call 20
SAMPLER_DISPATCHES = (20,) * 3 + (40,) * 18
# the fp16 pair holds |w * s| <= 60000 with s a power of two per column: the thresholds the scaled column can have
SAMPLER_THRESHOLDS = tuple(60000.0 / 2.0 ** k for k in (13, 14, 15))


def sampler_data():
    """The sampler case's table: one column multiplied by 2^12 (unstandardised), so that the fp16 threshold of its weights is a
    few units."""
    dat = cases.classification_data(71, SAMPLER_ROWS, N_FEATURES, 5)
    dat["data"] = f32(dat["data"])
    dat["data"][:, SAMPLER_COLUMN] *= SAMPLER_FACTOR
    dat["test_data"] = f32(dat["test_data"])
    return dat


def sampler_weights(bn, value):
    np.random.seed(4321)
    w = bn.init_weight_prm(SAMPLER_WIDTHS, N_FEATURES, 5, init_std=0.1, bias_node=2)
    w[0][SAMPLER_WEIGHT] = value
    return w


def sampler_chain(bn, dat, threshold):
    """npBNN + MCMC whose watched layer-0 weight starts at 0.98 of ``threshold``."""
    import contextlib
    import io
    np.random.seed(1234)
    with contextlib.redirect_stdout(io.StringIO()):
        bnn = bn.npBNN(dat, n_nodes=list(SAMPLER_WIDTHS), actFun=bn.ActFun(fun="tanh"), use_bias_node=2, prior_f=1, p_scale=1, seed=1234,
                       init_weights=sampler_weights(bn, 0.98 * threshold))
    return bnn, bn.MCMC(bnn, update_f=[0.05] * 3, update_ws=list(SAMPLER_UPDATE_WS), n_iteration=100000)


def recording_backend(record):
    """The stand-in, noting the watched weight of every candidate it evaluates for the chain."""
    import oracle_backend

    class Recording(oracle_backend.OracleChainBackend):
        def _chain_evaluate(self, weights, *a, **k):
            record.append(float(weights[0][SAMPLER_WEIGHT]))
            return super()._chain_evaluate(weights, *a, **k)
    return Recording


# ---- the general device chain (npbnn_chain_run_general) --------------------------------------------------------------------------

PROP_NORMAL, PROP_FIXED_NORMAL = 0, 2
# the fixed-normal proposal (drawn values replace the weights, a Hastings term over every draw) on the categorical network, and
# UpdateNormal with weight indicators (some iterations flip indicators of layer 0 and move later layers only) on four matrices
GENERAL = {
    "fixed_normal":      dict(kind=PROP_FIXED_NORMAL, widths=(16, 5), rows=300, indicators=False, accept=False),
    "normal_indicators": dict(kind=PROP_NORMAL, widths=(16, 5, 5), rows=641, indicators=True, accept=True),
}
GENERAL_WIDTH = 0.1            # the fixed-normal proposal's width (the start weights' own)
PRIOR_IND1 = 0.5


def draw_general(p, rs, K, kind, ind_shape=None, t_star=None, plant=None):
    sizes = [int(np.prod(s)) for s in p["shapes"]]
    n_w = sum(sizes)
    M = 31
    idx = np.full((K, M), -1, dtype=np.int32)
    val = np.zeros((K, M))
    cnt = rs.integers(5, 31, K).astype(np.int32)
    ind_ptr, ind_pos = np.zeros(K + 1, dtype=np.int32), []
    for t in range(K):
        flip = ind_shape is not None and t != t_star and rs.random() < 0.3
        lo = sizes[0] if flip else 0              # (an iteration that flips indicators leaves layer 0's weights alone)
        pool = n_w - lo - (1 if t == t_star else 0)
        sel = lo + np.sort(rs.choice(pool, cnt[t], replace=False))
        v = rs.normal(0, GENERAL_WIDTH if kind == PROP_FIXED_NORMAL else 0.05, cnt[t])
        if t == t_star:
            sel = np.where(sel >= plant, sel + 1, sel)
            sel, v = np.append(sel, plant), np.append(v, PLANT)
            order = np.argsort(sel)
            sel, v = sel[order], v[order]
            cnt[t] += 1
        idx[t, :cnt[t]], val[t, :cnt[t]] = sel, v
        if flip:
            ind_pos.extend(np.flatnonzero(rs.random(int(np.prod(ind_shape))) < 0.02).tolist())
        ind_ptr[t + 1] = len(ind_pos)
    g = dict(kind=kind, idx=idx, val=val, cnt=cnt, layer_mask=np.zeros(K, dtype=np.int32), h_idx=None, h_val=None, h_fac=None, h_cnt=None)
    if kind == PROP_FIXED_NORMAL:
        g.update(h_idx=idx.copy(), h_val=val.copy(), h_fac=np.full((K, M), 0.5 / GENERAL_WIDTH ** 2), h_cnt=cnt.copy())
    if ind_shape is not None:
        g.update(ind_ptr=ind_ptr, ind_pos=np.array(ind_pos, dtype=np.int32))
    return g


def slice_general(g, a, b):
    out = dict(g)
    for key in ("idx", "val", "cnt", "layer_mask", "h_idx", "h_val", "h_fac", "h_cnt", "find_use", "sigma_mult", "hastings"):
        if g.get(key) is not None:
            out[key] = g[key][a:b]
    for ptr_key, pos_key in (("ind_ptr", "ind_pos"), ("find_ptr", "find_pos")):
        if ptr_key in g:
            ptr = g[ptr_key][a:b + 1]
            out[ptr_key], out[pos_key] = ptr - ptr[0], g[pos_key][ptr[0]:ptr[-1]]
    return out


def general_kwargs(p, b):
    """What HipContext.chain_run_general and OracleChainBackend.run_chain_general take for batch ``b``.  The chain's settings are
    ``p["chain"]`` where the problem has one (tests/general_cases.py: prior, walls, tempering, a given sigma, fixed slopes) and
    the normal prior at temperature 1 without walls where it has none; the sigma multipliers and their Hastings terms travel
    with the draws; feature indicators and the current sigma with the state."""
    s, c, g = b["start"], p.get("chain", {}), b["draws"]
    kw = dict(draws=g, log_u=b["log_u"], mask=p["mask"], indicators=s["ind"], prior_ind1=c.get("prior_ind1", PRIOR_IND1),
              has_indicator_prior=s["ind"] is not None, prior_kind=c.get("prior_kind", PRIOR_NORMAL), prior_scale=p["prior_scale"],
              w_bound=c.get("w_bound", np.inf), temperature=c.get("temperature", 1.0), lik_temp=c.get("lik_temp", 1.0),
              cur_loglik=s["ll"], cur_logprior=s["lp"])
    if s.get("find") is not None:
        kw.update(feature_indicators=s["find"], feature_means=p["feature_means"])
    if s.get("sigma") is not None:
        kw["cur_sigma"] = s["sigma"]
    if c.get("sigma") is not None:
        kw["sigma"] = c["sigma"]
    if g.get("sigma_mult") is not None:
        kw.update(sigma_mult=g["sigma_mult"], hastings=g["hastings"])
    if c.get("fixed_slopes") is not None:
        kw["fixed_slopes"] = c["fixed_slopes"]
    return kw


def _general_step(be, p, state, g, t, log_u):
    b = dict(start=state, draws=slice_general(g, t, t + 1), log_u=np.array([log_u]))
    kw = general_kwargs(p, b)
    with np.errstate(over="ignore"):
        return be.run_chain_general(state["w"], **kw), kw


def state_after(p, out, res):
    """The chain's state as the next batch's start: what run_chain_general returned (weights, indicators, feature indicators)
    and its result dict."""
    w, ind, find = out[0], out[1], out[2]
    return dict(w=unpack(np.asarray(w), p["shapes"]), ll=res["loglik"], lp=res["logprior"], ind=ind, find=find, sigma=res["sigma"])


def plan_general(p, be, state, g, pattern, observe=None):
    """plan_batch for the general chain: every iteration is proposed once on the stand-in with a bar nothing passes (its proposed
    log values give the accept statistic) and, where the pattern accepts, once more with a bar everything passes.
    ``observe(t, state)`` sees the state every iteration is proposed from."""
    import scipy.stats
    K = len(pattern)
    log_u, stat, margin = np.zeros(K), np.zeros(K), np.zeros(K)
    for t in range(K):
        if observe is not None:
            observe(t, state)
        (_, _, _, acc, llp, lpp, _), kw = _general_step(be, p, state, g, t, np.inf)
        assert not acc[0]
        h = 0.0 if kw.get("hastings") is None else kw["hastings"][0]
        if g["kind"] == PROP_FIXED_NORMAL:
            n = g["h_cnt"][t]
            dd = np.sqrt(0.5 / g["h_fac"][t, :n])
            cur = pack(state["w"])
            h += np.sum(scipy.stats.norm.logpdf(cur[g["h_idx"][t, :n]], 0, dd) - scipy.stats.norm.logpdf(g["h_val"][t, :n], 0, dd))
        stat[t] = ((llp[0] + lpp[0]) - (state["ll"] + state["lp"])) * kw["temperature"] + h
        margin[t] = MARGIN_FACTOR * LL_BAR * max(1.0, abs(state["ll"]), abs(llp[0]))
        log_u[t] = stat[t] - margin[t] if pattern[t] else stat[t] + margin[t]
        if pattern[t]:
            out, _ = _general_step(be, p, state, g, t, -np.inf)
            assert out[3][0]
            state = state_after(p, out, out[6])
    return log_u, stat, margin


def run_standin_general(p, b, be):
    with np.errstate(over="ignore"):
        w, ind, find, acc, llp, lpp, res = be.run_chain_general(b["start"]["w"], **general_kwargs(p, b))
    return dict(w=np.array(w), ind=ind, find=find, acc=acc, llp=llp, lpp=lpp, ll=res["loglik"], lp=res["logprior"], sigma=res["sigma"])


@functools.lru_cache(maxsize=None)
def general_scenario(name):
    """Clean batch, planted batch (t* in the middle), clean batch on the general chain."""
    v = GENERAL[name]
    seed = 90 + sorted(GENERAL).index(name)
    p = make_problem("cat", v["rows"], v["widths"], seed)
    rs = np.random.default_rng(seed + 5)
    be = standin(p)
    ind = None
    state = start_state(p)
    if v["indicators"]:
        ind = (rs.random(p["shapes"][0]) < 0.8).astype(float)
        ll = loglik(p, [p["w"][0] * ind] + p["w"][1:])
        state = dict(w=p["w"], ll=ll, lp=state["lp"] + ind.size * np.log(PRIOR_IND1), sigma=None)
    state["ind"] = None if ind is None else ind.ravel()
    while True:            # a feature column's weight whose indicator is 1
        plant = plant_index(p, rs)
        if ind is None or ind.ravel()[plant] == 1:
            break
    out = []
    for K, t_star in ((20, None), (30, 15), (20, None)):
        b = dict(K=K, t_star=t_star, draws=draw_general(p, rs, K, v["kind"], None if ind is None else ind.shape, t_star, plant))
        b["pattern"] = pattern_for(rs, K, t_star, v["accept"], 0, "mid")
        b["start"] = state
        b["log_u"], b["stat"], b["margin"] = plan_general(p, be, state, b["draws"], b["pattern"])
        b["want"] = run_standin_general(p, b, be)
        w = b["want"]
        state = dict(w=unpack(w["w"], p["shapes"]), ll=w["ll"], lp=w["lp"], ind=w["ind"], sigma=None)
        out.append(b)
    return dict(name=name, variant=v, p=p, plant=plant, batches=out)
