"""GPU: the device chain's fast builds held to the float64 oracle.

The speculative passes (2 and 3 candidates per read of X), the five schedules, the fast-tail and outcome-speculative builds, the
group pass, the exchange run and the weight-streamed path were each tested only against another HIP path.  Here every one of them
runs a chain in short dispatches (7 to 40 iterations), and after every dispatch the state the chain says it holds is recomputed in
float64 from the host's weights (``check_state``):

  * ``_logLik`` to 2e-6 relative at every width (only last-layer values widen beyond 1024 features);
  * ``_logPrior`` to 1e-12;
  * the training (and test) accuracy to 1e-4, float32 near-ties of the top two outputs excused as test_hip_parity.check_confusion does.

This holds whatever the trajectory does.  Where the trajectory can be compared too, the same seeded chain also runs on the float64
stand-in (tests/oracle_backend.py, through ``npbnn_amd.sampler._make_backend``), and the two must share their first 150 accept /
reject decisions, or all of them.

CASES names the eval_kernel build (npbnn_eval_inst_*.hip) each resident case is meant to reach, by its template arguments
(MTI, D, LK, FAST, SPEC, CHAIN, BLK, MT0); tests/test_host_eval_builds.py checks on CPU that the table claims every build the
instantiation files emit.  Each case asserts what the library reports about the launch it ran (INFO_FAST_TAILS, INFO_L0_F16, the
schedule used, fewer passes than iterations for more than one candidate)."""
import contextlib
import io

import numpy as np
import pytest
import scipy.special

import cases
import oracle as orc

pytestmark = pytest.mark.gpu

LL_RTOL = 2e-6
LP_RTOL = 1e-12
ACC_TOL = 1e-4
COMMON = 150

# likelihood class of a build (npbnn::lik_class): 0 categorical, 1 Gaussian, 2 float64 row-wise (Poisson here)
LIK_OF_LK = {0: "cat", 1: "gauss", 2: "pois"}
# every likelihood the float64 row-wise (LK 2, "generic") builds serve: kind -> target columns
GENERIC = {"pois": 1, "nb": 1, "nb10": 1, "nb2d": 3, "err": 4}


def _group(mti, d, lk, fast, spec, chain, mt0s, blk_mt0s=()):
    """The builds of one npbnn_eval_inst_*.hip file: (MTI, D, LK, FAST, SPEC, CHAIN, BLK, MT0) for every MT0 it emits."""
    return ([(mti, d, lk, fast, spec, chain, 0, m) for m in mt0s] +
            [(mti, d, lk, fast, spec, chain, 1, m) for m in blk_mt0s])


_ALL = range(1, 9)
# (one line per instantiation file; CHAIN 0: the plain-evaluation builds, which npbnn_eval - mh_step - runs)
BUILDS = (_group(1, 1, 0, 0, 0, 1, _ALL) + _group(1, 1, 1, 0, 0, 1, _ALL) + _group(1, 1, 2, 0, 0, 1, _ALL)            # d1_cat, d1_gauss, d1_gen
          + _group(1, 2, 0, 0, 0, 1, _ALL) + _group(1, 2, 1, 0, 0, 1, _ALL)                                           # d2_cat, d2_gauss
          + _group(1, 3, 0, 0, 0, 1, (1, 2)) + _group(1, 3, 1, 0, 0, 1, (1, 2))                                       # d3_cat, d3_gauss
          + _group(8, 1, 0, 0, 0, 1, _ALL) + _group(8, 1, 1, 0, 0, 1, _ALL) + _group(8, 1, 2, 0, 0, 1, _ALL)         # mti8_cat, _gauss, _gen
          + _group(1, 1, 0, 1, 0, 1, (1, 2, 3, 4), (2, 3, 4)) + _group(1, 1, 1, 1, 0, 1, (1, 2, 3, 4), (2, 3, 4))   # d1_cat_fast, d1_gauss_fast
          + _group(1, 2, 0, 1, 0, 1, (1, 2, 3, 4), (2, 3, 4)) + _group(1, 2, 1, 1, 0, 1, (1, 2, 3, 4), (2, 3, 4))   # d2_cat_fast, d2_gauss_fast
          + _group(1, 3, 0, 1, 0, 1, (1, 2), (2,)) + _group(1, 3, 1, 1, 0, 1, (1, 2), (2,))                         # d3_cat_fast, d3_gauss_fast
          + _group(1, 1, 0, 1, 0, 0, (1, 2, 3, 4), (2, 3, 4)) + _group(1, 1, 1, 1, 0, 0, (1, 2, 3, 4), (2, 3, 4))   # d1_*_plain
          + _group(1, 1, 0, 1, 1, 1, (1, 2, 3, 4)) + _group(1, 1, 1, 1, 1, 1, (1, 2, 3, 4))                         # d1_*_spec
          + _group(1, 3, 0, 1, 1, 1, (1, 2)) + _group(1, 3, 1, 1, 1, 1, (1, 2)))                                    # d3_*_spec

# Builds an instantiation file emits that no launch can select: (build, the dispatch rule that excludes it).  None today.
UNREACHABLE = []

_ROWS = (37, 300, 641, 1025)           # under a tile, a few tiles, odd counts
_SCHEDS = (1, 2, 4, 0, 3)              # serial, overlapped, persistent, library's choice, two-stream


def _case(i, key):
    mti, d, lk, fast, spec, chain, blk, mt0 = key
    return dict(key=key, lik=LIK_OF_LK[lk], d=d, fast=fast, mti=mti, mt0=mt0, blk=blk,
                advance="run_steps" if chain else "mh_step",
                schedules=(5, 5) if spec else (_SCHEDS[i % len(_SCHEDS)], _SCHEDS[(i + 2) % len(_SCHEDS)]),
                l0="auto" if (blk or i % 2) else "f32",
                rows=_ROWS[i % len(_ROWS)])


# one row per build: what the resident-chain test runs to reach it
CASES = [_case(i, key) for i, key in enumerate(BUILDS)]


def _case_id(c):
    mti, d, lk, fast, spec, chain, blk, mt0 = c["key"]
    return "mti%d_d%d_%s%s%s%s%s_mt0%d" % (mti, d, c["lik"], "_fast" if fast else "", "_spec" if spec else "",
                                           "" if chain else "_plain", "_blk" if blk else "", mt0)


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **k)


def _f32(x):
    """Data the device holds exactly: the oracle sees the same numbers as the kernels."""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def heavy_tailed(kind, rs, n, f):
    if kind == "outlier":           # one 1e4 outlier per column over N(0, 1e-2) data (test_hip_parity._heavy_tailed)
        x = rs.normal(0, 1e-2, (n, f))
        x[rs.integers(0, n, f), np.arange(f)] = 1e4
    elif kind == "lognormal3":      # log-normal columns, sigma = 3
        x = np.exp(3.0 * rs.standard_normal((n, f)))
    else:
        x = rs.standard_normal((n, f))
    return x


def make_data(lik, n, f, n_test=0, seed=5, x_kind="normal", k=2):
    if lik == "cat":
        dat = cases.classification_data(seed, max(n, 5), f, 5, n_test)      # (it labels its first rows 0..4)
        dat["data"], dat["labels"] = dat["data"][:n], dat["labels"][:n]
    elif lik == "gauss":
        dat = cases.regression_data(seed, n, f, k, n_test)
    elif lik == "err":
        dat = cases.regression_data(seed, n, f, GENERIC["err"], n_test)
    elif lik == "nb2d":                 # three count columns, each with its own log-mean
        rs = np.random.default_rng(seed)
        x = rs.standard_normal((n + n_test, f))
        eta = 0.8 + x[:, :3] @ np.array([[0.5, -0.2, 0.1], [-0.4, 0.3, 0.2], [0.3, 0.1, -0.5]])
        y = rs.poisson(np.exp(eta)).astype(float)
        dat = dict(data=x[:n], labels=y[:n], test_data=x[n:], test_labels=y[n:])
    else:
        dat = cases.count_data(seed, n, f, n_test)
    if x_kind != "normal":
        rs = np.random.default_rng(seed + 99)
        x = heavy_tailed(x_kind, rs, n + n_test, f)
        dat["data"], dat["test_data"] = x[:n], x[n:]
    for key in ("data", "test_data"):
        dat[key] = _f32(dat[key])
    if lik != "cat":
        dat["labels"], dat["test_labels"] = _f32(dat["labels"]), _f32(dat["test_labels"])
    return dat


def make_chain(bn, lik, dat, widths, seed=1234, mask_blocks=0, fun="tanh", model_kw=None, **mcmc_kw):
    """npBNN + MCMC on ``dat``; ``mask_blocks``: a block-structured first layer (config-5 like: that many equal blocks of inputs,
    each feeding its own share of the first layer's nodes); ``model_kw``: further arguments of npBNN (they win over this
    function's own)."""
    extra, mk = {}, dict(update_f=[0.05] * 3, update_ws=[0.075] * 3, n_iteration=100000)
    if lik == "gauss":
        extra = dict(estimation_mode="regression", empirical_error=False)
        mk.update(estimate_error=False)            # (sigma stays 1: the state check needs no sigma bookkeeping)
    elif lik == "pois":
        extra = dict(estimation_mode="custom", size_output=1)
        mk.update(likelihood_f=bn.poi_likelihood, accuracy_f=bn.poi_acc)
    elif lik in ("nb", "nb10", "nb2d"):
        extra = dict(estimation_mode="custom", size_output=2 * GENERIC[lik])
        mk.update({"nb": dict(likelihood_f=bn.negbin_likelihood, accuracy_f=bn.negbin_acc),
                   "nb10": dict(likelihood_f=bn.negbin_likelihood_base10, accuracy_f=bn.negbin_acc_base10),
                   "nb2d": dict(likelihood_f=bn.negbin_likelihood2d, accuracy_f=bn.negbin2d_acc)}[lik])
    elif lik == "err":
        extra = dict(estimation_mode="regression-error", output_act_fun=bn.RegressTransformError)
    mk.update(mcmc_kw)
    np.random.seed(seed)
    model = dict(dict(n_nodes=list(widths), actFun=bn.ActFun(fun=fun), use_bias_node=2, prior_f=1, p_scale=1, seed=seed, init_std=0.1),
                 **extra)
    model.update(model_kw or {})
    bnn = quiet(bn.npBNN, dat, **model)
    if mask_blocks:
        f = dat["data"].shape[1]
        w0 = widths[0]
        per = [w0 // mask_blocks] * mask_blocks
        per[-1] += w0 - sum(per)
        m = bn.create_mask(bnn._w_layers, indx_input_list=[list(np.repeat(np.arange(mask_blocks), f // mask_blocks))] + [[]] * (len(widths)),
                           nodes_per_feature_list=[per] + [[]] * (len(widths)))
        quiet(bnn.apply_mask, m)
    return bnn, bn.MCMC(bnn, **mk)


def _out_fn(lik):
    if lik == "err":
        return orc.out_regress_error
    return orc.out_softmax if lik == "cat" else orc.out_identity


def generic_addends(lik, y, labels):
    """S for the row-wise likelihoods: the sum over rows and columns of the absolute values of the separate addends (the count
    log-likelihoods cancel by orders of magnitude, so their bar is relative to S, not to the sum)."""
    g = scipy.special.gammaln
    k = labels.shape[1]
    with np.errstate(all="ignore"):
        if lik == "err":
            r = (labels - y[:, :k]) / y[:, k:2 * k]
            return float(np.sum(0.9189385332046727 + np.abs(np.log(y[:, k:2 * k])) + 0.5 * r * r))
        if lik == "pois":
            return float(np.sum(np.abs(labels[:, 0] * y[:, 0]) + np.exp(y[:, 0]) + np.abs(g(labels[:, 0] + 1))))
        kk = k if lik == "nb2d" else 1
        b = np.log(10.0) if lik == "nb10" else 1.0
        mean, p = np.exp(b * y[:, :kk]), 1 / (1 + np.exp(-b * y[:, kk:2 * kk]))
        n = p * mean / (1 - p)
        c = labels[:, :kk]
        return float(np.sum(np.abs(g(c + n)) + np.abs(g(c + 1)) + np.abs(g(n)) + np.abs(n * np.log(p)) + np.abs(c * np.log1p(-p))))


def _accuracy_ok(got, y64, labels, tol=ACC_TOL):
    want = orc.acc_classification(y64, labels)
    top2 = np.sort(y64, axis=1)[:, -2:]
    near_ties = int(np.sum(top2[:, -1] - top2[:, 0] < 1e-5)) if y64.shape[1] > 1 else 0
    n = len(labels)
    return abs(got - want) <= tol + near_ties / n, (got, want, near_ties)


def oracle_loglik(lik, x, labels, weights, fun="tanh", act=None, sig2=None, class_w=()):
    """float64 log-likelihood and predictions; ``act``: an orc.Act in place of ``fun``, ``sig2``: the Gaussian's sigma per column
    (1 without), ``class_w``: class weights of the categorical."""
    y = orc.forward(x, weights, act or orc.Act(fun), _out_fn(lik))
    if lik == "cat":
        with np.errstate(divide="ignore"):
            return orc.lik_categorical(y, labels, np.arange(len(x)), class_weight=class_w), y
    if lik == "gauss":
        return orc.lik_gaussian(y, labels, None, sig2=np.ones(labels.shape[1]) if sig2 is None else sig2), y
    if lik == "err":
        return orc.lik_gaussian_error(y, labels, None), y
    return {"pois": orc.lik_poisson, "nb": orc.lik_negbin, "nb10": orc.lik_negbin_base10, "nb2d": orc.lik_negbin2d}[lik](y, labels), y


def check_state(lik, bnn, mcmc, worst=None, accuracy=True):
    """The chain's current state against float64: the log-likelihood and prior of the host's weights, and the accuracies.
    Returns the relative log-likelihood error."""
    return check_state_on(lik, bnn, mcmc, bnn._data, bnn._labels, bnn._test_data, bnn._test_labels, worst=worst, accuracy=accuracy)


def check_state_on(lik, bnn, mcmc, data, labels, test_data, test_labels, worst=None, accuracy=True, act=None, sig2=None, class_w=(),
                   prior_extra=0.0, ll_rtol=LL_RTOL, lp_rtol=LP_RTOL, acc_tol=ACC_TOL, rowwise_accuracy=True, min_abs=None):
    """check_state on explicit tables (a row-sharded chain holds a share of the rows and answers for all of them).  ``act``,
    ``sig2``, ``class_w``: see oracle_loglik; ``prior_extra``: what the chain's log prior holds beside the weights' (the slopes'
    term); the bars default to this module's and may only be tightened (the float64 stand-in); ``rowwise_accuracy`` False leaves
    out the accuracies whose callables run on the device; ``min_abs``: the least |logLik| at which the relative bar means
    something - asserted."""
    w = bnn._w_layers
    act = act or orc.Act("tanh")
    want, y = oracle_loglik(lik, data, labels, w, act=act, sig2=sig2, class_w=class_w)
    if lik in GENERIC and lik != "pois":         # (relative to S: test_hip_generic_lik's forward bar)
        err = abs(mcmc._logLik - want) / generic_addends(lik, y, labels)
    else:
        if min_abs is not None:
            assert abs(want) >= min_abs, ("logLik too near zero for a relative bar", want, min_abs)
        err = abs(mcmc._logLik - want) / max(abs(want), 1e-300)      # (one row of one class: both are 0 exactly)
    assert err <= ll_rtol, ("logLik", mcmc._logLik, want, err)
    lp = orc.log_prior(w, bnn._prior_kind() if bnn._prior else 0, bnn._prior_scale) + prior_extra
    assert abs(mcmc._logPrior - lp) <= lp_rtol * max(1.0, abs(lp)), ("logPrior", mcmc._logPrior, lp)
    if accuracy and lik == "cat":
        ok, info = _accuracy_ok(mcmc._accuracy, y, labels, acc_tol)
        assert ok, ("accuracy", info)
        if len(test_data):
            y_t = orc.forward(test_data, w, act, orc.out_softmax)
            ok, info = _accuracy_ok(mcmc._test_accuracy, y_t, test_labels, acc_tol)
            assert ok, ("test accuracy", info)
    elif accuracy and lik == "gauss" or accuracy and lik == "err" and rowwise_accuracy:
        want_mse = float(np.mean(orc.mse_per_column(y, labels)))
        assert abs(mcmc._accuracy - want_mse) <= acc_tol * max(1.0, want_mse), ("mse", mcmc._accuracy, want_mse)
    elif accuracy and rowwise_accuracy and lik in GENERIC and lik != "pois":       # negbin_acc / negbin_acc_base10 / negbin2d_acc (BNN_lik.py:81-91)
        kk = labels.shape[1] if lik == "nb2d" else 1
        mean = 10.0 ** y[:, :kk] if lik == "nb10" else np.exp(y[:, :kk])
        want_mse = float(np.mean((mean - labels[:, :kk]) ** 2))
        assert abs(mcmc._accuracy - want_mse) <= acc_tol * max(1.0, want_mse), ("count mse", mcmc._accuracy, want_mse)
    if worst is not None:
        worst.append(err)
    return err


def dispatch_sizes(n_iter, seed=0):
    rs = np.random.default_rng(seed)
    out, left = [], n_iter
    while left > 0:
        k = int(min(left, rs.integers(7, 41)))
        out.append(k)
        left -= k
    return out


def drive(lik, bnn, mcmc, n_iter, advance="run_steps", seed=0, worst=None, accuracy_every=3):
    """Advance the chain in dispatches of 7..40 iterations, checking the state after each; returns the accept / reject sequence."""
    decisions = []
    for j, k in enumerate(dispatch_sizes(n_iter, seed)):
        if advance == "run_steps":
            mcmc.run_steps(bnn, k)
        else:
            for _ in range(k):
                mcmc.mh_step(bnn)
        decisions += list(mcmc._last_accepted_mem[-k:])
        check_state(lik, bnn, mcmc, worst, accuracy=(j % accuracy_every == 0))
    return decisions


def oracle_twin(lik, build, backend_cls=None):
    """The same chain (``build()`` returns (bnn, mcmc)) on the float64 stand-in of the device chain."""
    import oracle_backend
    from npbnn_amd import sampler
    real = sampler._make_backend
    cls = backend_cls or oracle_backend.OracleChainBackend
    oracle_backend.serve_from_oracle(lambda b: cls(b, out_kind={"cat": 0, "err": 2}.get(lik, 1)))
    try:
        return build()
    finally:
        sampler._make_backend = real


def common_prefix(a, b):
    n = 0
    for x, y in zip(a, b):
        if x != y:
            break
        n += 1
    return n


def assert_trajectory(dev, ref):
    n = common_prefix(dev, ref)
    assert n >= min(COMMON, len(ref)), "left the float64 chain's accept / reject sequence after %d of %d decisions" % (n, len(ref))
    return n


@pytest.fixture(scope="module")
def bn():
    import npbnn_amd
    from npbnn_amd import _capi
    _capi.load_library()
    return npbnn_amd


@pytest.fixture(scope="module")
def report():
    """Worst relative logLik error and common trajectory prefix per family (printed with -s)."""
    rep = {}
    yield rep
    for fam, v in sorted(rep.items()):
        print("\n[chain-oracle] %-12s worst logLik rel err %.3e  shortest common prefix %s" % (fam, max(v["err"] or [0]),
                                                                                              min(v["prefix"]) if v["prefix"] else "-"))


def _note(report, fam, errs, prefix=None):
    r = report.setdefault(fam, dict(err=[], prefix=[]))
    r["err"] += errs
    if prefix is not None:
        r["prefix"].append(prefix)


def _info(mcmc, what):
    from npbnn_amd import _capi
    return mcmc._backend.ctx.info(getattr(_capi, what))


# ---- resident chains: every build of the instantiation files ------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_resident_build_against_float64(case, bn, report, monkeypatch):
    monkeypatch.setenv("NPBNN_L0", case["l0"])
    mt0, lik = case["mt0"], case["lik"]
    blk = case["blk"]
    f = 256 if blk else 12
    later = 40 if case["mti"] == 8 else 6
    n_iter = 200 if case["advance"] == "run_steps" else 90
    fam = "resident_d%d" % case["d"]
    for width, schedule in zip((16 * mt0, 16 * mt0 - 3), case["schedules"]):       # (the second: ragged, another schedule)
        dat = make_data(lik, case["rows"], f, seed=mt0 + 10 * case["d"], k=1 if blk else 2)

        def build():
            return make_chain(bn, lik, dat, (width, later), mask_blocks=4 if blk else 0)
        bnn, mcmc = build()
        mcmc._backend.ctx.set_fast_tails(bool(case["fast"]))
        mcmc.n_candidates, mcmc.device_schedule, mcmc.SUB_BATCH = case["d"], schedule, 16
        errs = [check_state(lik, bnn, mcmc)]
        dev = drive(lik, bnn, mcmc, n_iter, case["advance"], seed=width, worst=errs)
        assert _info(mcmc, "INFO_L0_F16") == (0 if case["l0"] == "f32" else 1)
        assert _info(mcmc, "INFO_FAST_TAILS") == case["fast"], "the launch did not take the build the case names"
        assert sum(dev) > 0, "no proposal was accepted"
        if case["advance"] == "run_steps":
            assert mcmc._device_iterations == n_iter
            if case["d"] > 1:
                assert mcmc._device_passes < n_iter, "the extra candidate slots were launched and thrown away"
            else:
                assert mcmc._device_passes == n_iter
            if case["key"][4]:
                assert mcmc._device_schedule_used == 5, "the outcome-speculative build did not run"
        prefix = None
        if width == 16 * mt0:
            rb, rm = oracle_twin(lik, build)
            rm.n_candidates, rm.device_schedule, rm.SUB_BATCH = case["d"], schedule, 16
            ref = drive(lik, rb, rm, n_iter, case["advance"], seed=width, accuracy_every=10 ** 9)
            prefix = assert_trajectory(dev, ref)
        _note(report, fam, errs, prefix)


@pytest.mark.parametrize("schedule", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("fast", [0, 1])
def test_every_schedule_and_candidate_count(schedule, d, fast, bn, report):
    """One network (layer 0 of 29 nodes: two tiles, ragged) under every schedule, 1..3 candidates, fast tails on and off."""
    dat = make_data("cat", 700, 20, n_test=90, seed=3)

    def build():
        return make_chain(bn, "cat", dat, (29, 7))
    bnn, mcmc = build()
    mcmc._backend.ctx.set_fast_tails(bool(fast))
    mcmc.n_candidates, mcmc.device_schedule, mcmc.SUB_BATCH = d, schedule, 16
    errs = []
    dev = drive("cat", bnn, mcmc, 240, seed=d, worst=errs)
    assert _info(mcmc, "INFO_FAST_TAILS") == fast
    assert (mcmc._device_passes < 240) == (d > 1)
    if schedule == 5 and fast and d != 2:
        assert mcmc._device_schedule_used == 5
    rb, rm = oracle_twin("cat", build)
    rm.n_candidates, rm.device_schedule, rm.SUB_BATCH = d, schedule, 16
    _note(report, "resident_d%d" % d, errs, assert_trajectory(dev, drive("cat", rb, rm, 240, seed=d, accuracy_every=10 ** 9)))


# ---- row counts where the plan changes ------------------------------------------------------------------------------------------

def _rows_per_workgroup(mcmc):
    return 64 * _info(mcmc, "INFO_WAVES_PER_BLOCK")


@pytest.mark.parametrize("n_rows", [1, 5, 63, "wg-1", "wg+1", 65535, 65537])
@pytest.mark.parametrize("lik", ["cat", "gauss"])
def test_row_counts_where_the_plan_changes(n_rows, lik, bn, report):
    """1 row, fewer than one tile, one row either side of a workgroup's rows, one either side of 65 536 (the 8-wave rule)."""
    f = 16
    if isinstance(n_rows, str):
        probe_dat = make_data(lik, 4096, f, seed=8)
        _, pm = make_chain(bn, lik, probe_dat, (20, 5))
        wg = _rows_per_workgroup(pm)
        pm._backend.ctx.close()
        n_rows = wg - 1 if n_rows == "wg-1" else wg + 1
    dat = make_data(lik, n_rows, f, seed=8)
    if lik == "cat" and n_rows < 5:
        dat["labels"][:] = np.arange(n_rows) % 5
    bnn, mcmc = make_chain(bn, lik, dat, (20, 5))
    mcmc.n_candidates, mcmc.SUB_BATCH = 3, 16
    errs = [check_state(lik, bnn, mcmc)]
    drive(lik, bnn, mcmc, 120 if n_rows > 60000 else 200, seed=n_rows, worst=errs)
    _note(report, "rows", errs)


def test_every_forced_wave_count(bn, report, monkeypatch):
    """NPBNN_WAVES from 1 to INFO_WAVES_PER_BLOCK, set before the context is built (the shape of the bug where resident launches
    of 1 to 3 waves summed a quarter to three quarters of the rows): below four waves plan_launch refuses the launch, from four
    on the chain's state is float64's."""
    dat = make_data("cat", 20000, 24, seed=4)
    _, probe = make_chain(bn, "cat", dat, (24, 6))
    wpb = _info(probe, "INFO_WAVES_PER_BLOCK")
    probe._backend.ctx.close()
    assert wpb >= 8
    errs = []
    for v in range(1, wpb + 1):
        monkeypatch.setenv("NPBNN_WAVES", str(v))
        if v < 4:
            with pytest.raises(Exception, match="too large for the LDS-resident path"):
                make_chain(bn, "cat", dat, (24, 6))
            continue
        bnn, mcmc = make_chain(bn, "cat", dat, (24, 6))
        mcmc.n_candidates, mcmc.SUB_BATCH = 2, 16
        errs.append(check_state("cat", bnn, mcmc))
        drive("cat", bnn, mcmc, 60, seed=v, worst=errs)
        mcmc._backend.ctx.close()
    _note(report, "waves", errs)


# ---- layer 0 --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("x_kind", ["normal", "lognormal3", "outlier"])
@pytest.mark.parametrize("l0", ["f32", "auto"])
@pytest.mark.parametrize("lik", ["cat", "gauss"])
def test_layer0_precision_on_heavy_tails(x_kind, l0, lik, bn, report, monkeypatch):
    """float32 and fp16-split first layer on normal and heavy-tailed features (the scales moved per column)."""
    monkeypatch.setenv("NPBNN_L0", l0)
    dat = make_data(lik, 900, 40, n_test=100, seed=6, x_kind=x_kind)
    bnn, mcmc = make_chain(bn, lik, dat, (30, 6))
    mcmc.n_candidates, mcmc.SUB_BATCH = 2, 16
    errs = [check_state(lik, bnn, mcmc)]
    drive(lik, bnn, mcmc, 200, seed=7, worst=errs)
    mcmc.run_steps(bnn, 7)
    if l0 == "auto":                 # (read after a chain launch: a test-table prediction the fp16 pair cannot hold runs in float32)
        assert _info(mcmc, "INFO_L0_F16") == 1
    check_state(lik, bnn, mcmc, errs)
    _note(report, "layer0", errs)


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("lik", ["cat", "gauss"])
def test_block_structured_layer0(d, lik, bn, report):
    """A config-5-like first layer (8 blocks of 32 inputs, 4 nodes each) through npbnn_set_layer_mask, 1 to 3 candidates
    (the largest it allows: two output tiles)."""
    dat = make_data(lik, 1500, 256, seed=9, k=1)

    def build():
        return make_chain(bn, lik, dat, (32, 8), mask_blocks=8)
    bnn, mcmc = build()
    mcmc.n_candidates, mcmc.SUB_BATCH = d, 16
    errs = [check_state(lik, bnn, mcmc)]
    dev = drive(lik, bnn, mcmc, 200, seed=d, worst=errs)
    assert _info(mcmc, "INFO_L0_F16") == 1 and _info(mcmc, "INFO_FAST_TAILS") == 1
    assert (mcmc._device_passes < 200) == (d > 1)
    for w, m in zip(bnn._w_layers, bnn._mask):
        assert np.all(w[m == 0] == 0)
    rb, rm = oracle_twin(lik, build)
    rm.n_candidates, rm.SUB_BATCH = d, 16
    _note(report, "layer0", errs, assert_trajectory(dev, drive(lik, rb, rm, 200, seed=d, accuracy_every=10 ** 9)))


# ---- group pass (npbnn_chains_run_batched) -------------------------------------------------------------------------------------

def _group_chains(bn, lik, dat, n):
    out = []
    for i in range(n):
        out.append(make_chain(bn, lik, dat, (24, 6), seed=1234 + i, mcmc_id=i, randomize_seed=True))
    return out


@pytest.mark.parametrize("n_chains", [2, 3, 4])
@pytest.mark.parametrize("lik", ["cat", "gauss"])
def test_group_pass_against_float64(n_chains, lik, bn, report):
    """2, 3 and 4 chains of one model through ex.run_steps_batched (groups of up to three: one proposal per chain per read of X);
    every chain's state against float64 after every call, and every chain's trajectory against its float64 twin."""
    from npbnn_amd import exchange as ex
    dat = make_data(lik, 800, 32, seed=11)
    chains = _group_chains(bn, lik, dat, n_chains)
    twins = oracle_twin(lik, lambda: _group_chains(bn, lik, dat, n_chains))
    assert chains[0][1]._backend.group_size >= 2
    errs, decisions, ref = [[] for _ in chains], [[] for _ in chains], [[] for _ in chains]
    for k in dispatch_sizes(240, seed=n_chains):
        before = [m._device_iterations for _, m in chains]
        ex.run_steps_batched(chains, k)
        for i, (bnn, mcmc) in enumerate(chains):
            assert mcmc._device_iterations - before[i] == k
            decisions[i] += list(mcmc._last_accepted_mem[-k:])
            check_state(lik, bnn, mcmc, errs[i], accuracy=False)
        for i, (bnn, mcmc) in enumerate(twins):
            mcmc.run_steps(bnn, k)
            ref[i] += list(mcmc._last_accepted_mem[-k:])
    for i in range(n_chains):
        assert sum(decisions[i]) > 0
        _note(report, "group", errs[i], assert_trajectory(decisions[i], ref[i]))


# ---- exchange run (npbnn_chains_run_exchange) ----------------------------------------------------------------------------------

def _exchange_chains(bn, lik, dat, temps):
    out = []
    for i, t in enumerate(temps):
        out.append(make_chain(bn, lik, dat, (16, 5), seed=1234 + i, mcmc_id=i, randomize_seed=True, temperature=t, adapt_f=0,
                              adapt_fM=1))
    return out


@pytest.mark.parametrize("lik", ["cat", "gauss"])
def test_exchange_run_against_float64(lik, bn, report):
    """ex.advance_intervals(..., batch=n_seg) on the device against the float64 exchange stand-in on the same chains and swap
    proposals: the cold-chain snapshot at every swap is float64's, the swap decisions share a common prefix (a swap decided on
    near-tie log-posteriors may flip), and so do the chains' decisions."""
    import oracle_backend
    from npbnn_amd import exchange as ex
    temps = [0.7, 0.85, 1.0]
    n_seg, seg_len = 8, 25
    dat = make_data(lik, 900, 24, seed=12)
    chains = _exchange_chains(bn, lik, dat, temps)
    twins = oracle_twin(lik, lambda: _exchange_chains(bn, lik, dat, temps), oracle_backend.OracleExchangeBackend)

    def run(cs):
        log = []
        swaps = ex.SwapProposals(len(cs), np.random.RandomState(7))
        done = ex.advance_intervals(cs, [0, 1, 2], 3, n_seg, seg_len, swaps, 0, batch=n_seg,
                                    on_interval=lambda s, info: log.append((info["swap"], info["scalars"].copy(), info["cold"])))
        assert done == n_seg
        return log
    log_d, log_r = run(chains), run(twins)
    errs = []
    n_cold = 0
    for sw, _, cold in log_d:
        assert cold is not None, "the interval did not run on the device"
        for c, (bnn, _) in zip(cold, chains):
            if c is None:
                continue
            n_cold += 1
            flat, w = np.ravel(np.asarray(c["w"], dtype=float)), []
            for ref_w in bnn._w_layers:                   # (the snapshot is the packed weight vector)
                w.append(flat[:ref_w.size].reshape(ref_w.shape))
                flat = flat[ref_w.size:]
            want, _ = oracle_loglik(lik, bnn._data, bnn._labels, w)
            err = abs(c["loglik"] - want) / abs(want)
            assert err <= LL_RTOL, ("cold logLik", c["loglik"], want)
            lp = orc.log_prior(w, bnn._prior_kind() if bnn._prior else 0, bnn._prior_scale)
            assert abs(c["logprior"] - lp) <= LP_RTOL * max(1.0, abs(lp))
            errs.append(err)
    assert n_cold == n_seg
    for bnn, mcmc in chains:
        errs.append(check_state(lik, bnn, mcmc, accuracy=False))
    swaps_d = [(sw[0], sw[1], sw[4]) for sw, _, _ in log_d]
    swaps_r = [(sw[0], sw[1], sw[4]) for sw, _, _ in log_r]
    n_sw = common_prefix(swaps_d, swaps_r)
    assert n_sw >= min(4, n_seg), (swaps_d, swaps_r)
    for (_, m), (_, r) in zip(chains, twins):
        assert m._current_iteration == r._current_iteration == n_seg * seg_len
    _note(report, "exchange", errs, n_sw)


# ---- weight-streamed path ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 2, 3])
def test_streamed_fused_pass_on_many_rows(d, bn, report, monkeypatch):
    """The streamed path forced (NPBNN_FORCE_WIDE, as NPBNN_OPT_WIDE for every context) on more than 65 536 rows: the fused pass
    with 1, 2 and 3 candidates."""
    monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    dat = make_data("cat", 70001, 32, seed=14)
    bnn, mcmc = make_chain(bn, "cat", dat, (32, 8))
    errs = [check_state("cat", bnn, mcmc)]
    assert mcmc._backend.ctx.is_wide()
    mcmc.n_candidates, mcmc.SUB_BATCH = d, 16
    drive("cat", bnn, mcmc, 80, seed=d, worst=errs, accuracy_every=2)
    if d > 1:
        assert mcmc._device_passes < 80
    _note(report, "streamed", errs)


@pytest.mark.parametrize("slices", [1, 3])
def test_streamed_k_sliced_path(slices, bn, report, monkeypatch):
    """A network that goes to the streamed path by itself (a 200-node layer), K-sliced (not fused) with a forced NPBNN_WIDE_SLICES."""
    monkeypatch.setenv("NPBNN_WIDE_SLICES", str(slices))
    dat = make_data("gauss", 5000, 1500, seed=15)
    bnn, mcmc = make_chain(bn, "gauss", dat, (200, 8))
    assert mcmc._backend.ctx.is_wide()
    mcmc.SUB_BATCH = 16
    errs = [check_state("gauss", bnn, mcmc)]
    drive("gauss", bnn, mcmc, 60, seed=slices, worst=errs)
    _note(report, "streamed", errs)


def test_streamed_chain_with_a_test_set(bn, report):
    """Train and test tables of different plans on the streamed path: the test accuracy after every dispatch is float64's."""
    dat = make_data("cat", 11200, 1024, n_test=6400, seed=13)
    bnn, mcmc = make_chain(bn, "cat", dat, (50, 5))
    assert mcmc._backend.ctx.is_wide()
    mcmc.SUB_BATCH = 16
    errs = [check_state("cat", bnn, mcmc)]
    drive("cat", bnn, mcmc, 60, seed=1, worst=errs, accuracy_every=1)
    _note(report, "streamed", errs)


# ---- the architecture set again between batches ----------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["resident", "streamed"])
def test_set_arch_again_between_batches(path, bn, report, monkeypatch):
    """npbnn_set_arch between device batches of one context - with the same architecture, then with another of the same number of
    weights ((16, 7) and (14, 11) on 32 features: 687 each) - lays the chain's result block out again: every later batch holds to
    float64.  (The per-weight buffers are released by set_arch; the current weights live in the result block.)"""
    if path == "streamed":
        monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    dat = make_data("cat", 3000, 32, seed=16)
    bnn, mcmc = make_chain(bn, "cat", dat, (16, 7))
    ctx = mcmc._backend.ctx
    assert ctx.is_wide() == (path == "streamed")
    mcmc.SUB_BATCH = 16
    errs = [check_state("cat", bnn, mcmc)]
    drive("cat", bnn, mcmc, 40, seed=1, worst=errs)
    mcmc._backend._shapes = None               # the next batch sets the same architecture again (HipBackend._configure)
    drive("cat", bnn, mcmc, 40, seed=2, worst=errs)
    bnn2, mcmc2 = make_chain(bn, "cat", dat, (14, 11), seed=99)
    assert sum(w.size for w in bnn2._w_layers) == sum(w.size for w in bnn._w_layers)
    mcmc2.SUB_BATCH = 16
    mcmc2._backend.ctx = ctx                   # the second network's batches on the first context: set_arch to equal weights, new shapes
    mcmc2._backend._shapes = None
    drive("cat", bnn2, mcmc2, 40, seed=3, worst=errs)
    assert ctx.is_wide() == (path == "streamed")
    _note(report, "set_arch again", errs)


# ---- every float64 row-wise likelihood --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["resident", "streamed"])
@pytest.mark.parametrize("widths", [(20, 6), (20, 40)], ids=["mti1", "mti8"])
@pytest.mark.parametrize("lik", list(GENERIC))
def test_generic_likelihood_chain_against_float64(lik, widths, path, bn, report, monkeypatch):
    """Chains of every kind the generic builds serve - Poisson, NegBin, NegBin base 10, NegBin2D (3 count columns) and the
    predicted-sigma Gaussian (4 targets) - on 20 000 rows with a test table, later layers <= 16 (MTI 1) and of 40 nodes (MTI 8),
    resident and with the streamed path forced: after every dispatch the chain's logLik is float64's on its current weights,
    within 2e-6 of S (the sum of the absolute values of the likelihood's addends: count log-likelihoods cancel)."""
    if path == "streamed":
        monkeypatch.setenv("NPBNN_FORCE_WIDE", "1")
    dat = make_data(lik, 20000, 16, n_test=700, seed=21)
    bnn, mcmc = make_chain(bn, lik, dat, widths)
    assert mcmc._backend.ctx.is_wide() == (path == "streamed")
    mcmc.SUB_BATCH = 16
    errs = [check_state(lik, bnn, mcmc)]
    before = mcmc._device_iterations
    dec = drive(lik, bnn, mcmc, 300, seed=len(lik), worst=errs, accuracy_every=2)
    assert mcmc._device_iterations - before == 300, "the chain did not run on the device"
    assert sum(dec) > 0, "no proposal was accepted"
    _note(report, "generic_%s" % lik, errs)
