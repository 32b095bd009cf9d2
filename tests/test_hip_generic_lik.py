"""GPU: the float64 row-wise likelihoods - predicted-sigma Gaussian (estimation_mode="regression-error") and the count plug-ins
poi_likelihood, negbin_likelihood, negbin_likelihood_base10, negbin_likelihood2d - held to float64.

These are the "generic" builds of the evaluation kernel (LK = kLikGen: npbnn_eval_inst_d1_gen.hip, npbnn_eval_inst_mti8_gen.hip,
their epilogue in npbnn_eval.hip.h) and the streamed path's wide_row_terms (npbnn_wide.hip.h).  Every case checks two bars, both
relative to S, the sum over rows and columns of the absolute values of the separate addends of the likelihood (count
log-likelihoods cancel by orders of magnitude: terms of 1e5 summing to a few units per row, so a tolerance on the sum itself says
nothing):

  * epilogue bar, |dev - lik(z32)| <= 1e-9 S: the float64 likelihood (oracle.lik_*) of the device's own float32 outputs
    (ctx.predict(apply_out_fn=False)).  It rests on the prediction build and the generic build computing the same float32
    outputs bit for bit, which test_predict_and_the_generic_build_share_their_outputs checks on its own;
  * forward bar, |dev - lik(z64)| <= 2e-6 S: oracle.forward in float64, LL_RTOL applied to S.

Targets are float32 on the device (npbnn_set_targets_f64); the oracle sees the same numbers, except in the test of counts above
2^24, which measures what that rounding does against the original integers."""
import zlib

import numpy as np
import pytest
import scipy.special

import oracle as orc

pytestmark = pytest.mark.gpu

LL_RTOL = 2e-6
EPI_RTOL = 1e-9
Z_TOL = 2e-5
ACT_KIND = {"relu": 0, "leaky": 1, "swish": 2, "tanh": 3}
LIK = {"err": 2, "poi": 3, "nb": 4, "nb2d": 5, "nb10": 6}
ORACLE = {"err": orc.lik_gaussian_error, "poi": orc.lik_poisson, "nb": orc.lik_negbin, "nb2d": orc.lik_negbin2d,
          "nb10": orc.lik_negbin_base10}
LN10 = np.log(10.0)


@pytest.fixture(scope="module")
def hip():
    import npbnn_amd
    from npbnn_amd import _capi
    _capi.load_library()
    return npbnn_amd


@pytest.fixture(scope="module")
def report():
    """Worst |error| / S per kind and path, for both bars (printed with -s)."""
    rep = {}
    yield rep
    for key in sorted(rep):
        print("\n[generic-lik] %-22s epilogue %.3e  forward %.3e  (cases %d)" % (key, rep[key][0], rep[key][1], rep[key][2]))


def _note(report, key, epi, fwd):
    r = report.setdefault(key, [0.0, 0.0, 0])
    r[0], r[1], r[2] = max(r[0], epi), max(r[1], fwd), r[2] + 1


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ---- float64 likelihood and the size of its addends --------------------------------------------------------------------------

def oracle_lik(kind, z, y, lik_temp=1.0):
    """oracle.lik_* on pre-activations ``z`` (softplus applied in float64 where the formula needs it)."""
    with np.errstate(all="ignore"):
        if kind == "err":
            return orc.lik_gaussian_error(orc.out_regress_error(z.copy()), y, None, lik_temp=lik_temp)
        return ORACLE[kind](z, y)


def addends(kind, z, y):
    """S: the sum over rows and columns of the absolute values of the likelihood's separate addends."""
    g = scipy.special.gammaln
    k = y.shape[1]
    with np.errstate(all="ignore"):
        if kind == "err":
            sg = orc.softplus(z[:, k:2 * k])
            r = (y - z[:, :k]) / sg
            return float(np.sum(0.9189385332046727 + np.abs(np.log(sg)) + 0.5 * r * r))
        if kind == "poi":
            eta, c = z[:, 0], y[:, 0]
            return float(np.sum(np.abs(c * eta) + np.exp(eta) + np.abs(g(c + 1))))
        kk = k if kind == "nb2d" else 1
        e0, e1 = z[:, :kk], z[:, (k if kind == "nb2d" else 1):][:, :kk]
        c = y[:, :kk]
        base = LN10 if kind == "nb10" else 1.0
        mean, p = np.exp(base * e0), 1 / (1 + np.exp(-base * e1))
        n = p * mean / (1 - p)
        return float(np.sum(np.abs(g(c + n)) + np.abs(g(c + 1)) + np.abs(g(n)) + np.abs(n * np.log(p)) + np.abs(c * np.log1p(-p))))


def same_class(got, want):
    """Non-finite references: the device must give the same class of value (NaN, +inf or -inf)."""
    if np.isnan(want):
        return bool(np.isnan(got))
    return got == want


def check_bars(kind, got, z32, z64, y32, y_forward=None, lik_temp=1.0, forward=True):
    """Both bars; returns (epilogue error / S, forward error / S).  ``y_forward``: the targets of the forward bar (default y32)."""
    want_e = oracle_lik(kind, z32, y32, lik_temp)
    if not np.isfinite(want_e):
        assert same_class(got, want_e), ("non-finite reference", kind, got, want_e)
        return 0.0, 0.0
    s_e = abs(lik_temp) * addends(kind, z32, y32)
    epi = abs(got - want_e) / s_e
    assert epi <= EPI_RTOL, ("epilogue bar", kind, got, want_e, epi)
    fwd = 0.0
    if forward:
        yf = y32 if y_forward is None else y_forward
        want_f = oracle_lik(kind, z64, yf, lik_temp)
        assert np.isfinite(want_f), ("forward reference", want_f)
        fwd = abs(got - want_f) / (abs(lik_temp) * addends(kind, z64, yf))
        assert fwd <= LL_RTOL, ("forward bar", kind, got, want_f, fwd)
    return epi, fwd


# ---- networks and tables ---------------------------------------------------------------------------------------------------------

def shapes(f, hidden, n_out, bias):
    """Weight shapes (out x in[+1]) of use_bias_node = bias (cases.layer_shapes), also for a network without hidden layers."""
    if not hidden:
        return [(n_out, f + (1 if bias != 0 else 0))]
    b1, b2, b3 = int(bias >= 1), int(bias >= 2), int(bias in (3, -1))
    dims = [f] + list(hidden)
    out = [(hidden[0], f + b1)] + [(dims[i + 1], dims[i] + b2) for i in range(1, len(hidden))]
    return out + [(n_out, hidden[-1] + b3)]


def make_act(fun, n_hidden):
    if fun == "genReLU":
        return orc.Act("genReLU", np.linspace(0.05, 0.3, max(n_hidden, 1)))
    return orc.Act(fun)


def act_prm(act, n_hidden):
    if act.kind != "leaky" or n_hidden == 0:
        return None
    return np.array([act.slope(i) for i in range(n_hidden)], dtype=float)


def make_weights(rs, f, hidden, n_out, bias, x_scale=None):
    w = [rs.normal(0, 1.0, s) / np.sqrt(s[1]) for s in shapes(f, hidden, n_out, bias)]
    if x_scale is not None:                           # heavy-tailed columns: pre-activations O(1) for the typical row
        off = w[0].shape[1] - f
        w[0][:, off:] /= np.maximum(x_scale, 1e-12)
    return w


def make_targets(kind, rs, n, k, z64):
    if kind == "err":
        return _f32(z64[:, :k] + orc.softplus(z64[:, k:2 * k]) * rs.standard_normal((n, k)))
    base = LN10 if kind == "nb10" else 1.0
    return rs.poisson(np.exp(np.clip(base * z64[:, :k], -20, 8))).astype(float)


def make_ctx(hip, x, w, act, kind, y, n_out, wide=False, l0="auto", test=None):
    ctx = hip.HipContext(0)
    ctx.set_l0_precision(l0)
    if wide:
        ctx.set_wide(True)
    ctx.set_data(x)
    ctx.set_targets(y)
    if test is not None:
        ctx.set_data(test[0], which=1)
        ctx.set_targets(test[1], which=1)
    out_kind = 2 if kind == "err" else 1
    ctx.set_arch_from_weights(w, x.shape[1], ACT_KIND[act.kind], out_kind, LIK[kind], y.shape[1])
    return ctx


def run_case(hip, report, kind, k, n_out, hidden, fun, bias, n, f, l0, seed, wide_modes=(False, True), test_rows=0,
             temp=False, x_kind="normal", expect_wide=None, y=None, w=None, x=None, tag=""):
    rs = np.random.default_rng(seed)
    if x is None:
        x = rs.standard_normal((n + test_rows, f)) if x_kind == "normal" else np.exp(3.0 * rs.standard_normal((n + test_rows, f)))
    x32 = _f32(x)
    act = make_act(fun, len(hidden))
    ap = act_prm(act, len(hidden))
    if w is None:
        w = make_weights(rs, f, hidden, n_out, bias, None if x_kind == "normal" else np.abs(x32).mean(axis=0) * np.sqrt(f))
    z64_all = orc.forward_logits(x32, w, act)
    if y is None:
        y = make_targets(kind, rs, n + test_rows, k, z64_all)
    y32 = _f32(y)
    xtr, ytr, z64 = x[:n], y[:n], z64_all[:n]
    test = (x[n:], y[n:]) if test_rows else None
    results = {}
    for wide in wide_modes:
        ctx = make_ctx(hip, xtr, w, act, kind, ytr, n_out, wide=wide, l0=l0, test=test)
        got = ctx.eval(w, act_prm=ap)["loglik"]
        path = "streamed" if ctx.is_wide() else "resident"
        if wide:
            assert ctx.is_wide()
        elif expect_wide is not None:
            assert ctx.is_wide() == expect_wide, "the network left its path"
        if l0 == "f32" or path == "resident":          # (auto: the resident path keeps the fp16 pair on these tables)
            assert ctx.l0_mode() == ("f32" if l0 == "f32" else "f16-split")
        z32 = ctx.predict(w, act_prm=ap, apply_out_fn=False)
        epi, fwd = check_bars(kind, got, z32, z64, y32[:n])
        _note(report, "%s/%s%s" % (kind, path, tag), epi, fwd)
        if test_rows:
            got_t = ctx.eval(w, act_prm=ap, which=1)["loglik"]
            zt32 = ctx.predict(w, act_prm=ap, which=1, apply_out_fn=False)
            assert zt32.shape == (test_rows, n_out)
            e2, f2 = check_bars(kind, got_t, zt32, z64_all[n:], y32[n:])
            _note(report, "%s/%s/test" % (kind, path), e2, f2)
        if temp:
            t = 0.37
            got_t = ctx.eval(w, act_prm=ap, lik_temp=t)["loglik"]
            if kind == "err":                           # tempered, BNN_lib.py:143
                np.testing.assert_allclose(got_t, t * got, rtol=1e-13)
                check_bars(kind, got_t, z32, z64, y32[:n], lik_temp=t)
            else:                                       # the count plug-ins take lik_temp and ignore it (BNN_lik.py)
                assert got_t == got
            y_dev = ctx.predict(w, act_prm=ap)          # the output function on the device
            want_y = orc.out_regress_error(z64.copy()) if kind == "err" else z64
            err = np.abs(y_dev - want_y) / np.maximum(1.0, np.abs(want_y))
            assert err.max() <= Z_TOL, err.max()
        results[wide] = got
        ctx.close()
    return results


# ---- the grid: kind x targets x outputs, builds, rows, features, layer 0 ---------------------------------------------------------

KIND_SHAPES = [("err", 1, 2), ("err", 2, 4), ("err", 3, 6), ("err", 5, 10), ("err", 8, 16),
               ("poi", 1, 1), ("poi", 1, 3), ("poi", 1, 16),
               ("nb", 1, 2), ("nb", 1, 7), ("nb10", 1, 2), ("nb10", 1, 7),
               ("nb2d", 1, 2), ("nb2d", 3, 6), ("nb2d", 8, 16)]
# (hidden, fun, bias): MTI 1 (later layers <= 16), MTI 8 (a later layer of 17..128), one layer, four layers
NETS = [((12, 7), "tanh", 2), ((24, 40), "ReLU", 1), ((), "tanh", 1), ((20, 12, 8), "swish", 3), ((9,), "genReLU", 2),
        ((33, 100), "tanh", -1), ((16, 16), "genReLU", 0), ((5, 128), "swish", 2)]
ROWS = [1, 15, 16, 17, 4097, 777, 100003]
FEATS = [(1, "f32"), (7, "auto"), (33, "f32"), (256, "auto"), (7, "f32"), (1, "auto"), (33, "auto"), (256, "f32")]

GRID = []
for _i, (_kind, _k, _n_out) in enumerate(KIND_SHAPES):
    for _j in range(2):
        _c = 2 * _i + _j
        GRID.append(dict(kind=_kind, k=_k, n_out=_n_out, net=NETS[_c % len(NETS)], n=ROWS[(_c * 3) % len(ROWS)],
                         feat=FEATS[(_c + _c // len(FEATS)) % len(FEATS)], seed=100 + _c))


def _grid_id(c):
    h, fun, b = c["net"]
    return "%s_k%d_o%d_h%s_%s_b%d_n%d_f%d_%s" % (c["kind"], c["k"], c["n_out"], "x".join(map(str, h)) or "none", fun, b, c["n"],
                                                  c["feat"][0], c["feat"][1])


def test_the_grid_reaches_every_build_row_and_feature_edge():
    """(A table check: the seeded grid below is meant to cover these, and a later edit of it must not quietly drop one.)"""
    nets = {c["net"] for c in GRID}
    assert any(max(h[1:], default=0) > 16 for h, _, _ in nets), "no MTI 8 case"
    assert any(h and max(h[1:], default=0) <= 16 for h, _, _ in nets), "no MTI 1 case"
    assert any(len(h) == 0 for h, _, _ in nets) and any(len(h) == 3 for h, _, _ in nets)
    assert {fun for _, fun, _ in nets} >= {"tanh", "ReLU", "swish", "genReLU"}
    assert {b for _, _, b in nets} >= {0, 1, 2, 3}
    assert {c["n"] for c in GRID} >= {1, 15, 16, 17, 4097, 100003}
    assert {c["feat"] for c in GRID} >= {(f, m) for f in (1, 7, 33, 256) for m in ("f32", "auto")}
    assert {(c["kind"], c["k"], c["n_out"]) for c in GRID} == set(KIND_SHAPES)


@pytest.mark.parametrize("case", GRID, ids=_grid_id)
def test_generic_builds_against_float64(case, hip, report):
    """Each case as the library places it and again with the streamed path forced; on every third case a test table of another
    row count, lik_temp and the output function."""
    f, l0 = case["feat"]
    hidden, fun, bias = case["net"]
    extra = case["seed"] % 3 == 0
    run_case(hip, report, case["kind"], case["k"], case["n_out"], hidden, fun, bias, case["n"], f, l0, case["seed"],
             test_rows=29 if extra else 0, temp=extra)


@pytest.mark.parametrize("n", [65535, 65536, 65537])
@pytest.mark.parametrize("kind,k,n_out", [("err", 2, 4), ("nb2d", 3, 6)])
def test_rows_where_the_plan_moves_other_kinds(kind, k, n_out, n, hip, report):
    """65 536 rows is where wide_needed moves fusable (categorical / Gaussian) networks with a narrow first layer; the generic kinds
    are not fusable, so their path stays where it is on either side."""
    run_case(hip, report, kind, k, n_out, (20, 5), "tanh", 2, n, 16, "auto", 7 + n, wide_modes=(False,), expect_wide=False)


def test_config4_shape_at_a_million_rows(hip, report):
    """1 M x 64, [16, 4], tanh, bias 2 (BASELINE config 4's shape): the float64 row sums at the size the benchmark runs."""
    run_case(hip, report, "err", 2, 4, (16, 4), "tanh", 2, 1_000_000, 64, "auto", 4, wide_modes=(False,), expect_wide=False)
    run_case(hip, report, "poi", 1, 1, (16, 4), "tanh", 2, 1_000_000, 64, "auto", 5, wide_modes=(False,), expect_wide=False)


@pytest.mark.parametrize("kind,k,n_out", [("err", 3, 6), ("nb", 1, 2)])
def test_heavy_tailed_table_on_the_fp16_pair(kind, k, n_out, hip, report):
    """Log-normal columns (sigma = 3, test_hip_parity._heavy_tailed): auto keeps the fp16 pair (scales moved per column)."""
    run_case(hip, report, kind, k, n_out, (24, 9), "tanh", 2, 5000, 48, "auto", 31, x_kind="lognormal3")


@pytest.mark.parametrize("kind,k,n_out", [("err", 4, 8), ("poi", 1, 3), ("nb2d", 2, 4), ("nb10", 1, 2)])
def test_a_shape_the_lds_cannot_hold_streams_by_itself(kind, k, n_out, hip, report):
    """[50, 5] on 1 024 features (the reference's default widths), an output layer <= 16: streamed without being forced."""
    run_case(hip, report, kind, k, n_out, (50, 5), "tanh", 2, 3001, 1024, "f32", 41, wide_modes=(False,), expect_wide=True,
             test_rows=70)


@pytest.mark.parametrize("kind,k,n_out", [("nb2d", 3, 6), ("err", 5, 10)])
def test_every_forced_wave_count(kind, k, n_out, hip, report, monkeypatch):
    """NPBNN_WAVES from 1 to the plan's count (test_hip_chain_oracle.test_every_forced_wave_count): below four waves the launch is
    refused, from four on the sum over every row is float64's."""
    from npbnn_amd import _capi
    rs = np.random.default_rng(51)
    n, f, hidden = 20000, 24, (24, 6)
    x = rs.standard_normal((n, f))
    w = make_weights(rs, f, hidden, n_out, 2)
    act = orc.Act("tanh")
    z64 = orc.forward_logits(_f32(x), w, act)
    y = make_targets(kind, rs, n, k, z64)
    probe = make_ctx(hip, x, w, act, kind, y, n_out)
    probe.eval(w)
    wpb = probe.info(_capi.INFO_WAVES_PER_BLOCK)
    probe.close()
    assert wpb >= 4
    for v in range(1, wpb + 1):
        monkeypatch.setenv("NPBNN_WAVES", str(v))
        ctx = make_ctx(hip, x, w, act, kind, y, n_out)
        if v < 4:
            with pytest.raises(Exception, match="too large for the LDS-resident path"):
                ctx.eval(w)
            ctx.close()
            continue
        got = ctx.eval(w)["loglik"]
        epi, fwd = check_bars(kind, got, ctx.predict(w, apply_out_fn=False), z64, _f32(y))
        _note(report, "%s/waves" % kind, epi, fwd)
        ctx.close()


# ---- the bar's premise ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,k,n_out,hidden", [("err", 3, 6, (12, 7)), ("nb2d", 2, 4, (24, 40)), ("poi", 1, 16, ()),
                                                 ("nb", 1, 7, (20, 12, 8))])
@pytest.mark.parametrize("wide", [False, True])
def test_predict_and_the_generic_build_share_their_outputs(kind, k, n_out, hidden, wide, hip):
    """The epilogue bar takes the device's float32 outputs from the prediction launch; the likelihood launch runs the generic build.
    Both must give the same outputs bit for bit: the generic build's likelihood of the predicted outputs, recomputed in float64 row
    by row, must match to the float64 rounding of the sum alone (1e-13 of S - 1e-9 is the bar the grid uses)."""
    rs = np.random.default_rng(61)
    n, f = 3001, 40
    x = rs.standard_normal((n, f))
    w = make_weights(rs, f, hidden, n_out, 2)
    act = orc.Act("swish")
    z64 = orc.forward_logits(_f32(x), w, act)
    y = make_targets(kind, rs, n, k, z64)
    ctx = make_ctx(hip, x, w, act, kind, y, n_out, wide=wide)
    got = ctx.eval(w)["loglik"]
    z32 = ctx.predict(w, apply_out_fn=False)
    assert np.array_equal(z32, _f32(z32)), "predictions are float32 values"
    want = oracle_lik(kind, z32, _f32(y))
    assert abs(got - want) <= 1e-13 * addends(kind, z32, _f32(y)), (got, want)
    ctx.close()


# ---- value edges -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,k,n_out", [("poi", 1, 1), ("nb", 1, 2), ("nb2d", 2, 4), ("nb10", 1, 2)])
@pytest.mark.parametrize("mean", [0.05, 1e3, 1e5])
@pytest.mark.parametrize("wide", [False, True])
def test_zero_heavy_and_large_counts(kind, k, n_out, mean, wide, hip, report):
    """Counts of mean 0.05 (mostly zeros), 1e3 and 1e5, the network's log-mean output moved there by its output bias."""
    rs = np.random.default_rng(int(mean * 10) + 7)
    n, f, hidden = 4099, 12, (10, 6)
    x = rs.standard_normal((n, f))
    w = make_weights(rs, f, hidden, n_out, 3)
    w[-1] *= 0.3
    base = LN10 if kind == "nb10" else 1.0
    kk = k if kind == "nb2d" else 1
    w[-1][:kk, 0] += np.log(mean) / base
    y = rs.poisson(mean, (n, k)).astype(float)
    run_case(hip, report, kind, k, n_out, hidden, "tanh", 3, n, f, "auto", 3, wide_modes=(wide,), y=y, w=w, x=x, tag="/counts")


@pytest.mark.parametrize("kind,k,n_out", [("poi", 1, 1), ("nb2d", 3, 6)])
@pytest.mark.parametrize("wide", [False, True])
def test_counts_above_2_24(kind, k, n_out, wide, hip, report):
    """Counts above 2^24 = 16 777 216 in one column: npbnn_set_targets_f64 rounds targets to float32, so an odd count there is not the
    count the reference sees.  Measured against the float64 oracle on the ORIGINAL integers, the rounding moves a row's term by
    |eta - digamma(y + 1)| at most (d/dy of y eta - lgamma(y + 1)), i.e. by the row's own misfit: at y ~ 3e7 that is a few
    units on addends of ~5e8, so the forward bar holds.  The epilogue bar is held on the rounded targets the device has."""
    rs = np.random.default_rng(2 ** 24)
    n, f, hidden = 2049, 10, (8, 5)
    x = rs.standard_normal((n, f))
    w = make_weights(rs, f, hidden, n_out, 3)
    w[-1] *= 0.05
    y = rs.poisson(3.0, (n, k)).astype(float)
    big = rs.integers(2 ** 24 + 1, 2 ** 25, n)
    big |= 1                                              # odd: none of them is a float32 number
    y[:, 0] = big
    w[-1][0, 0] += np.log(1.5 * 2 ** 24)
    assert np.all(_f32(y[:, 0]) != y[:, 0])
    act = orc.Act("tanh")
    z64 = orc.forward_logits(_f32(x), w, act)
    ctx = make_ctx(hip, x, w, act, kind, y, n_out, wide=wide)
    got = ctx.eval(w)["loglik"]
    z32 = ctx.predict(w, apply_out_fn=False)
    epi, fwd = check_bars(kind, got, z32, z64, _f32(y), y_forward=y)
    want_exact = oracle_lik(kind, z64, y)
    want_rounded = oracle_lik(kind, z64, _f32(y))
    print("\n[generic-lik] %s counts > 2^24 (%s): rounding moves the float64 likelihood by %.3e on S = %.3e (%.2e of S); "
          "device vs exact-count oracle %.2e of S" % (kind, "streamed" if wide else "resident", want_rounded - want_exact,
                                                       addends(kind, z64, y), abs(want_rounded - want_exact) / addends(kind, z64, y), fwd))
    _note(report, "%s/%s/>2^24" % (kind, "streamed" if wide else "resident"), epi, fwd)
    ctx.close()


def _scaled_to(w, z64, targets):
    """Scale each output row of the last layer so that column j of the pre-activations reaches |z| = targets[j] (tanh / bias-free
    last layer: z is linear in that row)."""
    w = [wi.copy() for wi in w]
    for j, t in enumerate(targets):
        if t is not None:
            w[-1][j] *= t / np.abs(z64[:, j]).max()
    return w


@pytest.mark.parametrize("edge", ["poi_eta80", "nb_logit30", "nb10_logit30", "nb2d_logit30", "err_sigma_exp-60"])
@pytest.mark.parametrize("wide", [False, True])
def test_output_value_edges(edge, wide, hip, report):
    """eta to +-80 (exp near float32's overflow, in float64 finite), NegBin logits to +-30 (p -> 0 / 1: 1 - p, log1p(-p)), the
    predicted sigma's softplus argument to -60 (sigma ~ e^-60).  The device must give float64's likelihood of its own outputs
    (the epilogue bar); where the float64 reference is not finite (base 10: p = 1 / (1 + 10^-30) rounds to 1, n = inf) the device
    must give the same class of value.  The forward bar does not apply here: a float32 output of 80 carries an error of ~1e-5
    whatever the kernel does, and exp / 1/sigma^2 amplify it past 2e-6 of S."""
    kind, rest = edge.split("_", 1)
    rs = np.random.default_rng(zlib.crc32(edge.encode()))
    n, f, hidden = 1025, 9, (8, 6)
    k = {"poi": 1, "nb": 1, "nb10": 1, "nb2d": 2, "err": 2}[kind]
    n_out = 1 if kind == "poi" else 2 * k
    x = rs.standard_normal((n, f))
    w = make_weights(rs, f, hidden, n_out, 2)
    act = orc.Act("tanh")
    z64 = orc.forward_logits(_f32(x), w, act)
    if kind == "poi":
        w = _scaled_to(w, z64, [80.0])
    elif kind == "err":
        w = _scaled_to(w, z64, [3.0] * k + [60.0] * k)
    else:
        w = _scaled_to(w, z64, [4.0] * (n_out // 2) + [30.0] * (n_out // 2))
    z64 = orc.forward_logits(_f32(x), w, act)
    assert np.abs(z64).max() >= (80 if kind == "poi" else 30) - 1e-9
    if kind == "poi":
        y = rs.poisson(np.exp(np.clip(z64[:, :1], -30, 30))).astype(float)
    elif kind == "err":
        y = _f32(rs.standard_normal((n, k)))
    else:
        y = rs.poisson(5.0, (n, k)).astype(float)
    ctx = make_ctx(hip, x, w, act, kind, y, n_out, wide=wide)
    got = ctx.eval(w)["loglik"]
    z32 = ctx.predict(w, apply_out_fn=False)
    want = oracle_lik(kind, z32, _f32(y))
    if kind == "nb10":
        assert not np.isfinite(want), "the base-10 edge is meant to reach p == 1"
    epi, _ = check_bars(kind, got, z32, z64, _f32(y), forward=False)
    _note(report, "%s/%s/edges" % (kind, "streamed" if wide else "resident"), epi, 0.0)
    ctx.close()
