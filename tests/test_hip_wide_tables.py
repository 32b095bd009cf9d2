"""GPU tests of the weight-streamed path (npbnn_amd/csrc/npbnn_wide.hip) on several tables per context.

The path sizes its launches from the table being evaluated - its tiling (128-row blocks below 32 513 rows) and the K-slices a layer's
contraction is cut into (more on fewer rows: fewer row blocks fill the chip) - while its device buffers live on the context.  These
tests evaluate tables of different plans one after the other on one context, in both orders, and hold every result to the float64
oracle and every repeated evaluation to the first one, bit for bit (a pass that wrote past its buffers would show there):

- a training and a test table whose plans differ (the smaller one cut into more K-slices; the tiling switch crossed; the test table
  the larger one), evaluated train / test / train and test / train / test;
- one context whose training table goes through row counts from 16 to 100 000 and back;
- every K-slice count NPBNN_WIDE_SLICES can force;
- a chain over a training table with a test table evaluated on every logged sample, through mh_step and run_steps;
- the same network and data whether the architecture or the data came first (the path reads the training table's row count)."""
import functools

import numpy as np
import pytest

import cases
import oracle as orc
import npbnn_amd as bn
from npbnn_amd import _capi as capi
from test_hip_wide import LL_RTOL, Z_TOL, assert_close, check_confusion

pytestmark = pytest.mark.gpu

TRAIN, TEST = capi.TRAIN, capi.TEST
TANH = orc.Act("tanh")


@pytest.fixture(scope="module")
def n_cu():
    ctx = bn.HipContext(0)
    v = ctx.info(capi.INFO_N_CU)
    ctx.close()
    return v


def scaled(rows, n_cu):
    """The row counts below are chosen for 256 compute units; the plans follow the units the device reports (row blocks per unit)."""
    return rows if n_cu == 256 else max(16, int(round(rows * n_cu / 256.0)))


@functools.lru_cache(maxsize=None)
def problem(seed, n, f, hidden, c):
    rs = np.random.default_rng(seed)
    x = rs.standard_normal((n, f)).astype(np.float32)
    lab = rs.integers(0, c, n)
    dims = [f] + list(hidden) + [c]
    w = [rs.normal(0, 1.5 / np.sqrt(dims[l] + 1), (dims[l + 1], dims[l] + 1)) for l in range(len(dims) - 1)]
    return x, lab, w


@functools.lru_cache(maxsize=None)
def _oracle(seed, n, f, hidden, c, lo, hi):
    x, lab, w = problem(seed, n, f, hidden, c)
    x64 = x[lo:hi].astype(np.float64)
    y64 = orc.forward(x64, w, TANH, orc.out_softmax)
    z64 = orc.forward_logits(x64, w, TANH)
    return orc.lik_categorical(y64, lab[lo:hi], np.arange(hi - lo)), y64, z64


def check_table(ctx, which, key, lo, hi, f):
    """eval (log-likelihood, confusion counts) and predict (last layer's values) of one table against the oracle."""
    x, lab, w = problem(*key)
    want, y64, z64 = _oracle(*key, lo, hi)
    r = ctx.eval(w, which=which, want_confusion=True)
    assert abs(r["loglik"] - want) <= LL_RTOL * abs(want), (which, hi - lo, r["loglik"], want)
    check_confusion(r["confusion"], y64, lab[lo:hi])
    z = ctx.predict(w, which=which, apply_out_fn=False)
    assert_close(z, z64, Z_TOL * max(1.0, np.sqrt(f / 1024.0)))
    return r["loglik"], r["confusion"], z


def k_slices(key, lo, hi, precision):
    """The K-slices of the first layer's product on this table alone (a context that holds only it: npbnn_time_wide)."""
    x, lab, w = problem(*key)
    ctx = bn.HipContext(0)
    ctx.set_l0_precision(precision)
    ctx.set_data(x[lo:hi])
    ctx.set_labels(lab[lo:hi])
    ctx.set_arch_from_weights(w, x.shape[1], capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_CATEGORICAL)
    assert ctx.is_wide()
    geo = ctx.time_wide(w, iters=1)[2]
    ctx.close()
    return geo["k_slices"]


# (network, features, train rows, test rows); on 256 compute units, first layer's K-slices train -> test in the comment
PAIRS = {
    "default-net-11200-6400-test-more-slices": ((50, 5), 1024, 11200, 6400),          # 2 -> 4 (the advisor's first row)
    "256-64-20000-8000-test-more-slices": ((256, 64), 2048, 20000, 8000),             # 3 -> 8 (its second row)
    "tiling-switch-40000-10000-test-more-slices": ((50, 5), 1024, 40000, 10000),      # 1 (256-row blocks, fused) -> 3 (128-row blocks)
    "tiling-switch-10000-40000-test-fewer-slices": ((50, 5), 1024, 10000, 40000),     # 3 -> 1
    "default-net-6400-11200-test-fewer-slices": ((50, 5), 1024, 6400, 11200),         # 4 -> 2
}


@pytest.mark.parametrize("precision", ["auto", "f32"])
@pytest.mark.parametrize("name", list(PAIRS))
def test_train_and_test_tables_of_different_plans_on_one_context(name, precision, n_cu):
    hidden, f, n_tr, n_te = PAIRS[name]
    n_tr, n_te = scaled(n_tr, n_cu), scaled(n_te, n_cu)
    key = (7, n_tr + n_te, f, hidden, 10)
    x, lab, w = problem(*key)
    span = {TRAIN: (0, n_tr), TEST: (n_tr, n_tr + n_te)}
    sl = {t: k_slices(key, *span[t], precision) for t in (TRAIN, TEST)}
    if name.endswith("test-more-slices"):
        assert sl[TEST] > sl[TRAIN], sl
    else:
        assert sl[TEST] < sl[TRAIN], sl
    for first, second in ((TRAIN, TEST), (TEST, TRAIN)):
        ctx = bn.HipContext(0)
        ctx.set_l0_precision(precision)
        for t in (first, second):              # (the table evaluated first is also the one allocated first)
            ctx.set_data(x[span[t][0]:span[t][1]], t)
            ctx.set_labels(lab[span[t][0]:span[t][1]], t)
        ctx.set_arch_from_weights(w, f, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_CATEGORICAL)
        assert ctx.is_wide()
        seen = {}
        for t in (first, second, first):
            ll, conf, z = check_table(ctx, t, key, *span[t], f)
            if t in seen:       # the other table's pass left this table's results alone, to the bit
                assert ll == seen[t][0], (t, ll, seen[t][0])
                assert np.array_equal(conf, seen[t][1])
                assert np.array_equal(z, seen[t][2])
            seen[t] = (ll, conf, z)
        assert ctx.l0_mode() == ("f16-split" if precision == "auto" else "f32")
        ctx.close()


SWEEP = [100000, 40005, 32768, 32767, 32513, 32512, 11200, 10000, 8000, 4099, 257, 255, 17, 16]


@pytest.mark.parametrize("precision", ["auto", "f32"])
def test_training_table_row_sweep_on_one_context(precision, n_cu):
    """[50, 5] on 1024 features, the training table re-set on one context from 100 000 rows down to 16 and back up: ragged last
    tiles, partial 128- / 256-row blocks, both tilings of the first layer, 1-4 K-slices (its 32 K-units allow no more).  Every
    evaluation is the oracle's, and the second visit to a row count the first one's, bit for bit."""
    rows = [scaled(n, n_cu) for n in SWEEP]
    key = (8, max(rows), 1024, (50, 5), 10)
    x, lab, w = problem(*key)
    ctx = bn.HipContext(0)
    ctx.set_l0_precision(precision)
    first = {}
    slices = set()
    for i, n in enumerate(rows + rows[::-1]):
        ctx.set_data(x[:n])
        ctx.set_labels(lab[:n])
        if i == 0:
            ctx.set_arch_from_weights(w, 1024, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_CATEGORICAL)
        assert ctx.is_wide()
        ll, conf, z = check_table(ctx, TRAIN, key, 0, n, 1024)
        if n in first:
            assert ll == first[n][0], (n, ll, first[n][0])
            assert np.array_equal(z, first[n][1])
        else:
            first[n] = (ll, z)
            slices.add(ctx.time_wide(w, iters=1)[2]["k_slices"])
    if n_cu == 256:
        assert slices == {1, 2, 3, 4}, slices
    ctx.close()


def _regression_problem(seed, n, f, hidden, k):
    rs = np.random.default_rng(seed)
    x = rs.standard_normal((n, f)).astype(np.float32)
    dims = [f] + list(hidden) + [k]
    w = [rs.normal(0, 1.0 / np.sqrt(dims[l] + 1), (dims[l + 1], dims[l] + 1)) for l in range(len(dims) - 1)]
    y64 = orc.forward(x.astype(np.float64), w, TANH, orc.out_identity)
    t = y64 + rs.normal(0, 0.7, y64.shape)
    return x, w, t, y64


FORCED = {
    # (rows, features, hidden, classes or Gaussian targets, regression)
    "classification-default-net": (3000, 1024, (50, 5), 10, False),
    "classification-4-k-units": (3000, 100, (50, 5), 10, False),          # 100 features: 4 K-units, the count is clamped to 4
    "regression-3-targets": (5000, 1500, (64, 8), 3, True),
}


@pytest.mark.parametrize("name", list(FORCED))
def test_every_forced_slice_count(name, monkeypatch):
    """NPBNN_WIDE_SLICES = 1..8 (read when the product is planned): the log-likelihood is the oracle's, and 2..8 slices agree with
    one to LL_RTOL; the first layer's product reports the count, clamped to its K-units."""
    n, f, hidden, c, regression = FORCED[name]
    if regression:
        x, w, t, y64 = _regression_problem(4, n, f, hidden, c)
        sig = np.linspace(0.6, 1.8, c)
        want = orc.lik_gaussian(y64, t, sig2=sig)
    else:
        x, lab, w = problem(9, n, f, hidden, c)
        want = _oracle(9, n, f, hidden, c, 0, n)[0]
    units = (f + 31) // 32
    lls = {}
    for s in range(1, 9):
        monkeypatch.setenv("NPBNN_WIDE_SLICES", str(s))
        ctx = bn.HipContext(0)
        ctx.set_wide(True)
        ctx.set_data(x)
        if regression:
            ctx.set_targets(t)
            ctx.set_arch_from_weights(w, f, capi.ACT_TANH, capi.OUT_IDENTITY, capi.LIK_GAUSS, c)
            lls[s] = ctx.eval(w, sigma=sig)["loglik"]
        else:
            ctx.set_labels(lab)
            ctx.set_arch_from_weights(w, f, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_CATEGORICAL)
            r = ctx.eval(w, want_confusion=True)
            lls[s] = r["loglik"]
            check_confusion(r["confusion"], _oracle(9, n, f, hidden, c, 0, n)[1], lab)
        assert ctx.is_wide()
        assert ctx.time_wide(w, iters=1)[2]["k_slices"] == min(s, units)
        assert abs(lls[s] - want) <= LL_RTOL * abs(want), (s, lls[s], want)
        ctx.close()
    for s in range(2, 9):
        assert abs(lls[s] - lls[1]) <= LL_RTOL * abs(lls[1]), (s, lls[s], lls[1])


def _test_accuracy_is_the_oracles(mcmc, bnn, dat):
    y64 = orc.forward(dat["test_data"], bnn._w_layers, TANH, orc.out_softmax)
    want = orc.acc_classification(y64, dat["test_labels"])
    top2 = np.sort(y64, axis=1)[:, -2:]
    near_ties = int(np.sum(top2[:, 1] - top2[:, 0] < 1e-5))
    n = len(dat["test_labels"])
    assert abs(mcmc._test_accuracy - want) * n <= near_ties + 1e-9, (mcmc._test_accuracy, want)


def test_chain_with_a_test_table_of_more_slices():
    """A run_mcmc-style chain on the reference's default network over 11 200 training and 6 400 test rows (the test table cut into
    twice the training table's K-slices): test accuracy logged every 30 iterations, through mh_step and through run_steps - the same
    decisions and weights bit for bit, the accuracies the oracle's."""
    from test_hip_wide import _chains
    dat = cases.classification_data(13, 11200, 1024, 10, n_test=6400)
    (bnn_a, mcmc_a), (bnn_b, mcmc_b) = _chains(dat, dict(n_nodes=[50, 5], use_bias_node=2, prior_f=1, p_scale=1), dict(fun="tanh"),
                                               dict(update_f=[0.02] * 3, update_ws=[0.05] * 3, n_iteration=100000))
    assert mcmc_a._backend.ctx.is_wide()
    _test_accuracy_is_the_oracles(mcmc_a, bnn_a, dat)
    _test_accuracy_is_the_oracles(mcmc_b, bnn_b, dat)
    for _ in range(3):
        for _ in range(30):
            mcmc_a.mh_step(bnn_a)
        mcmc_b.run_steps(bnn_b, 30)
        assert mcmc_a._last_accepted_mem == mcmc_b._last_accepted_mem
        for wa, wb in zip(bnn_a._w_layers, bnn_b._w_layers):
            np.testing.assert_array_equal(wa, wb)
        _test_accuracy_is_the_oracles(mcmc_a, bnn_a, dat)
        _test_accuracy_is_the_oracles(mcmc_b, bnn_b, dat)
        assert mcmc_a._test_accuracy == mcmc_b._test_accuracy
    assert mcmc_b._device_iterations == 90
    np.testing.assert_allclose(mcmc_b._logLik, mcmc_a._logLik, rtol=1e-12)
    y64 = orc.forward(dat["data"], bnn_b._w_layers, TANH, orc.out_softmax)
    want = orc.lik_categorical(y64, dat["labels"], np.arange(len(dat["labels"])))
    assert abs(mcmc_b._logLik - want) / abs(want) < LL_RTOL


def _short_chain(ctx, w):
    """40 device iterations of three-entry proposals with fixed draws: the accept / reject sequence, proposed log-likelihoods, weights."""
    rs = np.random.default_rng(21)
    n_w = sum(wi.size for wi in w)
    K, M = 40, 3
    idx = np.sort(np.stack([rs.choice(n_w, M, replace=False) for _ in range(K)]), axis=1).astype(np.int32)
    delta = rs.normal(0, 0.02, (K, M))
    cnt = np.full(K, M, dtype=np.int32)
    log_u = np.log(rs.uniform(size=K))
    ll0 = ctx.eval(w)["loglik"]
    lp0 = -0.5 * sum(float(np.sum(wi ** 2)) for wi in w)
    w_new, acc, llp, _, _ = ctx.chain_run(w, idx, delta, cnt, log_u, prior_kind=capi.PRIOR_NORMAL, prior_scale=np.ones(len(w)),
                                          w_bound=np.inf, temperature=1.0, lik_temp=1.0, cur_loglik=ll0, cur_logprior=lp0)
    return ll0, w_new, acc.copy(), llp


def test_call_order_does_not_choose_the_path():
    """[32, 8] on 1024 features: the streamed path from 65 536 training rows on, the resident one below (wide_needed).  Architecture
    before data, data before architecture, and a live context whose training table grows from 30 000 to 70 000 rows: each picks the
    path a fresh context picks for that table, evaluates to the oracle, and runs the same short chain bit for bit."""
    n_big, n_small, f = 70000, 30000, 1024
    key = (10, n_big, f, (32, 8), 6)
    x, lab, w = problem(*key)

    def fresh(n, arch_first=False):
        ctx = bn.HipContext(0)
        if arch_first:
            ctx.set_arch_from_weights(w, f, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_CATEGORICAL)
        ctx.set_data(x[:n])
        ctx.set_labels(lab[:n])
        if not arch_first:
            ctx.set_arch_from_weights(w, f, capi.ACT_TANH, capi.OUT_SOFTMAX, capi.LIK_CATEGORICAL)
        return ctx

    data_first = fresh(n_big)
    assert data_first.is_wide()
    check_table(data_first, TRAIN, key, 0, n_big, f)
    ref = _short_chain(data_first, w)
    data_first.close()
    small = fresh(n_small)
    assert not small.is_wide()
    check_table(small, TRAIN, key, 0, n_small, f)
    small.close()

    arch_first = fresh(n_big, arch_first=True)
    live = fresh(n_small)
    check_table(live, TRAIN, key, 0, n_small, f)
    live.set_data(x[:n_big])
    live.set_labels(lab[:n_big])
    for ctx in (arch_first, live):
        assert ctx.is_wide()
        check_table(ctx, TRAIN, key, 0, n_big, f)
        ll0, w_new, acc, llp = _short_chain(ctx, w)
        assert ll0 == ref[0]
        assert np.array_equal(acc, ref[2])
        np.testing.assert_array_equal(llp, ref[3])
        np.testing.assert_array_equal(w_new, ref[1])
        ctx.close()
