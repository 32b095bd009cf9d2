"""The shared preparation behind the stored-sample entries and the grouped chain calls, on the host (no GPU): every one of the twelve
``HipContext`` entries that take ``weight_sets`` refuses a wrong number of slope vectors and an empty list of sets before the library
is touched, the three input forms pack to the same bytes, the one ``ChainJob`` builder fills the struct both grouped calls hand over,
and ``sigma_matrix`` has its two levels of strictness.  (The bare context is the pattern of test_host_lppd._bare_context.)"""
import ctypes as C
import importlib

import numpy as np
import pytest

from npbnn_amd import _capi as capi

backend = importlib.import_module("npbnn_amd.backend")
stored = importlib.import_module("npbnn_amd.stored")

N_ROWS, N_OUT, N_SETS = 10, 3, 16
SHAPES = ((4, 6), (3, 5))                     # 5 inputs, 4 hidden nodes, 3 outputs, a bias each
N_W = sum(r * c for r, c in SHAPES)


class _NoDevice:
    touched = []

    def __getattr__(self, name):
        _NoDevice.touched.append(name)
        raise AssertionError("device call %s" % name)


def _bare_context(n_layers=2):
    ctx = backend.HipContext.__new__(backend.HipContext)
    ctx._lib = _NoDevice()
    ctx._ctx = None
    ctx.n_rows = {capi.TRAIN: N_ROWS, capi.TEST: 0}
    ctx.n_out = N_OUT
    ctx.arch = capi.Arch()
    ctx.arch.n_layers = n_layers
    ctx.close = lambda: None
    return ctx


LABELS = np.zeros(N_ROWS, dtype=np.int64)
ENTRIES = {
    "predict_sets": lambda ctx, sets, ap: ctx.predict_sets(sets, act_prm_sets=ap),
    "predict_sets_hpd": lambda ctx, sets, ap: ctx.predict_sets_hpd(sets, 0.9, act_prm_sets=ap),
    "predict_sets_summary": lambda ctx, sets, ap: ctx.predict_sets_summary(sets, 0, act_prm_sets=ap),
    "predict_sets_support": lambda ctx, sets, ap: ctx.predict_sets_support(sets, 0, LABELS, [0.5], act_prm_sets=ap),
    "predict_sets_lppd": lambda ctx, sets, ap: ctx.predict_sets_lppd(sets, capi.LIK_CATEGORICAL, act_prm_sets=ap),
    "predict_sets_uncertainty": lambda ctx, sets, ap: ctx.predict_sets_uncertainty(sets, act_prm_sets=ap),
    "predict_sets_calibration": lambda ctx, sets, ap: ctx.predict_sets_calibration(sets, act_prm_sets=ap),
    "predict_sets_convergence": lambda ctx, sets, ap: ctx.predict_sets_convergence(sets, 2, act_prm_sets=ap),
    "predict_pdp": lambda ctx, sets, ap: ctx.predict_pdp(sets, [0], [[0.0]], act_prm_sets=ap),
    "predict_ale": lambda ctx, sets, ap: ctx.predict_ale(sets, 0, [0.0, 1.0], act_prm_sets=ap),
    "predict_saliency": lambda ctx, sets, ap: ctx.predict_saliency(sets, act_prm_sets=ap),
    "predict_shapley": lambda ctx, sets, ap: ctx.predict_shapley(sets, [0], [1], [[0, 1]], act_prm_sets=ap),
}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n_slopes", [N_SETS - 1, N_SETS + 1])
def test_slope_vectors_must_match_the_sets(entry, n_slopes):
    """One slope vector fewer (the library would read past the buffer's end) and one more than weight sets."""
    _NoDevice.touched = []
    for sets in (np.zeros((N_SETS, N_W)), [np.zeros(N_W)] * N_SETS):
        with pytest.raises(ValueError, match="%s: %d slope vectors for %d weight sets" % (entry, n_slopes, N_SETS)):
            ENTRIES[entry](_bare_context(), sets, [np.full(1, 0.1)] * n_slopes)
    assert _NoDevice.touched == []


@pytest.mark.parametrize("entry", ENTRIES)
def test_no_weight_sets(entry):
    """All twelve entries: no test expects the library's answer to an empty list through one of them, so none is left out."""
    _NoDevice.touched = []
    for sets in ([], np.zeros((0, N_W))):
        with pytest.raises(ValueError, match="%s: no weight sets" % entry):
            ENTRIES[entry](_bare_context(), sets, None)
    assert _NoDevice.touched == []


def test_the_three_input_forms_pack_alike():
    rs = np.random.default_rng(5)
    layers = [[rs.standard_normal(s) for s in SHAPES] for _ in range(3)]
    vectors = [backend.pack_weights(w) for w in layers]
    matrix = np.stack(vectors)
    assert matrix.shape == (3, N_W) and matrix.dtype == np.float64 and matrix.flags.c_contiguous
    ctx = _bare_context()
    slopes = [np.array([0.1 * (i + 1), 9.0]) for i in range(3)]               # (an entry too many each: cut to the hidden layers)
    got = [ctx._pack_sets(form, slopes, "t") for form in (layers, vectors, matrix)]
    for packed, ap, n_sets in got:
        assert n_sets == 3 and packed.dtype == np.float64 and packed.flags.c_contiguous and packed.tobytes() == matrix.tobytes()
        assert ap.dtype == np.float64 and ap.flags.c_contiguous and ap.tolist() == [[0.1], [0.2], [0.30000000000000004]]
    assert got[2][0] is matrix                                                   # taken as it is: no copy
    f32 = matrix.astype(np.float32)
    assert ctx._pack_sets(f32, None, "t")[0].tobytes() == f32.astype(np.float64).tobytes()
    assert ctx._pack_sets(np.asfortranarray(matrix), None, "t")[0].flags.c_contiguous
    assert ctx._pack_sets(matrix, None, "t")[1] is None


def test_one_layer_has_no_slopes():
    ctx = _bare_context(n_layers=1)
    packed, ap, n_sets = ctx._pack_sets(np.zeros((4, 7)), [np.full(1, 0.1)] * 4, "t")
    assert ap is None and n_sets == 4
    assert ctx._pack_sets(np.zeros((4, 7)), [np.full(1, 0.1)] * 3, "t")[1] is None      # (nothing is read: nothing to count)


def test_one_vector():
    rs = np.random.default_rng(6)
    layers = [rs.standard_normal(s) for s in SHAPES]
    vec = backend.pack_weights(layers)
    assert backend.one_vector(layers).tobytes() == vec.tobytes() and backend.one_vector(tuple(layers), copy=True).tobytes() == vec.tobytes()
    assert backend.one_vector(vec) is vec
    copied = backend.one_vector(vec, copy=True)
    assert copied is not vec and not np.shares_memory(copied, vec) and copied.tobytes() == vec.tobytes()
    assert backend.one_vector(vec.astype(np.float32)).dtype == np.float64


# ---- the ChainJob builder -----------------------------------------------------------------------------------------------------------
K, M = 4, 2


def _job(rows=K, chain_id=5, mask=True):
    rs = np.random.default_rng(7)
    ctx = _bare_context()
    cfg = dict(prior_kind=capi.PRIOR_NORMAL, prior_scale=np.ones(2), w_bound=np.inf, temperature=1.0, lik_temp=1.0, cur_loglik=-3.0, cur_logprior=-2.0)
    return dict(ctx=ctx, chain_id=chain_id, weights=rs.standard_normal(N_W), idx=rs.integers(0, N_W, (rows, M)).astype(np.int64),
                delta=rs.standard_normal((rows, M)), cnt=np.full(rows, M, dtype=np.int64), log_u=-rs.random(rows),
                mask=[np.ones(s) for s in SHAPES] if mask else None, cfg=cfg)


def _at(pointer, array):
    return C.cast(pointer, C.c_void_p).value == array.ctypes.data


def test_chain_job_builder():
    _NoDevice.touched = []
    arr = (capi.ChainJob * 1)()
    job = _job()
    kept, out = backend.fill_chain_job(arr[0], 0, job, K, "%d" % K, 5, force_f32=1, n_seg=2, want_cold_w=True)
    w, idx, cnt, delta, log_u, m, cfg, res = kept
    J = arr[0]
    assert J.M == M and J.chain_id == 5 and J.ctx is None
    assert idx.dtype == np.int32 and idx.shape == (K, M) and idx.flags.c_contiguous and idx is not job["idx"] and np.array_equal(idx, job["idx"])
    assert cnt.dtype == np.int32 and cnt.shape == (K,) and cnt is not job["cnt"] and np.array_equal(cnt, job["cnt"])
    assert w.dtype == np.float64 and w.shape == (N_W,) and w is not job["weights"] and np.array_equal(w, job["weights"]) and out["w"] is w
    assert m.dtype == np.float64 and m.shape == (N_W,) and delta.shape == (K, M) and log_u.shape == (K,)
    assert _at(J.W_inout, w) and _at(J.mask_packed, m) and _at(J.idx, idx) and _at(J.cnt, cnt) and _at(J.delta, delta) and _at(J.log_u, log_u)
    assert (out["accepted"].dtype, out["accepted"].shape) == (np.uint8, (K,)) and _at(J.out_accepted, out["accepted"])
    for key, pointer in (("loglik_prop", J.out_loglik_prop), ("logprior_prop", J.out_logprior_prop)):
        assert (out[key].dtype, out[key].shape) == (np.float64, (K,)) and _at(pointer, out[key])
    assert out["state"].shape == (2, capi.XSTATE_DOUBLES) and _at(J.out_state, out["state"])
    assert out["cold_w"].shape == (2, N_W) and _at(J.out_cold_w, out["cold_w"])
    assert C.addressof(J.cfg.contents) == C.addressof(cfg) and C.addressof(J.result.contents) == C.addressof(res)
    assert cfg.force_f32 == 1 and cfg.cur_loglik == -3.0 and cfg.prior_kind == capi.PRIOR_NORMAL
    assert list(out) == ["w", "accepted", "loglik_prop", "logprior_prop", "_res", "_ctx", "state", "cold_w"]
    # the batched form: no per-exchange outputs, no mask; draws of the right type are passed through, not copied
    plain = _job(mask=False)
    plain["idx"], plain["cnt"] = plain["idx"].astype(np.int32), plain["cnt"].astype(np.int32)
    J = (capi.ChainJob * 1)()[0]                     # (a fresh struct, as both callers make one per call)
    kept, out = backend.fill_chain_job(J, 2, plain, K, "%d" % K, 2)
    assert kept[1] is plain["idx"] and kept[2] is plain["cnt"] and kept[5] is None and kept[6].force_f32 == 0
    assert not J.mask_packed and not J.out_state and not J.out_cold_w and J.chain_id == 2
    assert list(out) == ["w", "accepted", "loglik_prop", "logprior_prop", "_res", "_ctx"]
    J = (capi.ChainJob * 1)()[0]
    kept, out = backend.fill_chain_job(J, 0, _job(), K, "", 0, n_seg=2)
    assert out["cold_w"] is None and not J.out_cold_w and J.out_state
    assert _NoDevice.touched == []


def test_rows_of_draws_are_counted_before_the_library_is_used():
    _NoDevice.touched = []
    with pytest.raises(ValueError, match=r"job 1: 3 rows of draws for 2 x 2 iterations"):
        backend.chains_run_exchange([_job(), _job(rows=K - 1)], 2, 2, 2, [0], [1], [0.0])
    with pytest.raises(ValueError, match=r"job 0: 3 rows of draws for 4 iterations"):
        backend.chains_run_batched([_job(rows=K - 1), _job()], K)
    short_cnt = _job()
    short_cnt["cnt"] = short_cnt["cnt"][:-1]
    with pytest.raises(ValueError, match="rows of draws"):
        backend.chains_run_batched([short_cnt], K)
    assert _NoDevice.touched == []


# ---- sigma_matrix -------------------------------------------------------------------------------------------------------------------
S, T = 5, 3


@pytest.mark.parametrize("positive", [True, False])
def test_sigma_matrix_shapes(positive):
    rs = np.random.default_rng(8)
    per_sample = rs.uniform(0.5, 2.0, S)
    for given in (per_sample, per_sample.reshape(S, 1), np.repeat(per_sample, T).reshape(S, T), list(per_sample)):
        sig = stored.sigma_matrix(given, S, T, "t", positive=positive)
        assert sig.shape == (S, T) and sig.dtype == np.float64 and np.array_equal(sig, np.repeat(per_sample, T).reshape(S, T))
        assert sig.flags.c_contiguous or not positive
    for bad in (np.ones(S + 1), np.ones((S, T + 1)), np.ones((S, 2)), np.ones((S, T, 1)), np.ones((T, S))):
        with pytest.raises(ValueError, match="expected"):
            stored.sigma_matrix(bad, S, T, "t", positive=positive)
    with pytest.raises(ValueError, match="needs sigma_sets"):
        stored.sigma_matrix(None, S, T, "t", positive=positive)


def test_sigma_matrix_strictness():
    for positive in (True, False):
        sig = np.ones((S, T))
        sig[2, 1] = np.nan
        with pytest.raises(ValueError, match="t: "):
            stored.sigma_matrix(sig, S, T, "t", positive=positive)
    for entry in (0.0, -1.0, np.inf):
        sig = np.ones((S, T))
        sig[2, 1] = entry
        with pytest.raises(ValueError, match="positive and finite"):
            stored.sigma_matrix(sig, S, T, "t")
        assert np.array_equal(stored.sigma_matrix(sig, S, T, "t", positive=False), sig)
