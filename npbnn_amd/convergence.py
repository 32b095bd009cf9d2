"""Convergence diagnostics of stored posterior samples in function space: ``posterior_convergence``,
``get_posterior_convergence``.

The reference leaves convergence to an external trace viewer on the logged weights.  For a network that is the wrong quantity: hidden
units can be permuted and rescaled without changing the function, so two chains that agree on every prediction can sit in different
weight modes.  Here the diagnostic is taken per (row, output) of the stored samples' predictions: the S predictions of a cell are a
time series, and the questions are whether the chains agree (split R-hat) and how many independent draws they are worth (effective
sample size).  Float64 throughout.  A column is M chains of N draws each, chain-major (sample ``s = j*N + t``), 1 <= M <= 64, N >= 8,
M*N <= 16384.  Each chain is split into halves of ``n = N // 2`` draws, ``t in [0, n)`` and ``t in [N-n, N)`` (the middle draw of an
odd N is dropped): ``m = 2M`` split chains.  For each split chain k:

    mu_k = (1/n) sum x      d = x - mu_k      acov_k(t) = (1/n) sum_{i < n-t} d_i d_{i+t}      s2_k = acov_k(0) n/(n-1)

and over the split chains:

    W = mean_k s2_k      Bn = sum_k (mu_k - mean mu)^2 / (m-1)      varp = W (n-1)/n + Bn      rhat = sqrt(varp / W)
    rho(0) = 1           rho(t) = 1 - (W - mean_k acov_k(t)) / varp

Effective sample size: ``P_0 = rho(0) + rho(1)``; for k = 1, 2, ... while ``2k+1 <= n-1``: ``P_k = rho(2k) + rho(2k+1)``, stop at
the first ``P_k < 0`` (that pair is not added), otherwise ``P_k = min(P_k, P_{k-1})`` is added; ``tau = max(-1 + 2 sum P_k,
1 / log10(m n))`` and ``ess = m n / tau``.  A column with ``W == 0`` (every split chain constant) has ``rhat = ess = NaN`` and counts
as constant.  No rank normalisation, no tail ESS, no lag cap.

``posterior_convergence`` is that definition on a host ``[S, N_rows, outputs]`` array in plain numpy.
``get_posterior_convergence`` replays the stored samples of one checkpoint per chain into a float32 stack that stays on the device
(``npbnn_predict_sets_convergence``): one launch reads it once and only the diagnostics come back."""
import numpy as np

from .files import load_obj
from .stored import choose_table, open_predictor

MAX_CHAINS = 64
MIN_DRAWS = 8
MAX_SAMPLES = 16384
_CHUNK = 1 << 15              # columns of one pass of posterior_convergence


def check_shape(who, n_samples, n_chains):
    """The limits of a column; returns the draws per chain."""
    n_chains = int(n_chains)
    if n_samples < 1:
        raise ValueError("%s: no samples" % who)
    if not 1 <= n_chains <= MAX_CHAINS:
        raise ValueError("%s: %d chains, 1 to %d are supported" % (who, n_chains, MAX_CHAINS))
    if n_samples % n_chains:
        raise ValueError("%s: %d samples do not divide into %d chains of equal length" % (who, n_samples, n_chains))
    n_draws = n_samples // n_chains
    if n_draws < MIN_DRAWS:
        raise ValueError("%s: %d draws per chain, at least %d are needed" % (who, n_draws, MIN_DRAWS))
    if n_samples > MAX_SAMPLES:
        raise ValueError("%s: %d samples, at most %d are supported" % (who, n_samples, MAX_SAMPLES))
    return n_draws


def _columns(x, n_chains):
    """(rhat, ess) of the columns of x [S, cols], float64."""
    n_draws = x.shape[0] // n_chains
    n, m, cols = n_draws // 2, 2 * n_chains, x.shape[1]
    x = x.reshape(n_chains, n_draws, cols)
    d = np.stack([x[:, :n], x[:, n_draws - n:]], axis=1).reshape(m, n, cols)      # split chain k = 2 j + half
    mu = np.sum(d, axis=1) / n
    d = d - mu[:, None, :]
    s2 = np.sum(d * d, axis=1) / n * n / (n - 1)
    w = np.sum(s2, axis=0) / m
    bn = np.sum((mu - np.sum(mu, axis=0) / m) ** 2, axis=0) / (m - 1)
    varp = w * (n - 1) / n + bn
    rhat = np.full(cols, np.nan)
    ess = np.full(cols, np.nan)
    live = np.flatnonzero(w != 0)
    rhat[live] = np.sqrt(varp[live] / w[live])

    def rho(t, idx):
        a = np.sum(d[:, :n - t, idx] * d[:, t:, idx], axis=(0, 1)) / n / m
        return 1.0 - (w[idx] - a) / varp[idx]

    prev = 1.0 + rho(1, live)
    total = prev.copy()               # per live column; `on` indexes the columns whose sequence still runs
    on = np.arange(len(live))
    k = 1
    while 2 * k + 1 <= n - 1 and len(on):
        p = rho(2 * k, live[on]) + rho(2 * k + 1, live[on])
        keep = ~(p < 0)
        on, p = on[keep], p[keep]
        p = np.minimum(p, prev[on])
        total[on] += p
        prev[on] = p
        k += 1
    tau = np.maximum(-1.0 + 2.0 * total, 1.0 / np.log10(m * n))
    ess[live] = m * n / tau
    return rhat, ess


def summarise(rhat, ess, rhat_threshold):
    """[outputs, 4] of rhat / ess [rows, outputs]: the largest rhat, the smallest ess, the columns with rhat > threshold, the
    constant columns (NaN) - NaNs take no part in the largest / smallest, which are NaN when every column is constant."""
    out = np.full((rhat.shape[1], 4), np.nan)
    for o in range(rhat.shape[1]):
        a, e = rhat[:, o], ess[:, o]
        if np.any(~np.isnan(a)):
            out[o, 0] = np.nanmax(a)
        if np.any(~np.isnan(e)):
            out[o, 1] = np.nanmin(e)
        with np.errstate(invalid="ignore"):
            out[o, 2] = np.count_nonzero(a > rhat_threshold)
        out[o, 3] = np.count_nonzero(np.isnan(a))
    return out


def result_dict(rhat, ess, summary, n_rows, n_chains, n_draws):
    """The dict both routes return, from the per-output summary [outputs, 4]."""
    n_cols = n_rows * summary.shape[0]
    return dict(rhat=rhat, ess=ess,
                max_rhat=float(np.nanmax(summary[:, 0])) if np.any(~np.isnan(summary[:, 0])) else float("nan"),
                min_ess=float(np.nanmin(summary[:, 1])) if np.any(~np.isnan(summary[:, 1])) else float("nan"),
                frac_rhat_above=float(np.sum(summary[:, 2]) / n_cols), n_constant=int(np.sum(summary[:, 3])),
                per_output=summary, n_chains=int(n_chains), n_draws=int(n_draws))


def posterior_convergence(stack, n_chains=1, rhat_threshold=1.01):
    """The definition above on ``stack`` [S, N_rows, outputs], the samples' predictions in chain-major order (numpy on the host).
    Returns a dict with ``rhat`` and ``ess`` [N_rows, outputs] (NaN in a constant column), ``max_rhat`` and ``min_ess`` over the
    columns that are not constant (NaN when all are), ``frac_rhat_above`` (the share of all columns with rhat > ``rhat_threshold``),
    ``n_constant``, ``per_output`` [outputs, 4] (the four figures per output, the third as a count), ``n_chains`` and ``n_draws``.
    ``ValueError``: not a non-empty three-dimensional array, a NaN or infinite value, or a shape outside the limits above."""
    who = "posterior_convergence"
    y = np.asarray(stack, dtype=np.float64)
    if y.ndim != 3 or 0 in y.shape[1:]:
        raise ValueError("%s: stack must be a non-empty [samples, rows, outputs] array, got shape %s" % (who, y.shape))
    n_draws = check_shape(who, y.shape[0], n_chains)
    if rhat_threshold != rhat_threshold:
        raise ValueError("%s: the threshold is NaN" % who)
    if not np.all(np.isfinite(y)):
        raise ValueError("%s: stack holds NaN or infinite values" % who)
    n_samples, n_rows, n_out = y.shape
    x = y.reshape(n_samples, n_rows * n_out)
    rhat, ess = np.empty(x.shape[1]), np.empty(x.shape[1])
    for c in range(0, x.shape[1], _CHUNK):
        rhat[c:c + _CHUNK], ess[c:c + _CHUNK] = _columns(x[:, c:c + _CHUNK], int(n_chains))
    rhat, ess = rhat.reshape(n_rows, n_out), ess.reshape(n_rows, n_out)
    return result_dict(rhat, ess, summarise(rhat, ess, rhat_threshold), n_rows, n_chains, n_draws)


def _same_network(first, other):
    """Whether two checkpoints' (model, samples) describe the same architecture and activation."""
    (m0, s0), (m1, s1) = first, other
    w0, w1 = s0[0]['weights'], s1[0]['weights']
    if len(w0) != len(w1) or any(np.shape(a) != np.shape(b) for a, b in zip(w0, w1)):
        return False
    if m0._act_fun._function != m1._act_fun._function:         # (slopes are per sample: genReLU's alone reads them)
        return False
    f0, f1 = m0._output_act_fun, m1._output_act_fun
    return getattr(f0, "__name__", f0) == getattr(f1, "__name__", f1) and \
        getattr(m0, "_estimation_mode", None) == getattr(m1, "_estimation_mode", None)


def get_posterior_convergence(pkl_files, features=None, pointwise=True, rhat_threshold=1.01):
    """Split R-hat and effective sample size of the stored samples' predictions: one checkpoint (a path) or a list of them, one
    chain each, on the first checkpoint's test table (default), its training table (``features="train"``) or a feature matrix.
    The chains must share architecture and activation; they are cut to the common length by keeping each chain's last draws.
    Predictions are post-output, as ``get_posterior_est`` computes them (per-sample slopes).  Returns ``posterior_convergence``'s
    dict; without ``pointwise`` ``rhat`` and ``ess`` are left out (they then never leave the device).  A custom output callable goes
    through the host stack.  ``ValueError`` before any device call: chains of different networks, no samples, fewer than 8 draws
    per chain, more than 64 chains, more than 16384 samples, an empty table."""
    who = "get_posterior_convergence"
    files = [pkl_files] if isinstance(pkl_files, (str, bytes)) or hasattr(pkl_files, "__fspath__") else list(pkl_files)
    if len(files) == 0:
        raise ValueError("%s: no checkpoints" % who)
    if len(files) > MAX_CHAINS:
        raise ValueError("%s: %d chains, at most %d are supported" % (who, len(files), MAX_CHAINS))
    chains = []
    for f in files:
        model, _, logger = load_obj(f)
        samples = list(logger._post_weight_samples)
        if len(samples) == 0:
            raise ValueError("%s: the checkpoint %s holds no posterior samples" % (who, f))
        chains.append((model, samples))
    for c in chains[1:]:
        if not _same_network(chains[0], c):
            raise ValueError("%s: the chains must share architecture and activation" % who)
    n_draws = min(len(s) for _, s in chains)
    if n_draws < MIN_DRAWS:
        raise ValueError("%s: %d draws per chain, at least %d are needed" % (who, n_draws, MIN_DRAWS))
    samples = [s for _, chain in chains for s in chain[len(chain) - n_draws:]]
    check_shape(who, len(samples), len(chains))
    if rhat_threshold != rhat_threshold:
        raise ValueError("%s: the threshold is NaN" % who)
    model = chains[0][0]
    x, _ = choose_table(model, features, None, who, need_labels=False)
    with open_predictor(model, samples, x.shape[1]) as pred:
        res = pred.convergence(x, len(chains), rhat_threshold=rhat_threshold, pointwise=pointwise)
    if not pointwise:
        res = {k: v for k, v in res.items() if k not in ("rhat", "ess")}
    return res
