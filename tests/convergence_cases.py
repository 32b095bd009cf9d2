"""Cases of the convergence diagnostics (split R-hat and effective sample size per column) and an independent restatement of their
definition, column by column, in float64 and in ``np.longdouble`` - written from the definition's text, sharing no code with the
package.  The restatement also reports, per column, the smallest margin of any stop or monotone decision of the pair sequence:
min over k of |P_k| (stop at the first P_k < 0) and |P_k - P_{k-1}| (P_k = min(P_k, P_{k-1})).  A column whose margin is tiny may
legitimately truncate elsewhere under another summation order.

Columns are built from seeds: AR(1) series x_t = phi x_{t-1} + e_t from a stationary start, phi in PHIS, every chain on its own
stream, in three variants - plain, mapped to -1e6 + 10 x, squashed through a logistic into (0, 1) - plus one constant column and one
with ties (an iid series rounded to 0.5); all cast to the dtype asked for before anything is computed.  SHAPES (chains, draws) hold an
odd N, a sample count that is no power of two, a column that fills a tile alone and the chain cap."""
import functools

import numpy as np

PHIS = (0.0, 0.5, 0.9, -0.5, 0.99)
VARIANTS = ("plain", "offset", "logistic")
SHAPES = ((1, 8), (1, 9), (2, 50), (3, 341), (4, 250), (2, 2048), (1, 16384), (64, 8))
DTYPES = ("float64", "float32")
SEED = 20261018
MARGIN = 1e-6                  # a column below it may be left out of an ESS comparison
RHAT_RTOL = 1e-9
ESS_RTOL = 1e-8


def ar1(rs, phi, n_chains, n_draws):
    """[n_chains * n_draws] chain-major: independent stationary AR(1) chains of unit innovation variance."""
    out = np.empty((n_chains, n_draws))
    for j in range(n_chains):
        e = rs.standard_normal(n_draws)
        x = np.empty(n_draws)
        x[0] = e[0] / np.sqrt(1.0 - phi * phi)
        for t in range(1, n_draws):
            x[t] = phi * x[t - 1] + e[t]
        out[j] = x
    return out.reshape(-1)


def column_names():
    return ["%s_phi%g" % (v, p) for p in PHIS for v in VARIANTS] + ["constant", "ties"]


def columns(n_chains, n_draws, dtype="float64", seed=SEED):
    """[S, 17] of ``dtype``: the columns of ``column_names()`` for a shape."""
    cols = []
    for ip, phi in enumerate(PHIS):
        rs = np.random.default_rng([seed, n_chains, n_draws, ip])
        x = ar1(rs, phi, n_chains, n_draws)
        cols += [x, -1e6 + 10.0 * x, 1.0 / (1.0 + np.exp(-x))]
    rs = np.random.default_rng([seed, n_chains, n_draws, 99])
    cols.append(np.full(n_chains * n_draws, 0.375))
    cols.append(np.round(2.0 * rs.standard_normal(n_chains * n_draws)) / 2.0)
    return np.ascontiguousarray(np.stack(cols, axis=1).astype(dtype))


def restate(column, n_chains, real=np.float64):
    """(rhat, ess, margin) of one column (chain-major) with every quantity held in ``real``."""
    x = np.asarray(column).astype(real)
    M = int(n_chains)
    N = len(x) // M
    assert M * N == len(x)
    n = N // 2
    m = 2 * M
    rn, rm = real(n), real(m)
    one = real(1)
    d = []
    mu = []
    for j in range(M):
        chain = x[j * N:(j + 1) * N]
        for half in (chain[:n], chain[N - n:]):
            mk = half.sum() / rn
            mu.append(mk)
            d.append(half - mk)

    def acov(k, t):
        return (d[k][:n - t] * d[k][t:]).sum() / rn

    s2 = [acov(k, 0) * rn / (rn - one) for k in range(m)]
    W = sum(s2[1:], s2[0]) / rm
    if W == 0:
        return float("nan"), float("nan"), float("inf")
    mu_all = sum(mu[1:], mu[0]) / rm
    dev = [(mk - mu_all) ** 2 for mk in mu]
    Bn = sum(dev[1:], dev[0]) / (rm - one)
    varp = W * (rn - one) / rn + Bn
    rhat = np.sqrt(varp / W)

    def rho(t):
        if t == 0:
            return one
        a = [acov(k, t) for k in range(m)]
        return one - (W - sum(a[1:], a[0]) / rm) / varp

    prev = rho(0) + rho(1)
    total = prev
    margin = float("inf")
    k = 1
    while 2 * k + 1 <= n - 1:
        P = rho(2 * k) + rho(2 * k + 1)
        margin = min(margin, float(abs(P)))
        if P < 0:
            break
        margin = min(margin, float(abs(P - prev)))
        P = min(P, prev)
        total = total + P
        prev = P
        k += 1
    tau = max(real(-1) + real(2) * total, one / np.log10(rm * rn))
    ess = rm * rn / tau
    return rhat, ess, margin


@functools.lru_cache(maxsize=None)
def reference(n_chains, n_draws, dtype="float64"):
    """The columns of a shape and their restatements: ``values`` [S, 17] of ``dtype``; ``rhat`` / ``ess`` / ``margin`` [17] in float64
    arithmetic, ``rhat_ld`` / ``ess_ld`` / ``margin_ld`` in longdouble arithmetic (as longdouble).  Computed once; do not modify."""
    v = columns(n_chains, n_draws, dtype)
    f64 = [restate(v[:, c], n_chains, np.float64) for c in range(v.shape[1])]
    ld = [restate(v[:, c], n_chains, np.longdouble) for c in range(v.shape[1])]
    out = dict(values=v,
               rhat=np.array([r[0] for r in f64], dtype=np.float64), ess=np.array([r[1] for r in f64], dtype=np.float64),
               margin=np.array([r[2] for r in f64]),
               rhat_ld=np.array([r[0] for r in ld], dtype=np.longdouble), ess_ld=np.array([r[1] for r in ld], dtype=np.longdouble),
               margin_ld=np.array([r[2] for r in ld]))
    for a in out.values():
        a.setflags(write=False)
    return out


def compare(got_rhat, got_ess, ref, use_ld=True):
    """Relative deviations of (rhat, ess) from a ``reference`` over its columns that are not constant, NaNs required where the
    reference has them: (worst rhat deviation, worst ess deviation over the columns kept, number of columns left out of the ess
    comparison because their margin is below MARGIN)."""
    want_rhat = ref["rhat_ld"] if use_ld else ref["rhat"]
    want_ess = ref["ess_ld"] if use_ld else ref["ess"]
    margin = np.minimum(ref["margin"], ref["margin_ld"])
    const = np.isnan(want_rhat.astype(np.float64))
    assert np.array_equal(np.isnan(got_rhat), const) and np.array_equal(np.isnan(got_ess), const)
    live = ~const
    dr = np.abs(np.asarray(got_rhat, dtype=np.longdouble)[live] - want_rhat[live]) / np.abs(want_rhat[live])
    keep = live & (margin >= MARGIN)
    de = np.abs(np.asarray(got_ess, dtype=np.longdouble)[keep] - want_ess[keep]) / np.abs(want_ess[keep])
    return float(dr.max()) if dr.size else 0.0, float(de.max()) if de.size else 0.0, int(np.count_nonzero(live & ~keep))
