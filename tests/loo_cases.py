"""PSIS-LOO restated for the tests: the definition of include/npbnn_hip.h (npbnn_op_psis) column by column and term by term, with no
code shared with the package, in a floating-point type of the caller's choice, and the bar the device is held to.

The device and ``posterior_loo`` see the same float64 numbers and differ by rounding only, so the bar of a case is not chosen in
advance: the restatement is evaluated in float64 and in ``np.longdouble`` on the case's input, and the bar is 16 times the largest
distance between the two - separately for ``elpd_loo_i``, ``lppd_i`` (absolute) and the finite ``k`` - and never below 16 * 2^-52 of
the largest magnitude in the array.  Sixteen, because both sides add up to 384 tail terms and 49 weights in different orders, under the
conditioning the float64-to-longdouble distance already shows.  ``+inf`` in ``k`` must match exactly."""
import math

import numpy as np

FIELDS = ("elpd_loo_i", "lppd_i", "pareto_k")
BAR_FACTOR = 16.0
EPS = 2.0 ** -52


def tail_cap(n_samples):
    return int(math.ceil(min(n_samples / 5.0, 3.0 * math.sqrt(n_samples))))


def gpd_fit(t, dt):
    """(k, sigma) of Zhang and Stephens' estimate with the weakly informative prior, t ascending in type dt"""
    n = len(t)
    m = 30 + int(math.floor(math.sqrt(n)))
    t_quart, t_top = t[int(math.floor(n / 4.0 + 0.5)) - 1], t[n - 1]
    b, kq, lq = [], [], []
    for q in range(1, m + 1):
        bq = (dt(1) - np.sqrt(dt(m) / (dt(q) - dt(0.5)))) / (dt(3) * t_quart) + dt(1) / t_top
        kk = np.log1p(-bq * t).sum() / dt(n)
        b.append(bq)
        kq.append(kk)
        lq.append(dt(n) * (np.log(-bq / kk) - kk - dt(1)))
    b, lq = np.array(b, dtype=dt), np.array(lq, dtype=dt)
    w = np.array([dt(1) / np.exp(lq - lq[i]).sum() for i in range(m)], dtype=dt)
    keep = w >= dt(10) * dt(EPS)
    w = np.where(keep, w, dt(0))
    w = w / w.sum()
    b_hat = (b * w).sum()
    k_prime = np.log1p(-b_hat * t).sum() / dt(n)
    return (dt(n) * k_prime + dt(5)) / (dt(n) + dt(10)), -k_prime / b_hat


def lse(a):
    top = a.max()
    return top + np.log(np.exp(a - top).sum())


def loo_column(ll, dt=np.float64):
    """(elpd_loo_i, lppd_i, k) of one column of log-likelihoods, all arithmetic in dt"""
    ll = np.asarray(ll, dtype=np.float64).astype(dt)
    n_samples = len(ll)
    r = -ll
    x = r - r.max()
    cap = tail_cap(n_samples)
    cut = max(np.sort(x)[::-1][cap], np.log(dt(np.finfo(np.float64).tiny)))
    e_cut = np.exp(cut)
    where = np.nonzero(x > cut)[0]
    where = where[np.argsort(x[where], kind="stable")]          # the tail, ascending
    n = len(where)
    lw = x.copy()
    k = dt(np.inf)
    if n > 4:
        k, sigma = gpd_fit(np.exp(x[where]) - e_cut, dt)
        p = (np.arange(1, n + 1).astype(dt) - dt(0.5)) / dt(n)
        quot = -sigma * np.log1p(-p) if k == 0 else sigma * np.expm1(-k * np.log1p(-p)) / k
        lw[where] = np.minimum(np.log(quot + e_cut), dt(0))
    return lse(lw + ll) - lse(lw), lse(ll) - np.log(dt(n_samples)), k


def loo_columns(log_lik, dt=np.float64):
    """{field: [N] array in dt} of a [S, N] matrix"""
    cols = [loo_column(c, dt) for c in np.asarray(log_lik).T]
    return {f: np.array([c[i] for c in cols], dtype=dt) for i, f in enumerate(FIELDS)}


def reference(log_lik):
    """(the restatement in float64 {field: [N]}, the bar {field: float}) of a case"""
    lo, hi = loo_columns(log_lik, np.float64), loo_columns(log_lik, np.longdouble)
    bars = {}
    for f in FIELDS:
        a, b = lo[f], hi[f]
        fin = np.isfinite(a)
        assert np.array_equal(fin, np.isfinite(b)), f
        dist = float(np.max(np.abs(a[fin].astype(np.longdouble) - b[fin]))) if fin.any() else 0.0
        mag = float(np.max(np.abs(a[fin]))) if fin.any() else 0.0
        bars[f] = BAR_FACTOR * max(dist, EPS * mag)
    return lo, bars


def deviation(got, want, field):
    """largest absolute deviation over the finite entries; the infinite ones must sit in the same places"""
    g, w = np.asarray(got[field], dtype=np.float64), np.asarray(want[field], dtype=np.float64)
    fin = np.isfinite(w)
    assert np.array_equal(g[~fin], w[~fin]), "%s: +inf in other places" % field
    return float(np.max(np.abs(g[fin] - w[fin]))) if fin.any() else 0.0


def matrix(n_samples, n_cols, seed=0, spread=1.5):
    """A seeded [S, N] matrix of log-likelihoods as a posterior's look: a level per row, a spread per row, a heavy left tail"""
    rs = np.random.default_rng(100003 * n_samples + 101 * n_cols + seed)
    level = -rs.gamma(2.0, 1.0, n_cols)
    scale = spread * rs.uniform(0.05, 1.0, n_cols)
    return level[None] - scale[None] * rs.gamma(1.5, 1.0, (n_samples, n_cols))


def special_matrix(n_samples=64):
    """Columns: constant; two values tied across the cut; a pair of equal columns; a column shifted by 1e6; one near -700; ordinary"""
    rs = np.random.default_rng(7)
    base = matrix(n_samples, 6, seed=3)
    base[:, 0] = -1.25
    base[:, 1] = np.where(np.arange(n_samples) % 2 == 0, -0.5, -2.0)
    base[:, 3] = base[:, 2]
    base[:, 4] = base[:, 2] + 1e6
    base[:, 5] = -700.0 - rs.gamma(1.5, 2.0, n_samples)
    return base
