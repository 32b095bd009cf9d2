"""The posterior predictive distribution restated, and the cases of tests/test_host_predictive.py and tests/test_hip_predictive.py.

An independent restatement: it shares no code with npbnn_amd/predictive.py.  A cell has S components mu_s, sigma_s:

    F(x)      = (1/S) sum_s Phi((x - mu_s) / sigma_s),  Phi(u) = 0.5 erfc(-u / sqrt 2)
    A(m, v)   = 2 sqrt(v) phi(m / sqrt v) + m erf(m / sqrt(2 v))
    crps(y)   = T1 - T2 / 2,  T1 = (1/S) sum_s A(y - mu_s, sigma_s^2),
                T2 = (1/S^2) [sum_s 2 sigma_s / sqrt(pi) + 2 sum_{s<t} A(mu_s - mu_t, sigma_s^2 + sigma_t^2)]

Small cells are evaluated with mpmath at 40 digits, large ones as the ``math.fsum`` of float64 terms (libm's erfc, numpy's exp and
scipy's erf: a few ulp per term, the sum exact), which is good to about 2 * 2^-53 relative - the bounds absorb it.

The acceptance rule of a quantile q of probability p needs no assumption about the cell's conditioning.  delta = (S + 8) 2^-53 is the
worst relative error of a float64 sum of S terms in [0, 1], with an allowance of 8 ulp for erfc.  (The allowance would grow to a
larger figure if the device library documented one for its double-precision erfc; we know of no such statement - the 16 ulp of the
OpenCL C conformance table, which the library is built to, is a ceiling and not a measurement - so the 8 stays, and the tests
print how much of the bound the residuals use.)  q passes
when |F(q) - p| <= 4 delta max(p, 1 - p), or when q lies within 4 ulp of the restatement's own root (bisection on the restated F until
the bracket cannot narrow): that covers a cell whose F passes the first bound within one ulp of x.  Every cell falls under one rule
or the other; none is left out.

The bound of the CRPS: (64 + ceil(S (S - 1) / 2 / 64)) 2^-53 (T1 + T2 / 2) - a lane adds at most that many non-negative terms one
after the other, and A is taken as good to 16 ulp.

Cases: every mu and sigma is rounded through float32, so float32 and float64 input hold the same numbers; every mu is a multiple of
2^-12 besides, which makes each partial sum of mu - K exact in float64 and lets the mean be compared bit for bit whatever the order
of the sum."""
import math

import numpy as np

PROBS = (1e-6, 0.025, 0.5, 0.975, 1 - 1e-6)
PROBS16 = (0.5, 1e-12, 0.975, 1e-3, 1 - 1e-6, 0.25, 1e-9, 0.9, 0.025, 1 - 1e-9, 0.6, 0.1, 1e-6, 0.75, 0.4, 0.999)
FAMILIES = ("random", "wide", "identical", "bimodal", "step")
MP_CELLS = 130                    # S * cells up to which a case is restated with mpmath
GRID = 2.0 ** -12


def _mp():
    import mpmath
    mpmath.mp.dps = 40
    return mpmath


def make(family, n_samples, n_cols, sigma_cols=0, seed=0):
    """(mu [S, n_cols], sigma [S, n_cols] or [S, sigma_cols], y [n_cols]) of a family, float64 arrays of float32 values (y is any
    float64)."""
    rs = np.random.default_rng([seed, FAMILIES.index(family), n_samples, n_cols, sigma_cols])
    s_shape = (n_samples, sigma_cols if sigma_cols else n_cols)
    if family == "random":
        mu = rs.normal(0, 1, (n_samples, n_cols)) + rs.normal(0, 3, n_cols)[None]
        sg = np.exp(rs.normal(-0.5, 0.5, s_shape))
    elif family == "wide":
        mu = rs.normal(0, 2, (n_samples, n_cols))
        sg = np.exp(rs.normal(0, 3, s_shape))
    elif family == "identical":
        mu = np.broadcast_to(rs.normal(0, 5, n_cols)[None], (n_samples, n_cols))
        sg = np.broadcast_to(np.exp(rs.normal(0, 1, s_shape[1]))[None], s_shape)
    elif family == "bimodal":
        mu = np.where(np.arange(n_samples)[:, None] < n_samples // 2, -20.0, 20.0) * np.ones((1, n_cols))
        sg = np.full(s_shape, 0.5)
    else:
        mu = 1000.0 + rs.integers(-40, 41, (n_samples, n_cols)) * GRID
        sg = np.full(s_shape, 1e-20)
    mu = (np.round(np.asarray(mu, dtype=np.float64) / GRID) * GRID).astype(np.float32).astype(np.float64)
    sg = np.asarray(sg, dtype=np.float64).astype(np.float32).astype(np.float64)
    assert np.all(mu / GRID == np.round(mu / GRID)) and np.all(sg > 0) and np.all(np.isfinite(sg))
    y = mu.mean(axis=0) + rs.normal(0, 1, n_cols) * (mu.std(axis=0) + sigma_of_cells(sg, n_cols, sigma_cols > 0).mean(axis=0))
    return np.ascontiguousarray(mu), np.ascontiguousarray(sg), np.ascontiguousarray(y)


def sigma_of_cells(sg, n_cols, per_sample):
    """[S, n_cols]: the sigma of every cell"""
    return sg[:, np.arange(n_cols) % sg.shape[1]] if per_sample else sg


# ---- F and the quantile ----------------------------------------------------------------------------------------------------------
def residual(x, mu, sg, p, use_mp):
    """F(x) - p of one cell (mu, sg [S]); a float.  Without mpmath on the tail that keeps its precision."""
    n = len(mu)
    if use_mp:
        mp = _mp()
        xx = mp.mpf(x)
        f = sum(mp.erfc(-(xx - mp.mpf(m)) / (mp.mpf(s) * mp.sqrt(2))) for m, s in zip(mu.tolist(), sg.tolist())) / (2 * n)
        return float(f - mp.mpf(p))
    r2 = math.sqrt(2.0)
    if p > 0.5:
        tail = math.fsum(math.erfc(((x - m) / s) / r2) for m, s in zip(mu.tolist(), sg.tolist())) / (2.0 * n)
        return (1.0 - p) - tail
    return math.fsum(math.erfc(-((x - m) / s) / r2) for m, s in zip(mu.tolist(), sg.tolist())) / (2.0 * n) - p


def root(mu, sg, p, use_mp):
    """The restatement's quantile of one cell: bisection from [min (mu - 10 sigma), max (mu + 10 sigma)] (|z_p| <= 7.1 for
    min(p, 1 - p) >= 1e-12), moved out by its own width or by 1 (a sigma far below an ulp of mu leaves the ends on the components),
    until the bracket cannot narrow; the end of smaller residual."""
    lo, hi = float(np.min(mu - 10.0 * sg)), float(np.max(mu + 10.0 * sg))
    lo, hi = lo - max(hi - lo, 1.0), hi + max(hi - lo, 1.0)
    assert residual(lo, mu, sg, p, use_mp) < 0 < residual(hi, mu, sg, p, use_mp)
    while True:
        mid = lo + 0.5 * (hi - lo)
        if not lo < mid < hi:
            break
        if residual(mid, mu, sg, p, use_mp) < 0:
            lo = mid
        else:
            hi = mid
    return lo if abs(residual(lo, mu, sg, p, use_mp)) <= abs(residual(hi, mu, sg, p, use_mp)) else hi


def check_quantiles(q, mu, sg, probs, per_sample=False, label=""):
    """Every cell of q [len(probs), n_cols] under the acceptance rule; returns (the largest residual / bound among the cells the
    first rule passes, the number of cells the second rule had to pass).  AssertionError names the first cell neither rule passes."""
    n, n_cols = mu.shape
    sig = sigma_of_cells(sg, n_cols, per_sample)
    use_mp = n * n_cols <= MP_CELLS
    delta = (n + 8) * 2.0 ** -53
    worst, by_root = 0.0, 0
    assert q.shape == (len(probs), n_cols) and np.all(np.isfinite(q)), label
    for j, p in enumerate(probs):
        bound = 4.0 * delta * max(p, 1.0 - p)
        for c in range(n_cols):
            r = abs(residual(float(q[j, c]), mu[:, c], sig[:, c], p, use_mp))
            if r <= bound:
                worst = max(worst, r / bound)
                continue
            x = root(mu[:, c], sig[:, c], p, use_mp)
            by_root += 1
            assert abs(float(q[j, c]) - x) <= 4.0 * math.ulp(x), \
                "%s: cell %d, p = %r: q = %r has |F(q) - p| = %.3e over the bound %.3e and lies %.3g ulp from the root %r" % (
                    label, c, p, float(q[j, c]), r, bound, abs(float(q[j, c]) - x) / math.ulp(x), x)
    return worst, by_root


# ---- CRPS ------------------------------------------------------------------------------------------------------------------------
def crps_parts(mu, sg, y, use_mp):
    """(T1, T2 / 2) of one cell (mu, sg [S], y a float), both >= 0"""
    n = len(mu)
    if use_mp:
        mp = _mp()

        def a(m, v):
            sd = mp.sqrt(v)
            return 2 * sd * mp.npdf(m / sd) + m * mp.erf(m / mp.sqrt(2 * v))
        ms, ss = [mp.mpf(v) for v in mu.tolist()], [mp.mpf(v) for v in sg.tolist()]
        t1 = sum(a(mp.mpf(y) - m, s * s) for m, s in zip(ms, ss)) / n
        pair = sum(a(ms[i] - ms[j], ss[i] * ss[i] + ss[j] * ss[j]) for i in range(n) for j in range(i + 1, n))
        t2 = (sum(2 * s / mp.sqrt(mp.pi) for s in ss) + 2 * pair) / (n * n)
        return float(t1), float(t2 / 2)
    from scipy.special import erf

    def a(m, sd):
        z = m / sd
        return 2.0 * sd * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) + m * erf(z / math.sqrt(2.0))
    t1 = math.fsum(a(y - mu, sg).tolist()) / n
    i, j = np.triu_indices(n, 1)
    pair = math.fsum(a(mu[i] - mu[j], np.hypot(sg[i], sg[j])).tolist())
    t2 = (math.fsum((2.0 * sg / math.sqrt(math.pi)).tolist()) + 2.0 * pair) / (float(n) * float(n))
    return t1, t2 / 2.0


def check_crps(crps, mu, sg, y, per_sample=False, label=""):
    """Every cell of crps [n_cols] against the restatement under the bound; returns the largest |difference| / bound."""
    n, n_cols = mu.shape
    sig = sigma_of_cells(sg, n_cols, per_sample)
    use_mp = n * n * n_cols <= 40 * MP_CELLS
    factor = (64 + -(-(n * (n - 1) // 2) // 64)) * 2.0 ** -53
    worst = 0.0
    assert crps.shape == (n_cols,), label
    for c in range(n_cols):
        t1, t2h = crps_parts(mu[:, c], sig[:, c], float(y[c]), use_mp)
        bound = factor * (t1 + t2h)
        d = abs(float(crps[c]) - (t1 - t2h))
        assert d <= bound, "%s: cell %d: crps %r, restated %r, |difference| %.3e over the bound %.3e" % (label, c, float(crps[c]), t1 - t2h, d, bound)
        worst = max(worst, d / bound if bound > 0 else 0.0)
    return worst


def mean_of(mu):
    """K + mean(mu - K), K the first component: exact on the cases' grid"""
    return mu[0] + np.sum(mu - mu[0], axis=0) / len(mu)


def normal_quantile(p):
    """the standard normal quantile, from mpmath"""
    mp = _mp()
    return float(mp.sqrt(2) * mp.erfinv(2 * mp.mpf(p) - 1))
