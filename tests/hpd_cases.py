"""The HPD fixture (tests/golden/hpd.npz, written from the reference's calcHPD by tests/golden/make_hpd_golden.py): its inputs are
rebuilt here from seeds, the fixture holds only upstream's outputs.  Also a numpy restatement of calcHPD (np_bnn/BNN_lib.py:286-302)
over the columns of a sample stack, the yardstick of the device results."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hpd.npz")

SIZES = (2, 3, 5, 31, 32, 33, 100, 255, 256, 257, 1000, 1024, 1025, 4096, 16384)
LEVELS = (0.05, 0.5, 0.95, 0.99)
# round(level * S) exactly half-way (Python rounds half to even): 0.95 * 10 -> 10, 0.95 * 30 -> 28, 0.5 * 5 -> 2, 0.05 * 30 -> 2,
# 0.75 * 2 -> 2
HALF_EVEN = ((10, 0.95), (30, 0.95), (5, 0.5), (30, 0.05), (2, 0.75))
DTYPES = ("float64", "float32")
N_COLS = 7


def n_in(n_samples, level):
    return int(round(level * n_samples))


def cases():
    """[(name, S, level, dtype)]: every size and level whose window holds at least two values, and the half-way roundings."""
    out = []
    for dt in DTYPES:
        for s in SIZES:
            for lv in LEVELS:
                if n_in(s, lv) >= 2:
                    out.append(("S%d_L%g_%s" % (s, lv, dt), s, lv, dt))
        for s, lv in HALF_EVEN:
            out.append(("half_S%d_L%g_%s" % (s, lv, dt), s, lv, dt))
    return out


def case_data(n_samples, dtype, seed):
    """[S, N_COLS] columns: normal; ties (multiples of 0.5); integer-valued; constant; negative around -1e6; large magnitude;
    skewed (exponential)."""
    rs = np.random.default_rng(seed)
    x = np.empty((n_samples, N_COLS))
    x[:, 0] = rs.standard_normal(n_samples)
    x[:, 1] = np.round(rs.normal(0, 1.5, n_samples) * 2) / 2
    x[:, 2] = rs.integers(-4, 5, n_samples)
    x[:, 3] = 3.25
    x[:, 4] = -1e6 + rs.standard_normal(n_samples) * 10.0
    x[:, 5] = rs.standard_normal(n_samples) * (1e30 if dtype == "float32" else 1e200)
    x[:, 6] = rs.exponential(2.0, n_samples)
    return x.astype(dtype)


def case_seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003


def hpd_columns(stack, level):
    """calcHPD of every column of ``stack`` [S, ...] along axis 0, widths in the stack's own type: (lower, upper) of shape [...]
    and type.  The first narrowest window wins (np.argmin), as upstream's strict comparison makes it."""
    a = np.asarray(stack)
    k_in = n_in(a.shape[0], level)
    d = np.sort(a, axis=0)
    widths = d[k_in - 1:] - d[:a.shape[0] - k_in + 1]
    k = np.argmin(widths, axis=0)[None]
    return np.take_along_axis(d, k, axis=0)[0], np.take_along_axis(d, k + k_in - 1, axis=0)[0]


def load():
    """{name: dict(S, level, dtype, x [S, N_COLS], lo, hi)} with upstream's bounds as float64 (exact for float32 values)."""
    z = np.load(GOLDEN)
    out = {}
    for name, s, lv, dt in cases():
        out[name] = dict(S=s, level=lv, dtype=dt, x=case_data(s, dt, case_seed(name)), lo=z[name + "/lo"], hi=z[name + "/hi"])
    return out
