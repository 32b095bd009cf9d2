"""Numpy model of the fp16-split first layer's data side (npbnn_amd/csrc/npbnn_pack.hip.h, ensure_scales / ensure_x16 in
npbnn_capi.hip): the scales a training table gives, the pair of fp16 numbers an entry and a weight are held as, the rules that keep a
table on the pair or send it to the float32 layer 0, and the layer-0 sums of both paths.

It restates this project's own kernels and takes nothing from elsewhere.  It models what is stored and which products are kept, with
the sums in float64; the float32 path can also be summed in float32 (l0_f32's ``accumulate``), the order of the matrix cores apart."""
import numpy as np

F16_SAFE = 60000.0                  # kF16Safe
QUALITY_TOL = 2.0 ** -17            # kF16QualityTol
TYPICAL_TOL = 2.0 ** -12            # kF16TypicalTol
PAIR_REL = 2.0 ** -21               # kF16PairRel
MAX_SHIFT = 12                      # kF16MaxShift
Z_BAR = 2e-5                        # the prediction bar: Z_BAR * max(1, |value|)
FLOOR_S = Z_BAR / 4 * 2.0 ** 25     # kF16FloorSum (167.77...): see weight_floor_sum

USABLE, OUT_OF_RANGE, POOR_COLUMN, WEIGHT_FLOOR = 1, -1, -2, -3      # FeatureTable::f16_state of a table that was split

f32 = np.float32


def col_absmax(x32):
    return np.abs(np.asarray(x32, dtype=f32)).max(axis=0)


def col_scale(absmax, shift=None):
    """col_scale_kernel: x_scale = 2^-e, w_scale = 2^e with 2^(e-1) <= max|x_c| < 2^e (e = 0 for an all-zero or non-finite column),
    e lowered by the column's shift."""
    m = np.asarray(absmax, dtype=f32)
    e = np.zeros(m.shape, dtype=np.int64)
    ok = (m > 0) & np.isfinite(m)
    e[ok] = np.frexp(m[ok])[1]
    if shift is not None:
        e = e - np.asarray(shift, dtype=np.int64)
    return np.ldexp(f32(1), -e).astype(f32), np.ldexp(f32(1), e).astype(f32)


def split_f16(v):
    """split_f16: hi = fp16(v), lo = fp16(v - hi), round to nearest even, subnormals kept."""
    v = np.asarray(v, dtype=f32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(f32)).astype(np.float16)
    return hi, lo


def column_quality(x32, x_scale):
    """split_quality_kernel + column_quality: per column max(error / (2^-17 mean |x'|), error / (2^-12 typical |x'|)) of the largest
    entry error beyond the pair's own 22-bit rounding; <= 1 passes."""
    v = (np.asarray(x32, dtype=f32) * x_scale).astype(f32)
    hi, lo = split_f16(v)
    a = np.abs(v)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(v - (hi.astype(f32) + lo.astype(f32))).astype(f32)
        counted = e > (f32(PAIR_REL) * a).astype(f32)
    worst = np.where(counted, e, f32(0)).max(axis=0).astype(np.float64)
    n = v.shape[0]
    mean_abs = np.floor(np.minimum(a, f32(4096)).astype(np.float64) * 2.0 ** 28).sum(axis=0) / 2.0 ** 28 / n
    nz = (a > 0) & np.isfinite(a)
    with np.errstate(divide="ignore"):
        l2 = np.where(nz, np.trunc((np.log2(np.where(nz, a, f32(1))).astype(f32) * f32(65536)).astype(f32)), 0.0)
    cnt = nz.sum(axis=0)
    typical = np.exp2(l2.sum(axis=0) / 65536.0 / np.maximum(cnt, 1))
    bad = np.zeros(v.shape[1])
    for c in range(v.shape[1]):
        if cnt[c] == 0 or not worst[c] > 0:
            continue
        by_mean = worst[c] / mean_abs[c] / QUALITY_TOL if mean_abs[c] > 0 else 1e300
        bad[c] = max(by_mean, worst[c] / typical[c] / TYPICAL_TOL)
    return bad


def ensure_scales(x_train32):
    """ensure_scales: (x_scale, w_scale, shift per column, training table finite?).  A column past the quality bounds under the scale its
    largest entry gives has the scale moved up by ceil(log2(badness)) + 1 powers of two, 12 at the most."""
    m = col_absmax(x_train32)
    finite = bool(np.all(np.isfinite(m)))
    xs, ws = col_scale(m)
    shift = np.zeros(m.shape, dtype=np.int64)
    if finite:
        bad = column_quality(x_train32, xs)
        for c in np.nonzero(bad > 1.0)[0]:
            shift[c] = min(int(np.ceil(np.log2(bad[c]))) + 1, MAX_SHIFT)
        if shift.any():
            xs, ws = col_scale(m, shift)
    return xs, ws, shift, finite


def weight_floor_sum(x32, x_scale):
    """E of ensure_x16's rule for a table that did not give the scales: the sum over columns of what the scaled column maximum exceeds 1
    by.

    A scaled weight w' below 2^-3 is held by the pair with an absolute error of up to 2^-25 (half of fp16's subnormal spacing), whatever
    its size; on a row that error is multiplied by |x'_c| and the columns add up, so a row's layer-0 sum is off by up to
    2^-25 * sum_c m_c, m_c the scaled column maxima.  sum_c min(m_c, 1) is what a table of the training table's range gives (F * 2^-25
    at the most).  What the table adds must leave the prediction bar three quarters of its room: 2^-25 * E <= Z_BAR / 4, E <= 167.77."""
    m = col_absmax(x32).astype(np.float64) * np.asarray(x_scale, dtype=np.float64)
    return float((m[m > 1.0] - 1.0).sum())


def table_state(x32, x_scale, source):
    """ensure_x16's acceptance of a table under the scales: (state, worst column of the quality check or -1, E).  ``source``: the
    table the scales were taken from (its own rule: moved scales, the 2^12 cap)."""
    v = (np.asarray(x32, dtype=f32) * x_scale).astype(f32)
    m = np.abs(v).max()
    s = weight_floor_sum(x32, x_scale)
    if not (np.isfinite(m) and m <= F16_SAFE):
        return OUT_OF_RANGE, -1, s
    bad = column_quality(x32, x_scale)
    if bad.max() > 1.0:
        return POOR_COLUMN, int(np.argmax(bad)), s
    if not source and s > FLOOR_S:
        return WEIGHT_FLOOR, -1, s
    return USABLE, -1, s


def states(x_train32, x_test32):
    """(state of the training table, state of the test table, shifts) as a fresh context assigns them; a training table off the pair
    takes every table with it (state 0: never split)."""
    xs, ws, shift, finite = ensure_scales(x_train32)
    if not finite:
        return OUT_OF_RANGE, 0, shift
    tr = table_state(x_train32, xs, True)[0]
    return tr, table_state(x_test32, xs, False)[0], shift


def l0_pair(x32, w0, x_scale, w_scale):
    """Layer-0 sums of the pair path, bias excluded: w_hi*x_hi + w_lo*x_hi + w_hi*x_lo over x' = x * x_scale, w' = float32(w * w_scale).
    ``w0``: [units, features] float64."""
    xh, xl = split_f16((np.asarray(x32, dtype=f32) * x_scale).astype(f32))
    wh, wl = split_f16((np.asarray(w0, dtype=np.float64) * w_scale.astype(np.float64)).astype(f32))
    xh, xl, wh, wl = (a.astype(np.float64) for a in (xh, xl, wh, wl))
    return xh @ wh.T + xh @ wl.T + xl @ wh.T


def l0_f32(x32, w0, accumulate=False):
    """Layer-0 sums of the float32 path, bias excluded: float32 weights on the float32 table.  ``accumulate``: the sum kept in float32,
    one feature after the other, each product added with one rounding - a stand-in for the matrix cores' float32 accumulator (their
    order differs; the size of the rounding, 2^-24 of the running sum per step, is what a table's fairness depends on)."""
    x = np.asarray(x32, dtype=f32).astype(np.float64)
    w = np.asarray(w0, dtype=np.float64).astype(f32).astype(np.float64)
    if not accumulate:
        return x @ w.T
    acc = np.zeros((x.shape[0], w.shape[0]))
    for c in range(x.shape[1]):
        acc = (acc + np.outer(x[:, c], w[:, c])).astype(f32).astype(np.float64)
    return acc


def finish(z0, weights, n_features):
    """The rest of the network on layer-0 sums ``z0`` (bias excluded): values rounded to float32 between layers, float32 weights, tanh
    between layers, the last layer's values returned (float64 array of float32 numbers)."""
    z = z0
    for l, w in enumerate(weights):
        w = np.asarray(w, dtype=np.float64).astype(f32).astype(np.float64)
        n_in = n_features if l == 0 else weights[l - 1].shape[0]
        bias = w.shape[1] == n_in + 1
        if l > 0:
            z = a @ w[:, int(bias):].T
        if bias:
            z = z + w[:, 0]
        z = z.astype(f32).astype(np.float64)
        a = np.tanh(z).astype(f32).astype(np.float64)
    return z


def softmax(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def loglik_categorical(z, labels):
    zs = z - z.max(axis=1, keepdims=True)
    return float(np.sum(zs[np.arange(len(z)), labels] - np.log(np.exp(zs).sum(axis=1))))


def scaled_error(got, want):
    """Largest |error| / max(1, |value|): the quantity the prediction bar limits."""
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
