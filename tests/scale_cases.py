"""Training / test table pairs whose test table does NOT follow the training table's distribution, with the two networks and the
weight sets that tests/test_host_split_model.py (numpy model, CPU) and tests/test_hip_test_table_scales.py (device) run on them.

1000 x 40 training rows, 300 test rows, float32.  A kind names the columns it moves (``cols``) and by how much (``ratio``); its
"small weights" variant divides the first layer's weights on those columns by the ratio, so that the layer-0 sums stay O(1) while the
scaled entries are large - where the fp16 pair's absolute floor on a WEIGHT shows."""
import functools

import numpy as np

import cases

N_TRAIN, N_TEST, F = 1000, 300, 40
COL = 3                 # the column the col_* kinds move
ROW, ECOL = 17, 5       # the entry the one_entry_* kinds set
N_CLASSES = 5
N_SETS = 7
NETS = {"linear": (), "tanh": (12, 7)}        # no hidden layer, identity output: the outputs are the layer-0 sums; [12, 7] tanh, softmax

# kind -> (training table, test table, columns, ratio, layer-0 mode a TEST launch must report or None)
# Plain weights are N(0, 0.5) wherever float32's own rounding of the weights leaves them fair (tests/test_host_split_model.py: the
# float32 model inside half of the bars).  Two groups are not, and have their inputs changed (PLAIN_STD, NORMALISED):
#   all_x100: 40 columns of entries up to 400 put sum |w x| at 1600 per unit; float32's rounding of the weights alone leaves sums that
#   cancel at 0.6 of the bar and a float32 accumulator at 4 times the bar (N(0, 0.125): the model 1.02, the device's float32 layer 0
#   1.2 to 1.4).  N(0, 0.05): 0.4 in the model;
#   the log-normal tables: entries up to 1e5, sums of 1e4 that cancel, 0.7 to 1.2 of the bar by the weights' rounding alone.
KINDS = {
    "same": ("normal", "normal", (), 1.0, "f16-split"),
    "col_x1e2": ("normal", "col", (COL,), 1e2, None),
    "col_x1e3": ("normal", "col", (COL,), 1e3, None),
    "col_x1e4": ("normal", "col", (COL,), 1e4, None),
    "all_x100": ("normal", "all", tuple(range(F)), 1e2, None),
    "lognormal3": ("normal", "lognormal3", (), 1.0, None),
    "one_entry_2e5": ("normal", "entry", (ECOL,), 2e5, None),
    "one_entry_1e6": ("normal", "entry", (ECOL,), 1e6, "f32"),
    "col_x1e-3": ("normal", "col", (COL,), 1e-3, "f32"),
    "col_x1e-6": ("normal", "col", (COL,), 1e-6, "f32"),
    "zero_in_training": ("zero_col", "normal", (), 1.0, "f16-split"),
    "zero_in_training_x1000": ("zero_col", "col", (COL,), 1e3, None),
    "col_zero_in_test": ("normal", "zero_col", (), 1.0, None),
    "moved_train_lognormal": ("lognormal3", "lognormal3", (), 1.0, None),
    "moved_train_normal": ("lognormal3", "normal", (), 1.0, None),
}
PLAIN_STD = {"all_x100": 0.05}           # (every other kind: 0.5)
# layer 0's weights divided by the columns' mean |value| in this table, as test_hip_parity's heavy-tailed cases do
NORMALISED = {"lognormal3": "test", "moved_train_lognormal": "train", "moved_train_normal": "train"}
# every (kind, small weights?) a test runs
VARIANTS = [(k, False) for k in KINDS] + [(k, True) for k, v in KINDS.items() if v[3] != 1.0]


def variant_id(v):
    return v[0] + ("-small-weights" if v[1] else "")


@functools.lru_cache(maxsize=None)
def _base(seed, n):
    return np.random.default_rng(seed).standard_normal((n, F))


@functools.lru_cache(maxsize=None)
def train_table(shape):
    x = _base(101, N_TRAIN).copy()
    if shape == "zero_col":
        x[:, COL] = 0.0
    elif shape == "lognormal3":
        x = np.exp(3.0 * x)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def tables(kind):
    """(training table, test table), float32, read-only."""
    train, shape, cols, ratio, _ = KINDS[kind]
    x = _base(202, N_TEST).copy()
    if shape in ("col", "all"):
        x[:, list(cols)] *= ratio
    elif shape == "entry":
        x[ROW, ECOL] = ratio
    elif shape == "zero_col":
        x[:, COL] = 0.0
    elif shape == "lognormal3":
        x = np.exp(3.0 * x)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return train_table(train), x


@functools.lru_cache(maxsize=None)
def labels():
    rs = np.random.default_rng(303)
    return rs.integers(0, N_CLASSES, N_TRAIN), rs.integers(0, N_CLASSES, N_TEST)


def shapes(net):
    if not NETS[net]:
        return [(12, F + 1)]
    return cases.layer_shapes(F, list(NETS[net]), N_CLASSES, 2)


@functools.lru_cache(maxsize=None)
def weight_sets(net, kind, small):
    """N_SETS weight sets, N(0, 0.5) entries (PLAIN_STD, NORMALISED: the kinds that differ); small: layer 0's weights on the kind's
    columns divided by its ratio."""
    _, _, cols, ratio, _ = KINDS[kind]
    out = []
    for s in range(N_SETS):
        rs = np.random.default_rng(1000 + s)
        w = [rs.normal(0, 0.5, sh) for sh in shapes(net)]
        w[0] *= PLAIN_STD.get(kind, 0.5) / 0.5
        if kind in NORMALISED:
            x = tables(kind)[NORMALISED[kind] == "test"].astype(np.float64)
            w[0][:, 1:] /= np.abs(x).mean(axis=0)
        if small:
            w[0][:, [1 + c for c in cols]] /= ratio
        out.append(w)
    return out
