"""The permutation-importance cases of tests/golden/importance.npz (make_importance_golden.py): inputs, combinations, keys."""
import os

import numpy as np

import cases

SEED = 7
N_PERMUTATIONS = 3
N_ROWS = 400
N_SAMPLES = 9
CASES = [c["name"] for c in cases.POSTERIOR_CASES]
BLOCKS = {
    "single": dict(),
    "dict": {"a": [0, 1, 2], "b": [3, 4], "c": [5, 6, 7, 8, 9, 10]},
    "lists": [[0, 5], [2], [7, 8, 9], [1, 10, 3]],
}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "importance.npz")


def inputs(name):
    case = [c for c in cases.POSTERIOR_CASES if c["name"] == name][0]
    return cases.posterior_inputs(n_rows=N_ROWS, n_samples=N_SAMPLES, **{k: v for k, v in case.items() if k != "name"})


def combinations():
    return [(mode, unlink, tag) for mode in (0, 1) for unlink in (True, False) for tag in BLOCKS]


def key(name, mode, unlink, tag):
    return "%s/m%d_%s_%s" % (name, mode, "unlinked" if unlink else "linked", tag)


def load():
    return np.load(GOLDEN)


def act_for(bn, inp):
    return bn.ActFun(fun=inp["fun"], prm=np.zeros(2)) if inp["fun"] == "genReLU" else bn.ActFun(fun=inp["fun"])


def run(bn, name, mode, unlink, tag, **kw):
    """bn.feature_importance on a case, seeded as the golden run: (ranking, the four numeric columns)."""
    inp = inputs(name)
    np.random.seed(SEED)
    df = bn.feature_importance(inp["x"], weights_posterior=inp["samples"], true_labels=inp["labels"], n_permutations=N_PERMUTATIONS,
                               feature_blocks=BLOCKS[tag], write_to_file=False, post_summary_mode=mode,
                               unlink_features_within_block=unlink, actFun=act_for(bn, inp), output_act_fun=bn.SoftMax, **kw)
    return df["feature_block_index"].to_numpy().astype(np.int64), df.iloc[:, 2:].to_numpy().astype(np.float64), df


def assert_same_table(order, values, want_order, want_values, label=""):
    """The reference's table to the last bit: every block's four numbers, and the ranking by decreasing mean loss.  Blocks whose
    mean losses are EQUAL floats may stand in either order: the reference sorts an object column (a stable insertion sort at
    these sizes), pandas sorts this package's float column with numpy's quicksort, whose order among equal keys depends on the
    vector unit it was built for."""
    by_block, want_by_block = np.argsort(order), np.argsort(want_order)
    assert np.array_equal(np.sort(order), np.arange(len(want_order))), label
    np.testing.assert_array_equal(values[by_block], want_values[want_by_block], err_msg=label)
    np.testing.assert_array_equal(values[:, 0], want_values[:, 0], err_msg=label)           # the ranked column itself
    assert np.all(np.diff(values[:, 0]) <= 0), label
    moved = order != want_order
    assert np.array_equal(np.sort(order[moved]), np.sort(want_order[moved])), label
