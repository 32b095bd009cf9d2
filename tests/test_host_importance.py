"""Permutation importance on the host (no GPU): the row indices ``_SamplePredictor.permute`` draws, the routing of
``feature_importance`` between the device route and the route through ``get_posterior_cat_prob``, argument checks, and the
reference's tables (tests/golden/importance.npz) from a float64 stand-in of the device context."""
import importlib

import numpy as np
import pytest

import importance_cases as ic
import npbnn_amd as bn
import oracle as orc
from npbnn_amd import _capi as capi

posterior = importlib.import_module("npbnn_amd.posterior")
backend = importlib.import_module("npbnn_amd.backend")

ACT_KINDS = {capi.ACT_RELU: "ReLU", capi.ACT_LEAKY: "genReLU", capi.ACT_SWISH: "swish", capi.ACT_TANH: "tanh"}


class Float64Context:
    """HipContext's posterior interface on float64 numpy arrays (the oracle's forward pass): what the device calls compute, in the
    precision of the reference, with a log of the calls."""
    log = []

    def __init__(self, device=None):
        self.n_rows = {}

    def set_data(self, X, which=capi.TRAIN):
        Float64Context.log.append("set_data")
        self.x0 = np.array(X, dtype=np.float64)
        self.x = self.x0.copy()
        self.n_rows[which] = len(self.x)

    def set_arch_from_weights(self, weights, in_dim, act_kind, out_kind, lik_kind):
        self.shapes = [w.shape for w in weights]
        self.fun = ACT_KINDS[act_kind]
        assert out_kind == capi.OUT_SOFTMAX

    def _layers(self, packed):
        out, at = [], 0
        for s in self.shapes:
            out.append(np.asarray(packed[at:at + s[0] * s[1]]).reshape(s))
            at += s[0] * s[1]
        return out

    def predict_sets(self, weight_sets, act_prm_sets=None, which=capi.TRAIN, apply_out_fn=True):
        Float64Context.log.append("predict_sets")
        probs = []
        for i, w in enumerate(weight_sets):
            act = orc.Act(self.fun, np.zeros(1) if act_prm_sets is None else act_prm_sets[i])
            probs.append(orc.forward(self.x, self._layers(w), act, orc.out_softmax))
        return np.array(probs)

    def permute_columns(self, cols, perms, which=capi.TRAIN):
        Float64Context.log.append("permute_columns")
        self.x = self.x0.copy()
        if perms is None or len(cols) == 0:
            return
        perms = np.asarray(perms)
        assert perms.shape in ((1, len(self.x)), (len(cols), len(self.x))) and len(set(cols)) == len(cols)
        for j, c in enumerate(cols):
            self.x[:, c] = self.x0[perms[j if len(perms) > 1 else 0], c]

    def predict_sets_summary(self, weight_sets, mode, labels=None, act_prm_sets=None, which=capi.TRAIN, want_summary=True,
                             apply_out_fn=True):
        Float64Context.log.append("predict_sets_summary")
        n = Float64Context.log.count("predict_sets")
        summary = posterior._summarise(self.predict_sets(list(weight_sets), act_prm_sets), mode)
        del Float64Context.log[-1]
        assert Float64Context.log.count("predict_sets") == n
        conf = None
        if labels is not None:
            conf = orc.confusion_counts(summary, np.asarray(labels), summary.shape[1])
        return (summary if want_summary else None), conf

    def close(self):
        pass


@pytest.fixture
def float64_seam(monkeypatch):
    Float64Context.log = []
    monkeypatch.setattr(backend, "HipContext", Float64Context)
    monkeypatch.setattr(posterior, "CalcAccuracy", lambda y, lab: orc.acc_classification(y, np.asarray(lab)))
    monkeypatch.delenv("NPBNN_FI_HOST", raising=False)
    return Float64Context


# ---- the permutation indices ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(57,), (57, 3), (1,), (2, 2)])
def test_permutation_of_the_row_count_is_the_permutation_of_the_values(shape):
    """np.random.permutation(n) leaves the global stream where np.random.permutation(values) does, and values[indices] is the
    array the latter returns - for a 1-D column and a 2-D block."""
    values = np.random.default_rng(3).standard_normal(shape)
    np.random.seed(11)
    shuffled = np.random.permutation(values)
    after = np.random.random()
    np.random.seed(11)
    idx = np.random.permutation(shape[0])
    assert np.random.random() == after
    np.testing.assert_array_equal(values[idx], shuffled)


def _predictor(x, monkeypatch):
    inp = ic.inputs("tanh")
    return posterior._SamplePredictor(x.shape[1], inp["samples"], bn.ActFun(fun="tanh"), bn.SoftMax)


@pytest.mark.parametrize("columns", [[4], [1, 4, 9], [9, 1], [3, 3], [2, 5, 2], np.array([6]), np.array([0]), 5, np.int64(2), [0], 0, [], None, [-1, 2]],
                         ids=repr)
@pytest.mark.parametrize("independently", [True, False])
def test_permute_draws_and_gathers_as_shuffled_copy(columns, independently, float64_seam, monkeypatch):
    x = ic.inputs("tanh")["x"]
    np.random.seed(5)
    want = posterior._shuffled_copy(x, columns, independently)
    after = np.random.random()
    pred = _predictor(x, monkeypatch)
    pred.load(x)
    np.random.seed(5)
    pred.permute(columns, independently)
    assert np.random.random() == after
    np.testing.assert_array_equal(pred._ctx.x, want)
    pred.permute(None, independently)            # restores
    np.testing.assert_array_equal(pred._ctx.x, x)


# ---- routing ----------------------------------------------------------------------------------------------------------
def _fi(mode, out_fn=None, labels=None, n_permutations=2, **kw):
    inp = ic.inputs("tanh")
    np.random.seed(3)
    return bn.feature_importance(inp["x"], weights_posterior=inp["samples"], true_labels=inp["labels"] if labels is None else labels,
                                 n_permutations=n_permutations, feature_blocks=[[0, 3], [5]], write_to_file=False,
                                 post_summary_mode=mode, actFun=bn.ActFun(fun="tanh"),
                                 output_act_fun=bn.SoftMax if out_fn is None else out_fn, **kw)


@pytest.mark.parametrize("mode", [0, 1])
def test_modes_0_and_1_upload_once_and_stay_on_the_device(mode, float64_seam):
    _fi(mode)
    log = float64_seam.log
    assert log.count("set_data") == 1
    assert "predict_sets" not in log
    assert log.count("predict_sets_summary") == 1 + 2 * 2
    assert log.count("permute_columns") == 1 + 2 * 2 + 1 and log[-1] == "permute_columns"      # (the last one restores)


def test_mode_2_takes_the_host_route(float64_seam):
    _fi(2)
    assert "predict_sets_summary" not in float64_seam.log and "permute_columns" not in float64_seam.log
    assert float64_seam.log.count("set_data") == float64_seam.log.count("predict_sets") == 5


def test_custom_output_callable_takes_the_host_route(float64_seam, monkeypatch):
    monkeypatch.setattr(Float64Context, "set_arch_from_weights",
                        lambda self, w, *a: (setattr(self, "shapes", [m.shape for m in w]), setattr(self, "fun", "tanh")))
    _fi(1, out_fn=lambda z: z)
    assert "predict_sets_summary" not in float64_seam.log and "permute_columns" not in float64_seam.log


def test_fi_host_forces_the_host_route(float64_seam, monkeypatch):
    monkeypatch.setenv("NPBNN_FI_HOST", "1")
    _fi(1)
    assert "predict_sets_summary" not in float64_seam.log and float64_seam.log.count("set_data") == 5


@pytest.mark.parametrize("labels", [np.full(ic.N_ROWS, 0.5), np.full(ic.N_ROWS, 7), np.full(ic.N_ROWS, -1), np.zeros((ic.N_ROWS, 1))],
                         ids=["fractions", "past_the_classes", "negative", "matrix"])
def test_labels_that_are_not_class_indices_take_the_host_route(labels, float64_seam, monkeypatch):
    monkeypatch.setattr(posterior, "CalcAccuracy", lambda y, lab: 0.0)
    _fi(1, labels=labels)
    assert "predict_sets_summary" not in float64_seam.log


@pytest.mark.parametrize("mode", [0, 1])
def test_both_routes_give_the_same_table(mode, float64_seam, monkeypatch):
    a = _fi(mode)
    monkeypatch.setenv("NPBNN_FI_HOST", "1")
    b = _fi(mode)
    assert a.equals(b)


# ---- argument checks raise before any device call ------------------------------------------------------------------------
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError("device call %s" % name)


def _bare_context(n_rows=10, n_out=3):
    ctx = backend.HipContext.__new__(backend.HipContext)
    ctx._lib = _NoDevice()
    ctx._ctx = None
    ctx.n_rows = {capi.TRAIN: n_rows}
    ctx.n_out = n_out
    ctx.arch = capi.Arch()
    ctx.arch.n_layers = 2
    return ctx


def test_argument_checks_in_python():
    ctx = _bare_context()
    sets = [np.zeros(5)]
    with pytest.raises(ValueError):
        ctx.permute_columns([1, 2], np.zeros((3, 10), dtype=np.int64))         # neither one nor one per column
    with pytest.raises(ValueError):
        ctx.permute_columns([1], np.zeros((1, 9), dtype=np.int64))             # not the matrix's rows
    with pytest.raises(ValueError):
        ctx.predict_sets_summary(sets, 2, labels=np.zeros(10))                 # mode 2 has no device summary
    with pytest.raises(ValueError):
        ctx.predict_sets_summary(sets, 0, labels=None, want_summary=False)     # nothing asked for
    with pytest.raises(ValueError):
        ctx.predict_sets_summary(sets, 0, labels=np.zeros(9))                  # not one label per row
    ctx.close = lambda: None


def test_permute_rejects_columns_outside_the_matrix(float64_seam, monkeypatch):
    x = ic.inputs("tanh")["x"]
    pred = _predictor(x, monkeypatch)
    pred.load(x)
    n = len(float64_seam.log)
    for bad in ([11], [0, -12], [1.5]):
        with pytest.raises(IndexError):
            pred.permute(bad, True)
    assert len(float64_seam.log) == n


# ---- the reference's tables ------------------------------------------------------------------------------------------------
def test_golden_file_is_complete():
    g = ic.load()
    assert sorted(g.files) == sorted(ic.key(c, m, u, t) + s for c in ic.CASES for m, u, t in ic.combinations() for s in ("/index", "/values"))
    top = [g[k][0, 0] for k in g.files if k.endswith("/values")]
    assert max(top) > 0.02 and len(set(np.round(top, 6))) > 10                 # not degenerate


@pytest.mark.parametrize("name", ic.CASES)
def test_float64_oracle_reproduces_the_reference_exactly(name):
    """The inputs leave no near-tie for float64 to fall on either side of: the oracle's own feature_importance gives the
    reference's tables to the last bit (importance_cases.assert_same_table: every number, and the ranking up to blocks of
    equal mean loss), so the GPU test's one-instance allowance cannot hide a wrong shuffle."""
    g = ic.load()
    inp = ic.inputs(name)
    for mode, unlink, tag in ic.combinations():
        np.random.seed(ic.SEED)
        order, _, table = orc.feature_importance(inp["x"], inp["samples"], orc.Act(inp["fun"]), orc.out_softmax, inp["labels"],
                                                 n_permutations=ic.N_PERMUTATIONS, feature_blocks=ic.BLOCKS[tag], summary_mode=mode,
                                                 unlink_features_within_block=unlink)
        k = ic.key(name, mode, unlink, tag)
        ic.assert_same_table(order, table, g[k + "/index"], g[k + "/values"], k)


@pytest.mark.parametrize("host", [False, True], ids=["device_route", "host_route"])
@pytest.mark.parametrize("name", ic.CASES)
def test_feature_importance_reproduces_the_reference(name, host, float64_seam, monkeypatch):
    """bn.feature_importance over the float64 stand-in: the same draws, blocks, summaries, accuracies, ranking and columns as the
    reference's data frame, on either route."""
    if host:
        monkeypatch.setenv("NPBNN_FI_HOST", "1")
    g = ic.load()
    for mode, unlink, tag in ic.combinations():
        order, values, df = ic.run(bn, name, mode, unlink, tag)
        k = ic.key(name, mode, unlink, tag)
        ic.assert_same_table(order, values, g[k + "/index"], g[k + "/values"], k)
        assert list(df.columns) == ['feature_block_index', 'feature_name', 'delta_acc_mean', 'delta_acc_std',
                                    'acc_with_feature_randomized_mean', 'acc_with_feature_randomized_std']
    assert ("predict_sets_summary" in float64_seam.log) != host
