"""The weight gradient of the log-likelihood (npbnn_loglik_grad, bn.loglik_grad) restated in float64 on the oracle's layers
(``restate``), the same restatement in numpy float32 with the sums over the rows in float64 as on the device, the scale ``A`` that
float32 rounding acts on, deliberately wrong variants for the guards of tests/test_host_grad.py, the case table (CASES) with its inputs,
and a float64 stand-in for the device seam of npbnn_amd.gradient (``GradOracleBackend``).

A case is one of tests/pdp_cases.py's envelope draws (same keys, ``sets`` = 1), one or two axes away from the defaults; labels,
targets, sigmas and row weights come from a generator of the case's own.  For ReLU and leaky cases the rows within
saliency_cases.MARGIN of a kink are drawn again, as saliency's cases do (saliency_cases.inputs)."""
import numpy as np

import oracle as orc
import pdp_cases
import saliency_cases as sc
from attrib_common import _act, _apply_override
from oracle_backend import OracleBackend

WRONG = ("no_factor", "bias_as_feature", "drop_last_row", "softmax_no_p", "no_lik_temp")
MARGIN_BAR = 16.0            # the margin tests/test_hip_loo.py gives over a restatement's distance
EPS32 = 2.0 ** -24


def restate(x, labels, weights, act, lik, sigma=None, lik_temp=1.0, row_weight=None, override=None, dtype=np.float64, wrong=None):
    """{'grads', 'A': per layer; 'loglik', 'sum_r', 'sum_r2'} of one weight set on the rows of ``x`` after ``override``.  Per row
    everything is computed in ``dtype``; the sums over the rows are float64 sums of those values.  ``lik``: "cat" (labels: class
    indices; ``row_weight`` per row), "gauss" (``sigma`` per target) or "pred" (mu = z[:k], s = softplus(z[k:]))."""
    x = _apply_override(x, override)
    labels = np.asarray(labels)
    if wrong == "drop_last_row":
        x, labels = x[:-1], labels[:-1]
        row_weight = None if row_weight is None else row_weight[:-1]
    n = x.shape[0]
    w = [np.asarray(m, dtype=np.float64).astype(dtype) for m in weights]
    tmp = x.astype(dtype)
    inputs, factors = [], []
    for i in range(len(w) - 1):
        inputs.append(tmp)
        z = orc.dense(tmp, w[i]).astype(dtype)
        factors.append(np.asarray(sc._act_derivative(z, act, i)).astype(dtype))
        tmp = orc.activate(z, act, i).astype(dtype)
    inputs.append(tmp)
    z = orc.dense(tmp, w[-1]).astype(dtype)
    res = dict(sum_r=None, sum_r2=None)
    if lik == "cat":
        y = labels.astype(int).ravel()
        e = np.exp(z - z.max(axis=1, keepdims=True))
        p = (e / e.sum(axis=1, keepdims=True)).astype(dtype)
        rw = np.ones(n, dtype=dtype) if row_weight is None else np.asarray(row_weight).astype(dtype)
        g = np.zeros_like(p)
        g[np.arange(n), y] = 1
        if wrong != "softmax_no_p":
            g = g - p
        g = (g * rw[:, None]).astype(dtype)
        ll = np.sum(rw.astype(np.float64) * np.log(p[np.arange(n), y].astype(np.float64)))
    else:
        t = labels.reshape(n, -1).astype(dtype)
        k = t.shape[1]
        if lik == "gauss":
            s = np.asarray(sigma, dtype=np.float64)
            r = (t - z).astype(np.float64)
            res.update(sum_r=r.sum(axis=0), sum_r2=(r * r).sum(axis=0))
            ll = orc.lik_gaussian(z.astype(np.float64), t.astype(np.float64), sig2=s)
            g = ((t - z) * (1.0 / (s * s)).astype(dtype)).astype(dtype)
        else:
            mu, zs = z[:, :k], z[:, k:]
            s = orc.softplus(zs).astype(dtype)
            ll = orc.lik_gaussian_error(np.concatenate([mu, s], axis=1).astype(np.float64), t.astype(np.float64))
            sig = ((1 + np.exp(-zs)) ** (-1)).astype(dtype)
            g = np.concatenate([(t - mu) / (s * s), ((t - mu) ** 2 / s ** 3 - 1 / s) * sig], axis=1).astype(dtype)
    if wrong == "no_factor" and factors:
        factors[0] = np.ones_like(factors[0])
    scale = 1.0 if wrong == "no_lik_temp" else lik_temp
    grads, big = [None] * len(w), [None] * len(w)
    delta = g
    for l in range(len(w) - 1, -1, -1):
        h = inputs[l]
        d64, h64 = delta.astype(np.float64), h.astype(np.float64)
        gw, aw = d64.T @ h64, np.abs(d64).T @ np.abs(h64)
        if w[l].shape[1] == h.shape[1] + 1:
            b = d64.T @ h64[:, 0] if wrong == "bias_as_feature" else d64.sum(axis=0)
            gw = np.concatenate([b[:, None], gw], axis=1)
            aw = np.concatenate([np.abs(d64).sum(axis=0)[:, None], aw], axis=1)
        grads[l], big[l] = scale * gw, abs(scale) * float(aw.max())
        if l > 0:
            delta = ((delta @ sc._matrix(w[l], w[l - 1].shape[0])) * factors[l - 1]).astype(dtype)
    res.update(grads=grads, A=big, loglik=scale * float(ll))
    return res


# ---- the cases ------------------------------------------------------------------------------------------------------------------
CASES = {}
_EXTRA = dict(lik="cat", k=0, lik_temp=1.0, class_w=False, inst_w=False, last_scale=1.0)


def _case(name, **kw):
    assert name not in CASES, name
    unknown = set(kw) - set(pdp_cases._DEFAULTS) - set(_EXTRA)
    assert not unknown, (name, unknown)
    c = dict(pdp_cases._DEFAULTS, **_EXTRA)
    c.update(name=name, sets=1, seed=12000 + len(CASES), **kw)
    if c["lik"] == "gauss":
        c["n_out"], c["out"] = c["k"], "identity"
    elif c["lik"] == "pred":
        c["n_out"], c["out"] = 2 * c["k"], "softplus_half"
    CASES[name] = c


for _rows in (1, 255, 256, 257, 2111):
    _case("rows_%d" % _rows, rows=_rows)
for _f in (31, 32, 33, 65):
    _case("features_%d" % _f, features=_f)
for _h0 in (1, 31, 32, 33, 65, 130):
    _case("h0_%d" % _h0, nodes=(_h0, 6))
for _w in (1, 33):
    _case("later_%d" % _w, nodes=(20, _w))
_case("outputs_1_gauss", lik="gauss", k=1)
for _c in (2, 7, 33):
    _case("outputs_%d" % _c, n_out=_c)
_case("one_matrix", nodes=(), n_out=3)
_case("one_matrix_no_bias", nodes=(), n_out=3, bias="none")
_case("five_matrices_mixed01", nodes=(20, 12, 9, 6), bias="mixed01")
_case("five_matrices_mixed10", nodes=(20, 12, 9, 6), bias="mixed10")
for _tag, _kw in [("relu", dict(fun="ReLU")), ("leaky", dict(fun="ReLU", trainable=True)), ("genrelu_a", dict(fun="genReLU", slopes="shared")),
                  ("genrelu_b", dict(fun="genReLU", slopes="per_set")), ("swish", dict(fun="swish")), ("tanh", dict(fun="tanh"))]:
    _case("act_%s_33x9" % _tag, nodes=(33, 9), **_kw)
_case("cat_class_weights", class_w=True)
_case("cat_instance_weights", inst_w=True)
_case("cat_lik_temp_037", lik_temp=0.37)
for _k in (1, 3, 16):
    _case("gauss_k%d" % _k, lik="gauss", k=_k)
for _k in (1, 2):
    _case("pred_sigma_k%d" % _k, lik="pred", k=_k, last_scale=0.5)
_case("override_two_columns", override={5: 1.25, 17: -0.75})
_case("test_table", which=1, test_rows=173)
# five chunks of 512, 512, 512, 512 and 63 rows (tests/test_host_grad_plan.py asserts the cut these bytes give)
_case("scratch_in_chunks", rows=2111, env=(("NPBNN_GRAD_SCRATCH_BYTES", "300000"),))
_case("streamed_257x700", rows=257, features=700, nodes=(50, 5))
_case("config2_network", rows=3000, features=256, nodes=(32, 8), n_out=10)
# row weights are the training table's alone: on the test table the entry must leave them out
_case("test_table_with_row_weights", which=1, test_rows=173, class_w=True, inst_w=True)

FD_CASES = ("act_tanh_33x9", "act_swish_33x9", "rows_257", "one_matrix", "cat_class_weights", "cat_lik_temp_037", "gauss_k3", "pred_sigma_k2",
            "five_matrices_mixed01", "override_two_columns")
_shared = {}


def inputs(case):
    """saliency_cases.inputs' arrays (kinks redrawn), the first set's weights, and the case's labels or targets for both tables,
    sigmas, row weights and slopes"""
    inp = sc.inputs(case)
    rs = np.random.default_rng(case["seed"] + 7)
    w = [np.array(m, copy=True) for m in inp["weights"][0]]
    w[-1] *= case["last_scale"]
    inp["w"] = w
    inp["slopes1"] = None if inp["slopes"] is None else np.asarray(inp["slopes"][0], dtype=float)

    def labels(n):
        if case["lik"] == "cat":
            return rs.integers(0, case["n_out"], n)
        return rs.standard_normal((n, case["k"]))

    inp["y"] = labels(case["rows"])
    inp["y_test"] = labels(case["test_rows"]) if case["test_rows"] else None
    inp["sigma"] = rs.uniform(0.3, 2.0, case["k"]) if case["lik"] == "gauss" else None
    inp["class_w"] = rs.uniform(0.5, 2.0, case["n_out"]) if case["class_w"] else None
    inp["inst_w"] = rs.uniform(0.2, 3.0, case["rows"]) if case["inst_w"] else None
    inp["labels"] = inp["y_test"] if case["which"] == 1 else inp["y"]
    return inp


def row_weight(case, inp):
    """the rows' weights as the device holds them: float32 instance weights, float64 class weights; training table only"""
    if case["which"] == 1 or (inp["inst_w"] is None and inp["class_w"] is None):
        return None
    rw = np.ones(case["rows"])
    if inp["inst_w"] is not None:
        rw = rw * inp["inst_w"].astype(np.float32).astype(np.float64)
    if inp["class_w"] is not None:
        rw = rw * inp["class_w"][inp["labels"]]
    return rw


def reference(case, inp, dtype=np.float64, wrong=None):
    """``restate`` of the case on the table, targets and instance weights the device holds (float32 entries)"""
    table = inp["table"].astype(np.float32).astype(np.float64)
    lab = inp["labels"] if case["lik"] == "cat" else inp["labels"].astype(np.float32).astype(np.float64)
    return restate(table, lab, inp["w"], _act(case["fun"], inp["slopes1"], case["trainable"]), case["lik"], sigma=inp["sigma"],
                   lik_temp=case["lik_temp"], row_weight=row_weight(case, inp), override=inp["override"], dtype=dtype, wrong=wrong)


def bars(want, want32):
    """per layer: MARGIN_BAR times the larger of the float32 restatement's distance to float64 and 2^-24 A; and the two quantities"""
    a = [float(np.abs(g32 - g).max()) for g32, g in zip(want32["grads"], want["grads"])]
    b = [EPS32 * big for big in want["A"]]
    return [MARGIN_BAR * max(x, y) for x, y in zip(a, b)], a, b


def case_data(name):
    """(case, inputs, float64 restatement, float32 restatement), computed once"""
    if name not in _shared:
        case = CASES[name]
        inp = inputs(case)
        _shared[name] = (case, inp, reference(case, inp), reference(case, inp, dtype=np.float32))
    return _shared[name]


# ---- a stand-in for the device seam -------------------------------------------------------------------------------------------------
class GradOracleBackend(OracleBackend):
    """OracleBackend with ``loglik_grad`` served by ``restate`` in ``dtype`` on the model's host arrays."""
    dtype = np.float64
    _LIK = {0: "cat", 1: "gauss", 2: "pred"}

    def loglik_grad(self, weights, slopes=None, col_override=None, lik_temp=1.0, sigma=None, which=0):
        x, lab = self._data(which)
        rw = None
        if self.lik_kind == 0 and which == 0:
            # (the instance weight times the class weight, each 1 where the model has none: as the entry and npbnn_eval apply them)
            if self.bnn._instance_weights is not None or len(self.bnn._class_w):
                rw = np.ones(len(x))
            if self.bnn._instance_weights is not None:
                rw = rw * np.asarray(self.bnn._instance_weights, dtype=float)
            if len(self.bnn._class_w):
                rw = rw * np.asarray(self.bnn._class_w)[lab]
        r = restate(np.asarray(x, dtype=np.float64), lab, weights, self._act(slopes), self._LIK[self.lik_kind], sigma=sigma, lik_temp=lik_temp,
                    row_weight=rw, override=col_override, dtype=self.dtype)
        return dict(loglik=r["loglik"], sigma=None if sigma is None else np.asarray(sigma, dtype=float), sum_r=r["sum_r"], sum_r2=r["sum_r2"],
                    n_rows=len(x), confusion=None), r["grads"]


class GradOracleBackend32(GradOracleBackend):
    dtype = np.float32


# ---- the model of map_estimate's run on the device (tests/test_hip_grad.py) and of its float32 confirmation on the CPU
# (tests/test_host_grad.py): 600 x 12, [8, 4], 3 classes, tanh, labels from a seeded teacher network, TEACHER_STEPS steps
TEACHER_STEPS = 60


def teacher_model():
    import contextlib
    import io

    import npbnn_amd as bn
    rs = np.random.default_rng(21)
    x = rs.standard_normal((600, 12))
    z = orc.forward_logits(x, [rs.normal(0, 1.0, (6, 13)), rs.normal(0, 1.0, (3, 6))], orc.Act("tanh"))
    labels = np.digitize(z[:, 0], np.quantile(z[:, 0], [1 / 3, 2 / 3]))
    dat = dict(data=x, labels=labels, test_data=np.zeros((0, 12)), test_labels=np.zeros(0))
    np.random.seed(1234)
    with contextlib.redirect_stdout(io.StringIO()):
        return bn.npBNN(dat, n_nodes=[8, 4], actFun=bn.ActFun(fun="tanh"))
