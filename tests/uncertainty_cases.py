"""The cases of tests/golden/uncertainty.npz (make_uncertainty_golden.py): seeded inputs, keys, and an independent float64 restatement
of the uncertainty decomposition from pre-output values.

Classification and ``"regression"`` inputs are ``lppd_cases.inputs`` (203 ragged rows, 11 features, C in {2, 3, 4, 10}, S in
{1, 2, 3, 4, 7, 64}, genReLU with per-sample slopes, one to three hidden layers; their labels and targets are not read).  The
``"regression-error"`` cases are this file's: T in {1, 2, 3} targets, so 2, 4 and 6 outputs - a width read output by output, a
16-byte vector that straddles the boundary between means and sigmas, and a width that is no multiple of four - with S in {1, 3, 7}
and one genReLU case."""
import os

import numpy as np

import cases
import lppd_cases as lc

N_ROWS = lc.N_ROWS
N_FEATURES = lc.N_FEATURES
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uncertainty.npz")
CLASS_FIELDS = ("mean_prob", "predictive_entropy_i", "expected_entropy_i", "mutual_information_i")
CLASS_TOTALS = {"predictive_entropy": "predictive_entropy_i", "expected_entropy": "expected_entropy_i", "mutual_information": "mutual_information_i"}
REGRESSION_FIELDS = ("mean", "epistemic_var", "aleatoric_var")       # (total_var is their sum: not stored)
# name -> activation, hidden layers, outputs (means then sigmas), stored samples, bias mode
ERROR_CASES = {
    "tanh_h2_err2_s7": dict(fun="tanh", nodes=(6, 5), n_out=4, s=7, bias=2, kind="err"),
    "genrelu_h2_err1_s3": dict(fun="genReLU", nodes=(6, 4), n_out=2, s=3, bias=2, kind="err"),
    "swish_h1_err3_s1": dict(fun="swish", nodes=(7,), n_out=6, s=1, bias=1, kind="err"),
    "relu_h3_err3_s7": dict(fun="ReLU", nodes=(6, 5, 4), n_out=6, s=7, bias=3, kind="err"),
}
CASES = dict(lc.CASES, **ERROR_CASES)
KINDS = {"cat": "classification", "reg": "regression", "err": "regression-error"}


def key(name, field):
    return "%s/%s" % (name, field)


def kind_of(name):
    return KINDS[CASES[name]["kind"]]


def fields_of(name):
    return CLASS_FIELDS if CASES[name]["kind"] == "cat" else REGRESSION_FIELDS


def inputs(name, n_rows=N_ROWS, spec=None, seed=None):
    """x and the stored samples (weights, alphas, and error_prm for ``"regression"``), with the case's description.  ``spec`` and
    ``seed``: a description in ERROR_CASES' or lppd_cases.CASES' form and the string the generator is seeded from, for a case of
    another table (fold_envelope_cases)."""
    if (name in lc.CASES) if spec is None else (spec["kind"] != "err"):
        return lc.inputs(name, n_rows, spec, seed)
    spec = ERROR_CASES[name] if spec is None else spec
    rs = np.random.default_rng(cases.hash_name("uncertainty/" + name if seed is None else seed) % (2 ** 31))
    x = rs.standard_normal((n_rows, N_FEATURES))
    shapes = cases.layer_shapes(N_FEATURES, list(spec["nodes"]), spec["n_out"], spec["bias"])
    teacher = [rs.normal(0, 0.6, s) for s in shapes]
    genrelu = spec["fun"] == "genReLU"
    samples = [dict(weights=[t + rs.normal(0, 0.15, t.shape) for t in teacher],
                    alphas=rs.uniform(0.0, 0.3, len(spec["nodes"])) if genrelu else np.zeros(1), mcmc_it=100 * i) for i in range(spec["s"])]
    return dict(x=x, samples=samples, labels=None, fun=spec["fun"], kind="err", n_out=spec["n_out"], bias=spec["bias"], nodes=spec["nodes"])


act_for = lc.act_for
slopes_of = lc.slopes_of
sigmas_of = lc.sigmas_of


def restatement(z, kind, sigma=None):
    """The definitions, term by term in float64, from pre-output values z [S, N, outputs] (no shared code with the package)."""
    z = np.asarray(z, dtype=np.float64)
    n_samples = z.shape[0]
    if kind == "classification":
        top = z.max(axis=2, keepdims=True)
        e = np.exp(z - top)
        se = e.sum(axis=2, keepdims=True)
        p = e / se
        lse = (top + np.log(se))[:, :, 0]
        h = lse - np.sum(p * z, axis=2)
        m = p.sum(axis=0) / n_samples
        with np.errstate(divide="ignore", invalid="ignore"):
            predictive = -np.where(m > 0, m * np.log(m), 0.0).sum(axis=1)
        expected = h.sum(axis=0) / n_samples
        mutual = np.maximum(0.0, predictive - expected) if n_samples > 1 else np.zeros(z.shape[1])
        return dict(mean_prob=m, predictive_entropy_i=predictive, expected_entropy_i=expected, mutual_information_i=mutual)
    if kind == "regression-error":
        t = z.shape[2] // 2
        mu = z[:, :, :t]
        zs = z[:, :, t:]
        sig = np.maximum(zs, 0.0) + np.log1p(np.exp(-np.abs(zs)))
        aleatoric = (sig * sig).sum(axis=0) / n_samples
    else:
        mu = z
        s = np.asarray(sigma, dtype=np.float64)
        aleatoric = np.tile((s * s).sum(axis=0) / n_samples, (z.shape[1], 1))
    mean = mu.sum(axis=0) / n_samples
    epistemic = ((mu - mean[None]) ** 2).sum(axis=0) / n_samples
    return dict(mean=mean, epistemic_var=epistemic, aleatoric_var=aleatoric, total_var=epistemic + aleatoric)


def outputs_from_values(z, kind):
    """Post-output predictions in float64 from pre-output values: what ``posterior_uncertainty`` takes."""
    z = np.asarray(z, dtype=np.float64)
    if kind == "classification":
        e = np.exp(z - z.max(axis=2, keepdims=True))
        return e / e.sum(axis=2, keepdims=True)
    if kind == "regression-error":
        t = z.shape[2] // 2
        return np.concatenate([z[:, :, :t], np.logaddexp(0.0, z[:, :, t:])], axis=2)
    return z


def oracle_values(inp):
    """Pre-output values [S, N, outputs] of a case from the float64 oracle's forward pass."""
    import oracle as orc
    return np.array([orc.forward_logits(inp["x"], s["weights"], orc.Act(inp["fun"], s["alphas"])) for s in inp["samples"]])


def load():
    return np.load(GOLDEN)
