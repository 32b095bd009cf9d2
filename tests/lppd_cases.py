"""The cases of tests/golden/lppd.npz (make_lppd_golden.py): seeded inputs, keys, and the float64 log-likelihood matrix of a case.

Inputs: a teacher network, the stored samples perturbations of it, the labels the teacher's calls with a share flipped
(classification) or its output plus noise (regression) - so that the log-likelihoods differ between rows and samples the way a
posterior's do.  Every activation, one to three hidden layers, C in {2, 3, 4, 10}, S in {1, 2, 3, 4, 7, 64}, genReLU with a slope
vector per sample (the replay then splits into groups of one), regression with 1 and 3 targets."""
import os

import numpy as np

import cases

N_ROWS = 203                    # ragged: not a multiple of 4, 16 or 64
N_FEATURES = 11
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lppd.npz")
FIELDS = ("lppd_i", "mean_log_lik_i", "p_waic_i", "log_lik_sample")
# name -> activation, hidden layers, outputs, stored samples, bias mode, kind
CASES = {
    "relu_h1_c2_s1": dict(fun="ReLU", nodes=(6,), n_out=2, s=1, bias=1, kind="cat"),
    "tanh_h2_c4_s7": dict(fun="tanh", nodes=(6, 5), n_out=4, s=7, bias=2, kind="cat"),
    "swish_h3_c3_s4": dict(fun="swish", nodes=(6, 5, 4), n_out=3, s=4, bias=3, kind="cat"),
    "genrelu_h2_c10_s64": dict(fun="genReLU", nodes=(8, 6), n_out=10, s=64, bias=2, kind="cat"),
    "genrelu_h2_c4_s3": dict(fun="genReLU", nodes=(6, 5), n_out=4, s=3, bias=2, kind="cat"),
    "tanh_h2_c10_s2": dict(fun="tanh", nodes=(6, 5), n_out=10, s=2, bias=2, kind="cat"),
    "relu_h2_c3_s64": dict(fun="ReLU", nodes=(6, 5), n_out=3, s=64, bias=0, kind="cat"),
    "tanh_h2_reg1_s7": dict(fun="tanh", nodes=(6, 4), n_out=1, s=7, bias=2, kind="reg"),
    "swish_h1_reg3_s4": dict(fun="swish", nodes=(7,), n_out=3, s=4, bias=2, kind="reg"),
    "genrelu_h3_reg3_s3": dict(fun="genReLU", nodes=(6, 5, 4), n_out=3, s=3, bias=2, kind="reg"),
    "relu_h2_reg4_s64": dict(fun="ReLU", nodes=(6, 4), n_out=4, s=64, bias=1, kind="reg"),
}


def key(name, field):
    return "%s/%s" % (name, field)


def inputs(name, n_rows=N_ROWS, spec=None, seed=None):
    """x, the stored samples (weights, alphas, and error_prm for regression), labels (class indices) or targets [rows, outputs].
    ``spec`` and ``seed``: a description in CASES' form and the string the generator is seeded from, for a case of another table
    (fold_envelope_cases); a single class has no other class to flip a label to."""
    spec = CASES[name] if spec is None else spec
    rs = np.random.default_rng(cases.hash_name("lppd/" + name if seed is None else seed) % (2 ** 31))
    x = rs.standard_normal((n_rows, N_FEATURES))
    shapes = cases.layer_shapes(N_FEATURES, list(spec["nodes"]), spec["n_out"], spec["bias"])
    reg = spec["kind"] == "reg"
    teacher = [rs.normal(0, 0.5 if reg else 0.8, s) for s in shapes]
    genrelu = spec["fun"] == "genReLU"
    samples = []
    for i in range(spec["s"]):
        smp = dict(weights=[t + rs.normal(0, 0.05 if reg else 0.3, t.shape) for t in teacher],
                   alphas=rs.uniform(0.0, 0.3, len(spec["nodes"])) if genrelu else np.zeros(1), mcmc_it=100 * i)
        if reg:
            smp["error_prm"] = rs.uniform(0.5, 1.5, spec["n_out"])
        samples.append(smp)
    import oracle as orc                                  # (the float64 oracle's forward pass: the teacher's output)
    z = orc.forward_logits(x, teacher, orc.Act(spec["fun"], np.full(len(spec["nodes"]), 0.15)))
    if spec["kind"] == "cat":
        labels = np.argmax(z, axis=1).astype(np.int64)
        if spec["n_out"] > 1:
            flip = rs.random(n_rows) < 0.1
            labels = np.where(flip, (labels + rs.integers(1, spec["n_out"], n_rows)) % spec["n_out"], labels).astype(np.int64)
    else:
        # (targets a float32 holds exactly: the device keeps them in float32, and the cases are about the likelihood, not that rounding)
        labels = (z + 0.7 * rs.standard_normal(z.shape)).astype(np.float32).astype(np.float64)
    return dict(x=x, samples=samples, labels=labels, fun=spec["fun"], kind=spec["kind"], n_out=spec["n_out"], bias=spec["bias"],
                nodes=spec["nodes"])


def act_for(bn, fun, n_hidden):
    return bn.ActFun(fun=fun, prm=np.zeros(n_hidden)) if fun == "genReLU" else bn.ActFun(fun=fun)


def slopes_of(inp):
    return [np.asarray(s["alphas"], dtype=float)[:len(inp["nodes"])] for s in inp["samples"]] if inp["fun"] == "genReLU" else None


def sigmas_of(inp):
    return np.array([s["error_prm"] for s in inp["samples"]]) if inp["kind"] == "reg" else None


def log_lik_from_values(z, labels, kind, sigma=None):
    """ll [S, N] in float64 from pre-output values z [S, N, outputs]: the log-softmax at the label, or the Gaussian log-density
    summed over the targets, written out term by term (no shared code with the package)."""
    z = np.asarray(z, dtype=np.float64)
    if kind == "cat":
        top = z.max(axis=2)
        lse = top + np.log(np.exp(z - top[:, :, None]).sum(axis=2))
        return z[:, np.arange(z.shape[1]), np.asarray(labels, dtype=np.int64)] - lse
    sig = np.asarray(sigma, dtype=np.float64)[:, None, :]
    u = (np.asarray(labels, dtype=np.float64)[None] - z) / sig
    return np.sum(-0.5 * np.log(2 * np.pi) - np.log(sig) - 0.5 * u * u, axis=2)


def oracle_log_lik(inp):
    """ll [S, N] of a case from the float64 oracle's forward pass."""
    import oracle as orc
    z = np.array([orc.forward_logits(inp["x"], s["weights"], orc.Act(inp["fun"], s["alphas"])) for s in inp["samples"]])
    return log_lik_from_values(z, inp["labels"], inp["kind"], sigmas_of(inp))


def load():
    return np.load(GOLDEN)
