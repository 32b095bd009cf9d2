"""The partial-dependence fixture (tests/golden/pdp.npz, written from the reference by tests/golden/make_pdp_golden.py) as calls of
this package, and a float64 stand-in for the device seam of npbnn_amd.pdp built on the oracle's forward pass."""
import os

import numpy as np

import oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pdp.npz")


def load():
    """{case: dict of its inputs and the reference's outputs}"""
    z = np.load(GOLDEN)
    cases = {}
    for key in z.files:
        name, field = key.split("/", 1)
        cases.setdefault(name, {})[field] = z[key]
    for c in cases.values():
        c["weights"] = [[c["w_%d_%d" % (s, l)] for l in range(int(c["n_layers"]))] for s in range(int(c["n_samples"]))]
        c["focal"] = [int(v) for v in c["focal"]]
        c["fun"] = str(c["fun"])
        c["mode"] = str(c["mode"])
    return cases


def call_args(bn, case):
    """Arguments of ``get_pdp`` for a fixture case (a fresh activation object every time)."""
    act = bn.ActFun(fun=case["fun"])
    out_fn = bn.SoftMax if case["mode"] == "classification" else bn.RegressTransform
    transform = bn.data_transform_obj(case["indicators"], case["means"]) if bool(case["has_transform"]) else None
    return (case["x"], case["focal"], case["mode"], int(case["n_out"]), act, out_fn, case["weights"], list(case["alphas"]), transform)


def oracle_row_means(data, focal_features, grid, weights, alphas, actFun, output_act_fun, data_transform):
    """float64 stand-in for npbnn_amd.pdp._pdp_row_means: grid values, then the feature indicators, then every sample's forward pass
    with its own slopes."""
    from npbnn_amd import _capi as capi
    from npbnn_amd.layers import output_kind
    kind = output_kind(output_act_fun)
    out_fn = {capi.OUT_SOFTMAX: orc.out_softmax, capi.OUT_IDENTITY: orc.out_identity}[kind]
    res = []
    for point in grid:
        x = np.array(data, dtype=np.float64, copy=True)
        x[:, focal_features] = point
        if data_transform is not None:
            x = data_transform.transform(x)
        preds = [out_fn(orc.forward_logits(x, w, orc.Act(actFun._function, prm=np.asarray(a, dtype=float))))
                 for w, a in zip(weights, alphas)]
        res.append(np.mean(preds, axis=0))
    return np.array(res)
