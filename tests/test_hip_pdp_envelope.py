"""npbnn_predict_pdp against the float64 oracle over the whole envelope of its two routes (tests/pdp_cases.py's ENVELOPE): depths and
bias patterns, the widths, feature counts and tail sizes at which the grid-batched kernel (route 1) hands over to one pass per grid
point (route 2), every activation and output kind, row and set counts around a workgroup and a launch, overrides, the test table,
grid values far outside the data and a posterior of 300 sets.  Every case asserts the route it names.  tests/test_host_pdp.py checks
on the host that the references tell a wrong kernel from a right one."""
import numpy as np
import pytest

import pdp_cases
from npbnn_amd import _capi as capi
from test_hip_pdp import TOL, device_means

pytestmark = pytest.mark.gpu

OUT_KINDS = {"softmax": capi.OUT_SOFTMAX, "identity": capi.OUT_IDENTITY, "softplus_half": capi.OUT_SOFTPLUS_HALF}
ROUTES_AGREE = 1e-5      # as test_hip_pdp.test_routes_agree_on_config2_shapes
worst = {}               # (route, output kind) -> (largest |device - oracle|, case), printed as the run goes (-s shows it)


def _device(case, inp):
    return device_means(inp["x"], inp["weights"], inp["focal"], inp["grid"], fun=case["fun"], out_kind=OUT_KINDS[case["out"]],
                        slopes=inp["slopes"], override=inp["override"], which=case["which"], apply_out_fn=case["apply_out"],
                        x_test=inp["x_test"], trainable=case["trainable"], want_l0=True)


def _note(case, route, err):
    key = (route, case["out"] if case["apply_out"] else "raw")
    if err >= worst.get(key, (0.0, ""))[0]:
        worst[key] = (err, case["name"])
    print("\npdp envelope %-40s route %d  max|device - oracle| %.3e   worst so far %s" % (
        case["name"], route, err, "  ".join("%d/%s %.2e" % (k + (v[0],)) for k, v in sorted(worst.items()))))


@pytest.mark.parametrize("name", list(pdp_cases.ENVELOPE))
def test_envelope(name, monkeypatch):
    case = pdp_cases.ENVELOPE[name]
    inp = pdp_cases.envelope_inputs(case)
    want = pdp_cases.envelope_oracle(case, inp)
    # many sets: a fixed-order float32 sum of S terms, divided by S, is off by at most S 2^-24 max|term| on top of each term's own error
    bar = TOL + (case["sets"] * 2.0 ** -24 * np.abs(want).max() if case["many_sets"] else 0.0)
    for k, v in case["env"]:
        monkeypatch.setenv(k, v)
    got, route, l0 = _device(case, inp)
    err = float(np.abs(got - want).max())
    _note(case, route, err)
    assert route == case["route"]
    if case["l0"]:
        assert l0 == case["l0"]
    assert got.shape == want.shape
    assert err <= bar, (err, bar)
    if case["both_routes"]:
        monkeypatch.setenv("NPBNN_PDP_PER_GRID", "1")
        other, other_route, _ = _device(case, inp)
        other_err = float(np.abs(other - want).max())
        _note(case, other_route, other_err)
        assert other_route == 2
        assert other_err <= bar, (other_err, bar)
        assert np.abs(got - other).max() < ROUTES_AGREE
