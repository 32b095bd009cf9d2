"""What the one softmax fold behind npbnn_predict_sets_uncertainty and npbnn_predict_sets_calibration makes structural
(softmax_mean_accumulate_kernel, npbnn_fold.hip.h): both entries form the per-class sums of the sets' probabilities with the same
expressions in the same order and both final kernels divide them by the number of sets, so calibration's confidence and predicted
class are, bit for bit, the maximum and the first argmax of uncertainty's mean probabilities."""
import numpy as np
import pytest

import npbnn_amd as bn
import uncertainty_cases as uc
from npbnn_amd import HipContext, _capi as capi

pytestmark = pytest.mark.gpu

N_SETS = 7                                         # replayed in groups of three, three and one


@pytest.mark.parametrize("name", ["tanh_h2_c4_s7", "swish_h3_c3_s4"])       # C = 4: rows read as float4; C = 3: value by value
def test_calibration_reads_the_mean_probabilities_uncertainty_reports(name):
    inp = uc.inputs(name)
    sets = [inp["samples"][i % len(inp["samples"])]["weights"] for i in range(N_SETS)]      # (four stored samples: the first three twice)
    ctx = HipContext(0)
    try:
        ctx.set_data(inp["x"])
        ctx.set_arch_from_weights(sets[0], inp["x"].shape[1], uc.act_for(bn, inp["fun"], len(inp["nodes"])).device_kind(), capi.OUT_SOFTMAX,
                                  capi.LIK_NONE)
        ctx.set_labels(inp["labels"])
        unc = ctx.predict_sets_uncertainty(sets)
        assert ctx.replay_info() == (3, 3)
        cal = ctx.predict_sets_calibration(sets)
        assert ctx.replay_info() == (3, 3)
    finally:
        ctx.close()
    mean_prob = unc["mean_prob"]
    assert mean_prob.shape == (uc.N_ROWS, uc.CASES[name]["n_out"]) and mean_prob.shape[1] % 4 == (0 if name == "tanh_h2_c4_s7" else 3)
    assert np.array_equal(cal["confidence"], mean_prob.max(axis=1))
    assert np.array_equal(cal["predicted_class"], mean_prob.argmax(axis=1))
