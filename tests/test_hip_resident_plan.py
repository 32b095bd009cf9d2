"""GPU: the HIP library and the host library plan the LDS-resident path by one rule (npbnn_amd/csrc/npbnn_resident_plan.h).  For ten
small networks, what a context reports about its launches (npbnn_get_info: waves per workgroup, candidates per pass, fast tails,
the layer-0 layout) is what libnpbnn_host.so's exports of the rule return for the same request - on the float32 layout npbnn_set_arch
builds and on the fp16-split one the first launch moves to."""
import numpy as np
import pytest

import npbnn_amd as bn
from npbnn_amd import _capi as capi
from test_host_resident_plan import OK, block_table, launch_of, layout_of, lib      # noqa: F401 (lib: a fixture)

pytestmark = pytest.mark.gpu

N_ROWS = 403
CAT, GAUSS, POISSON = capi.LIK_CATEGORICAL, capi.LIK_GAUSS, capi.LIK_POISSON

# widths of every matrix, features, likelihood, target columns, and what else the context is given
SHAPES = [
    dict(dims=[32, 8, 5], f=40, lik=CAT),
    dict(dims=[50, 5, 7], f=256, lik=CAT, max_cand=2),           # (tests/test_hip_compact_rows.py: the compact image lets two share a read of X)
    dict(dims=[16, 4, 2], f=24, lik=GAUSS, k=2),
    dict(dims=[45], f=40, lik=CAT),
    dict(dims=[61, 16, 4, 7], f=256, lik=CAT),
    dict(dims=[20, 6, 1], f=30, lik=POISSON, k=1),
    dict(dims=[32, 8, 5], f=64, lik=CAT, mask_blocks=4),
    dict(dims=[100, 20, 5], f=64, lik=CAT),
    dict(dims=[32, 8, 5], f=1024, lik=CAT, row_w=True),
    dict(dims=[32, 8, 5], f=40, lik=CAT, class_w=True),
]


def _id(s):
    return "_".join(str(d) for d in s["dims"]) + "_f%d" % s["f"] + "".join("_" + k for k in ("mask_blocks", "row_w", "class_w") if s.get(k)) + \
        {CAT: "", GAUSS: "_gauss", POISSON: "_poisson"}[s["lik"]]


@pytest.fixture(autouse=True)
def _library_rule(monkeypatch):
    for name in ("NPBNN_NO_PAD_MASK", "NPBNN_NO_L1_F16", "NPBNN_NO_TILE_PERM", "NPBNN_NO_COMPACT_ROWS", "NPBNN_WAVES", "NPBNN_L0", "NPBNN_FORCE_WIDE",
                 "NPBNN_WIDE_MIN_WAVES"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_the_context_reports_what_the_host_rule_plans(shape, lib):
    rs = np.random.default_rng(len(shape["dims"]) * 1000 + shape["f"])
    dims, f, lik, k = shape["dims"], shape["f"], shape["lik"], shape.get("k", 0)
    x = rs.standard_normal((N_ROWS, f))
    w, cur = [], f
    for o in dims:
        w.append(rs.normal(0, 0.5 / np.sqrt(cur + 1), (o, cur + 1)))
        cur = o
    blocks = None
    ctx = bn.HipContext(0)
    ctx.set_data(x)
    if lik == CAT:
        ctx.set_labels(rs.integers(0, dims[-1], N_ROWS))
    else:
        ctx.set_targets(rs.poisson(2.0, (N_ROWS, k)).astype(float) if lik == POISSON else rs.standard_normal((N_ROWS, k)))
    if shape.get("row_w") or shape.get("class_w"):
        ctx.set_row_weights(rs.uniform(0.5, 1.5, N_ROWS) if shape.get("row_w") else None, rs.uniform(0.5, 1.5, dims[-1]) if shape.get("class_w") else None)
    ctx.set_arch_from_weights(w, f, capi.ACT_TANH, capi.OUT_SOFTMAX if lik == CAT else capi.OUT_IDENTITY, lik, k)
    if shape.get("mask_blocks"):
        nb = shape["mask_blocks"]
        m0 = np.zeros_like(w[0])
        m0[:, 0] = 1
        for o in range(dims[0]):
            b = o // (dims[0] // nb)
            m0[o, 1 + b * (f // nb):1 + (b + 1) * (f // nb)] = 1
        ctx.set_layer_mask([m0] + [np.ones_like(a) for a in w[1:]])
        w[0] = w[0] * m0
        blocks = block_table(dims[0], f, nb)
    assert not ctx.is_wide()
    n_cu = ctx.info(capi.INFO_N_CU)
    table = dict(has_labels=lik == CAT, has_targets=lik != CAT, has_row_w=bool(shape.get("row_w")), n_tiles=(N_ROWS + 15) // 16, n_cu=n_cu)

    def agree(f16):
        rc, y = layout_of(lib, ctx.arch, f16=f16, blocks=blocks, classw=int(bool(shape.get("class_w"))))
        assert rc == OK and y.l0_f16 == f16 == ctx.info(capi.INFO_L0_F16)
        _, one = launch_of(lib, y, want_cand=1, lik_only=0, **table)        # (the waves a single candidate leaves room for)
        _, most = launch_of(lib, y, want_cand=3, lik_only=1, **table)       # (a chain pass that asks for as many as fit)
        got = (ctx.info(capi.INFO_WAVES_PER_BLOCK), ctx.info(capi.INFO_MAX_CANDIDATES), ctx.info(capi.INFO_FAST_TAILS))
        assert got == (one.waves_full, most.n_cand, most.fast), (f16, got)
        return got

    agree(0)                                            # npbnn_set_arch lays the float32 image out first
    assert np.isfinite(ctx.eval(w)["loglik"])           # the first launch moves to the fp16-split layout
    got = agree(1)
    if "max_cand" in shape:
        assert got[1] == shape["max_cand"]
    ctx.close()
