"""CPU: the planted fp16-range batches of tests/range_cases.py, before a GPU sees them.

Every variant runs through the float64 stand-in (``OracleChainBackend.run_chain``): it must reproduce the accept pattern the
batch was built for, every log value must stay finite, and the margin between the accept statistic and ``log_u`` must hold at
every iteration.  The table of direct-entry runs must cover what the GPU module promises."""
import numpy as np
import pytest

import range_cases as rc


@pytest.mark.parametrize("name", list(rc.VARIANTS))
def test_standin_reproduces_the_planted_pattern(name):
    sc = rc.scenario(name)
    v, p = sc["variant"], sc["p"]
    assert 37 <= len(p["x"]) <= 1025 and p["x"].shape[1] == 40
    clean0, planted, clean1, clean2 = sc["batches"]
    for b in sc["batches"]:
        K = b["K"]
        assert K <= 40
        want = b["want"]
        assert np.array_equal(want["acc"].astype(bool), b["pattern"]), "the stand-in left the pattern"
        for key in ("llp", "lpp"):
            assert np.all(np.isfinite(want[key]))
        assert np.isfinite(want["ll"]) and np.isfinite(want["lp"]) and np.all(np.isfinite(b["log_u"]))
        # the walk and the stand-in are two computations of one chain
        assert np.array_equal(want["llp"], b["llp_walk"])
        assert np.array_equal(want["w"], rc.pack(b["after_walk"]["w"]))
        assert want["ll"] == b["after_walk"]["ll"] and want["lp"] == b["after_walk"]["lp"]
        # the margin: 100 float32 log-likelihood bars on either side (less the rounding of statistic -+ margin in float64)
        gap = np.abs(b["stat"] - b["log_u"])
        assert np.all(b["margin"] >= rc.MARGIN_FACTOR * rc.LL_BAR)
        assert np.all(gap >= b["margin"] - 2 * np.spacing(np.abs(b["stat"]) + b["margin"]))
        assert np.all((b["stat"] >= b["log_u"]) == b["pattern"])
        n = b["cnt"] - (np.arange(K) == b["t_star"] if b["t_star"] is not None else 0)
        assert n.min() >= 5 and n.max() <= 30
    # the plant: a feature column's weight (not the bias) whose scaled value leaves fp16
    t_star, plant = planted["t_star"], sc["plant"]
    row, col = divmod(plant, p["shapes"][0][1])
    assert plant < p["shapes"][0][0] * p["shapes"][0][1] and col >= 1
    assert np.max(np.abs(p["x"][:, col - 1])) >= 1.0
    if p["mask"] is not None:
        assert p["mask"][0][row, col] == 1
        assert all(np.all(w[m == 0] == 0) for w, m in zip(p["w"], p["mask"]))
    at = np.flatnonzero(planted["idx"][t_star, :planted["cnt"][t_star]] == plant)
    assert len(at) == 1 and planted["delta"][t_star, at[0]] == rc.PLANT
    assert abs(p["w"][0][row, col] + rc.PLANT) * np.max(np.abs(p["x"][:, col - 1])) > rc.F16_MAX
    assert t_star == {"first": 0, "mid": planted["K"] // 2, "last": planted["K"] - 1}[v["pos"]]
    assert bool(planted["pattern"][t_star]) == v["accept"]
    held = abs(planted["want"]["w"][plant]) > 1e5
    assert held == v["accept"]
    for b in (clean0, clean1, clean2):
        assert b["t_star"] is None and np.max(np.abs(b["delta"])) < 1.0
    # accepts on either side of t*
    before = int(clean0["pattern"].sum() + planted["pattern"][:t_star].sum())
    after = int(planted["pattern"][t_star + 1:].sum() + clean1["pattern"].sum())
    assert before >= 2 and after >= 1
    if v["pos"] == "mid":
        assert planted["pattern"][:t_star].sum() >= 2 and planted["pattern"][t_star + 1:].sum() >= 1
    share = np.mean(np.concatenate([b["pattern"] for b in sc["batches"]]))
    assert 0.05 <= share <= 0.35
    if v["slot"]:      # three candidates per pass: prepared in slot 1 or 2 of a pass whose slot 0 is accepted, and dropped
        decided, prepared = rc.pass_slots(planted["pattern"], 3)
        dropped = [c for c in prepared if t_star in c and decided[t_star][0] != c[0]]
        assert len(dropped) == 1
        assert dropped[0].index(t_star) == v["slot"] and planted["pattern"][dropped[0][0]]
        assert decided[t_star] == (t_star - v["slot"] + 1, v["slot"] - 1)      # (proposed again, from the state slot 0 left)


def test_pass_slots():
    decided, prepared = rc.pass_slots(np.array([0, 1, 0, 0, 0, 1, 1, 0], dtype=bool), 3)
    assert prepared == [[0, 1, 2], [2, 3, 4], [5, 6, 7], [6, 7], [7]]
    assert decided[1] == (0, 1) and decided[2] == (2, 0) and decided[6] == (6, 0) and decided[7] == (7, 0)


def test_variant_table_and_runs_cover_what_the_gpu_module_promises():
    vs = rc.VARIANTS
    assert {v["pos"] for v in vs.values()} == {"first", "mid", "last"}
    for pos in ("first", "mid", "last"):
        assert {v["accept"] for v in vs.values() if v["pos"] == pos} == {True, False}
    assert {v["slot"] for v in vs.values()} == {0, 1, 2}
    assert any(v["mask_blocks"] for v in vs.values()) and any(v["lik"] == "gauss" for v in vs.values())
    assert {v["widths"] for v in vs.values() if v["lik"] == "cat"} == {(16, 5), (32, 8)}
    assert {v["widths"] for v in vs.values() if v["lik"] == "gauss"} == {(16, 5)}
    runs = rc.direct_runs()
    assert {r[0] for r in runs} == set(vs)
    assert {r[1] for r in runs} == {1, 2, 3}
    assert sum(r[2] == 3 for r in runs) == 1
    # what counts is the schedule the library runs, not the one the run names: on the resident path every schedule at every t*
    resident = [r for r in runs if r[3] == "resident"]
    for s in rc.SCHEDULES:
        ran = [r for r in resident if rc.effective_schedule(*r) == s]
        assert {vs[r[0]]["pos"] for r in ran} == {"first", "mid", "last"}, s
        assert all(r[2] == s for r in ran), "a run that falls back to another schedule stands in for it"
    assert all(rc.effective_schedule(*r) == r[2] for r in runs), "a run names a schedule that does not run"
    assert rc.effective_schedule("mid_rejected", 2, 5, "resident") == 4 and rc.effective_schedule("masked_rejected", 3, 5, "resident") == 4
    assert rc.effective_schedule("mid_rejected", 3, 4, "streamed") == 1
    for path in ("resident", "streamed"):
        assert {vs[r[0]]["accept"] for r in runs if r[3] == path} == {True, False}, path
        assert {r[1] for r in runs if r[3] == path} == {1, 2, 3}
    assert {r[0] for r in runs if r[3] == "streamed"} == set(vs)
    for name, v in vs.items():
        if v["slot"]:
            assert any(r[0] == name and r[1] == 3 and r[3] == "resident" for r in runs)


def test_the_layer0_option_getter_is_in_the_header():
    import os
    import re
    from npbnn_amd import _capi as capi
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "npbnn_hip.h")
    with open(header) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    values = {name: int(value) for name, value in re.findall(r"\b(NPBNN_(?:INFO|L0)_\w+)\s*=\s*(\d+)", text)}
    assert values["NPBNN_INFO_L0_OPTION"] == capi.INFO_L0_OPTION
    assert (values["NPBNN_L0_AUTO"], values["NPBNN_L0_F32"], values["NPBNN_L0_F16"]) == (capi.L0_AUTO, capi.L0_F32, capi.L0_F16)


@pytest.mark.parametrize("name", list(rc.GENERAL))
def test_general_chain_standin_reproduces_the_planted_pattern(name):
    sc = rc.general_scenario(name)
    v, p = sc["variant"], sc["p"]
    clean0, planted, clean1 = sc["batches"]
    for b in sc["batches"]:
        want = b["want"]
        assert np.array_equal(want["acc"].astype(bool), b["pattern"]), "the stand-in left the pattern"
        assert np.all(np.isfinite(want["llp"])) and np.all(np.isfinite(want["lpp"])) and np.all(np.isfinite(b["log_u"]))
        gap = np.abs(b["stat"] - b["log_u"])
        assert np.all(gap >= b["margin"] - 2 * np.spacing(np.abs(b["stat"]) + b["margin"]))
        assert np.all(b["margin"] >= rc.MARGIN_FACTOR * rc.LL_BAR)
    t_star, plant = planted["t_star"], sc["plant"]
    row, col = divmod(plant, p["shapes"][0][1])
    assert plant < p["shapes"][0][0] * p["shapes"][0][1] and col >= 1 and np.max(np.abs(p["x"][:, col - 1])) >= 1.0
    g = planted["draws"]
    at = np.flatnonzero(g["idx"][t_star, :g["cnt"][t_star]] == plant)
    assert len(at) == 1 and g["val"][t_star, at[0]] == rc.PLANT
    assert bool(planted["pattern"][t_star]) == v["accept"] == (abs(planted["want"]["w"][plant]) > 1e5)
    assert planted["pattern"][:t_star].sum() >= 2 and planted["pattern"][t_star + 1:].sum() >= 1
    if v["indicators"]:
        assert len(p["shapes"]) == 4
        assert planted["start"]["ind"][plant] == 1 and planted["want"]["ind"][plant] == 1, "the planted weight is switched off"
        assert g["ind_ptr"][t_star] == g["ind_ptr"][t_star + 1]
        flips = sum(len(b["draws"]["ind_pos"]) for b in sc["batches"])
        assert flips > 0 and not np.array_equal(clean0["start"]["ind"], clean1["want"]["ind"]), "no indicator flip was ever accepted"
    else:
        assert g["kind"] == rc.PROP_FIXED_NORMAL and g["h_cnt"][t_star] == g["cnt"][t_star]


def test_served_draws_drive_the_samplers_and_the_exchange_driver():
    """range_cases.serve_draws on the float64 stand-in: chains that take planted draws where they would draw make the planned
    decisions interval by interval, and so does the exchange driver when the cold chain stops short inside interval 1 (the
    stand-in's ``starve``: what a chain stopped before an out-of-range proposal looks like to the driver)."""
    import npbnn_amd as bn
    import oracle_backend
    from npbnn_amd import exchange as ex
    from test_hip_chain_oracle import _exchange_chains, make_data, oracle_twin

    class NoSwaps:
        def get(self, first, n=1):
            return np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n)

        def release(self, upto):
            pass
    temps, n_seg, seg_len, t_star = [0.85, 1.0], 4, 20, 27
    K = n_seg * seg_len
    dat = make_data("cat", 300, rc.N_FEATURES, seed=12)
    plans = []

    def build():
        chains = oracle_twin("cat", lambda: _exchange_chains(bn, "cat", dat, temps), oracle_backend.OracleExchangeBackend)
        for i, (bnn, m) in enumerate(chains):
            if len(plans) < len(chains):
                p = rc.problem_of(bnn)
                plant = rc.plant_index(p, np.random.default_rng(5))
                plans.append(rc.build_batches(p, 80 + i, [(K, t_star if i == 1 else None, plant if i == 1 else None, False, 0, "mid")],
                                              temperature=temps[i])[0])
            rc.serve_draws(m, plans[i])
        return chains
    a = build()
    with np.errstate(over="ignore"):
        assert ex.advance_intervals(a, [0, 1], 2, n_seg, seg_len, NoSwaps(), 0, device=False) == n_seg
    c = build()

    class Once(dict):              # (the stand-in keys ``starve`` by the interval within a batch: the first batch only)
        def get(self, key, default=None):
            return self.pop(key, default)
    oracle_backend.OracleExchangeBackend.starve = Once({(1, 1): t_star - seg_len})
    try:
        on_device = []
        with np.errstate(over="ignore"):
            assert ex.advance_intervals(c, [0, 1], 2, n_seg, seg_len, NoSwaps(), 0, batch=n_seg,
                                        on_interval=lambda s, info: on_device.append(info["cold"] is not None)) == n_seg
    finally:
        oracle_backend.OracleExchangeBackend.starve = {}
        oracle_backend.OracleExchangeBackend.exchange_slack = 1.5
    assert on_device == [True, False, True, True]
    for chains in (a, c):
        for (bnn, m), plan in zip(chains, plans):
            assert m._current_iteration == K
            assert m._last_accepted_mem[-K:] == [int(x) for x in plan["want"]["acc"]]
            assert rc.pack(bnn._w_layers).tobytes() == plan["want"]["w"].tobytes()
            assert m._logLik == plan["want"]["ll"]


@pytest.mark.parametrize("threshold", rc.SAMPLER_THRESHOLDS)
def test_sampler_case_crosses_the_threshold_where_the_gpu_test_needs_it(threshold):
    """The sampler case on the stand-in, for every threshold the scaled column can have: a candidate carries the watched weight
    past it within the first 60 iterations - in the third dispatch (iterations 40 to 59), the first one the kept dispatch runs -
    and the chain moves."""
    import npbnn_amd as bn
    from test_hip_chain_oracle import oracle_twin
    dat = rc.sampler_data()
    assert np.max(np.abs(dat["data"][:, rc.SAMPLER_COLUMN])) > 2.0 ** 12
    seen = []
    with np.errstate(over="ignore"):
        bnn, m = oracle_twin("cat", lambda: rc.sampler_chain(bn, dat, threshold), rc.recording_backend(seen))
        assert bnn._w_layers[0][rc.SAMPLER_WEIGHT] == 0.98 * threshold
        flags = []
        for k in rc.SAMPLER_DISPATCHES[:8]:
            m.run_steps(bnn, k)
            flags += list(m._last_accepted_mem[-k:])
    crossed = [t for t, v in enumerate(seen) if abs(v) > threshold]
    assert crossed and crossed[0] < 60
    assert any(40 <= t < 60 for t in crossed)
    assert sum(flags[:150]) >= 2
    assert rc.SAMPLER_DISPATCHES[:3] == (20, 20, 20) and len(rc.SAMPLER_DISPATCHES) >= 3 + 16 + 1


def test_row_sharded_planted_batch_rehearsal():
    """rank_worker.py rowshard_range on the float64 stand-in over the TCP communicator: two ranks take the planted draws and
    hold the planned chain (what the GPU test runs on the device)."""
    import os
    import sys
    from npbnn_amd.launch import spawn_ranks
    import rowshard_cases
    worker = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "rank_worker.py")]
    world = rowshard_cases.RANGE_CASE["world"]
    status, out0, outs = spawn_ranks(worker + ["rowshard_range", "oracle", "socket"], world, capture_all=True, timeout=600)
    assert status == 0, "\n".join(outs)
    assert all("RANK %d OK" % r in outs[r] for r in range(world))


def test_a_candidate_out_of_range_only_while_it_is_dropped():
    """range_cases.dropped_only_batch: no proposal of the float64 chain leaves the range; the candidate a three-candidate pass
    prepares in slot 1 beside an accepted slot 0 does."""
    threshold = 1000.0
    p = rc.make_problem("cat", 300, (16, 5), 33)
    plant = rc.plant_index(p, np.random.default_rng(2))
    b = rc.dropped_only_batch(p, plant, threshold)
    assert np.array_equal(b["want"]["acc"].astype(bool), b["pattern"])
    assert np.all(np.abs(b["stat"] - b["log_u"]) >= b["margin"] - 2 * np.spacing(np.abs(b["stat"]) + b["margin"]))
    assert np.max(np.abs(b["watch_prop"])) < 0.6 * threshold, "the float64 chain itself proposes a weight out of range"
    t = rc.DROPPED_T
    decided, prepared = rc.pass_slots(b["pattern"], 3)
    assert [t, t + 1, t + 2] in prepared and b["pattern"][t] and decided[t + 1] == (t + 1, 0)
    assert abs(b["watch_cur"][t] + b["delta"][t + 1][b["idx"][t + 1] == plant][0]) > threshold      # as slot 1 of the pass t opens
    assert abs(b["watch_prop"][t + 1]) < 0.6 * threshold                                              # as slot 0 of the next pass
    decided1, prepared1 = rc.pass_slots(b["pattern"], 1)
    assert all(len(c) == 1 for c in prepared1)
