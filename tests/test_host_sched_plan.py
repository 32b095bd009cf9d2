"""CPU checks of the rule that puts a device chain's batch on a schedule (npbnn_amd/csrc/npbnn_sched_plan.h, exported by
libnpbnn_host.so as npbnn_host_sched_*; the HIP library chooses, records and counts launches by the same header).

The expected schedules are literals worked out by hand from the rule.  Every input is at least 1 % away from a threshold of the
rule, so that nothing here depends on how a compiler rounds: with no cost measured the model compares (30 + extra) * 1.03 against
30 * (1 + a), extra = 4.5 + 0.0175 * M, a = 1 - (1 - p)^D; with costs it compares c_between * 1.03 (0.97 when the chain is on
that form) against c_overlapped."""
import ctypes as C
import os

import pytest

import range_cases
from npbnn_amd import predraw

SERIAL, OVERLAP, OVERLAP2, PERSIST, PERSIST_SERIAL = 1, 2, 3, 4, 5
REQ_FIELDS = ("asked", "D", "K", "M", "eval_wgs", "alone", "plain", "group", "boundaries_only", "sync_failed", "persist_option",
              "has_spec_build", "own_slopes", "prior_fits_spec", "no_spec_step")
# a chain alone on a 256-unit part, plain batches of 100 iterations of 33 weights, everything the speculative step needs
REQ_DEFAULT = dict(asked=0, D=1, K=100, M=33, eval_wgs=255, alone=1, plain=1, group=0, boundaries_only=0, sync_failed=0,
                   persist_option=1, has_spec_build=1, own_slopes=0, prior_fits_spec=1, no_spec_step=0)
# (persist, overlap, sync, spec) that go with a schedule
FLAGS = {SERIAL: (0, 0, 0, 0), OVERLAP: (0, 1, 0, 0), OVERLAP2: (0, 1, 1, 0), PERSIST: (1, 1, 1, 0), PERSIST_SERIAL: (1, 1, 1, 1)}


class Hist(C.Structure):
    """npbnn_sched_hist"""
    _fields_ = [("last_schedule", C.c_int), ("turn_batches", (C.c_int * 2) * 2), ("turn_us", C.c_double * 2), ("it_n", (C.c_int * 2) * 2),
                ("it_us", (C.c_double * 2) * 2), ("its_per_pass", C.c_double), ("accept_rate", C.c_double)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(predraw.HOST_LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(predraw.HOST_LIB_PATH)
    hp = C.POINTER(Hist)
    lib.npbnn_host_sched_hist_init.argtypes = [hp]
    lib.npbnn_host_sched_hist_init.restype = None
    lib.npbnn_host_sched_choose.argtypes = [C.POINTER(C.c_int32), hp, C.POINTER(C.c_int32)]
    lib.npbnn_host_sched_record_outcome.argtypes = [hp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.npbnn_host_sched_record_outcome.restype = None
    lib.npbnn_host_sched_record_timing.argtypes = [hp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]
    lib.npbnn_host_sched_record_timing.restype = None
    lib.npbnn_host_sched_passes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
    lib.npbnn_host_sched_passes_segment.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
    lib.npbnn_host_sched_passes_group.argtypes = [C.c_int, C.c_double]
    return lib


@pytest.fixture
def hist(lib):
    """hist(p=..., last=..., it_us=[[short, long] of the overlapped form, of the form with the decision between the passes],
    it_n=..., since=...): a fresh history with those members set."""
    def make(p=-1.0, last=0, it_us=None, it_n=None, since=None):
        h = Hist()
        lib.npbnn_host_sched_hist_init(C.byref(h))
        h.accept_rate, h.last_schedule = p, last
        for name, val in (("it_us", it_us), ("it_n", it_n), ("turn_batches", since)):
            if val is not None:
                for f in range(2):
                    for k in range(2):
                        getattr(h, name)[f][k] = val[f][k]
        return h
    return make


@pytest.fixture
def choose(lib, hist):
    """choose(h=None, **request fields) -> the schedule; the four booleans must be those of that schedule."""
    def call(h=None, **kw):
        assert set(kw) <= set(REQ_FIELDS), kw
        r = dict(REQ_DEFAULT, **kw)
        req = (C.c_int32 * len(REQ_FIELDS))(*[int(r[f]) for f in REQ_FIELDS])
        out = (C.c_int32 * 5)()
        h = hist() if h is None else h
        s = lib.npbnn_host_sched_choose(req, C.byref(h), out)
        assert out[0] == s and tuple(out[1:5]) == FLAGS[s], (r, list(out))
        return s
    return call


def counters(h):
    return [[h.turn_batches[f][k] for k in range(2)] for f in range(2)]


def test_a_fresh_history(hist):
    h = hist()
    assert (h.last_schedule, h.its_per_pass, h.accept_rate) == (0, 0.0, -1.0)
    assert counters(h) == [[0, 0], [0, 0]] and list(h.turn_us) == [0.0, 0.0]
    assert all(h.it_n[f][k] == 0 and h.it_us[f][k] == 0.0 for f in range(2) for k in range(2))


# ---- asked for by number ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("asked", [SERIAL, OVERLAP, OVERLAP2, PERSIST, PERSIST_SERIAL])
def test_a_schedule_asked_for_runs_on_a_gpu_the_chain_has_to_itself(choose, hist, asked):
    h = hist(p=0.9, it_us=[[10.0, 10.0], [90.0, 90.0]], since=[[100, 100], [100, 100]])     # (history has no say)
    assert choose(h, asked=asked) == asked
    assert counters(h) == [[100, 100], [100, 100]]


def test_the_flag_ordered_forms_need_the_gpu_and_a_plain_run(choose):
    assert choose(asked=OVERLAP2, alone=0) == OVERLAP
    assert choose(asked=OVERLAP2, plain=0) == OVERLAP2          # (one chain of an exchange run, alone on its GPU)
    assert choose(asked=PERSIST, alone=0) == OVERLAP
    assert choose(asked=PERSIST, plain=0) == OVERLAP
    assert choose(asked=PERSIST_SERIAL, alone=0) == OVERLAP
    assert choose(asked=PERSIST_SERIAL, plain=0) == OVERLAP


@pytest.mark.parametrize("why", [dict(has_spec_build=0), dict(own_slopes=1), dict(prior_fits_spec=0), dict(no_spec_step=1), dict(eval_wgs=257)])
def test_the_decision_between_the_passes_falls_back_to_the_persistent_overlapped_form(choose, why):
    """prior_fits_spec = 0 stands for a Laplace prior and for a normal one with per-weight scales alike: the caller folds them."""
    assert choose(asked=PERSIST_SERIAL, **why) == PERSIST
    assert choose(asked=PERSIST_SERIAL, alone=0, **why) == OVERLAP
    assert choose(asked=PERSIST_SERIAL, plain=0, **why) == OVERLAP
    assert choose(asked=PERSIST_SERIAL, group=1, alone=0, **why) == OVERLAP
    assert choose(asked=PERSIST_SERIAL, eval_wgs=256) == PERSIST_SERIAL


def test_after_a_timed_out_wait_the_context_stays_on_kernel_boundaries(choose):
    for asked in (OVERLAP2, PERSIST, PERSIST_SERIAL):
        assert choose(asked=asked, sync_failed=1) == OVERLAP
    assert choose(asked=SERIAL, sync_failed=1) == SERIAL


@pytest.mark.parametrize("asked", range(0, 7))
def test_kernel_boundaries_only_and_group_passes_take_no_request(choose, hist, asked):
    assert choose(hist(p=0.2), asked=asked, boundaries_only=1) == SERIAL
    assert choose(hist(p=0.2), asked=asked, group=1, alone=0) == OVERLAP
    assert choose(hist(p=0.2), asked=asked, group=1, alone=1) == OVERLAP


def test_the_direct_runs_of_the_range_tests(choose):
    """tests/range_cases.effective_schedule says the same of every run tests/test_hip_chain_f16_range.py sends: a chain alone on
    its GPU, plain batches, a normal prior with one scale per layer; the weight-streamed path runs on kernel boundaries only, and
    there is a build with the speculative step for one and three candidates of a dense first layer."""
    runs = range_cases.direct_runs()
    assert len(runs) > 20
    for name, d, schedule, path in runs:
        v = range_cases.VARIANTS[name]
        got = choose(asked=schedule, D=d, K=v["K"], boundaries_only=path == "streamed", has_spec_build=not (d == 2 or v["mask_blocks"]))
        assert got == range_cases.effective_schedule(name, d, schedule, path), (name, d, schedule, path)


# ---- NPBNN_SCHED_AUTO, nothing measured ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("asked", [0, 6])
def test_auto_with_no_acceptance_rate_yet(choose, asked):
    assert choose(asked=asked) == PERSIST
    for why in (dict(alone=0), dict(plain=0), dict(persist_option=0), dict(sync_failed=1)):
        assert choose(asked=asked, **why) == OVERLAP


@pytest.mark.parametrize("d, p, want", [(1, 0.15, PERSIST), (1, 0.25, PERSIST_SERIAL), (3, 0.05, PERSIST), (3, 0.10, PERSIST_SERIAL)])
def test_auto_by_the_model_alone(choose, hist, d, p, want):
    """M = 33: (30 + 5.0775) * 1.03 = 36.13 against 30 * (1 + a) - the forms meet at a = 0.204; a = p with one candidate, and
    0.143 / 0.271 at p = 0.05 / 0.10 with three."""
    h = hist(p=p)
    assert choose(h, D=d) == want
    assert counters(h) == [[0, 0], [0, 0]]
    for why in (dict(alone=0), dict(plain=0), dict(persist_option=0), dict(sync_failed=1)):
        assert choose(hist(p=p), D=d, **why) == OVERLAP
    for why in (dict(has_spec_build=0), dict(own_slopes=1), dict(prior_fits_spec=0), dict(M=641)):
        assert choose(hist(p=p), D=d, **why) == PERSIST
    if want == PERSIST_SERIAL:
        assert choose(hist(p=p), D=d, no_spec_step=1) == PERSIST       # (picked, then demoted like one asked for by number)


def test_auto_on_a_chain_that_accepts_in_most_passes(choose, hist):
    """a = 0.8: overlapping no longer pays.  Too wide for the decision between the passes: kernel boundaries; else that form."""
    assert choose(hist(p=0.8), M=641) == SERIAL
    assert choose(hist(p=0.8), M=33) == PERSIST_SERIAL
    assert choose(hist(p=0.42), D=3, M=641) == SERIAL               # (a = 0.805)
    assert choose(hist(p=0.8), M=33, alone=0) == SERIAL


# ---- NPBNN_SCHED_AUTO with history -----------------------------------------------------------------------------------------------

def test_a_forms_first_batch_is_followed_by_a_second(choose, hist):
    h = hist(p=0.2, last=PERSIST, it_us=[[50.0, 0.0], [20.0, 0.0]], it_n=[[1, 0], [2, 0]])
    assert choose(h) == PERSIST
    h = hist(p=0.2, last=PERSIST_SERIAL, it_us=[[20.0, 0.0], [50.0, 0.0]], it_n=[[2, 0], [1, 0]])
    assert choose(h) == PERSIST_SERIAL
    h = hist(p=0.2, last=PERSIST, it_us=[[50.0, 0.0], [20.0, 0.0]], it_n=[[2, 0], [2, 0]])
    assert choose(h) == PERSIST_SERIAL


@pytest.mark.parametrize("last, c_between, want", [(PERSIST, 39.5, PERSIST), (PERSIST, 38.0, PERSIST_SERIAL),
                                                   (PERSIST_SERIAL, 40.5, PERSIST_SERIAL), (PERSIST_SERIAL, 42.0, PERSIST)])
def test_three_per_cent_in_favour_of_the_form_the_chain_is_on(choose, hist, last, c_between, want):
    """Against 40 us on the overlapped form: the chain leaves it below 38.83, and comes back to it above 41.24."""
    h = hist(p=0.2, last=last, it_us=[[40.0, 0.0], [c_between, 0.0]], it_n=[[2, 0], [2, 0]])
    assert choose(h) == want


def test_a_form_never_run_is_probed_when_the_model_puts_it_within_reach(choose, hist):
    """Overlapped at 40 us, p = 0.05: the model prices the other form at 40 / 1.05 + extra - 43.17 (ratio 1.079) at M = 33, 50.09
    (1.252) at M = 428."""
    def run(since, m):
        h = hist(p=0.05, last=PERSIST, it_us=[[40.0, 0.0], [0.0, 0.0]], it_n=[[2, 0], [0, 0]], since=[[0, 7], [since, 9]])
        return choose(h, M=m), counters(h)
    assert run(3, 33) == (PERSIST, [[0, 7], [3, 9]])
    assert run(4, 33) == (PERSIST_SERIAL, [[0, 7], [0, 9]])
    assert run(4, 428) == (PERSIST, [[0, 7], [4, 9]])
    assert run(199, 428) == (PERSIST, [[0, 7], [199, 9]])
    assert run(200, 428) == (PERSIST_SERIAL, [[0, 7], [0, 9]])
    # the other way round - the decision between the passes at 40 us, p = 0.28: the overlapped form at (40 - 5.0775) * 1.28 = 44.70 (1.118)
    h = hist(p=0.28, last=PERSIST_SERIAL, it_us=[[0.0, 0.0], [40.0, 0.0]], it_n=[[0, 0], [2, 0]], since=[[4, 7], [0, 9]])
    assert choose(h) == PERSIST and counters(h) == [[0, 7], [0, 9]]
    h = hist(p=0.28, last=PERSIST_SERIAL, it_us=[[0.0, 0.0], [40.0, 0.0]], it_n=[[0, 0], [2, 0]], since=[[3, 7], [0, 9]])
    assert choose(h) == PERSIST_SERIAL and counters(h) == [[3, 7], [0, 9]]


def test_a_measured_form_is_run_again_while_within_a_factor_two(choose, hist):
    def run(since, c_between):
        h = hist(p=0.2, last=PERSIST, it_us=[[40.0, 0.0], [c_between, 0.0]], it_n=[[2, 0], [2, 0]], since=[[0, 7], [since, 9]])
        return choose(h), counters(h)
    assert run(47, 60.0) == (PERSIST, [[0, 7], [47, 9]])
    assert run(48, 60.0) == (PERSIST_SERIAL, [[0, 7], [0, 9]])
    assert run(48, 90.0) == (PERSIST, [[0, 7], [0, 9]])           # (out of reach: not run, counted from anew)
    assert run(47, 90.0) == (PERSIST, [[0, 7], [47, 9]])
    # the overlapped form, measured at 60 us, while the chain is on the other at 40
    h = hist(p=0.2, last=PERSIST_SERIAL, it_us=[[60.0, 0.0], [40.0, 0.0]], it_n=[[2, 0], [2, 0]], since=[[48, 7], [0, 9]])
    assert choose(h) == PERSIST and counters(h) == [[0, 7], [0, 9]]


def test_short_and_long_batches_are_decided_apart(choose, hist):
    def h():
        return hist(p=0.2, last=PERSIST, it_us=[[40.0, 30.0], [30.0, 40.0]], it_n=[[2, 2], [2, 2]], since=[[0, 0], [0, 48]])
    assert choose(h(), K=255) == PERSIST_SERIAL
    assert choose(h(), K=256) == PERSIST_SERIAL                    # (its 48th batch without the other form: within a factor two)
    a, b = h(), h()
    b.turn_batches[1][1] = 0
    assert choose(b, K=256) == PERSIST
    assert choose(a, K=255) == PERSIST_SERIAL and counters(a) == [[0, 0], [0, 48]]
    assert choose(a, K=256) == PERSIST_SERIAL and counters(a) == [[0, 0], [0, 0]]


# ---- what a batch leaves in the history ------------------------------------------------------------------------------------------

def test_timing_is_recorded_of_one_round_persistent_batches_only(lib, hist):
    for schedule, persist, rounds, turns in ((OVERLAP, 0, 1, 50), (PERSIST, 1, 2, 50), (PERSIST, 1, 1, 7)):
        h = hist()
        lib.npbnn_host_sched_record_timing(C.byref(h), schedule, persist, 100, rounds, turns, 2000.0)
        assert list(h.turn_us) == [0.0, 0.0] and h.it_n[0][0] == 0 and h.it_us[0][0] == 0.0 and counters(h) == [[0, 0], [0, 0]]
    h = hist()
    lib.npbnn_host_sched_record_timing(C.byref(h), PERSIST, 1, 100, 1, 8, 2000.0)
    assert h.turn_us[0] == 250.0 and h.it_us[0][0] == 20.0 and h.it_n[0][0] == 1


def test_what_an_iteration_cost(lib, hist):
    h = hist(since=[[5, 6], [7, 8]])
    rec = lambda us, schedule=PERSIST, k=100: lib.npbnn_host_sched_record_timing(C.byref(h), schedule, 1, k, 1, 50, us)
    rec(2000.0)                                    # the first sample
    assert (h.turn_us[0], h.it_us[0][0], h.it_n[0][0]) == (40.0, 20.0, 1)
    assert counters(h) == [[0, 6], [8, 8]]
    rec(3000.0)                                    # the better of the first two (a turn: 60 counts as 1.25 x 40)
    assert (h.turn_us[0], h.it_us[0][0], h.it_n[0][0]) == (42.5, 20.0, 2)
    rec(2200.0)                                    # 0.75 / 0.25
    assert h.it_us[0][0] == pytest.approx(0.75 * 20.0 + 0.25 * 22.0, rel=1e-12) and h.it_n[0][0] == 3
    h.it_us[0][0] = 20.0
    rec(10000.0)                                   # a stalled call counts as 1.25 x the estimate
    assert h.it_us[0][0] == pytest.approx(0.75 * 20.0 + 0.25 * 25.0, rel=1e-12)
    assert counters(h) == [[0, 6], [11, 8]]
    rec(1500.0, PERSIST_SERIAL, 256)               # the other form, long batches: members of their own
    assert (h.turn_us[1], h.it_us[1][1], h.it_n[1][1]) == (30.0, 1500.0 / 256, 1)
    assert counters(h) == [[0, 7], [11, 0]]
    rec(1000.0, PERSIST_SERIAL, 256)               # the better of the first two, downwards
    assert h.it_us[1][1] == 1000.0 / 256 and h.it_n[1][1] == 2
    for start, want in ((999, 1000), (1000, 1000)):
        h.it_n[0][0] = start
        rec(2000.0)
        assert h.it_n[0][0] == want


def test_what_a_batch_decided(lib, hist):
    h = hist()
    out = lambda schedule, k, turns, acc: lib.npbnn_host_sched_record_outcome(C.byref(h), schedule, k, turns, acc)
    out(PERSIST, 100, 80, 25)
    assert (h.last_schedule, h.its_per_pass, h.accept_rate) == (PERSIST, 1.25, 0.25)
    out(SERIAL, 0, 3, 0)                           # (an exchange run that handed nothing back)
    assert (h.last_schedule, h.its_per_pass, h.accept_rate) == (SERIAL, 1.25, 0.25)
    out(OVERLAP, 50, 0, 10)
    assert (h.last_schedule, h.its_per_pass, h.accept_rate) == (OVERLAP, 1.25, 0.2)


# ---- launches per round ----------------------------------------------------------------------------------------------------------

def test_passes_of_a_round(lib):
    f = lib.npbnn_host_sched_passes             # (rem, D, persist, overlap, its_per_pass, slack)
    assert f(100, 3, 1, 1, 2.0, 1.0) == 204 and f(100, 3, 1, 1, 0.0, 1.0) == 204 and f(1, 1, 1, 1, 0.0, 1.0) == 6
    assert f(100, 3, 0, 0, 0.0, 1.0) == 34 and f(100, 3, 0, 1, 0.0, 1.0) == 35 and f(100, 1, 0, 0, 0.0, 1.0) == 100
    assert f(100, 3, 0, 0, 0.9, 1.0) == 34                     # (fewer than one iteration per pass: no history)
    assert f(100, 3, 0, 0, 2.0, 1.0) == 50 + 3 + 50 // 8 and f(100, 3, 0, 1, 2.0, 1.0) == 60
    assert f(100, 3, 0, 0, 2.9, 1.0) == 35 + 3 + 35 // 8       # (ceil(34.48))
    assert f(100, 3, 0, 0, 2.0, 1.25) == 63 + 3 + 63 // 8      # (ceil(62.5))


def test_passes_of_a_segment(lib):
    f = lib.npbnn_host_sched_passes_segment     # (seg_len, D, overlap, its_per_pass, slack)
    assert f(50, 3, 1, 0.0, 1.25) == 125 + 2 + 1 and f(50, 3, 0, 0.0, 1.25) == 63 + 2
    assert f(50, 3, 1, 2.0, 1.25) == 32 + 2 + 1                 # (ceil(31.25))
    assert f(50, 3, 0, 5.0, 1.25) == 22 + 2                     # (never fewer than ceil(50 / 3) = 17 before the slack: ceil(21.25))
    assert f(50, 3, 0, 2.0, 0.5) == 13 + 2                      # (a slack below one starves the segment: ceil(12.5))


def test_launches_of_a_group_pass(lib):
    f = lib.npbnn_host_sched_passes_group
    assert f(100, 0.3) == 137 + 3 and f(90, 0.0) == 95 + 3 and f(1, 1.0) == 3 + 3      # (136.5, 94.5, 2.1)
