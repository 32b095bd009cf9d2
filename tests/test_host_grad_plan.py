"""CPU checks of npbnn_loglik_grad's work plan (npbnn_attrib_grad_of in npbnn_amd/csrc/npbnn_attrib_plan.h, exported by
libnpbnn_host.so as npbnn_host_attrib_grad): the cut of a table into chunks of rows under the scratch budget and the element count
of every buffer.  The test replays the entry's loop from the plan's numbers and asserts what the kernels rely on: every row is
covered exactly once, every index a launch forms lies inside the buffer the plan sized for it, and the bytes stay within the budget
down to the floor of one slot.  The literal figures are the ones tests/grad_cases.py runs under on the GPU."""
import ctypes as C

import pytest

import grad_cases as gc
from test_host_attrib_plan import SALIENCY, Route, case_dims, cdiv, lib, route_of  # noqa: F401  (lib: the fixture)

SLOT, LIK_TERMS = 256, 33
DEFAULT = 128 << 20
_I8 = C.c_int * 8


class Grad(C.Structure):
    """npbnn_attrib_grad"""
    _fields_ = ([(n, C.c_int) for n in ("rows_cap", "n_slot_cap", "n_chunks", "n_tot", "bsum_off", "lik_off")] + [("a_off", _I8)] +
                [(n, C.c_longlong) for n in ("row_bytes", "n_act", "n_fac", "n_dl", "n_D0", "n_part", "n_acc")])


def grad_of(lib, r, rows, scratch=DEFAULT):
    lib.npbnn_host_attrib_grad.argtypes = [C.POINTER(Route), C.POINTER(C.c_int64), C.POINTER(Grad)]
    p = Grad()
    assert lib.npbnn_host_attrib_grad(C.byref(r), (C.c_int64 * 3)(r.q.wn, rows, scratch), C.byref(p)) == 0
    return p


def plan_of(lib, case, scratch=None):
    flags = gc.pdp_cases._bias_flags(case["bias"], len(case["nodes"]) + 1)
    r = route_of(lib, case_dims(case), case["features"], SALIENCY, bias=flags, off=1)
    rows = case["test_rows"] if case["which"] == 1 else case["rows"]
    budget = dict(case["env"]).get("NPBNN_GRAD_SCRATCH_BYTES", DEFAULT) if scratch is None else scratch
    return r, rows, int(budget), grad_of(lib, r, rows, int(budget))


@pytest.mark.parametrize("name", list(gc.CASES))
def test_every_case_is_covered_inside_its_buffers(lib, name):
    case = gc.CASES[name]
    r, rows, budget, p = plan_of(lib, case)
    dims = case_dims(case)
    assert r.route == 2 and r.NS == 1 and r.H0P == cdiv(dims[0], 32) * 32 and r.sum_w == sum(dims)
    assert p.rows_cap % SLOT == 0 and p.rows_cap >= SLOT and p.n_slot_cap * SLOT == p.rows_cap
    assert p.n_chunks == cdiv(rows, p.rows_cap) and (p.n_chunks - 1) * p.rows_cap < rows <= p.n_chunks * p.rows_cap
    assert (p.bsum_off, p.lik_off, p.n_tot) == (r.q.wn, r.q.wn + r.H0P, r.q.wn + r.H0P + LIK_TERMS) and p.n_acc == p.n_tot
    assert list(p.a_off[:len(dims)]) == [sum(dims[:l]) for l in range(len(dims))]
    # the largest index of every buffer over a full chunk: unit-major scratches, row-major D0, a slot's partials
    assert (p.a_off[len(dims) - 1] + dims[-1] - 1) * p.rows_cap + p.rows_cap - 1 < p.n_act == p.n_fac == p.n_dl
    assert (p.rows_cap - 1) * r.H0P + r.H0P - 1 < p.n_D0
    assert (p.n_slot_cap - 1) * p.n_tot + p.n_tot - 1 < p.n_part
    bytes_used = 4 * (p.n_act + p.n_fac + p.n_dl + p.n_D0) + 8 * p.n_part
    assert bytes_used <= max(budget, SLOT * p.row_bytes)
    assert p.row_bytes == 4 * (3 * r.sum_w + r.H0P) + cdiv(8 * p.n_tot, SLOT)


def test_the_budgets_of_the_case_table(lib):
    _, _, _, p = plan_of(lib, gc.CASES["scratch_in_chunks"])
    assert (p.rows_cap, p.n_chunks, p.n_tot, p.row_bytes) == (512, 5, 981 + 32 + 33, 533)
    _, _, _, p = plan_of(lib, gc.CASES["rows_2111"])
    assert (p.rows_cap, p.n_chunks) == (2304, 1)                      # (the default budget holds the table: 2111 rounded up to slots)
    _, _, _, p = plan_of(lib, gc.CASES["rows_1"])
    assert (p.rows_cap, p.n_chunks, p.n_slot_cap) == (256, 1, 1)


def test_a_budget_below_one_slot_still_gives_one_slot(lib):
    _, rows, _, p = plan_of(lib, gc.CASES["rows_2111"], scratch=1)
    assert p.rows_cap == SLOT and p.n_chunks == cdiv(rows, SLOT)


def test_a_large_table_is_cut_at_2_24_rows(lib):
    r = route_of(lib, [4, 2], 8, SALIENCY, off=1)
    p = grad_of(lib, r, 1 << 30, scratch=1 << 50)
    assert p.rows_cap == 1 << 24 and p.n_chunks == 64
