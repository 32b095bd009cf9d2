"""CPU checks of the rule that sizes the weight-streamed path's K-slice buffer (npbnn_amd/csrc/npbnn_wide_plan.h, exported by
libnpbnn_host.so as npbnn_host_wide_slice_room; the HIP library sizes the buffer by the same header and refuses a launch that would
write past it).

A smaller table is cut into MORE K-slices than a larger one - fewer row blocks fill the chip - so a buffer sized for the training
set does not hold a pass over a smaller test set.  These are the two table rows that pass wrote past the buffer with before the
buffer had a capacity of its own: [50, 5] on 1024 features, 11 200 / 6 400 rows; [256, 64] on 2048 features, 20 000 / 8 000 rows."""
import ctypes as C
import os

import pytest

from npbnn_amd import predraw

N_CU = 256


@pytest.fixture(scope="module")
def room():
    if not os.path.exists(predraw.HOST_LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(predraw.HOST_LIB_PATH)
    f = lib.npbnn_host_wide_slice_room
    f.restype = C.c_longlong
    f.argtypes = [C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int64, C.c_int]

    def call(out_dims, in_dim, n_rows, n_cu=N_CU):
        dims = (C.c_int32 * len(out_dims))(*out_dims)
        return f(len(out_dims), dims, in_dim, n_rows, n_cu)
    return call


@pytest.fixture(autouse=True)
def _library_rule(monkeypatch):
    monkeypatch.delenv("NPBNN_WIDE_SLICES", raising=False)
    monkeypatch.delenv("NPBNN_WIDE_CFG", raising=False)


def tiles(n_rows):
    return (n_rows + 15) // 16


@pytest.mark.parametrize("net, f, train, test, sl_train, sl_test", [
    ([50, 5], 1024, 11200, 6400, 2, 4),
    ([256, 64], 2048, 20000, 8000, 3, 8),
])
def test_the_smaller_table_needs_more_room(room, net, f, train, test, sl_train, sl_test):
    """The rows of the table: the first layer's slices x [rows][16 x its output tiles], and the test pass needs more than the train pass."""
    ld = 16 * ((net[0] + 15) // 16)
    assert room(net, f, train) == sl_train * tiles(train) * 16 * ld
    assert room(net, f, test) == sl_test * tiles(test) * 16 * ld
    assert room(net, f, test) > room(net, f, train)


def test_one_slice_needs_no_room(room):
    """Tables that fill the chip with row blocks alone (and contractions too short to cut) need no slice buffer."""
    assert room([50, 5], 1024, 100000) == 0
    assert room([50, 5], 1024, 40005) == 0
    assert room([50, 5], 100, 11200) == 0          # (4 K-units: no slice keeps 8)
    assert room([8], 16, 16) == 0


@pytest.mark.parametrize("forced", range(1, 9))
def test_forced_slice_counts(room, monkeypatch, forced):
    """NPBNN_WIDE_SLICES forces the count on every layer, within 1..min(8, K-units): the room is exactly the largest layer's
    slices x [rows][16 x output tiles], whatever the row count."""
    monkeypatch.setenv("NPBNN_WIDE_SLICES", str(forced))
    for n in (1, 16, 17, 255, 257, 4099, 11200, 32513, 100000):
        for net, f in (([50, 5], 1024), ([50, 5], 100), ([300, 33], 100), ([256, 64], 2048)):
            want, in_dim = 0, f
            for out in net:
                sl = min(forced, 8, (in_dim + 31) // 32)
                if sl > 1:
                    want = max(want, sl * tiles(n) * 16 * 16 * ((out + 15) // 16))
                in_dim = out
            assert room(net, f, n) == want, (forced, n, net, f)


def test_room_is_whole_slices_of_the_table_asked_about(room):
    """Every row count from 1 to 120 000 (steps of 1-16 rows, and both sides of every tiling and slice switch): the room is 0 or
    2..8 whole slices of this table's activations, never more than 8, and no layer of the table needs more than it reports."""
    nets = (([50, 5], 1024), ([256, 64], 2048), ([64, 8], 1500), ([300, 33], 100), ([4096, 7], 64))
    rows = sorted(set(list(range(1, 600)) + list(range(600, 40000, 7)) + list(range(40000, 120001, 997)) + [32512, 32513, 32767, 32768]))
    for net, f in nets:
        widest = 16 * 16 * max((o + 15) // 16 for o in net)
        for n in rows:
            r = room(net, f, n)
            assert r >= 0 and r <= 8 * tiles(n) * widest, (net, f, n, r)
            # (the room is n_sl x [rows][16 mt] of one layer)
            ok = r == 0 or any(r % (tiles(n) * 256 * ((o + 15) // 16)) == 0 and 2 <= r // (tiles(n) * 256 * ((o + 15) // 16)) <= 8 for o in net)
            assert ok, (net, f, n, r)


def test_row_sweep_slice_counts(room):
    """The slice counts tests/test_hip_wide_tables.py's row sweep runs [50, 5] on 1024 features through (first layer: 4 output tiles,
    32 K-units - at most 4 slices, the 128-row blocks below 32 513 rows)."""
    per_slice = lambda n: tiles(n) * 16 * 64
    want = {16: 4, 17: 4, 255: 4, 257: 4, 4099: 4, 8000: 4, 10000: 3, 11200: 2, 32512: 1, 32513: 2, 32767: 2, 32768: 2, 40005: 1, 100000: 1}
    for n, sl in want.items():
        assert room([50, 5], 1024, n) == (sl * per_slice(n) if sl > 1 else 0), n


def test_other_chip_sizes_scale(room):
    """The rule follows the compute units it is given: half the units, half the rows for the same plan."""
    for n in (6400, 11200, 20000):
        assert room([50, 5], 1024, n, 256) // tiles(n) == room([50, 5], 1024, (n // 2 // 16) * 16, 128) // tiles((n // 2 // 16) * 16)


def test_bad_arguments(room):
    assert room([50, 5], 0, 100) == -1
    assert room([50, 5], 1024, 0) == -1
    assert room([50, 5], 1024, 100, 0) == -1
