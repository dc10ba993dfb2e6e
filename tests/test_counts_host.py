"""CPU tests of a session's per-pixel sample counts (include/pt.h pt_session_trace_counts /
pt_session_import_ragged / pt_session_samples_range) -- no GPU needed: the symbols,
the refusals that need no device, and the two pieces of arithmetic the count kernels run, compiled for
the host: the record of an export that a slot's pixel is (Scene.selftest_count_records) and a call's
bias of the `done` fields with the lag table (pt_selftest_count_step).  Expected values are computed
here from the definitions: the tile deal of tests/test_states_host.py, and a pixel's count as a plain
integer.  tests/test_counts.py runs the calls themselves on the GPU.
"""
import ctypes as C

import numpy as np
import pytest

import _pixels as X
import _util as U
from test_states_host import FRAMES, GEOMETRIES, expected_pixels, geometry

pt = U.ptrace()
NEW = ("pt_session_trace_counts", "pt_session_trace_counts_host", "pt_session_import_ragged",
       "pt_session_import_ragged_host", "pt_session_samples_range", "pt_selftest_count_records", "pt_selftest_count_step")


@pytest.fixture(scope="module")
def scenes():
    opened = {size: pt.Scene.load(X.golden(name)[1]) for size, name in FRAMES.items()}
    yield opened
    for s in opened.values():
        s.close()


def step(S, lag, counts):
    """pt_selftest_count_step: (return code, S2, done, lag after)"""
    lag, counts = np.ascontiguousarray(lag, np.uint32), np.ascontiguousarray(counts, np.uint32)
    done, after = np.full(len(lag), 0xA5A5A5A5, np.uint32), np.full(len(lag), 0xA5A5A5A5, np.uint32)
    S2 = C.c_uint32(0xA5A5A5A5)
    rc = pt._lib.pt_selftest_count_step(S, len(lag), U._p(lag), U._p(counts), U._p(done), U._p(after), C.byref(S2))
    return rc, S2.value, done, after


def test_symbols_and_null_arguments(scenes):
    for name in NEW:
        assert name in pt.EXPORTED and hasattr(pt._lib, name)
    for name in ("trace_counts", "import_states", "samples_range", "ragged"):
        assert hasattr(pt.Session, name)
    assert pt.abi_version() == pt.ABI_VERSION == 6
    buf = np.zeros(32, np.uint8)
    n = C.c_uint64(7)
    lo, hi = C.c_uint32(5), C.c_uint32(6)
    assert pt._lib.pt_session_trace_counts(None, 1, U._p(buf)) == pt.PT_E_INVALID
    assert pt._lib.pt_session_trace_counts(None, 0, None) == pt.PT_E_INVALID
    assert pt._lib.pt_session_trace_counts_host(None, 1, U._p(buf)) == pt.PT_E_INVALID
    assert pt._lib.pt_session_import_ragged(None, 1, U._p(buf), C.byref(n)) == pt.PT_E_INVALID and n.value == 7
    assert pt._lib.pt_session_import_ragged_host(None, 1, U._p(buf), None) == pt.PT_E_INVALID
    assert pt._lib.pt_session_samples_range(None, C.byref(lo), C.byref(hi)) == pt.PT_E_INVALID
    assert (lo.value, hi.value) == (5, 6)
    s = scenes[(40, 24)]
    o = pt.SessionOpts(0, 0, 1, 0, 0, 0, 0, 0)
    rec = np.zeros(6 * 256, np.int64)
    assert pt._lib.pt_selftest_count_records(None, C.byref(o), len(rec), U._p(rec), C.byref(n)) == pt.PT_E_INVALID
    assert pt._lib.pt_selftest_count_records(s._h, None, len(rec), U._p(rec), C.byref(n)) == pt.PT_E_INVALID
    assert pt._lib.pt_selftest_count_records(s._h, C.byref(o), len(rec), U._p(rec), None) == pt.PT_E_INVALID
    assert pt._lib.pt_selftest_count_records(s._h, C.byref(o), len(rec), None, C.byref(n)) == pt.PT_E_INVALID
    assert pt._lib.pt_selftest_count_records(s._h, C.byref(o), len(rec) - 1, U._p(rec), C.byref(n)) == pt.PT_E_INVALID
    assert n.value == 6 * 256 and not rec.any()
    bad = pt.SessionOpts(0, 2, 2, 0, 0, 0, 0, 0)   # rank >= world
    assert pt._lib.pt_selftest_count_records(s._h, C.byref(bad), len(rec), U._p(rec), C.byref(n)) == pt.PT_E_INVALID
    one = np.zeros(1, np.uint32)
    S2 = C.c_uint32()
    assert pt._lib.pt_selftest_count_step(0, 1, None, U._p(one), U._p(one), U._p(one), C.byref(S2)) == pt.PT_E_INVALID
    assert pt._lib.pt_selftest_count_step(0, 1, U._p(one), U._p(one), U._p(one), U._p(one), None) == pt.PT_E_INVALID
    assert pt._lib.pt_selftest_count_step(9, 0, None, None, None, None, C.byref(S2)) == pt.PT_OK and S2.value == 0


@pytest.mark.parametrize("size,world,window", GEOMETRIES)
def test_a_slots_record_is_its_pixels_place_in_rank_pixels(scenes, size, world, window):
    s = scenes[size]
    x0, y0, w, h = geometry(size, window)
    total = 0
    for rank in range(world):
        want = expected_pixels(w, h, rank, world, x0, y0)   # (x, y, slot) in export order, from the tile deal
        xy = pt.rank_pixels(w, h, rank, world, x0, y0)
        assert np.array_equal(xy, want[:, :2])
        rec = s.selftest_count_records(rank=rank, world=world, window=window)
        assert len(rec) == 256 * len(pt.rank_tiles(w, h, rank, world))
        assert len(rec) == s.wave_plan(256, rank=rank, world=world, window=window)["n_slots"]
        assert np.array_equal(rec[want[:, 2]], np.arange(len(want)))
        padding = np.ones(len(rec), bool)
        padding[want[:, 2]] = False
        assert (rec[padding] == -1).all() and (rec >= 0).sum() == len(want)
        # ... and the import's own slot of every record of rank_pixels leads back to the record
        slots = s.selftest_state_slots(s.pixel_init(xy), rank=rank, world=world, window=window)
        assert np.array_equal(rec[slots], np.arange(len(xy)))
        total += len(want)
    assert total == w * h
    if size == (40, 24) and world == 1 and window is None:
        # the partial right and bottom tiles: 8 x 16, 16 x 8 and 8 x 8 pixels
        assert [(rec[256 * t:256 * (t + 1)] >= 0).sum() for t in range(6)] == [256, 256, 128, 128, 128, 64]
        assert rec[256 * 2 + 16] == 512 + 8 and rec[256 * 2 + 8] == -1   # tile 2's rows are 8 pixels wide


def test_a_step_biases_done_so_that_one_target_means_every_pixels_own_count():
    rng = np.random.default_rng(5)
    n = 1000
    S, lag = 0, np.zeros(n, np.uint32)
    taken = np.zeros(n, np.int64)   # every pixel's count, as plain integers
    for k in range(6):
        counts = rng.integers(0, 9, n).astype(np.uint32)
        if k == 2:
            counts[:] = 0            # a call that adds nothing
        if k == 3:
            counts[:] = 5            # a uniform call
        if k == 4:
            counts[:] = 0
            counts[17] = 200         # one long chain
        rc, S2, done, after = step(S, lag, counts)
        assert rc == pt.PT_OK
        taken += counts
        assert S2 == taken.max() and after.min() == 0
        assert np.array_equal(S2 - done.astype(np.int64), counts), "the pass runs a pixel from done to S2"
        assert np.array_equal(S2 - after.astype(np.int64), taken), "a pixel's count is S2 - lag"
        if k == 2:
            assert S2 == S and (done == S).all() and np.array_equal(after, lag)
        if k == 3:
            assert S2 == S + 5 and np.array_equal(after, lag)
        S, lag = S2, after
    # a then b ends where a + b ends
    a, b = rng.integers(0, 5, n).astype(np.uint32), rng.integers(0, 5, n).astype(np.uint32)
    _, Sa, _, la = step(S, lag, a)
    _, Sab, _, lab = step(Sa, la, b)
    _, Sc, _, lc = step(S, lag, a + b)
    assert Sab == Sc and np.array_equal(lab, lc)


def test_a_step_refuses_a_count_past_2_to_the_32_minus_1():
    top = 0xfffffff0
    lag = np.array([0, 40, top], np.uint32)
    for counts, ok in (([15, 55, 0], True), ([0, 0, 0xffffffff], True), ([16, 0, 0], False), ([0, 56, 0], False),
                       ([32, 32, 32], False), ([0, 0, 0xffffffff], True)):
        rc, S2, done, after = step(top, lag, counts)
        if ok:
            assert rc == pt.PT_OK and S2 == 0xffffffff
            assert ((S2 - after.astype(np.int64)) == (top - lag.astype(np.int64)) + np.array(counts)).all()
        else:
            assert rc == pt.PT_E_INVALID and S2 == 0xA5A5A5A5
            assert (done == 0xA5A5A5A5).all() and (after == 0xA5A5A5A5).all()
    assert step(3, [4], [0])[0] == pt.PT_E_INVALID   # (no session holds a lag above its virtual count)
