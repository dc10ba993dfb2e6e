"""CPU tests of the session-state hand-over's host side (include/pt.h "session states";
ptrace.rank_pixels, Scene.selftest_state_slots) -- no GPU needed: the order of an export's records,
and the import's classification of a record (the functions k_states_mark and k_states_write run,
compiled for the host).  Expected values are computed here from the tile deal's definition: tile
(tx, ty) of the window belongs to rank (tx + ty) % world, a rank's tiles ascend, a tile's pixels are
row-major.  tests/test_states.py runs the hand-over itself on the GPU.
"""
import ctypes as C

import numpy as np
import pytest

import _pixels as X
import _util as U

pt = U.ptrace()
FRAMES = {(40, 24): "dragon_glass_40x24x7", (64, 64): "dragon_glass_64x64x8"}
WINDOW = (5, 3, 30, 18)
GEOMETRIES = [(size, world, window) for size in FRAMES for world in (1, 2, 3) for window in (None, WINDOW)]


def expected_pixels(w, h, rank, world, x0=0, y0=0):
    """(global x, y, slot) of a rank's pixels in export order, pixel by pixel from the definition"""
    tiles_x, tiles_y = (w + 15) // 16, (h + 15) // 16
    out, local = [], 0
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            if (tx + ty) % world != rank:
                continue
            for j in range(16):
                for i in range(16):
                    if tx * 16 + i < w and ty * 16 + j < h:
                        out.append((x0 + tx * 16 + i, y0 + ty * 16 + j, local * 256 + j * 16 + i))
            local += 1
    return np.array(out, np.int64).reshape(-1, 3)


def geometry(size, window):
    x0, y0, w, h = window or (0, 0) + size
    return x0, y0, w, h


@pytest.fixture(scope="module")
def scenes():
    opened = {size: pt.Scene.load(X.golden(name)[1]) for size, name in FRAMES.items()}
    for size, s in opened.items():
        assert (s.info["width"], s.info["height"]) == size
    yield opened
    for s in opened.values():
        s.close()


@pytest.mark.parametrize("size,world,window", GEOMETRIES)
def test_rank_pixels_is_the_tiles_of_rank_tiles_pixel_by_pixel(size, world, window):
    x0, y0, w, h = geometry(size, window)
    tiles_x = (w + 15) // 16
    total = 0
    for rank in range(world):
        xy = pt.rank_pixels(w, h, rank, world, x0, y0)
        want = expected_pixels(w, h, rank, world, x0, y0)
        assert xy.dtype == np.uint32 and xy.shape == (len(want), 2)
        assert np.array_equal(xy, want[:, :2])
        # ... and tile by tile against rank_tiles
        tiles = ((xy[:, 1] - y0) // 16 * tiles_x + (xy[:, 0] - x0) // 16).tolist()
        assert sorted(set(tiles)) == pt.rank_tiles(w, h, rank, world) and tiles == sorted(tiles)
        total += len(xy)
    assert total == w * h
    if size == (40, 24) and world == 1 and window is None:
        # the partial right and bottom tiles: 8 x 16, 16 x 8 and 8 x 8 pixels
        counts = np.bincount((xy[:, 1] // 16 * 3 + xy[:, 0] // 16))
        assert counts.tolist() == [256, 256, 128, 128, 128, 64]


@pytest.mark.parametrize("size,world,window", GEOMETRIES)
def test_slots_of_a_ranks_own_pixels(scenes, size, world, window):
    s = scenes[size]
    x0, y0, w, h = geometry(size, window)
    padding = 0
    for rank in range(world):
        want = expected_pixels(w, h, rank, world, x0, y0)
        state = s.pixel_init(pt.rank_pixels(w, h, rank, world, x0, y0))
        slots = s.selftest_state_slots(state, rank=rank, world=world, window=window)
        assert np.array_equal(slots, want[:, 2])
        assert len(set(slots.tolist())) == len(slots) and (np.diff(slots) > 0).all()
        n_slots = s.wave_plan(256, rank=rank, world=world, window=window)["n_slots"]
        assert len(slots) == 0 or slots.max() < n_slots
        # (a rank may own whole tiles only; the padding lanes of the others' edge tiles are skipped)
        assert n_slots - len(slots) == 256 * len(pt.rank_tiles(w, h, rank, world)) - len(want)
        padding += n_slots - len(slots)
        # any order of the records, the same slots
        perm = np.random.default_rng(3).permutation(len(state))
        assert np.array_equal(s.selftest_state_slots(state[perm], rank=rank, world=world, window=window), slots[perm])
    assert padding == 256 * ((w + 15) // 16) * ((h + 15) // 16) - w * h and (padding > 0) == bool(w % 16 or h % 16)


@pytest.mark.parametrize("size,world,window", GEOMETRIES)
def test_every_pixel_of_the_frame_is_taken_by_exactly_one_rank(scenes, size, world, window):
    s = scenes[size]
    W, H = size
    x0, y0, w, h = geometry(size, window)
    state = s.pixel_init(X.window_xy((0, 0, W, H)))
    takers = np.zeros(W * H, np.int64)
    for rank in range(world):
        slots = s.selftest_state_slots(state, rank=rank, world=world, window=window)
        assert ((slots >= 0) | (slots == -1)).all()
        takers += slots >= 0
    inside = ((state["x"] >= x0) & (state["x"] < x0 + w) & (state["y"] >= y0) & (state["y"] < y0 + h))
    assert np.array_equal(takers, inside.astype(np.int64))


def test_foreign_outside_and_bad_rng_records(scenes):
    s = scenes[(40, 24)]
    W, H = 40, 24
    mine = s.pixel_init([[17, 3]])             # tile (1, 0): rank 1 of 2
    assert s.selftest_state_slots(mine, rank=1, world=2).tolist() == [256 * 0 + 3 * 16 + 1]
    assert s.selftest_state_slots(mine, rank=0, world=2).tolist() == [-1]
    assert s.selftest_state_slots(mine, window=(0, 0, 16, 16)).tolist() == [-1]    # outside the window
    assert s.selftest_state_slots(mine, window=(17, 3, 1, 1)).tolist() == [0]
    rec = np.repeat(mine, 7)
    rec["x"][:3] = (W, 0, 2 ** 32 - 1)
    rec["y"][:3] = (0, H, 2 ** 32 - 1)
    rec["rng"][3:] = (0, 2 ** 31 - 1, 2 ** 31, (1 << 31) | 5)
    #               x = W  y = H  huge  rng 0  2^31-1  flag alone (low bits 0)  flag + valid low bits
    assert s.selftest_state_slots(rec, rank=1, world=2).tolist() == [-2, -2, -2, -2, -2, -2, 49]
    rec["rng"][3:] = (1, 2 ** 31 - 2, (1 << 31) | 1, (1 << 31) | (2 ** 31 - 2))
    assert s.selftest_state_slots(rec[3:], rank=1, world=2).tolist() == [49, 49, 49, 49]
    # another rank's record is skipped whatever its rng word holds; one outside the image never is
    rec["rng"] = 0
    assert s.selftest_state_slots(rec, rank=0, world=2).tolist() == [-2, -2, -2, -1, -1, -1, -1]


def test_symbols_and_arguments(scenes):
    for name in ("pt_session_pixels", "pt_session_export", "pt_session_import", "pt_session_export_host",
                 "pt_session_import_host", "pt_selftest_state_slots"):
        assert name in pt.EXPORTED
    assert pt.abi_version() == 6
    s = scenes[(40, 24)]
    n = C.c_uint64(7)
    buf = np.zeros(32, np.uint8)
    assert pt._lib.pt_session_pixels(None, C.byref(n)) == pt.PT_E_INVALID and n.value == 7
    assert pt._lib.pt_session_export(None, U._p(buf), 1) == pt.PT_E_INVALID
    assert pt._lib.pt_session_import(None, 1, U._p(buf), None) == pt.PT_E_INVALID
    assert pt._lib.pt_session_export_host(None, U._p(buf), 1) == pt.PT_E_INVALID
    assert pt._lib.pt_session_import_host(None, 1, U._p(buf), None) == pt.PT_E_INVALID
    o = pt.SessionOpts(0, 0, 1, 0, 0, 0, 0, 0)
    out = np.zeros(1, np.int64)
    assert pt._lib.pt_selftest_state_slots(None, C.byref(o), 1, U._p(buf), U._p(out)) == pt.PT_E_INVALID
    assert pt._lib.pt_selftest_state_slots(s._h, None, 1, U._p(buf), U._p(out)) == pt.PT_E_INVALID
    assert pt._lib.pt_selftest_state_slots(s._h, C.byref(o), 1, None, U._p(out)) == pt.PT_E_INVALID
    assert pt._lib.pt_selftest_state_slots(s._h, C.byref(o), 1, U._p(buf), None) == pt.PT_E_INVALID
    assert pt._lib.pt_selftest_state_slots(s._h, C.byref(o), 0, None, None) == pt.PT_OK
    bad = pt.SessionOpts(0, 2, 2, 0, 0, 0, 0, 0)   # rank >= world
    assert pt._lib.pt_selftest_state_slots(s._h, C.byref(bad), 1, U._p(buf), U._p(out)) == pt.PT_E_INVALID
    assert pt.rank_pixels(16, 16, 1, 2).shape == (0, 2)   # a rank without a tile
