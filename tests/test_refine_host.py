"""CPU tests of a session's noise estimate and the adaptive step planned from it (include/pt.h "session
noise") -- no GPU needed: pt_selftest_refine_plan runs the functions of pt_noise.h that
k_noise_plan runs, compiled for the host, with the same in-tile neighbour rule.  Expected values come
from the numpy float32 restatement of tests/_refine.py alone, on the pixel-sample engine's host twin's
states at 4 samples (the mark) and at 8 (now), and on synthetic records; noise is compared on f32 bits.
tests/test_refine.py runs the calls themselves on the GPU.
"""
import ctypes as C

import numpy as np
import pytest

import _refine as R
import _util as U

pt = U.ptrace()
NEW = ("pt_session_mark", "pt_session_noise", "pt_session_noise_host", "pt_session_plan", "pt_session_plan_host",
       "pt_session_refine", "pt_selftest_refine_plan")
INVALID_OPTS = {"NaN threshold": (float("nan"), 4, 0, 0), "negative threshold": (-0.5, 4, 0, 0),
                "-inf threshold": (float("-inf"), 4, 0, 0), "step 0": (0.1, 0, 0, 0), "spread 2": (0.1, 4, 0, 2)}


@pytest.fixture(scope="module", params=sorted(R.INPUTS))
def data(request):
    """(scene, window, origin, {world: [(xy, mark, now) per rank]}) of one input"""
    s, window, origin = R.open_input(pt, request.param)
    ranks = {}
    for world in (1, 3):
        ranks[world] = []
        for rank in range(world):
            xy = pt.rank_pixels(R.W, R.H, rank, world, *origin)
            ranks[world].append((xy, R.twin(s, xy, 4), R.twin(s, xy, 8)))
    yield s, window, origin, ranks
    s.close()


def check(s, now, mark, opts, origin=(0, 0), what="", **geo):
    noise, counts, res = s.selftest_refine_plan(now, mark, *opts, **geo)
    wn, wc, wres, _ = R.plan_of(now, mark, *opts, origin=origin)
    assert np.array_equal(R.bits(noise), R.bits(wn)), what + ": noise bits"
    assert np.array_equal(counts, wc), what + ": counts"
    R.assert_result(res, wres, what)
    return noise, counts, res


def test_symbols():
    for name in NEW:
        assert name in pt.EXPORTED and hasattr(pt._lib, name)
    for name in ("mark", "noise", "plan", "refine"):
        assert hasattr(pt.Session, name)
    assert hasattr(pt.Scene, "selftest_refine_plan") and C.sizeof(pt.RefineOpts) == 16 and C.sizeof(pt.RefineResult) == 56
    assert pt.abi_version() == pt.ABI_VERSION == 6
    o, r = pt.RefineOpts(0.1, 4, 0, 0), pt.RefineResult()
    buf = np.zeros(4, np.uint32)
    assert pt._lib.pt_session_mark(None) == pt.PT_E_INVALID
    assert pt._lib.pt_session_noise(None, U._p(buf), 4) == pt.PT_E_INVALID
    assert pt._lib.pt_session_noise_host(None, U._p(buf), 4) == pt.PT_E_INVALID
    assert pt._lib.pt_session_plan(None, C.byref(o), U._p(buf), 4, C.byref(r)) == pt.PT_E_INVALID
    assert pt._lib.pt_session_plan_host(None, C.byref(o), U._p(buf), 4, C.byref(r)) == pt.PT_E_INVALID
    assert pt._lib.pt_session_refine(None, C.byref(o), C.byref(r)) == pt.PT_E_INVALID
    assert not buf.any()


def test_the_median_threshold_splits_the_frame(data):
    s, window, origin, ranks = data
    xy, mark, now = ranks[1][0]
    noise, est = R.noise_of(now, mark)
    assert est.all() and np.isfinite(noise).all()
    thr = R.rank_element(noise, 50)
    got, counts, res = check(s, now, mark, (thr, 4, 0, 0), origin, "median", window=window)
    hot = int((noise > np.float32(thr)).sum())
    print("hot %d cold %d zeros %d" % (hot, len(noise) - hot, int((noise == 0).sum())))
    assert 0 < hot < len(noise) and res["refined"] == hot and res["samples"] == 4 * hot
    assert res["unmarked"] == 0 and res["nonfinite"] == 0 and res["capped"] == 0 and (res["least"], res["most"]) == (8, 8)
    assert (counts[got == np.float32(thr)] == 0).all() and (got == np.float32(thr)).any()   # (strict: the element itself is cold)


def test_spread_stays_inside_a_tile(data):
    s, window, origin, ranks = data
    xy, mark, now = ranks[1][0]
    thr = R.rank_element(R.noise_of(now, mark)[0], 95)
    _, counts, res = check(s, now, mark, (thr, 4, 0, 1), origin, "spread", window=window)
    _, plain, _ = check(s, now, mark, (thr, 4, 0, 0), origin, "no spread", window=window)
    loose = R.plan_of(now, mark, thr, 4, 0, 1, origin=origin, tile_rule=False)[3]
    print("hot %d, spread in tiles %d, across tiles %d" % ((plain > 0).sum(), (counts > 0).sum(), loose.sum()))
    assert 0 < (plain > 0).sum() < (counts > 0).sum() < loose.sum(), "the input does not tell the tile rule from its absence"
    assert ((counts > 0) >= (plain > 0)).all() and res["refined"] == (counts > 0).sum()


def test_three_ranks_plan_what_one_rank_plans(data):
    s, window, origin, ranks = data
    xy1, mark1, now1 = ranks[1][0]
    thr = R.rank_element(R.noise_of(now1, mark1)[0], 95)
    whole = np.zeros((R.H, R.W), np.uint32)
    _, c1, r1 = check(s, now1, mark1, (thr, 4, 0, 1), origin, "world 1", window=window)
    whole[xy1[:, 1] - origin[1], xy1[:, 0] - origin[0]] = c1
    sizes, total = [], 0
    for rank, (xy, mark, now) in enumerate(ranks[3]):
        _, c, r = check(s, now, mark, (thr, 4, 0, 1), origin, "rank %d of 3" % rank, rank=rank, world=3, window=window)
        assert np.array_equal(c, whole[xy[:, 1] - origin[1], xy[:, 0] - origin[0]]), "the plan depends on the sharding"
        sizes.append(len(xy))
        total += r["refined"]
    assert total == r1["refined"] and sum(sizes) == R.W * R.H
    assert sizes == [256 + 64, 256 + 128, 128 + 128]   # every rank of 3 owns a partial tile, rank 2 nothing else


def synthetic(s, rows):
    """records of the first pixels of the frame: rows of (sum now, k, sum at the mark, a)"""
    xy = pt.rank_pixels(R.W, R.H, 0, 1)
    now, mark = s.pixel_init(xy), s.pixel_init(xy)
    now["samples"], mark["samples"] = 8, 4
    now["sum"], mark["sum"] = (2.0, 2.0, 2.0), (1.0, 1.0, 1.0)   # (noise 0: cold at any threshold)
    for i, (sn, k, sm, a) in enumerate(rows):
        at = 17 * i   # pixel (i, i) of tile 0: each beside the next
        now["sum"][at], now["samples"][at], mark["sum"][at], mark["samples"][at] = sn, k, sm, a
    return now, mark


def test_synthetic_records():
    s, _, _ = R.open_input(pt, "frame")
    inf, nan = float("inf"), float("nan")
    rows = [((3, 3, 3), 8, (1, 1, 1), 0),            # no mark
            ((3, 3, 3), 8, (1, 1, 1), 8),            # k == a
            ((3, 3, 3), 4, (1, 1, 1), 8),            # k < a
            ((nan, 3, 3), 8, (1, 1, 1), 4),          # a NaN sum
            ((inf, 3, 3), 8, (1, 1, 1), 4),          # +inf in a channel: inf / inf
            ((inf, -inf, 3), 8, (1, 1, 1), 4),       # +inf and -inf: a NaN brightness takes the floor
            ((0, 0, 0), 8, (0, 0, 0), 4),            # all-zero sums: the floor, noise 0
            ((0, 0, 0), 8, (1, 0, 0), 4),            # the floor under a movement
            ((8, 16, 24), 8, (0, 0, 0), 4)]          # an ordinary hot pixel: 6 / sqrt(6)
    now, mark = synthetic(s, rows)
    noise, est = R.noise_of(now, mark)
    at = [17 * i for i in range(len(rows))]
    assert not est[at[:3]].any() and (noise[at[:3]] == np.inf).all()
    assert np.isnan(noise[at[3]]) and np.isnan(noise[at[4]]) and noise[at[5]] == np.inf and est[at[5]]
    assert noise[at[6]] == 0 and noise[at[7]] == np.float32(0.25) / np.sqrt(R.FLOOR) == 8.0
    for spread in (0, 1):
        _, counts, res = check(s, now, mark, (1.0, 4, 0, spread), what="synthetic, spread %d" % spread)
        assert res["unmarked"] == 3 and res["nonfinite"] == 2 and res["worst"] == 8.0
        assert (counts[at[3:5]] == 0).all() and (counts[[at[0], at[1], at[2], at[5], at[7], at[8]]] == 4).all()
        assert res["refined"] == (6 if spread == 0 else (counts > 0).sum()) and counts[at[6]] == (4 if spread else 0)
    # a noise exactly at the threshold is not hot; one float below it is
    for thr, hot in ((8.0, False), (float(np.nextafter(np.float32(8), np.float32(0))), True)):
        _, counts, res = check(s, now, mark, (thr, 4, 0, 0), what="threshold %r" % thr)
        assert (counts[at[7]] == 4) == hot
    # the cap: k >= max_samples, max_samples - k < step, and max_samples = 0 with k = 2^32 - 2
    _, counts, res = check(s, now, mark, (1.0, 4, 8, 0), what="at the cap")
    assert res["capped"] == 5 and res["refined"] == 1 and counts[at[2]] == 4   # (the k = 4 record alone is below it)
    _, counts, res = check(s, now, mark, (1.0, 4, 10, 0), what="short of the cap")
    assert (counts[[at[0], at[1], at[5], at[7], at[8]]] == 2).all() and counts[at[2]] == 4 and res["capped"] == 0
    now["samples"][at[8]], mark["samples"][at[8]] = 0xfffffffe, 0xfffffff0
    now["samples"][at[0]] = 0xffffffff
    _, counts, res = check(s, now, mark, (0.0, 4, 0, 0), what="the last sample a count has room for")
    assert counts[at[8]] == 1 and counts[at[0]] == 0 and res["capped"] == 1 and res["most"] == 0xffffffff
    s.close()


def test_invalid_options_and_arguments_are_refused():
    s, _, _ = R.open_input(pt, "frame")
    xy = pt.rank_pixels(R.W, R.H, 0, 1)
    now = s.pixel_init(xy)
    for what, opts in INVALID_OPTS.items():
        with pytest.raises(pt.PTError) as e:
            s.selftest_refine_plan(now, now, *opts)
        assert e.value.code == pt.PT_E_INVALID, what
    with pytest.raises(pt.PTError) as e:
        s.selftest_refine_plan(now[:-1], now[:-1], 0.1, 4)
    assert e.value.code == pt.PT_E_INVALID
    so, o, r = pt.SessionOpts(0, 0, 1, 0, 0, 0, 0, 0), pt.RefineOpts(0.1, 4, 0, 0), pt.RefineResult()
    r.refined = 77
    args = (len(now), U._p(now), U._p(now))
    assert pt._lib.pt_selftest_refine_plan(s._h, C.byref(so), *args, None, None, None, C.byref(r)) == pt.PT_E_INVALID
    assert pt._lib.pt_selftest_refine_plan(s._h, C.byref(so), *args, C.byref(o), None, None, None) == pt.PT_E_INVALID
    assert pt._lib.pt_selftest_refine_plan(s._h, C.byref(so), len(now), None, U._p(now), C.byref(o), None, None,
                                           C.byref(r)) == pt.PT_E_INVALID
    assert r.refined == 77
    # never marked: every pixel without an estimate takes the step (the bootstrap); -0 and +inf are thresholds
    assert pt._lib.pt_selftest_refine_plan(s._h, C.byref(so), *args, C.byref(o), None, None, C.byref(r)) == pt.PT_OK
    assert r.refined == r.unmarked == len(now) and r.samples == 4 * len(now) and r.worst == 0
    for thr in (-0.0, float("inf")):
        _, counts, res = s.selftest_refine_plan(now, now, thr, 4)
        assert res["refined"] == (0 if thr else len(now))
    # a rank that owns no pixel
    _, counts, res = s.selftest_refine_plan(now[:0], now[:0], 0.1, 4, rank=1, world=2, window=(0, 0, 16, 16))
    assert len(counts) == 0 and not any(res.values())
    s.close()
