"""GPU tests of a session's own noise estimate and its adaptive step (include/pt.h "session noise":
pt_session_mark / noise / plan / refine and the host forms; ptrace.Session.mark / noise / plan / refine;
DESIGN.md §4.10).

Expected values never come from the code under test: the numpy float32 restatement of tests/_refine.py
applied to exports, the pixel-sample engine's host twin for whole 32-byte records, and the CPU oracle
at each pixel's own count (tests/test_counts.py oracle_at).  Comparisons are on bytes and f32 bits;
every run asserts errors == 0 and short_pixels == 0.  Each case runs on the engine choices of
tests/test_counts.py, on two 40 x 24 inputs: a whole frame, and a window of the 64 x 64 dragon that is
not tile-aligned (3 x 2 tiles, the right and bottom ones partial).  tests/test_refine_host.py has the
arithmetic without a GPU.
"""
import ctypes as C

import numpy as np
import pytest

import _pixels as X
import _refine as R
import _util as U
from test_counts import ENGINES, WORK, checked_stats, finish, oracle_at

pytestmark = pytest.mark.gpu
RESULT = tuple(f for f in R.FIELDS if f not in ("least", "most"))
_twins = {}


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


@pytest.fixture(params=sorted(ENGINES))
def engine(request, monkeypatch):
    if ENGINES[request.param]:
        monkeypatch.setenv("PT_TUNE", ENGINES[request.param])   # read at session creation and by every pass
    else:
        monkeypatch.delenv("PT_TUNE", raising=False)
    return request.param


@pytest.fixture(params=sorted(R.INPUTS))
def case(request, pt):
    s, window, origin = R.open_input(pt, request.param)
    yield request.param, s, window, origin
    s.close()


def twin_at(pt, which, s, counts):
    """the host twin's records of the input's pixels (a one-rank export's order), pixel i after counts[i]
    samples; a uniform count's records are computed once and shared"""
    name, window = R.INPUTS[which]
    xy = pt.rank_pixels(R.W, R.H, 0, 1, *((window[0], window[1]) if window else (0, 0)))
    counts = np.broadcast_to(np.asarray(counts, np.uint32), (len(xy),))
    out = np.zeros(len(xy), pt.PIXEL_DTYPE)
    for c in sorted(set(counts.tolist())):
        if (which, c) not in _twins:
            _twins[which, c] = R.twin(s, xy, c)
            _twins[which, c].setflags(write=False)
        out[counts == c] = _twins[which, c][counts == c]
    return out


def thresholds(pt, which, s):
    """the rank-n/2 and the rank-95 % element of the noise of the input at 8 samples, marked at 4"""
    noise, _ = R.noise_of(twin_at(pt, which, s, 8), twin_at(pt, which, s, 4))
    return R.rank_element(noise, 50), R.rank_element(noise, 95)


def marked_session(pt, which, s, window, **kw):
    """a session at 8 samples, marked at 4: (session, the export at the mark, the export now)"""
    ss = pt.Session(s, window=window, **kw)
    ss.trace(4)
    ss.mark()            # (runs the trace not yet run first)
    mark = ss.export_states()
    ss.trace(4)
    now = ss.export_states()
    if not kw:
        assert mark.tobytes() == twin_at(pt, which, s, 4).tobytes() and now.tobytes() == twin_at(pt, which, s, 8).tobytes()
    return ss, mark, now


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def assert_plan(got, want, what):
    counts, res = got
    assert np.array_equal(counts, want[1]), what + ": counts"
    R.assert_result(res, want[2], what)


# ---- 1. noise and plan on the device ---------------------------------------------------------------
def test_noise_and_plan_are_the_restatement_of_two_exports(pt, case, engine):
    import torch
    which, s, window, origin = case
    ss, mark, now = marked_session(pt, which, s, window)
    n = ss.n_pixels
    st0 = checked_stats(ss)
    want_noise, est = R.noise_of(now, mark)
    assert est.all()
    assert np.array_equal(R.bits(ss.noise()), R.bits(want_noise)), "noise, the host form"
    dn = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # (the session's stream is not torch's)
    ss.noise(dev=dn)
    assert np.array_equal(u32(dn), R.bits(want_noise)), "noise, the device form"
    t50, t95 = thresholds(pt, which, s)
    for opts in ((t50, 4, 0, 0), (t95, 4, 0, 1), (t95, 3, 10, 1)):
        want = R.plan_of(now, mark, *opts, origin=origin)
        assert 0 < want[2]["refined"] < n
        assert_plan(ss.plan(*opts), want, "plan%r, the host form" % (opts,))
        dc = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        _, res = ss.plan(*opts, dev=dc)
        assert_plan((u32(dc), res), want, "plan%r, the device form" % (opts,))
        r = pt.RefineResult()
        pt._check(pt._lib.pt_session_plan(ss._h, C.byref(pt.RefineOpts(*opts)), None, 0, C.byref(r)))   # the result alone
        R.assert_result(r.as_dict(), want[2], "plan without counts")
    assert ss.export_states().tobytes() == now.tobytes(), "noise / plan changed the session"
    st1 = checked_stats(ss)
    assert [st1[k] for k in WORK + ("samples",)] == [st0[k] for k in WORK + ("samples",)] and not ss.ragged
    ss.close()


# ---- 2. a step is its plan; 3. marks move only with samples -----------------------------------------
def test_a_step_is_its_plan_and_marks_move_only_with_samples(pt, case, engine):
    which, s, window, origin = case
    path = X.golden(R.INPUTS[which][0])[1]
    ss, mark, now = marked_session(pt, which, s, window)
    n = ss.n_pixels
    opts = (thresholds(pt, which, s)[1], 4, 0, 1)
    want = R.plan_of(now, mark, *opts, origin=origin)
    counts, planned = ss.plan(*opts)
    assert_plan((counts, planned), want, "the plan before the step")
    res = ss.refine(*opts)
    assert [res[f] for f in RESULT] == [planned[f] for f in RESULT], "the step's result is not its plan's"
    total = 8 + counts.astype(np.int64)
    assert (res["least"], res["most"]) == ss.samples_range() == (8, 12) and ss.ragged
    after = ss.export_states()
    assert after.tobytes() == twin_at(pt, which, s, total).tobytes(), "a pixel is not where the host twin is at its count"
    assert checked_stats(ss)["samples"] == int(total.sum())
    # marks moved to `now` where the pixel took samples, and nowhere else
    mark2 = mark.copy()
    mark2[counts > 0] = now[counts > 0]
    noise2, est2 = R.noise_of(after, mark2)
    got_noise = ss.noise()
    assert np.array_equal(R.bits(got_noise), R.bits(noise2)), "the noise after the step"
    cold = counts == 0
    assert cold.any() and np.array_equal(R.bits(got_noise[cold]), R.bits(want[0][cold])), "a cold pixel's noise moved"
    assert est2.all()
    for opts2 in (opts, (float(np.median(noise2)), 2, 13, 0)):
        assert_plan(ss.plan(*opts2), R.plan_of(after, mark2, *opts2, origin=origin), "the plan after the step")
    # the resolve: the oracle at every pixel's own count
    per_pixel = np.zeros((R.H, R.W), np.uint32)
    at = (after["y"] - origin[1], after["x"] - origin[0])
    per_pixel[at] = total
    rgb, rad = finish(pt, ss, (R.W, R.H))
    X.assert_bits(rad.reshape(-1, 3), oracle_at(path, window or (0, 0, R.W, R.H), per_pixel), "the resolve after a step")
    assert checked_stats(ss)["samples"] == int(total.sum()) and ss.samples_range() == (8, 12)
    ss.close()


# ---- 4. the loop ends -------------------------------------------------------------------------------
def test_a_loop_of_refine_bootstraps_itself_and_ends(pt, case, engine):
    which, s, window, origin = case
    thr = thresholds(pt, which, s)[0]
    opts = (thr, 4, 16, 0)
    ss = pt.Session(s, window=window)
    ss.trace(4)
    n = ss.n_pixels
    mark = np.array(twin_at(pt, which, s, 4))
    mark["samples"] = 0                       # (the restatement's "no mark")
    now = twin_at(pt, which, s, 4)
    steps = 0
    while True:
        want = R.plan_of(now, mark, *opts, origin=origin)
        res = ss.refine(*opts)
        steps += 1
        assert [res[f] for f in RESULT] == [want[2][f] for f in RESULT], "step %d" % steps
        if steps == 1:
            assert res["unmarked"] == res["refined"] == n and res["samples"] == 4 * n and (want[1] == 4).all()
        if res["refined"] == 0:
            break
        assert steps < 5, "the loop did not end"
        mark[want[1] > 0] = now[want[1] > 0]
        now = twin_at(pt, which, s, now["samples"] + want[1])
        assert (res["least"], res["most"]) == (int(now["samples"].min()), int(now["samples"].max()))
    assert 1 + 2 < steps <= 1 + 4   # (the bootstrap; 8 -> 12 -> 16; the step that finds nothing to do)
    end = ss.export_states()
    assert end.tobytes() == now.tobytes(), "the frame is not the host twin's at every pixel's count"
    assert end["samples"].max() == 16 and end["samples"].min() == 8
    still_hot = want[3] & ~np.isnan(want[0])
    assert still_hot.any() and (end["samples"][still_hot] == 16).all() and res["capped"] == still_hot.sum()
    assert checked_stats(ss)["samples"] == int(end["samples"].sum()) and ss.samples_range() == (8, 16)
    ss.close()


# ---- 5. sharding does not change the plan -----------------------------------------------------------
def test_three_ranks_plan_what_one_rank_plans(pt, case, engine):
    which, s, window, origin = case
    opts = (thresholds(pt, which, s)[1], 4, 0, 1)
    want = R.plan_of(twin_at(pt, which, s, 8), twin_at(pt, which, s, 4), *opts, origin=origin)
    xy1 = pt.rank_pixels(R.W, R.H, 0, 1, *origin)
    whole = np.zeros((R.H, R.W), np.uint32)
    whole[xy1[:, 1] - origin[1], xy1[:, 0] - origin[0]] = want[1]
    got = np.full((R.H, R.W), 0xA5A5A5A5, np.uint32)
    refined = 0
    for rank in range(3):
        ss, _, _ = marked_session(pt, which, s, window, rank=rank, world=3)
        xy = pt.rank_pixels(R.W, R.H, rank, 3, *origin)
        counts, res = ss.plan(*opts)
        got[xy[:, 1] - origin[1], xy[:, 0] - origin[0]] = counts
        refined += res["refined"]
        checked_stats(ss)
        ss.close()
    assert np.array_equal(got, whole), "the plan depends on the sharding"
    assert refined == want[2]["refined"]


# ---- 6. nothing hot, nothing done -------------------------------------------------------------------
def test_a_step_without_a_hot_pixel_does_nothing(pt, case, engine):
    which, s, window, origin = case
    ss, mark, now = marked_session(pt, which, s, window)
    st0 = checked_stats(ss)
    noise0 = ss.noise()
    worst = ss.plan(0.0, 4)[1]["worst"]
    assert worst == float(R.noise_of(now, mark)[0].max()) > 0
    for thr in (worst, 2 * worst):
        res = ss.refine(thr, 4, 0, 1)
        assert res["refined"] == res["samples"] == 0 and (res["least"], res["most"]) == (8, 8) and R.bits(res["worst"]) == R.bits(worst)
    st1 = checked_stats(ss)
    assert [st1[k] for k in WORK + ("samples",)] == [st0[k] for k in WORK + ("samples",)] and not ss.ragged
    assert ss.export_states().tobytes() == now.tobytes()
    assert np.array_equal(R.bits(ss.noise()), R.bits(noise0)), "a step that did nothing moved a mark"
    ss.close()


# ---- 7. marks are cleared ---------------------------------------------------------------------------
def test_reset_and_imports_clear_the_marks(pt, case, engine):
    which, s, window, origin = case
    ss, mark, now = marked_session(pt, which, s, window)
    n = ss.n_pixels
    assert ss.plan(0.0, 4)[1]["unmarked"] == 0
    ss.reset()
    res = ss.plan(0.0, 4)[1]
    assert res["unmarked"] == n and res["refined"] == n and (res["least"], res["most"]) == (0, 0)
    ss.trace(2)
    ss.mark()
    ss.trace(1)
    assert ss.plan(0.0, 4)[1]["unmarked"] == 0
    assert ss.import_states(np.array(now)) == n
    assert ss.plan(0.0, 4)[1]["unmarked"] == n and (ss.noise() == np.inf).all()
    ss.mark()
    ss.trace(1)
    assert ss.plan(0.0, 4)[1]["unmarked"] == 0
    ragged = twin_at(pt, which, s, 4 + 4 * (np.arange(n) % 2))
    assert ss.import_states(np.array(ragged), ragged=True) == n
    res = ss.plan(0.0, 4)[1]
    assert res["unmarked"] == n and (res["least"], res["most"]) == (4, 8)
    assert ss.export_states().tobytes() == ragged.tobytes()
    checked_stats(ss)
    ss.close()


# ---- 8. non-finite sums -----------------------------------------------------------------------------
def test_non_finite_sums(pt, case, engine):
    which, s, window, origin = case
    n = R.W * R.H
    start = np.array(twin_at(pt, which, s, 4 + 4 * (np.arange(n) % 3 == 0)))
    bad = {5: (np.nan, 1, 1), 40: (np.inf, 1, 1), 77: (np.inf, -np.inf, 1), 300: (1, -np.inf, 1), 301: (1, 1, np.nan),
           959: (np.nan, np.nan, np.nan)}
    for i, v in bad.items():
        start["sum"][i] = v
    ss = pt.Session(s, window=window)
    assert ss.import_states(start, ragged=True) == n
    ss.mark()
    mark = ss.export_states()
    assert mark.tobytes() == start.tobytes()
    ss.trace_counts((1 + np.arange(n) % 4).astype(np.uint32))
    now = ss.export_states()
    for opts in ((0.0, 4, 0, 1), (0.0, 4, 0, 0), (0.0, 4, 11, 1)):
        want = R.plan_of(now, mark, *opts, origin=origin)
        assert want[2]["nonfinite"] == len(bad) and want[2]["unmarked"] == 0
        counts, res = ss.plan(*opts)
        assert_plan((counts, res), want, "non-finite sums %r" % (opts,))
        assert (counts[list(bad)] == 0).all()
        if opts[3]:
            assert want[3][list(bad)].any(), "no NaN pixel lies beside a hot one"
    assert np.array_equal(R.bits(ss.noise()), R.bits(want[0]))
    # ... and a step leaves them where they are
    res = ss.refine(0.0, 4, 0, 1)
    end = ss.export_states()
    assert end[list(bad)].tobytes() == now[list(bad)].tobytes()
    assert np.array_equal(end["samples"], now["samples"] + R.plan_of(now, mark, 0.0, 4, 0, 1, origin=origin)[1])
    checked_stats(ss)
    ss.close()


# ---- 9. refusals ------------------------------------------------------------------------------------
def test_refused_calls_leave_the_session_alone(pt):
    which = "frame"
    s, window, origin = R.open_input(pt, which)
    ss, mark, now = marked_session(pt, which, s, window)
    n = ss.n_pixels
    noise0, st0 = ss.noise(), checked_stats(ss)
    lib, ok, res = pt._lib, pt.RefineOpts(0.1, 4, 0, 0), pt.RefineResult()
    res.refined = 77
    buf = np.full(n, 0xA5A5A5A5, np.uint32)
    ss.trace(3)   # (a refused call does not run it either)
    for what, o in [("NaN threshold", (float("nan"), 4, 0, 0)), ("negative threshold", (-1e-30, 4, 0, 0)),
                    ("step 0", (0.1, 0, 0, 0)), ("spread 2", (0.1, 4, 0, 2))]:
        o = pt.RefineOpts(*o)
        assert lib.pt_session_plan_host(ss._h, C.byref(o), U._p(buf), n, C.byref(res)) == pt.PT_E_INVALID, what
        assert lib.pt_session_plan(ss._h, C.byref(o), None, 0, C.byref(res)) == pt.PT_E_INVALID, what
        assert lib.pt_session_refine(ss._h, C.byref(o), C.byref(res)) == pt.PT_E_INVALID, what
    assert lib.pt_session_plan_host(ss._h, None, U._p(buf), n, C.byref(res)) == pt.PT_E_INVALID
    assert lib.pt_session_plan_host(ss._h, C.byref(ok), U._p(buf), n, None) == pt.PT_E_INVALID
    assert lib.pt_session_refine(ss._h, None, C.byref(res)) == pt.PT_E_INVALID
    assert lib.pt_session_refine(ss._h, C.byref(ok), None) == pt.PT_E_INVALID
    # room for one value too few, and a null buffer
    import torch
    d = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.pt_session_noise_host(ss._h, U._p(buf), n - 1) == pt.PT_E_INVALID
    assert lib.pt_session_noise(ss._h, d.data_ptr(), n - 1) == pt.PT_E_INVALID
    assert lib.pt_session_plan_host(ss._h, C.byref(ok), U._p(buf), n - 1, C.byref(res)) == pt.PT_E_INVALID
    assert lib.pt_session_plan(ss._h, C.byref(ok), d.data_ptr(), n - 1, C.byref(res)) == pt.PT_E_INVALID
    assert lib.pt_session_noise_host(ss._h, None, n) == pt.PT_E_INVALID
    assert lib.pt_session_noise(ss._h, None, n) == pt.PT_E_INVALID
    assert res.refined == 77 and (buf == 0xA5A5A5A5).all() and (u32(d) == 0xffffffff).all()
    assert ss.samples_range() == (11, 11) and checked_stats(ss)["rays"] > st0["rays"]   # (stats ran the trace)
    assert ss.export_states().tobytes() == twin_at(pt, which, s, 11).tobytes()
    want_noise, _ = R.noise_of(twin_at(pt, which, s, 11), mark)
    assert np.array_equal(R.bits(ss.noise()), R.bits(want_noise)), "a refused call moved a mark"
    ss.close()
    # a megakernel session refuses all four calls
    mk = pt.Session(s, window=window, traversal=pt.TRAVERSAL_EXACT)
    mk.trace(2)
    before = mk.export_states()
    for call in (mk.mark, mk.noise, lambda: mk.plan(0.1, 4), lambda: mk.refine(0.1, 4)):
        with pytest.raises(pt.PTError) as e:
            call()
        assert e.value.code == pt.PT_E_INVALID and "k_trace advances by a uniform spp" in str(e.value)
    assert mk.export_states().tobytes() == before.tobytes() and not mk.ragged
    assert checked_stats(mk)["rounds"] == 0
    mk.close()
    # a session that owns no pixel accepts every call and reports zeros
    none = pt.Session(s, rank=1, world=2, window=(0, 0, 16, 16))
    assert none.n_pixels == 0
    none.mark()
    assert len(none.noise()) == 0 and pt._lib.pt_session_noise(none._h, None, 0) == pt.PT_OK
    counts, r = none.plan(0.1, 4)
    assert len(counts) == 0 and not any(r[f] for f in RESULT) and (r["least"], r["most"]) == (0, 0)
    r = none.refine(0.1, 4, 0, 1)
    assert not any(r[f] for f in RESULT)
    none.close()
    s.close()


# ---- 10. a frame of more tiles than the plan has workgroups ------------------------------------------
BIG = ("DIMENSIONS 780 670\nRAY_DEPTH 1\nSAMPLES 1\nBG_COLOR 0.2 0.3 0.4\nCAMERA_POSITION 0 0 4\nCAMERA_RIGHT 1 0 0\n"
       "CAMERA_UP 0 1 0\nCAMERA_FORWARD 0 0 -1\nCAMERA_FOV_X 1.2\nNEW_PRIMITIVE\nBOX 0.5 0.5 0.5\nCOLOR 1 0 0\n"
       "NEW_PRIMITIVE\nELLIPSOID 0.3 0.3 0.3\nPOSITION 1 0 0\nEMISSION 2 2 2\n")


def test_a_workgroup_plans_several_tiles(pt):
    """49 x 42 = 2,058 tiles, the right and bottom ones partial: k_noise_plan's 1,024 workgroups take two or
    three tiles each, summing their share of the result over them.  The sums are the test's own (seeded),
    so that the noise differs from pixel to pixel on a scene that costs nothing to trace."""
    w, h = 780, 670
    with pt.Scene.loads(BIG) as s:
        s.prepare()
        ss = pt.Session(s)
        assert ss.n_tiles == 2058 and ss.n_pixels == w * h
        start = s.pixel_init(pt.rank_pixels(w, h, 0, 1))
        rng = np.random.default_rng(23)
        start["sum"] = rng.random((w * h, 3), np.float32) * 8
        start["samples"] = 4 + rng.integers(0, 3, w * h)
        assert ss.import_states(start, ragged=True) == w * h
        ss.mark()
        ss.trace(1)
        now = ss.export_states()
        noise, est = R.noise_of(now, start)
        assert est.all() and len(np.unique(noise)) > w * h // 2
        assert np.array_equal(R.bits(ss.noise()), R.bits(noise))
        for opts in ((R.rank_element(noise, 50), 2, 7, 0), (R.rank_element(noise, 95), 2, 0, 1)):
            want = R.plan_of(now, start, *opts)
            assert 0 < want[2]["refined"] < w * h
            assert_plan(ss.plan(*opts), want, "the large frame %r" % (opts,))
        res = ss.refine(*opts)
        assert [res[f] for f in RESULT] == [want[2][f] for f in RESULT]
        end = ss.export_states()
        assert np.array_equal(end["samples"], now["samples"] + want[1])
        assert end[want[1] == 0].tobytes() == now[want[1] == 0].tobytes()
        mark2 = start.copy()
        mark2[want[1] > 0] = now[want[1] > 0]
        assert np.array_equal(R.bits(ss.noise()), R.bits(R.noise_of(end, mark2)[0]))
        assert checked_stats(ss)["samples"] == int(end["samples"].sum(dtype=np.uint64))
        ss.close()
