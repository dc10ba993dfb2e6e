"""GPU tests of a session's per-pixel sample counts (include/pt.h pt_session_trace_counts /
pt_session_import_ragged and their host forms, pt_session_samples_range; ptrace.Session.trace_counts /
import_states(ragged=True) / samples_range / ragged): an adaptive pass on the session's
own engines leaves every pixel exactly where pt_pixq_run leaves it after the pixel's own count.

Expected values never come from the code under test: the CPU oracle at each count
(tests/_pixels.py oracle_render, picked per pixel), the reference's recorded radiance and images,
the pixel-sample engine and its host twin for whole 32-byte records.  Comparisons are on bytes and
f32 bits; every run asserts errors == 0.  Each case runs on every engine choice of
tests/test_light_sampling.py.  tests/test_counts_host.py has the arithmetic without a GPU.
"""
import numpy as np
import pytest

import _paths as P
import _pixels as X
import _util as U

pytestmark = pytest.mark.gpu
ENGINES = {"default": None, "path": "coop=0", "exact": "coop=0,lstack=1", "coop": "coop=100000000"}
FRAME = "dragon_glass_40x24x7"      # 3 x 2 tiles, the right and bottom ones partial
W, H, S = 40, 24, 7
WINDOW = (8, 8, 40, 24)             # of the 64 x 64 dragon: not tile-aligned, partial tiles
WORK = ("rays", "node_visits", "prim_tests", "plane_tests", "aux_visits", "isect_launches", "rounds", "coop_rays")


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


@pytest.fixture()
def scene(pt):
    with pt.Scene.load(X.golden(FRAME)[1]) as s:
        s.prepare()
        assert (s.info["width"], s.info["height"], s.info["samples"]) == (W, H, S)
        yield s


def export_perm(pt, window):
    """row-major index, in `window`, of every record of a one-rank export of that window"""
    x0, y0, w, h = window
    xy = pt.rank_pixels(w, h, 0, 1, x0, y0).astype(np.int64)
    return (xy[:, 1] - y0) * w + (xy[:, 0] - x0)


def frame_counts(pt, window, per_pixel):
    """a row-major count map of `window` in a one-rank export's order"""
    return np.ascontiguousarray(np.asarray(per_pixel, np.uint32).reshape(-1)[export_perm(pt, window)])


def checked_stats(ss):
    st = ss.stats()
    assert st["errors"] == 0 and st["short_pixels"] == 0
    return st


def run_session(s, state, counts=None, spp=0):
    """tests/_pixels.py's `run`, backed by a session: the states -- a window's, row-major -- imported
    ragged, one trace_counts (the device form) or trace, and the export brought back to their order;
    the statistics are this run's own"""
    import torch
    pt = U.ptrace()
    x0, y0 = int(state["x"].min()), int(state["y"].min())
    window = (x0, y0, int(state["x"].max()) - x0 + 1, int(state["y"].max()) - y0 + 1)
    assert np.array_equal(np.stack([state["x"], state["y"]], axis=1), X.window_xy(window))
    perm = export_perm(pt, window)
    s.prepare()
    ss = pt.Session(s, window=window)
    assert ss.n_pixels == len(state)
    assert ss.import_states(np.array(state[perm]), ragged=True) == len(state)
    before = checked_stats(ss)
    assert before["rays"] == 0
    if counts is None:
        ss.trace(spp)
    else:
        dc = torch.from_numpy(np.ascontiguousarray(counts, np.uint32)[perm].view(np.int32)).cuda()
        torch.cuda.synchronize()
        ss.trace_counts(dc)
    got = ss.export_states()
    st = checked_stats(ss)
    lo, hi = ss.samples_range()
    assert (lo, hi) == (int(got["samples"].min()), int(got["samples"].max())) and ss.ragged == (lo != hi)
    assert st["samples"] == int(got["samples"].sum(dtype=np.uint64))
    ss.close()
    out = np.zeros(len(state), pt.PIXEL_DTYPE)
    out[perm] = got
    st["samples"] -= before["samples"]
    return out, st


def finish(pt, ss, size, rank=0, world=1):
    """resolve: (image, radiance) of the session's window with its own tiles filled in"""
    import torch
    drad = torch.empty(max(ss.n_tiles, 1) * 256 * 3, dtype=torch.float32, device="cuda")
    ss.resolve(dev_rad=drad.data_ptr())
    ss.sync()
    checked_stats(ss)
    rgb = pt.unpack_tiles(ss.read_packed(), size[0], size[1], rank, world)
    rad = pt.unpack_tiles_f32(drad.cpu().numpy(), size[0], size[1], rank, world)
    return rgb, rad


def oracle_at(path, window, counts):
    """the oracle's radiance of `window`, row-major, every pixel at its own count"""
    counts = np.asarray(counts).reshape(-1)
    want = np.zeros((len(counts), 3), np.float32)
    for c in sorted(set(counts.tolist())):
        assert c > 0
        want[counts == c] = X.oracle_render(path, window, c)[1][counts == c]
    return want


def twin_states(s, xy, counts):
    """the pixel-sample engine's host twin: fresh states of the pixels xy after counts[i] samples"""
    out, ctr = s.selftest_pixels_host(s.pixel_init(xy), counts=np.ascontiguousarray(counts, np.uint32))
    assert ctr["errors"] == 0
    return out


# ---- 1. per-pixel counts against the reference ------------------------------------------------------
def test_per_pixel_counts_against_the_oracle_and_the_reference(pt, engine):
    X.case_counts(pt, run_session, X.DRAGON, WINDOW)


# ---- 2. cross-engine bytes --------------------------------------------------------------------------
def test_a_sessions_states_are_the_pixel_querys_byte_for_byte(pt, engine):
    import torch
    name, (w, h) = "hw3s4_24x40x5", (24, 40)
    with pt.Scene.load(X.golden(name)[1]) as s:
        s.prepare()
        assert (s.info["width"], s.info["height"]) == (w, h)
        xy = pt.rank_pixels(w, h, 0, 1)
        counts = (1 + (np.arange(len(xy)) * 7) % 8).astype(np.uint32)
        ss = pt.Session(s)
        ss.trace_counts(counts)   # (the host form)
        got = ss.export_states()
        st = checked_stats(ss)
        ss.close()
        d = torch.from_numpy(s.pixel_init(xy).view(np.uint8)).cuda()
        dc = torch.from_numpy(counts.view(np.int32)).cuda()
        torch.cuda.synchronize()
        with pt.PixelQuery(s, max_pixels=len(xy)) as q:
            q.run(d, counts=dc, n=len(xy))
            qst = q.stats()
        want = d.cpu().numpy().view(pt.PIXEL_DTYPE)
        assert qst["errors"] == 0
    assert np.array_equal(got["samples"], counts) and (got["rng"] & X.SAVED_BIT).any()
    assert got.tobytes() == want.tobytes(), "the session's ragged export differs from PixelQuery.run's states"
    assert st["rays"] == qst["rays"] and st["samples"] == qst["samples"] == int(counts.sum())


# ---- 3. ragged resolve ------------------------------------------------------------------------------
def test_a_ragged_resolve_divides_every_pixel_by_its_own_count(pt, engine):
    path = X.golden(X.DRAGON)[1]
    x0, y0, w, h = WINDOW
    per_pixel = (1 + (np.arange(w * h) * 7) % 8).astype(np.uint32)
    with pt.Scene.load(path) as s:
        s.prepare()
        ss = pt.Session(s, window=WINDOW)
        ss.trace_counts(frame_counts(pt, WINDOW, per_pixel))
        assert ss.ragged and ss.samples_range() == (1, 8)
        rgb, rad = finish(pt, ss, (w, h))
        states = ss.export_states()
        mean, rgb8 = s.pixel_resolve(states)
        at = (states["y"] - y0, states["x"] - x0)
        assert np.array_equal(states["samples"], per_pixel.reshape(h, w)[at])
        X.assert_bits(rad[at], mean, "the ragged resolve against pixel_resolve of the export")
        assert np.array_equal(rgb[at], rgb8)
        X.assert_bits(rad.reshape(-1, 3), oracle_at(path, WINDOW, per_pixel), "the ragged resolve against the oracle")
        ss.close()
        # a pixel without a sample: refused, the session intact
        ss = pt.Session(s, window=WINDOW)
        per_pixel[333] = 0
        ss.trace_counts(frame_counts(pt, WINDOW, per_pixel))
        before = ss.export_states()
        assert ss.samples_range() == (0, 8) and (before["samples"] == 0).sum() == 1
        with pytest.raises(pt.PTError) as e:
            ss.resolve()
        assert e.value.code == pt.PT_E_INVALID
        assert ss.export_states().tobytes() == before.tobytes()
        checked_stats(ss)
        # ... and accepted once that pixel has one
        ss.trace(1)
        rgb, rad = finish(pt, ss, (w, h))
        X.assert_bits(rad.reshape(-1, 3), oracle_at(path, WINDOW, per_pixel + 1), "one more sample for every pixel")
        ss.close()


# ---- 4. composition ---------------------------------------------------------------------------------
def test_passes_compose(pt, scene, engine):
    path = X.golden(FRAME)[1]
    xy = pt.rank_pixels(W, H, 0, 1)
    rng = np.random.default_rng(19)
    a, b = rng.integers(0, 4, len(xy)).astype(np.uint32), rng.integers(0, 4, len(xy)).astype(np.uint32)
    assert (a == 0).any() and (b == 0).any() and ((a + b) == 0).any()

    def after(*steps):
        ss = pt.Session(scene)
        for kind, arg in steps:
            getattr(ss, kind)(arg)
        out = ss.export_states()
        st = checked_stats(ss)
        assert st["samples"] == int(out["samples"].sum())
        ss.close()
        return out

    # counts a then counts b = counts a + b (= the host twin's states at a + b)
    ab = after(("trace_counts", a), ("trace_counts", b))
    assert ab.tobytes() == after(("trace_counts", a + b)).tobytes()
    assert ab.tobytes() == twin_states(scene, xy, a + b).tobytes()
    # every count 3 = trace(3)
    three = after(("trace_counts", np.full(len(xy), 3, np.uint32)))
    assert three.tobytes() == after(("trace", 3)).tobytes()
    mean, _ = scene.pixel_resolve(three)
    X.assert_bits(mean, X.oracle_render(path, (0, 0, W, H), 3)[1][xy[:, 1] * W + xy[:, 0]], "every count 3")
    # counts c, then trace(2): the oracle at c + 2
    c = (np.arange(len(xy)) % 4).astype(np.uint32)
    c2 = after(("trace_counts", c), ("trace", 2))
    assert np.array_equal(c2["samples"], c + 2)
    assert c2.tobytes() == twin_states(scene, xy, c + 2).tobytes()
    mean, _ = scene.pixel_resolve(c2)
    per_pixel = np.zeros(W * H, np.uint32)
    per_pixel[xy[:, 1] * W + xy[:, 0]] = c + 2
    X.assert_bits(mean, oracle_at(path, (0, 0, W, H), per_pixel)[xy[:, 1] * W + xy[:, 0]], "counts c, then trace(2)")
    # all-zero counts: no work, no change
    ss = pt.Session(scene)
    ss.trace_counts(a)
    before, st0 = ss.export_states(), checked_stats(ss)
    ss.trace_counts(np.zeros(len(xy), np.uint32))
    st1 = checked_stats(ss)
    assert ss.export_states().tobytes() == before.tobytes()
    assert [st1[k] for k in WORK] == [st0[k] for k in WORK] and st1["samples"] == st0["samples"] == int(a.sum())
    ss.close()


# ---- 5. one long chain ------------------------------------------------------------------------------
def test_one_long_chain_among_short_ones(pt, engine):
    path = P.s1_scene("hw3s3_48x48")
    long_xy = (29, 31)
    per_pixel = np.ones(48 * 48, np.uint32)
    per_pixel[long_xy[1] * 48 + long_xy[0]] = 200
    want = np.array(X.oracle_render(path, (0, 0, 48, 48), 1)[1])
    want[long_xy[1] * 48 + long_xy[0]] = X.oracle_render(path, (long_xy[0], long_xy[1], 1, 1), 200)[1][0]
    assert want[long_xy[1] * 48 + long_xy[0]].any()
    with pt.Scene.load(path) as s:
        s.prepare()
        ss = pt.Session(s)
        ss.trace_counts(frame_counts(pt, (0, 0, 48, 48), per_pixel))
        out = ss.export_states()
        st = checked_stats(ss)
        mean, _ = s.pixel_resolve(out)
        rgb, rad = finish(pt, ss, (48, 48))
        ss.close()
    X.assert_bits(mean, want[out["y"] * 48 + out["x"]], "one long chain: the export")
    X.assert_bits(rad.reshape(-1, 3), want, "one long chain: the resolve")
    assert st["samples"] == 48 * 48 - 1 + 200
    if engine == "default":
        assert st["coop_rays"] > 0   # (the long chain's tail ran in the cooperative engine)


# ---- 6. ranks and windows ---------------------------------------------------------------------------
def test_three_ranks_take_their_slices_of_one_count_map(pt, scene, engine):
    per_pixel = ((np.arange(W * H) * 5) % 7).astype(np.uint32)   # by pixel, y * W + x (zeros among them)
    parts = []
    for r in range(3):
        xy = pt.rank_pixels(W, H, r, 3)
        ss = pt.Session(scene, rank=r, world=3)
        assert ss.n_pixels == len(xy)
        ss.trace_counts(per_pixel[xy[:, 1] * W + xy[:, 0]])
        parts.append(ss.export_states())
        assert np.array_equal(np.stack([parts[-1]["x"], parts[-1]["y"]], axis=1), xy)
        checked_stats(ss)
        ss.close()
    one = pt.Session(scene)
    xy = pt.rank_pixels(W, H, 0, 1)
    one.trace_counts(per_pixel[xy[:, 1] * W + xy[:, 0]])
    whole = one.export_states()
    checked_stats(one)
    one.close()
    union = np.concatenate(parts)
    assert len(union) == W * H

    def by_pixel(states):
        return states[np.argsort(states["y"] * W + states["x"], kind="stable")]
    assert by_pixel(union).tobytes() == by_pixel(whole).tobytes()
    assert np.array_equal(by_pixel(whole)["samples"], per_pixel)


# ---- 7. checkpoint ----------------------------------------------------------------------------------
def test_a_ragged_frame_is_checkpointed_into_a_new_session(pt, scene, engine):
    import torch
    xy = pt.rank_pixels(W, H, 0, 1)
    counts = ((np.arange(len(xy)) * 3) % 5).astype(np.uint32)
    a = pt.Session(scene)
    a.trace_counts(counts)
    saved = a.export_states()
    b = pt.Session(scene)
    fresh = b.export_states()
    # the strict import goes on refusing unequal counts, and so does the ragged one what any import refuses
    k = 333
    bad_rng = saved.copy()
    bad_rng["rng"][k] = X.M31
    refused = {"strict": (saved, False), "one given twice": (np.concatenate([saved, saved[k:k + 1]]), True),
               "one owned pixel missing": (np.delete(saved, k), True), "rng low bits 2^31 - 1": (bad_rng, True)}
    for what, (states, ragged) in refused.items():
        for form in ("host", "device"):
            d = torch.from_numpy(np.array(states).view(np.uint8)).cuda()
            torch.cuda.synchronize()
            with pytest.raises(pt.PTError) as e:
                b.import_states(states if form == "host" else d, n=len(states), ragged=ragged)
            assert e.value.code == pt.PT_E_INVALID, what
            assert b.export_states().tobytes() == fresh.tobytes(), "%s (%s): the session changed" % (what, form)
            assert not b.ragged and b.stats()["samples"] == 0
    assert b.import_states(saved[::-1], ragged=True) == len(xy)
    assert b.ragged and b.samples_range() == (0, 4) and b.stats()["samples"] == int(counts.sum())
    assert b.export_states().tobytes() == saved.tobytes()
    a.trace(2)
    b.trace(2)
    end = b.export_states()
    assert end.tobytes() == a.export_states().tobytes()
    assert end.tobytes() == twin_states(scene, xy, counts + 2).tobytes()
    assert checked_stats(b)["samples"] == checked_stats(a)["samples"] == int(counts.sum()) + 2 * len(xy)
    # a strict import of equal counts makes the session uniform again
    assert b.import_states(np.array(twin_states(scene, xy, np.full(len(xy), 3)))) == len(xy)
    assert not b.ragged and b.samples_range() == (3, 3)
    b.trace(4)
    rgb, rad = finish(pt, b, (W, H))
    _, _, img, want = X.golden(FRAME)
    X.assert_bits(rad.reshape(-1, 3), want.reshape(-1, 3), "a uniform import after a ragged one")
    assert np.array_equal(rgb, img)
    a.close()
    b.close()


# ---- 8. refusals ------------------------------------------------------------------------------------
def test_refused_calls_leave_the_session_alone(pt, scene):
    xy = pt.rank_pixels(W, H, 0, 1)
    n = len(xy)
    ss = pt.Session(scene)
    ss.trace_counts((np.arange(n) % 3).astype(np.uint32))
    before, st0 = ss.export_states(), checked_stats(ss)
    for counts in (np.ones(n - 1, np.uint32), np.ones(n + 1, np.uint32), np.ones(0, np.uint32)):
        with pytest.raises(pt.PTError) as e:
            ss.trace_counts(counts)
        assert e.value.code == pt.PT_E_INVALID
    assert pt._lib.pt_session_trace_counts(ss._h, n, None) == pt.PT_E_INVALID
    assert pt._lib.pt_session_trace_counts_host(ss._h, n, None) == pt.PT_E_INVALID
    assert ss.export_states().tobytes() == before.tobytes()
    assert [checked_stats(ss)[k] for k in WORK + ("samples",)] == [st0[k] for k in WORK + ("samples",)]
    ss.close()
    # overflow: every pixel at 0xfffffff0 samples, 32 more asked for
    high = scene.pixel_init(xy)
    high["samples"] = 0xfffffff0
    ss = pt.Session(scene)
    assert ss.import_states(high) == n
    before = ss.export_states()
    assert before.tobytes() == high.tobytes()
    with pytest.raises(pt.PTError) as e:
        ss.trace_counts(np.full(n, 32, np.uint32))
    assert e.value.code == pt.PT_E_INVALID and "2^32" in str(e.value)
    one = np.zeros(n, np.uint32)
    one[7] = 16
    with pytest.raises(pt.PTError) as e:
        ss.trace_counts(one)
    assert e.value.code == pt.PT_E_INVALID
    assert ss.export_states().tobytes() == before.tobytes() and ss.samples_range() == (0xfffffff0, 0xfffffff0)
    # ... and 2^32 - 1 itself is a count a pixel may reach
    one[7] = 15
    ss.trace_counts(one)
    out = ss.export_states()
    assert out["samples"][7] == 0xffffffff and np.delete(out, 7).tobytes() == np.delete(before, 7).tobytes()
    want, _ = scene.selftest_pixels_host(high[7:8], spp=15)
    assert out[7:8].tobytes() == want.tobytes()
    checked_stats(ss)
    ss.close()
    # a session that owns no pixel accepts n = 0
    ss = pt.Session(scene, rank=1, world=2, window=(0, 0, 16, 16))
    assert ss.n_pixels == 0
    ss.trace_counts(np.zeros(0, np.uint32))
    ss.trace_counts(0, n=0)
    with pytest.raises(pt.PTError):
        ss.trace_counts(np.ones(1, np.uint32))
    assert ss.import_states(np.array(high), ragged=True) == 0 and not ss.ragged
    ss.close()


@pytest.mark.parametrize("how", ["traversal", "tune"])
def test_a_megakernel_session_refuses_per_pixel_counts(pt, scene, how, monkeypatch):
    if how == "tune":
        monkeypatch.setenv("PT_TUNE", "engine=mega")
    ss = pt.Session(scene, traversal=pt.TRAVERSAL_EXACT if how == "traversal" else pt.TRAVERSAL_REPLAY)
    ss.trace(2)
    before = ss.export_states()
    with pytest.raises(pt.PTError) as e:
        ss.trace_counts(np.ones(W * H, np.uint32))
    assert e.value.code == pt.PT_E_INVALID and "k_trace advances by a uniform spp" in str(e.value)
    for ragged_states in (before, before[::-1]):
        with pytest.raises(pt.PTError) as e:
            ss.import_states(np.array(ragged_states), ragged=True)
        assert e.value.code == pt.PT_E_INVALID and "uniform spp" in str(e.value)
    assert ss.export_states().tobytes() == before.tobytes() and not ss.ragged
    assert checked_stats(ss)["rounds"] == 0   # (the megakernel ran, as tests/test_gpu.py knows it)
    ss.close()


# ---- 9. reset ---------------------------------------------------------------------------------------
def test_reset_after_a_ragged_pass_renders_the_fixture(pt, scene, engine):
    ss = pt.Session(scene)
    ss.trace_counts((np.arange(W * H) % 5).astype(np.uint32))
    assert ss.ragged
    ss.reset()
    assert not ss.ragged and ss.samples_range() == (0, 0) and ss.stats()["samples"] == 0
    assert ss.export_states().tobytes() == scene.pixel_init(pt.rank_pixels(W, H, 0, 1)).tobytes()
    ss.trace(S)
    rgb, rad = finish(pt, ss, (W, H))
    _, _, img, want = X.golden(FRAME)
    X.assert_bits(rad.reshape(-1, 3), want.reshape(-1, 3), FRAME + " after a reset")
    assert np.array_equal(rgb, img) and ss.stats()["samples"] == W * H * S
    ss.close()
