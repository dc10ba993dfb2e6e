"""GPU tests of the first-hit feature engine (k_feats / k_feats_exact through pt_features,
pt_featq_* and pt_session_features): for image-plane positions, the closest hit of the camera's
ray and the hit primitive's scene data, byte for byte.

Expected values never come from the code under test (tests/_features.py): the camera restated in
numpy float32 from the scene text, the CPU oracle's ray_intersection and prim_info, and a parser
of the scene text for the colours.  For the work counters: the host execution of the same query
state machine (Scene.selftest_features), whose step sequence depends on the ray and the scene
only.  tests/test_features_host.py has the layouts, the accessors and the host mirror itself.
"""
import ctypes as C

import numpy as np
import pytest

import _features as F
import _pixels as X
import _util as U

pytestmark = pytest.mark.gpu
DRAGON = "dragon_64x64x16"
GUARD = 64   # records of 0xA5 behind a device buffer's n records


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


def assert_counters(st, host, n, n_planes):
    assert st["errors"] == 0 and st["rays"] == n
    assert st["plane_tests"] == n * n_planes
    assert (st["node_visits"], st["prim_tests"], st["aux_visits"], st["fallbacks"], st["fallbacks_ray"]) == \
        (host["node_visits"], host["prim_tests"], host["aux_visits"], host["fallbacks"], host["fallbacks_ray"])


# ---- 1. every scene's pixel centres ---------------------------------------------------------------
@pytest.mark.parametrize("name", F.SCENES)
def test_pixel_centres_match_the_oracle_and_the_host_counters(pt, name):
    path, want, _ = F.expected_centres(name)
    F.check_conditions(name, want)
    xy = F.centres(path)
    with pt.Scene.load(path) as s:
        _, host = s.selftest_features(xy)
        got, st = s.features(xy)
        n_planes = s.info["n_planes"]
    F.assert_records(got, want)
    assert_counters(st, host, len(want), n_planes)
    assert st["fallbacks_ray"] == 0


# ---- 2. sub-pixel positions in and around the frame, and non-finite ones ------------------------------
@pytest.mark.parametrize("name", F.SCENES)
def test_subpixel_and_nonfinite_positions(pt, name):
    path, xy, want, _ = F.expected_subpixel(name)
    with pt.Scene.load(path) as s:
        _, host = s.selftest_features(xy)
        got, st = s.features(xy)
        n_planes = s.info["n_planes"]
    F.assert_records(got, want)
    assert_counters(st, host, len(want), n_planes)
    assert st["fallbacks_ray"] == 32 and st["fallbacks"] == host["fallbacks"] >= 32


# ---- 3. edges of a wave and of the output buffer ------------------------------------------------------
def _device_buffers(torch, xy, n):
    d_xy = torch.from_numpy(np.array(xy[:max(n, 1)])).cuda()   # (a copy: the shared positions are read-only)
    d_out = torch.full(((n + GUARD) * 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return d_xy, d_out


def _check_buffer(pt, d_out, want, n):
    raw = d_out.cpu().numpy()
    assert (raw[n * 64:] == 0xA5).all(), "the run wrote past its n records"
    F.assert_records(raw[:n * 64].view(pt.FEATURE_DTYPE), want[:n])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_wave_edges_on_device_tensors(pt, n):
    import torch
    path, want, _ = F.expected_centres(DRAGON)
    # (rows from the frame's middle: the dragon, the lamp and the walls, not 257 floor pixels)
    xy, want = F.centres(path)[1900:], want[1900:]
    with pt.Scene.load(path) as s:
        with pt.FeatureQuery(s, max_points=512) as q:
            d_xy, d_out = _device_buffers(torch, xy, n)
            q.run(d_xy, d_out, n=n)
            st = q.stats()
            _check_buffer(pt, d_out, want, n)
    assert st["rays"] == n and st["errors"] == 0


# ---- 4. refill: more points than the chip has lanes ---------------------------------------------------
def tiled(xy, want, n, seed):
    idx = np.random.default_rng(seed).permutation(n) % len(xy)
    return np.ascontiguousarray(xy[idx]), want[idx]


def test_refill_more_points_than_resident_lanes(pt):
    n = (1 << 20) + 37   # > 524,288 = 256 CUs x 2,048 lanes: lanes certainly took a second point
    path, want, _ = F.expected_centres(DRAGON)
    xy, want = tiled(F.centres(path), want, n, 3)
    with pt.Scene.load(path) as s:
        got_a, st_a = s.features(xy)
        got_b, st_b = s.features(xy)
    assert got_a.tobytes() == got_b.tobytes()
    F.assert_records(got_a, want)
    assert st_a["rays"] == n and st_b["rays"] == n and st_a["errors"] == 0 and st_b["errors"] == 0


# ---- 5. refusals and ordering -----------------------------------------------------------------------------
def test_run_refuses_more_than_max_points(pt):
    import torch
    path, _, _ = F.expected_centres(DRAGON)
    xy = F.centres(path)
    with pt.Scene.load(path) as s:
        with pt.FeatureQuery(s, max_points=64) as q:
            d_xy, d_out = _device_buffers(torch, xy, 65)
            with pytest.raises(pt.PTError) as e:
                q.run(d_xy, d_out)
            assert e.value.code == pt.PT_E_INVALID
            # a misaligned buffer, a null one
            for args in ((d_xy.data_ptr() + 4, d_out), (d_xy, d_out.data_ptr() + 8), (0, d_out), (d_xy, 0)):
                with pytest.raises(pt.PTError) as e:
                    q.run(*args, n=8)
                assert e.value.code == pt.PT_E_INVALID
            assert (d_out.cpu().numpy() == 0xA5).all()
            st = q.stats()
            assert st["rays"] == 0 and st["node_visits"] == 0 and st["plane_tests"] == 0


def test_two_runs_back_to_back_on_one_stream(pt):
    import torch
    path, want, _ = F.expected_centres(DRAGON)
    xy = F.centres(path)
    with pt.Scene.load(path) as s:
        with pt.FeatureQuery(s, max_points=4096) as q:
            a_xy, a_out = _device_buffers(torch, xy, 4096)
            b_xy, b_out = _device_buffers(torch, xy[1000:], 257)
            stream = torch.cuda.Stream()
            q.run(a_xy, a_out, stream=stream.cuda_stream)
            q.run(b_xy, b_out, n=257, stream=stream.cuda_stream)
            st = q.stats()
            _check_buffer(pt, a_out, want, 4096)
            _check_buffer(pt, b_out, want[1000:], 257)
    assert st["rays"] == 4096 + 257 and st["errors"] == 0 and st["kernel_ms"] > 0.0


def test_features_in_chunks(pt):
    n = pt.FEATS_CHUNK + 5
    path, want, _ = F.expected_centres(DRAGON)
    xy, want = tiled(F.centres(path), want, n, 5)
    with pt.Scene.load(path) as s:
        got, st = s.features(xy)
    F.assert_records(got, want)
    assert st["rays"] == n and st["errors"] == 0


# ---- 6. sessions ------------------------------------------------------------------------------------------
def of_pixels(want, pixels, width):
    """the records of `want` (a frame's centres, row-major) for the (n, 2) pixels"""
    p = np.asarray(pixels).astype(np.int64)
    return want[p[:, 1] * width + p[:, 0]]


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 3), (1, 3), (2, 3)])
def test_a_sessions_features_are_its_pixels_centres(pt, rank, world):
    path, want, _ = F.expected_centres(DRAGON)
    pixels = pt.rank_pixels(64, 64, rank, world)
    with pt.Scene.load(path) as s:
        s.prepare()
        ss = pt.Session(s, rank=rank, world=world)
        assert ss.n_pixels == len(pixels)
        got, st = ss.features(stats=True)
        ss.close()
    F.assert_records(got, of_pixels(want, pixels, 64))
    assert st["rays"] == len(pixels) and st["errors"] == 0


def test_three_ranks_cover_every_pixel_once(pt):
    parts = [pt.rank_pixels(64, 64, r, 3) for r in range(3)]
    every = np.concatenate(parts).astype(np.int64)
    assert len(every) == 4096 and len(np.unique(every[:, 1] * 64 + every[:, 0])) == 4096


def test_a_session_with_edge_tiles(pt):
    name = "mat_camera_23x17x8"
    path, want, _ = F.expected_centres(name)
    pixels = pt.rank_pixels(23, 17, 0, 1)
    with pt.Scene.load(path) as s:
        s.prepare()
        ss = pt.Session(s)
        assert ss.n_pixels == 23 * 17 == len(pixels)
        got = ss.features()
        ss.close()
    assert len(got) == 23 * 17
    F.assert_records(got, of_pixels(want, pixels, 23))


def test_a_windows_features_keep_global_pixels(pt):
    win = (5, 3, 30, 20)
    path, want, _ = F.expected_centres(DRAGON)
    pixels = pt.rank_pixels(win[2], win[3], 0, 1, x0=win[0], y0=win[1])
    with pt.Scene.load(path) as s:
        s.prepare()
        ss = pt.Session(s, window=win)
        assert ss.n_pixels == 600 == len(pixels)
        got = ss.features()
        ss.close()
    F.assert_records(got, of_pixels(want, pixels, 64))


def test_a_cap_one_too_small_is_refused(pt):
    import torch
    path, want, _ = F.expected_centres(DRAGON)
    with pt.Scene.load(path) as s:
        s.prepare()
        ss = pt.Session(s)
        n = ss.n_pixels
        d = torch.full(((n + GUARD) * 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        st = pt.Stats()
        assert pt._lib.pt_session_features(ss._h, pt._addr(d), n - 1, C.byref(st)) == pt.PT_E_INVALID
        host = np.full(n * 64, 0xA5, np.uint8)
        assert pt._lib.pt_session_features_host(ss._h, pt._ptr(host), n - 1, None) == pt.PT_E_INVALID
        assert (d.cpu().numpy() == 0xA5).all() and (host == 0xA5).all()
        # ... and the session still answers, into a buffer with a guard
        ss.features(dev=d)
        _check_buffer(pt, d, of_pixels(want, pt.rank_pixels(64, 64, 0, 1), 64), n)
        ss.close()
        # a session that owns no pixel accepts cap = 0
        empty = pt.Session(s, rank=1, world=2, window=(0, 0, 16, 16))
        assert empty.n_pixels == 0 and len(empty.features()) == 0
        assert pt._lib.pt_session_features(empty._h, None, 0, None) == pt.PT_OK
        empty.close()


def test_an_exact_session_gives_the_same_bytes(pt):
    path, want, _ = F.expected_centres(DRAGON)
    with pt.Scene.load(path) as s:
        s.prepare()
        a = pt.Session(s)
        b = pt.Session(s, traversal=pt.TRAVERSAL_EXACT)
        got_a, got_b = a.features(), b.features()
        a.close()
        b.close()
    assert got_a.tobytes() == got_b.tobytes()
    F.assert_records(got_b, of_pixels(want, pt.rank_pixels(64, 64, 0, 1), 64))


# ---- 7. the session is not disturbed ----------------------------------------------------------------------
def _finish(pt, ss, size):
    import torch
    drad = torch.empty(max(ss.n_tiles, 1) * 256 * 3, dtype=torch.float32, device="cuda")
    ss.resolve(dev_rad=drad.data_ptr())
    ss.sync()
    st = ss.stats()
    assert st["errors"] == 0 and st["short_pixels"] == 0
    rgb = pt.unpack_tiles(ss.read_packed(), size[0], size[1], 0, 1)
    rad = pt.unpack_tiles_f32(drad.cpu().numpy(), size[0], size[1], 0, 1)
    return rgb, rad, st


def test_features_leave_the_session_as_it_was(pt):
    m, path, img, rad = X.golden(DRAGON)
    _, want, _ = F.expected_centres(DRAGON)
    orays = X.oracle_render(path, (0, 0, 64, 64), 16)[2]["rays"]
    with pt.Scene.load(path) as s:
        s.prepare()
        ss, twin = pt.Session(s), pt.Session(s)
        ss.trace(8)
        twin.trace(8)
        got = ss.features()
        # the pass of the trace() above is still pending: nothing ran, and the next trace() joins it
        # (were it flushed here, the session would run two passes of 8 and count other rounds than its twin's
        # one pass of 16 -- compared below, after the same resolve; pt_session_stats itself would flush)
        assert ss.samples_range() == (8, 8)
        ss.trace(8)
        twin.trace(8)
        rgb, r, st = _finish(pt, ss, (64, 64))
        rgb_t, r_t, st_t = _finish(pt, twin, (64, 64))
        again = ss.features()
        assert ss.stats()["rays"] == st["rays"]   # (the features' work is not the session's)
        exp, exp_t = ss.export_states(), twin.export_states()
        ss.close()
        twin.close()
    F.assert_records(got, of_pixels(want, pt.rank_pixels(64, 64, 0, 1), 64))
    assert again.tobytes() == got.tobytes()
    X.assert_bits(r.reshape(-1, 3), rad.reshape(-1, 3), "radiance after features()")
    assert np.array_equal(rgb, img) and np.array_equal(rgb_t, img)
    assert st["rays"] == orays == st_t["rays"]
    assert st["rounds"] == st_t["rounds"] and st["samples"] == st_t["samples"] == 4096 * 16
    assert exp.tobytes() == exp_t.tobytes()


# ---- 8. beside other work, on the scene's one device copy --------------------------------------------------
def test_features_and_a_render_share_the_scene(pt):
    import torch
    m, img, rad = U.golden_image(DRAGON)
    path, want, _ = F.expected_centres(DRAGON)
    xy = F.centres(path)
    with pt.Scene.load(path) as s:
        with pt.FeatureQuery(s, max_points=4096) as q:
            a_xy, a_out = _device_buffers(torch, xy, 4096)
            q.run(a_xy, a_out)
            rgb, r, st = s.render(radiance=True)
            b_xy, b_out = _device_buffers(torch, xy, 4096)
            q.run(b_xy, b_out)
            qs = q.stats()
            _check_buffer(pt, a_out, want, 4096)
            _check_buffer(pt, b_out, want, 4096)
    assert st["errors"] == 0 and np.array_equal(rgb, img)
    assert np.array_equal(r.view(np.uint32), rad.view(np.uint32))
    assert qs["rays"] == 8192 and qs["errors"] == 0


# ---- a context's statistics are those of the runs since the last call -----------------------------
def test_stats_report_each_run_once(pt):
    """Two equal runs of 65 positions (a wave and a lane) on one context, a stats() after each: the second
    reports what the first did -- the context's counters run on, a stats() is the difference since
    the last one --, and a third stats(), with no run since, no work and no time."""
    import torch
    xy = np.array([(k % 13 + 5.5, k // 13 + 9.5) for k in range(65)], np.float32)
    with pt.Scene.load(U.golden_scene_path("mat_matrix_24x24x8")) as s:
        with pt.FeatureQuery(s, max_points=65) as q:
            d_xy, d_out = _device_buffers(torch, xy, 65)
            q.run(d_xy, d_out, n=65)
            a = q.stats()
            q.run(d_xy, d_out, n=65)
            b = q.stats()
            c = q.stats()
    assert a["rays"] == 65 and a["node_visits"] > 0 and a["prim_tests"] > 0 and a["kernel_ms"] > 0.0
    assert (b["rays"], b["node_visits"], b["prim_tests"]) == (a["rays"], a["node_visits"], a["prim_tests"])
    assert c["rays"] == 0 and c["kernel_ms"] == 0
