"""GPU tests of the guided filter (k_filter_guides / k_filter through pt_filter and pt_filtq_*): a
feature-guided a-trous denoise of a frame, byte for byte.

Expected values never come from the code under test (tests/_filter.py): the definition restated in numpy
float32 over tests/_features.py's records and the committed radiance fixtures.  The host mirror
(tests/test_filter_host.py) is compared as well.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _features as F
import _filter as FL
import _util as U

pytestmark = pytest.mark.gpu
DRAGON = "dragon_64x64x16"
GUARD = 4096   # bytes of 0xA5 behind a device buffer
PT_E_INVALID = -1


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


def guarded(torch, nbytes):
    t = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return t


def frame_of(t, h, w):
    raw = t.cpu().numpy()
    assert (raw[h * w * 12:] == 0xA5).all(), "the run wrote past its frame"
    return raw[:h * w * 12].view(np.float32).reshape(h, w, 3)


def bytes_of(t, h, w):
    raw = t.cpu().numpy()
    assert (raw[h * w * 3:] == 0xA5).all(), "the run wrote past its image"
    return raw[:h * w * 3].reshape(h, w, 3)


def tonemapped(rad):
    return U.oracle_tonemap(rad).reshape(rad.shape)


# ---- 1. the fixtures, through the host-pointer form and through a context on device tensors --------------
@pytest.mark.parametrize("levels", FL.LEVELS)
@pytest.mark.parametrize("name", FL.SCENES)
def test_fixtures_match_the_restatement_and_the_host_mirror(pt, name, levels):
    import torch
    path, feat = FL.scene_features(name)
    want, census = FL.expected_scene(name, levels=levels)
    FL.print_census("%s levels %d" % (name, levels), census)
    rad = FL.poisoned(name)
    h, w = rad.shape[:2]
    mirror = pt.selftest_filter_host(feat, rad, w, h, levels=levels)
    with pt.Scene.load(path) as s:
        got, rgb = s.filter(rad, rgb=True, levels=levels)
        with pt.FilterQuery(s) as q:
            made = q.stats()
            d_in = torch.from_numpy(rad).cuda()
            d_out, d_rgb = guarded(torch, h * w * 12), guarded(torch, h * w * 3)
            q.run(d_in, d_out, d_rgb, levels=levels)
            st = q.stats()
            got_q, rgb_q = frame_of(d_out, h, w), bytes_of(d_rgb, h, w)
    FL.assert_frames(got, want, "Scene.filter")
    FL.assert_frames(got_q, want, "FilterQuery")
    FL.assert_frames(got, mirror, "host mirror")
    assert np.array_equal(rgb, tonemapped(want)) and np.array_equal(rgb_q, rgb)
    assert made["rays"] == w * h and st["rays"] == 0 and st["kernel_ms"] > 0 and st["errors"] == 0


# ---- 2. synthetic frames through set_features --------------------------------------------------------------
@pytest.fixture(scope="module")
def wide_scene(pt):
    # (any scene whose image holds the largest synthetic frame: its own guides are replaced)
    with pt.Scene.load(U.scene_path("hw3_sample4.txt", (96, 48, 1, False, "diffuse"))) as s:
        yield s


@pytest.mark.parametrize("size", FL.SYNTH_SIZES)
def test_synthetic_frames_through_set_features(pt, wide_scene, size):
    import torch
    w, h = size
    feat, rad = FL.synthetic(pt, w, h)
    d_feat = torch.from_numpy(np.ascontiguousarray(feat).view(np.uint8).reshape(-1)).cuda()
    d_in = torch.from_numpy(rad).cuda()
    assert d_feat.data_ptr() % 16 == 0
    with pt.FilterQuery(wide_scene, window=(3, 2, w, h)) as q:
        q.set_features(d_feat)
        for o in ({"levels": 1}, {"levels": 4}, {"levels": 8, "sigma_c": 2.5, "normal_pow2": 1},
                  {"levels": 2, "sigma_z": 0.0, "normal_pow2": 8}, {"levels": 2, "sigma_c": 0.0, "sigma_a": 0.0, "normal_pow2": 0}):
            want, _ = FL.filtered(feat, rad, **o)
            d_out, d_rgb = guarded(torch, h * w * 12), guarded(torch, h * w * 3)
            q.run(d_in, d_out, d_rgb, **o)
            q.stats()
            FL.assert_frames(frame_of(d_out, h, w), want, "%dx%d %s" % (w, h, o))
            assert np.array_equal(bytes_of(d_rgb, h, w), tonemapped(want))
        # without rgb
        d_out = guarded(torch, h * w * 12)
        q.run(d_in, d_out, None, levels=4)
        q.stats()
        FL.assert_frames(frame_of(d_out, h, w), FL.filtered(feat, rad, levels=4)[0], "no rgb")


# ---- 3. a window: the guides are those of the global pixel centres ---------------------------------------
def test_window_uses_global_centres(pt):
    x0, y0, w, h = 13, 9, 37, 41
    path, feat = FL.scene_features(DRAGON)
    rad = np.ascontiguousarray(FL.poisoned(DRAGON)[y0:y0 + h, x0:x0 + w])
    fw = feat[y0:y0 + h, x0:x0 + w]
    want, census = FL.filtered(fw, rad)
    FL.print_census("window", census)
    elsewhere, _ = FL.filtered(feat[:h, :w], rad)
    assert want.tobytes() != elsewhere.tobytes()   # (the window's guides differ from the corner's)
    with pt.Scene.load(path) as s:
        got = s.filter(rad, window=(x0, y0, w, h))
        for bad in ((60, 0, 5, 5), (0, 60, 5, 5), (0, 0, 65, 1), (0, 0, 5, 0)):
            with pytest.raises(pt.PTError) as e:
                pt.FilterQuery(s, window=bad)
            assert e.value.code == PT_E_INVALID
    FL.assert_frames(got, want, "window")


# ---- 4. a session's packed radiance as the input ---------------------------------------------------------
@pytest.mark.parametrize("name,window", [(DRAGON, None), ("mat_camera_23x17x8", None), (DRAGON, (13, 9, 37, 41))])
def test_tile_layout_reads_a_session_resolve(pt, name, window):
    import torch
    path, feat = FL.scene_features(name)
    W, H = F.dims(path)
    x0, y0, w, h = window or (0, 0, W, H)
    fw = feat[y0:y0 + h, x0:x0 + w]
    with pt.Scene.load(path) as s:
        s.prepare()
        ses = pt.Session(s, window=window)
        try:
            d_rad = torch.zeros(ses.n_tiles * 256 * 3, dtype=torch.float32, device="cuda")
            ses.trace(4)
            ses.resolve(None, d_rad.data_ptr())
            ses.sync()
            packed = d_rad.cpu().numpy()
            rows = pt.unpack_tiles_f32(packed, w, h, 0, 1)
            with pt.FilterQuery(s, window=window) as q:
                d_a, d_b = guarded(torch, h * w * 12), guarded(torch, h * w * 12)
                d_rows = torch.from_numpy(rows).cuda()
                q.run(d_rad, d_a, layout=pt.FILTER_TILES)
                q.run(d_rows, d_b)
                q.stats()
                a, b = frame_of(d_a, h, w), frame_of(d_b, h, w)
        finally:
            ses.close()
    want, _ = FL.filtered(fw, rows.reshape(h, w, 3))
    FL.assert_frames(a, b, "tiles against row-major")
    FL.assert_frames(a, want, "tiles")
    assert a.tobytes() != rows.tobytes()


# ---- 5. ordering ---------------------------------------------------------------------------------------------
def test_two_runs_back_to_back_and_repeats(pt):
    import torch
    path, feat = FL.scene_features(DRAGON)
    rad = FL.poisoned(DRAGON)
    h, w = rad.shape[:2]
    want3, _ = FL.expected_scene(DRAGON, levels=3)
    want2, _ = FL.filtered(feat, rad, levels=2, sigma_c=0.5, normal_pow2=2)
    with pt.Scene.load(path) as s:
        with pt.FilterQuery(s) as q:
            d_in = torch.from_numpy(rad).cuda()
            outs = [guarded(torch, h * w * 12) for _ in range(4)]
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            q.run(d_in, outs[0], stream=stream.cuda_stream, levels=3)
            q.run(d_in, outs[1], stream=stream.cuda_stream, levels=2, sigma_c=0.5, normal_pow2=2)
            q.run(d_in, outs[2], stream=stream.cuda_stream, levels=3)
            q.run(d_in, outs[3], stream=stream.cuda_stream, levels=2, sigma_c=0.5, normal_pow2=2)
            st = q.stats()
            stream.synchronize()
            got = [frame_of(o, h, w) for o in outs]
    assert st["kernel_ms"] > 0
    FL.assert_frames(got[0], want3, "first run")
    FL.assert_frames(got[1], want2, "second run")
    assert got[2].tobytes() == got[0].tobytes() and got[3].tobytes() == got[1].tobytes()


# ---- 6. refusals ---------------------------------------------------------------------------------------------
def test_refusals_write_nothing(pt):
    import torch
    lib = pt._lib
    path, _ = FL.scene_features(DRAGON)
    rad = FL.poisoned(DRAGON)
    h, w = rad.shape[:2]
    n = h * w
    with pt.Scene.load(path) as s:
        with pt.FilterQuery(s) as q:
            d_in = torch.from_numpy(rad).cuda()
            d_out, d_rgb = guarded(torch, n * 12), guarded(torch, n * 3)
            ok = pt.FilterOpts.default()

            def run(o, i=d_in.data_ptr(), out=d_out.data_ptr(), rgb=d_rgb.data_ptr()):
                return lib.pt_filtq_run(q._h, None, C.byref(o) if o is not None else None, i, out, rgb)

            for o in (pt.FilterOpts.default(levels=0), pt.FilterOpts.default(levels=9), pt.FilterOpts.default(sigma_c=-1.0),
                      pt.FilterOpts.default(sigma_z=float("nan")), pt.FilterOpts.default(sigma_a=-0.25),
                      pt.FilterOpts.default(normal_pow2=9), pt.FilterOpts.default(layout=2)):
                assert run(o) == PT_E_INVALID, o.as_dict()
            assert run(None) == PT_E_INVALID
            assert run(ok, i=None) == PT_E_INVALID and run(ok, out=None) == PT_E_INVALID
            # unaligned; ranges that overlap: in with out (either end), rgb with out, rgb with in
            assert run(ok, i=d_in.data_ptr() + 2) == PT_E_INVALID
            assert run(ok, out=d_in.data_ptr()) == PT_E_INVALID
            assert run(ok, out=d_in.data_ptr() + n * 12 - 4) == PT_E_INVALID
            assert run(ok, i=d_out.data_ptr() + 8) == PT_E_INVALID
            assert run(ok, rgb=d_out.data_ptr() + 16) == PT_E_INVALID
            assert run(ok, rgb=d_in.data_ptr() + n * 12 - 1) == PT_E_INVALID
            assert lib.pt_filtq_set_features(q._h, None, None) == PT_E_INVALID
            assert lib.pt_filtq_set_features(q._h, None, d_in.data_ptr() + 4) == PT_E_INVALID
            st = q.stats()
            torch.cuda.synchronize()
            assert st["kernel_ms"] == 0   # nothing was enqueued
            assert (d_out.cpu().numpy() == 0xA5).all() and (d_rgb.cpu().numpy() == 0xA5).all()
            assert d_in.cpu().numpy().tobytes() == rad.tobytes()
            # adjoining ranges are fine
            both = guarded(torch, n * 24)
            both[:n * 12] = d_in.view(torch.uint8).reshape(-1)
            assert run(ok, i=both.data_ptr(), out=both.data_ptr() + n * 12, rgb=None) == pt.PT_OK
            q.stats()
            want, _ = FL.expected_scene(DRAGON, levels=3)
            raw = both.cpu().numpy()
            assert (raw[n * 24:] == 0xA5).all()
            FL.assert_frames(raw[n * 12:n * 24].view(np.float32).reshape(h, w, 3), want, "adjoining")


# ---- 7. the CLI ----------------------------------------------------------------------------------------------
def test_cli_filter_switch(pt, tmp_path):
    name = "standin_48x32x4"
    m, img, rad = U.golden_image(name)
    path, feat = FL.scene_features(name)
    want, _ = FL.filtered(feat, rad, levels=3)
    exe = U.os.path.join(U.PKG, "build", "pt_render")
    outs = {}
    for tag, env in (("unset", {}), ("zero", {"PT_FILTER": "0"}), ("three", {"PT_FILTER": "3"})):
        out = tmp_path / ("%s.ppm" % tag)
        e = {k: v for k, v in U.os.environ.items() if k != "PT_FILTER"}
        r = subprocess.run([exe, path, str(out)], capture_output=True, text=True, timeout=120, env=dict(e, PT_QUIET="1", **env))
        assert r.returncode == 0, r.stderr
        outs[tag] = out.read_bytes()
    golden = tmp_path / "golden.ppm"
    pt.write_ppm(str(golden), img)
    assert outs["unset"] == outs["zero"] == golden.read_bytes()
    expect = tmp_path / "expect.ppm"
    pt.write_ppm(str(expect), tonemapped(want))
    assert outs["three"] == expect.read_bytes() and outs["three"] != outs["unset"]
    # levels outside 1..8: the library's refusal, no image
    out = tmp_path / "bad.ppm"
    r = subprocess.run([exe, path, str(out)], capture_output=True, text=True, timeout=120,
                       env=dict(U.os.environ, PT_QUIET="1", PT_FILTER="9"))
    assert r.returncode == 1 and "filter options" in r.stderr and not out.exists()
