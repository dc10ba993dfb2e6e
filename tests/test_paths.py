"""GPU tests of the batch radiance engine (k_paths through pt_radiance and pt_pathq_*):
Scene::RayTrace for the caller's rays, bit for bit.

Expected values never come from the code under test: the CPU oracle's one-sample render of the
pixel a record was built from (tests/_paths.py), the untouched reference's recorded radiance of
SAMPLES-1 scenes (rad_s1_*.f32), and -- for the work counters and for rays that are no camera
rays -- the host execution of the same vertex, fold and query code (selftest_paths_host): a
path's steps depend on its ray, its seed and the scene only, never on which lane ran it.
"""
import os

import numpy as np
import pytest

import _paths as P
import _rays as R
import _util as U

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "node_visits", "prim_tests", "aux_visits", "fallbacks", "fallbacks_ray")
DRAGON = "dragon_glass_64x64x8"
DEPTH0 = ("DIMENSIONS 8 6\nRAY_DEPTH 0\nSAMPLES 1\nBG_COLOR 0.2 0.3 0.4\nCAMERA_POSITION 0 0 4\nCAMERA_RIGHT 1 0 0\n"
          "CAMERA_UP 0 1 0\nCAMERA_FORWARD 0 0 -1\nCAMERA_FOV_X 1.2\nNEW_PRIMITIVE\nBOX 0.5 0.5 0.5\nCOLOR 1 0 0\n"
          "NEW_PRIMITIVE\nELLIPSOID 0.3 0.3 0.3\nPOSITION 1 0 0\nEMISSION 2 2 2\n")


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


def counters(st):
    return tuple(st[k] for k in COUNTERS)


def tiled(e, n, seed):
    """n records: a fixture's records tiled in a seeded permutation, and the oracle's radiance and
    the per-record ray counts' total indexed the same way"""
    idx = np.random.default_rng(seed).permutation(n) % len(e["records"])
    return np.ascontiguousarray(e["records"][idx]), np.ascontiguousarray(e["rad"][idx]), idx


# ---- 1. the oracle, and the host's work counters ------------------------------------------------
@pytest.mark.parametrize("name", P.FRAMES + P.WINDOWS)
def test_radiance_matches_the_oracle_and_the_host_counters(pt, name):
    e = P.expected(pt, name)
    _, host = P.host_run(pt, name, e["path"], e["records"])
    with pt.Scene.load(e["path"]) as s:
        got, st = s.radiance(e["records"])
    P.assert_radiance(got, e["rad"])
    assert int(got["rays"].sum()) == e["rays"] and (got["rays"] >= 1).all()
    assert st["errors"] == 0 and st["rays"] == e["rays"]
    assert counters(st) == counters(host)


# ---- 2. the untouched reference's SAMPLES-1 radiance ---------------------------------------------
@pytest.mark.parametrize("name", sorted(P.S1))
def test_radiance_matches_the_reference_at_one_sample(pt, name):
    m = P.paths_manifest()["radiance"][name]
    raw = open(os.path.join(U.GOLDEN, "rad_s1_%s.f32" % name), "rb").read()
    assert U.md5(raw) == m["rad_md5"]
    want = np.frombuffer(raw, np.float32).reshape(-1, 3)
    path = P.s1_scene(name)
    assert U.md5(open(path, "rb").read()) == m["scene_md5"]
    with pt.Scene.load(path) as s:
        rec = P.pixel_records(pt, s, m["width"], (0, 0, m["width"], m["height"]))
        got, st = s.radiance(rec)
    assert len(want) == len(rec) and (want != 0).any(axis=1).sum() * 2 >= len(want)
    P.assert_radiance(got, want)
    assert st["errors"] == 0 and st["rays"] == int(got["rays"].sum()) > len(rec)


# ---- 3. rays that are no camera rays ---------------------------------------------------------------
def scene_background(path):
    bg = None
    with open(path) as f:
        for line in f:
            w = line.split()
            if w and w[0] == "BG_COLOR":
                bg = np.array([float(v) for v in w[1:4]], np.float32)
    assert bg is not None
    return bg


@pytest.mark.parametrize("name", ["dragon_64x64x16", "standin_48x32x4"])
def test_bvh_heavy_and_special_rays_match_the_host_execution(pt, name):
    path = U.golden_scene_path(name)
    bg = scene_background(path)
    o = U.OracleScene(path)
    with pt.Scene.load(path) as s:
        s.prepare()
        for k, rays in enumerate(R.ray_sets(s)):
            rec = np.zeros(len(rays), pt.PATH_DTYPE)
            rec["o"], rec["d"], rec["seed"] = rays[:, :3], rays[:, 3:], np.arange(len(rays))
            want, host = s.selftest_paths_host(rec)
            got, st = s.radiance(rec)
            assert got.tobytes() == want.tobytes()
            assert st["errors"] == 0 and host["errors"] == 0 and counters(st) == counters(host)
            assert st["plane_tests"] == host["plane_tests"]
            # a ray the oracle's RayIntersection misses returns the background after its one query
            miss = o.ray_intersection(rays)[0] == -1
            print("%s set %d: %d misses, fallbacks %d (non-finite rays %d)" %
                  (name, k, miss.sum(), st["fallbacks"], st["fallbacks_ray"]))
            assert (got["rgb"][miss].view(np.uint32) == bg.view(np.uint32)).all() and (got["rays"][miss] == 1).all()
            if k == 1:
                assert miss.sum() >= 32
                # 32 rays with a non-finite component; child rays may add more
                assert st["fallbacks"] >= 32 and st["fallbacks_ray"] >= 32


# ---- 4. refill: more paths than the chip has lanes -----------------------------------------------
def test_refill_more_paths_than_resident_lanes(pt):
    n = (1 << 20) + 37   # > 524,288 = 256 CUs x 2,048 lanes: lanes certainly took a second path
    e = P.expected(pt, DRAGON)
    rec, want, idx = tiled(e, n, 3)
    rays = int(P.host_run(pt, DRAGON, e["path"], e["records"])[0]["rays"][idx].sum())
    with pt.Scene.load(e["path"]) as s:
        got_a, st_a = s.radiance(rec)
        got_b, st_b = s.radiance(rec)
    assert got_a.tobytes() == got_b.tobytes()
    P.assert_radiance(got_a, want)
    assert st_a["rays"] == st_b["rays"] == rays == int(got_a["rays"].sum())
    assert st_a["errors"] == 0 and st_b["errors"] == 0


# ---- 5. edges of a wave and of the buffers ---------------------------------------------------------
def _device_buffers(torch, rec, n):
    """n records at the front of an input buffer, and an output buffer, both filled with 0xA5 first"""
    d_in = torch.full(((n + 64) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
    d_in[:n * 32] = torch.from_numpy(np.array(rec[:n]).view(np.uint8)).cuda()
    d_out = torch.full(((n + 64) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return d_in, d_out


def _check_buffers(pt, d_in, d_out, rec, want_rad, n):
    raw_in, raw = d_in.cpu().numpy(), d_out.cpu().numpy()
    assert (raw[n * 16:] == 0xA5).all(), "the run wrote past its n records"
    assert raw_in[:n * 32].tobytes() == rec[:n].tobytes() and (raw_in[n * 32:] == 0xA5).all(), "the run wrote its input"
    got = raw[:n * 16].view(pt.RADIANCE_DTYPE)
    P.assert_radiance(got, want_rad[:n])
    return got


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_wave_edges_on_device_tensors(pt, n):
    import torch
    e = P.expected(pt, DRAGON)
    host = P.host_run(pt, DRAGON, e["path"], e["records"])[0]
    with pt.Scene.load(e["path"]) as s:
        with pt.PathQuery(s, max_paths=512) as q:
            d_in, d_out = _device_buffers(torch, e["records"], n)
            q.run(d_in, d_out, n=n)
            st = q.stats()
            got = _check_buffers(pt, d_in, d_out, e["records"], e["rad"], n)
    assert st["rays"] == int(host["rays"][:n].sum()) == int(got["rays"].sum()) and st["errors"] == 0


# ---- 6. run rules ------------------------------------------------------------------------------------
def test_run_refuses_more_than_max_paths(pt):
    import torch
    e = P.expected(pt, DRAGON)
    with pt.Scene.load(e["path"]) as s:
        with pt.PathQuery(s, max_paths=64) as q:
            d_in, d_out = _device_buffers(torch, e["records"], 65)
            with pytest.raises(pt.PTError) as err:
                q.run(d_in, d_out, n=65)
            assert err.value.code == pt.PT_E_INVALID
            assert (d_out.cpu().numpy() == 0xA5).all()
            assert q.stats()["rays"] == 0


def test_two_runs_back_to_back_on_one_stream(pt):
    import torch
    e = P.expected(pt, DRAGON)
    rec, rad = e["records"], e["rad"]
    host = P.host_run(pt, DRAGON, e["path"], rec)[0]
    with pt.Scene.load(e["path"]) as s:
        with pt.PathQuery(s, max_paths=4096) as q:
            a_in, a_out = _device_buffers(torch, rec, 4096)
            b_in, b_out = _device_buffers(torch, rec[1000:], 257)
            stream = torch.cuda.Stream()
            q.run(a_in, a_out, n=4096, stream=stream.cuda_stream)
            q.run(b_in, b_out, n=257, stream=stream.cuda_stream)
            st = q.stats()
            _check_buffers(pt, a_in, a_out, rec, rad, 4096)
            _check_buffers(pt, b_in, b_out, rec[1000:], rad[1000:], 257)
    assert st["rays"] == int(host["rays"].sum()) + int(host["rays"][1000:1257].sum())
    assert st["errors"] == 0 and st["kernel_ms"] > 0.0


def test_radiance_in_chunks(pt):
    n = pt.PATHS_CHUNK + 5
    e = P.expected(pt, "hw3s3_48x48x8")
    rec, want, idx = tiled(e, n, 5)
    rays = int(P.host_run(pt, "hw3s3_48x48x8", e["path"], e["records"])[0]["rays"][idx].sum())
    with pt.Scene.load(e["path"]) as s:
        got, st = s.radiance(rec)
    P.assert_radiance(got, want)
    assert st["rays"] == rays == int(got["rays"].sum()) and st["errors"] == 0


# ---- 7. the service threshold changes when work is done, never what is computed ---------------------
@pytest.mark.parametrize("name", ["mat_matrix_24x24x8", DRAGON])
def test_paths_service_does_not_change_the_answers(pt, name, monkeypatch):
    e = P.expected(pt, name)
    _, host = P.host_run(pt, name, e["path"], e["records"])
    with pt.Scene.load(e["path"]) as s:
        for service in (1, 8, 64):
            monkeypatch.setenv("PT_TUNE", "paths_service=%d" % service)   # read when the context is made
            got, st = s.radiance(e["records"])
            P.assert_radiance(got, e["rad"])
            assert int(got["rays"].sum()) == e["rays"]
            assert st["errors"] == 0 and counters(st) == counters(host), service


# ---- 8. beside a render, on the scene's one device copy -------------------------------------------
def test_paths_and_a_render_share_the_scene(pt):
    import torch
    m, img, rad = U.golden_image(DRAGON)
    e = P.expected(pt, DRAGON)
    rec = e["records"]
    with pt.Scene.load(e["path"]) as s:
        with pt.PathQuery(s, max_paths=4096) as q:
            a_in, a_out = _device_buffers(torch, rec, 4096)
            q.run(a_in, a_out, n=4096)
            rgb, r, st = s.render(radiance=True)
            b_in, b_out = _device_buffers(torch, rec, 4096)
            q.run(b_in, b_out, n=4096)
            qs = q.stats()
            _check_buffers(pt, a_in, a_out, rec, e["rad"], 4096)
            _check_buffers(pt, b_in, b_out, rec, e["rad"], 4096)
    assert st["errors"] == 0 and np.array_equal(rgb, img)
    assert np.array_equal(r.view(np.uint32), rad.view(np.uint32))
    assert qs["rays"] == 2 * e["rays"] and qs["errors"] == 0


# ---- 9. RAY_DEPTH 0 ------------------------------------------------------------------------------------
def test_ray_depth_0_gives_zeros_and_no_rays(pt):
    with pt.Scene.loads(DEPTH0) as s:
        rec = np.zeros(300, pt.PATH_DTYPE)
        rec["o"], rec["d"], rec["seed"] = (0.0, 0.0, 4.0), (0.0, 0.0, -1.0), np.arange(300)
        got, st = s.radiance(rec)
    assert not got.view(np.uint32).any()
    assert st["rays"] == 0 and st["errors"] == 0


# ---- a context's statistics are those of the runs since the last call -----------------------------
def test_stats_report_each_run_once(pt):
    """Two equal runs of 65 paths (a wave and a lane) on one context, a stats() after each: the second
    reports what the first did -- the context's counters run on, a stats() is the difference since
    the last one --, and a third stats(), with no run since, no work and no time."""
    import torch
    with pt.Scene.load(U.golden_scene_path("mat_matrix_24x24x8")) as s:
        rec = P.pixel_records(pt, s, 24, (5, 9, 13, 5))
        with pt.PathQuery(s, max_paths=65) as q:
            d_in, d_out = _device_buffers(torch, rec, 65)
            q.run(d_in, d_out, n=65)
            a = q.stats()
            q.run(d_in, d_out, n=65)
            b = q.stats()
            c = q.stats()
    assert a["rays"] >= 65 and a["node_visits"] > 0 and a["prim_tests"] > 0 and a["kernel_ms"] > 0.0
    assert (b["rays"], b["node_visits"], b["prim_tests"]) == (a["rays"], a["node_visits"], a["prim_tests"])
    assert c["rays"] == 0 and c["kernel_ms"] == 0
