"""GPU tests of the ray-query engine (k_rays / k_rays_exact through pt_intersect and pt_rayq_*):
Scene::RayIntersection for the caller's rays, bit for bit.

Expected values never come from the code under test: the reference's recorded answers
(trav_*.bin, first block = RayIntersection), the CPU oracle (U.OracleScene.ray_intersection),
and -- for the work counters -- the host execution of the same query state machine
(selftest_ray_intersection(traversal=0)): a ray's step sequence depends on the ray and the scene
only, never on which lane ran it.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _rays as R
import _util as U

pytestmark = pytest.mark.gpu
M = U.manifest()
SCENES = ["dragon_64x64x16", "standin_48x32x4", "hw3s3_48x48x8", "rabbid_48x48x4"]


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


def assert_hits(pt, got, want):
    """ids exactly; hit rows: the bits of t, n and interior; miss rows: all zero apart from id = -1"""
    assert got.dtype == pt.HIT_DTYPE and got.shape == want.shape
    assert np.array_equal(got["id"], want["id"])
    hit = want["id"] != -1
    assert np.array_equal(got["t"][hit].view(np.uint32), want["t"][hit].view(np.uint32))
    assert np.array_equal(got["n"][hit].view(np.uint32), want["n"][hit].view(np.uint32))
    assert np.array_equal(got["interior"][hit], want["interior"][hit])
    miss = np.ascontiguousarray(got[~hit]).view(np.uint32).reshape(-1, 6)
    assert np.array_equal(miss[:, 0], np.full(len(miss), 0xFFFFFFFF, np.uint32)) and not miss[:, 1:].any()


_kat = {}


def kat(pt, name):
    """a traversal fixture: its rays and the reference's recorded RayIntersection answers"""
    if name not in _kat:
        rays, ((ids, f, inter), _) = U.read_trav(name)
        _kat[name] = (rays, R.expected_hits(pt, ids, f, inter))
        for a in _kat[name]:
            a.setflags(write=False)
    return _kat[name]


def oracle_hits(pt, path, rays):
    """the CPU oracle's answers (its ray loop is serial: the rays in parallel pieces)"""
    o = U.OracleScene(path)
    parts = np.array_split(np.arange(len(rays)), 16)
    with ThreadPoolExecutor(16) as ex:
        res = list(ex.map(lambda p: o.ray_intersection(rays[p]), parts))
    ids = np.concatenate([r[0] for r in res])
    h = np.concatenate([r[1] for r in res])
    return R.expected_hits(pt, ids, h[:, :4], h[:, 4])


def tiled(rays, want, n, seed):
    """n rays: the set tiled in a seeded permutation, and the answers indexed the same way"""
    idx = np.random.default_rng(seed).permutation(n) % len(rays)
    return np.ascontiguousarray(rays[idx]), want[idx]


# ---- 1. the reference's recorded answers, and the host's work counters --------------------
@pytest.mark.parametrize("name", sorted(M["trav"]))
def test_kat_matches_the_recorded_answers_and_the_host_counters(pt, name):
    rays, want = kat(pt, name)
    with pt.Scene.load(U.scene_path(M["trav"][name]["scene"])) as s:
        s.prepare()
        _, _, host = s.selftest_ray_intersection(rays, traversal=0)
        got, st = s.intersect(rays)
        n_planes = s.info["n_planes"]
    assert_hits(pt, got, want)
    n = len(rays)
    assert n == 4096 and st["errors"] == 0 and st["rays"] == n and st["plane_tests"] == n * n_planes
    assert (st["node_visits"], st["prim_tests"], st["aux_visits"], st["fallbacks"]) == \
        (host["nodes"], host["prim_tests"], host["aux"], host["fallbacks"])


# ---- 2. BVH-heavy and special rays against the oracle ---------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_bvh_heavy_and_special_rays_match_the_oracle(pt, name):
    path = U.golden_scene_path(name)
    with pt.Scene.load(path) as s:
        s.prepare()
        first, second = R.ray_sets(s)
        n_bvh = s.info["n_bvh_prims"]
        want1, want2 = oracle_hits(pt, path, first), oracle_hits(pt, path, second)
        _, _, host2 = s.selftest_ray_intersection(second, traversal=0)
        # the inputs reach what they are meant to (on the oracle's answers: not plane hits alone)
        bvh_hits = int(((want1["id"] >= 0) & (want1["id"] < n_bvh)).sum())
        plane_hits = int((want1["id"] >= n_bvh).sum())
        misses2 = int((want2["id"] == -1).sum())
        print("%s: BVH hits %d, plane hits %d, misses (second set) %d, host fallbacks %d" %
              (name, bvh_hits, plane_hits, misses2, host2["fallbacks"]))
        assert len(first) == 4096 and len(second) == 2048
        assert bvh_hits >= 300 and plane_hits >= 300 and misses2 >= 32 and host2["fallbacks"] >= 32
        for w in (want1, want2):
            hit = w["id"] != -1
            assert not np.isnan(w["t"][hit]).any() and not np.isnan(w["n"][hit]).any()
        got1, st1 = s.intersect(first)
        got2, st2 = s.intersect(second)
    assert_hits(pt, got1, want1)
    assert_hits(pt, got2, want2)
    assert st1["errors"] == 0 and st2["errors"] == 0
    assert st1["rays"] == 4096 and st2["rays"] == 2048
    # the exact-list tail ran (non-finite rays, and lists full of entered hits)
    assert st2["fallbacks"] >= 32 and st2["fallbacks"] == host2["fallbacks"]
    assert st2["fallbacks_ray"] == 32   # 4 x 8 rays with a non-finite component


# ---- 3. refill: more rays than the chip has lanes -------------------------------------------
def test_refill_more_rays_than_resident_lanes(pt):
    n = (1 << 20) + 37   # > 524,288 = 256 CUs x 2,048 lanes: lanes certainly took a second ray
    rays, want = tiled(*kat(pt, "dragon10k"), n, 3)
    with pt.Scene.load(U.scene_path(M["trav"]["dragon10k"]["scene"])) as s:
        got_a, st_a = s.intersect(rays)
        got_b, st_b = s.intersect(rays)
    assert got_a.tobytes() == got_b.tobytes()
    assert_hits(pt, got_a, want)
    assert st_a["rays"] == n and st_b["rays"] == n and st_a["errors"] == 0 and st_b["errors"] == 0


# ---- 4. edges of a wave and of the output buffer --------------------------------------------
def _device_buffers(torch, rays, n):
    d_rays = torch.from_numpy(np.array(rays[:n])).cuda()   # (a copy: the shared rays are read-only)
    d_hits = torch.full(((n + 64) * 24,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return d_rays, d_hits


def _check_buffer(pt, d_hits, want, n):
    raw = d_hits.cpu().numpy()
    assert (raw[n * 24:] == 0xA5).all(), "the run wrote past its n records"
    assert_hits(pt, raw[:n * 24].view(pt.HIT_DTYPE), want[:n])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_wave_edges_on_device_tensors(pt, n):
    import torch
    rays, want = kat(pt, "dragon10k")
    with pt.Scene.load(U.scene_path(M["trav"]["dragon10k"]["scene"])) as s:
        with pt.RayQuery(s, max_rays=512) as q:
            d_rays, d_hits = _device_buffers(torch, rays, n)
            q.run(d_rays, d_hits)
            st = q.stats()
            _check_buffer(pt, d_hits, want, n)
    assert st["rays"] == n and st["errors"] == 0


def test_run_refuses_more_than_max_rays(pt):
    import torch
    rays, _ = kat(pt, "dragon10k")
    with pt.Scene.load(U.scene_path(M["trav"]["dragon10k"]["scene"])) as s:
        with pt.RayQuery(s, max_rays=64) as q:
            d_rays, d_hits = _device_buffers(torch, rays, 65)
            with pytest.raises(pt.PTError) as e:
                q.run(d_rays, d_hits)
            assert e.value.code == pt.PT_E_INVALID
            assert (d_hits.cpu().numpy() == 0xA5).all()
            assert q.stats()["rays"] == 0


def test_two_runs_back_to_back_on_one_stream(pt):
    import torch
    rays, want = kat(pt, "dragon10k")
    with pt.Scene.load(U.scene_path(M["trav"]["dragon10k"]["scene"])) as s:
        with pt.RayQuery(s, max_rays=4096) as q:
            a_rays, a_hits = _device_buffers(torch, rays, 4096)
            b_rays, b_hits = _device_buffers(torch, rays[1000:], 257)
            stream = torch.cuda.Stream()
            q.run(a_rays, a_hits, stream=stream.cuda_stream)
            q.run(b_rays, b_hits, stream=stream.cuda_stream)
            st = q.stats()
            _check_buffer(pt, a_hits, want, 4096)
            _check_buffer(pt, b_hits, want[1000:], 257)
    assert st["rays"] == 4096 + 257 and st["errors"] == 0 and st["kernel_ms"] > 0.0


# ---- 5. chunks ----------------------------------------------------------------------------------
def test_intersect_in_chunks(pt):
    n = pt.RAYS_CHUNK + 5
    rays, want = tiled(*kat(pt, "dragon10k"), n, 5)
    with pt.Scene.load(U.scene_path(M["trav"]["dragon10k"]["scene"])) as s:
        got, st = s.intersect(rays)
    assert_hits(pt, got, want)
    assert st["rays"] == n and st["errors"] == 0


# ---- 6. beside a render, on the scene's one device copy ---------------------------------------
def test_queries_and_a_render_share_the_scene(pt):
    import torch
    name = "dragon_64x64x16"
    m, img, rad = U.golden_image(name)
    path = U.golden_scene_path(name)
    with pt.Scene.load(path) as s:
        s.prepare()
        rays, _ = R.ray_sets(s)
        rays = rays[:1024]
        want = oracle_hits(pt, path, rays)
        with pt.RayQuery(s, max_rays=1024) as q:
            a_rays, a_hits = _device_buffers(torch, rays, 1024)
            q.run(a_rays, a_hits)
            rgb, r, st = s.render(radiance=True)
            b_rays, b_hits = _device_buffers(torch, rays, 1024)
            q.run(b_rays, b_hits)
            qs = q.stats()
            _check_buffer(pt, a_hits, want, 1024)
            _check_buffer(pt, b_hits, want, 1024)
    assert st["errors"] == 0 and np.array_equal(rgb, img)
    assert np.array_equal(r.view(np.uint32), rad.view(np.uint32))
    assert qs["rays"] == 2048 and qs["errors"] == 0


# ---- 7. a context's statistics are those of the runs since the last call ------------------------
def test_stats_report_each_run_once(pt):
    """Two equal runs of 65 rays (a wave and a lane) on one context, a stats() after each: the second
    reports what the first did -- the context's counters run on, a stats() is the difference since
    the last one --, and a third stats(), with no run since, no work and no time."""
    import torch
    with pt.Scene.load(U.golden_scene_path("mat_matrix_24x24x8")) as s:
        rays = s.camera_rays(np.array([(k % 13 + 5.5, k // 13 + 9.5) for k in range(65)], np.float32))
        with pt.RayQuery(s, max_rays=65) as q:
            d_rays, d_hits = _device_buffers(torch, rays, 65)
            q.run(d_rays, d_hits)
            a = q.stats()
            q.run(d_rays, d_hits)
            b = q.stats()
            c = q.stats()
    assert a["rays"] == 65 and a["node_visits"] > 0 and a["prim_tests"] > 0 and a["kernel_ms"] > 0.0
    assert (b["rays"], b["node_visits"], b["prim_tests"]) == (a["rays"], a["node_visits"], a["prim_tests"])
    assert c["rays"] == 0 and c["kernel_ms"] == 0
