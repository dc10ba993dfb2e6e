"""Materials on every primitive kind, and rays on the primitives' edges, on the GPU.

The scenes of _material_scenes.py -- glass and metal on boxes, ellipsoids, moved and rotated
triangles and planes, IOR 0.7 / 1.0 / 1.5 / 2.4, a metallic emitter, the camera inside a glass
box inside a glass ellipsoid, a skew camera at 23 x 17 pixels -- in every engine that runs the
vertex step (test_light_sampling.py's ENGINES) and with almost every query suspended
(budget=1): the reference's recorded image bytes and radiance bits, no errors, and the CPU
oracle's ray count.  test_materials_host.py shows on the oracle that the scenes reach the
specular branches of shade_vertex_e on every primitive kind and side.  (test_gpu.py's
batteries over manifest["images"] run the same fixtures under 3 traversals and 7 engines.)

The edge rays -- through box corners and along box edges, tangent to the ellipsoids, starting
on surfaces, in and parallel to the planes, at t on both sides of the plane test's 1e5, at the
vertices and edges of the triangles and of their copies on the plane through the origin --
through both entry points of the ray query: the reference's recorded answers, and the work
counters of the same query run on the host.
"""
import numpy as np
import pytest

import _material_scenes as MS
import _rays as R
import _util as U
from test_light_sampling import ENGINES

pytestmark = pytest.mark.gpu

FIXTURE = {"matrix": "mat_matrix_24x24x8", "inside": "mat_inside_24x24x8", "camera": "mat_camera_23x17x8"}
TUNES = dict(ENGINES, budget1="budget=1,sparse=100000000,coop=0")


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


_oracle_rays = {}   # scene -> the oracle's ray count: rendered once


@pytest.mark.parametrize("engine", sorted(TUNES))
@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_material_scene_bit_exact(pt, name, engine, monkeypatch):
    if TUNES[engine]:
        monkeypatch.setenv("PT_TUNE", TUNES[engine])
    m, img, rad = U.golden_image(FIXTURE[name])
    path = U.scene_path(MS.PREFIX + name)
    if name not in _oracle_rays:
        _, orad, octr = U.OracleScene(path).render()
        assert np.array_equal(orad.view(np.uint32), rad.view(np.uint32))
        _oracle_rays[name] = octr["rays"]
    with pt.Scene.load(path) as s:
        rgb, r, st = s.render(radiance=True)
    assert st["errors"] == 0
    assert r.view(np.uint32).tolist() == rad.view(np.uint32).tolist()
    assert np.array_equal(rgb, img)
    assert st["rays"] == _oracle_rays[name]
    if engine == "budget1":
        assert st["rounds"] > 0


_edges = {}


def edges(pt):
    """the edge rays, the reference's recorded RayIntersection answers, and the host's counters"""
    if not _edges:
        rays, ((ids, f, inter), _) = U.read_trav("edges")
        want = R.expected_hits(pt, ids, f, inter)
        with pt.Scene.load(U.scene_path(MS.PREFIX + "edges")) as s:
            s.prepare()
            _, _, host = s.selftest_ray_intersection(rays, traversal=0)
            n_planes = s.info["n_planes"]
        for a in (rays, want):
            a.setflags(write=False)
        _edges["v"] = (rays, want, host, n_planes)
    return _edges["v"]


def assert_hits(pt, got, want):
    """test_rays.py's rules: ids exactly; hit rows: the bits of t, n and interior; miss rows: all
    zero apart from id = -1"""
    assert got.dtype == pt.HIT_DTYPE and got.shape == want.shape
    assert np.array_equal(got["id"], want["id"])
    hit = want["id"] != -1
    assert np.array_equal(got["t"][hit].view(np.uint32), want["t"][hit].view(np.uint32))
    assert np.array_equal(got["n"][hit].view(np.uint32), want["n"][hit].view(np.uint32))
    assert np.array_equal(got["interior"][hit], want["interior"][hit])
    miss = np.ascontiguousarray(got[~hit]).view(np.uint32).reshape(-1, 6)
    assert np.array_equal(miss[:, 0], np.full(len(miss), 0xFFFFFFFF, np.uint32)) and not miss[:, 1:].any()


def assert_counters(st, host, n, n_planes):
    assert st["errors"] == 0 and st["rays"] == n and st["plane_tests"] == n * n_planes
    assert (st["node_visits"], st["prim_tests"], st["aux_visits"], st["fallbacks"]) == \
        (host["nodes"], host["prim_tests"], host["aux"], host["fallbacks"])


def test_edge_rays_through_intersect(pt):
    rays, want, host, n_planes = edges(pt)
    with pt.Scene.load(U.scene_path(MS.PREFIX + "edges")) as s:
        got, st = s.intersect(rays)
    assert_hits(pt, got, want)
    assert_counters(st, host, len(rays), n_planes)


@pytest.mark.parametrize("n", [1, 63, 65, 4096])
def test_edge_rays_through_ray_query(pt, n):
    import torch
    rays, want, host, n_planes = edges(pt)
    with pt.Scene.load(U.scene_path(MS.PREFIX + "edges")) as s:
        with pt.RayQuery(s, max_rays=4096) as q:
            d_rays = torch.from_numpy(np.array(rays[:n])).cuda()
            d_hits = torch.full(((n + 64) * 24,), 0xA5, dtype=torch.uint8, device="cuda")   # 64 records of guard
            torch.cuda.synchronize()
            q.run(d_rays, d_hits)
            st = q.stats()
            raw = d_hits.cpu().numpy()
        if n < len(rays):
            s.prepare()
            _, _, host = s.selftest_ray_intersection(np.array(rays[:n]), traversal=0)
    assert (raw[n * 24:] == 0xA5).all(), "the run wrote past its n records"
    assert_hits(pt, raw[:n * 24].view(pt.HIT_DTYPE), want[:n])
    assert_counters(st, host, n, n_planes)
