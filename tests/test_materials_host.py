"""Materials on every primitive kind, and rays on the primitives' edges, on the host (no GPU).

The scenes and rays are _material_scenes.py's; their expected values were recorded from the
unmodified reference (tests/golden/make_golden.py --images / --rays), and the manifest's md5 of
each scene's text keeps a scene and its fixture together.

* The coverage gate: a scene that merely looks complete need not reach its cells, so the CPU
  oracle counts, per primitive, the vertices that took each branch of the material switch
  (render(census=True)); its radiance equals the reference's fixture, which ties the counted
  branches to the ones the reference ran.  Every required cell holds at least NEED events.  A
  failure here means the scene is wrong, not the product.
* The recorded answers to the edge rays reach every primitive, interior hits and misses.
* The device integrator compiled for the host renders the three scenes bit for bit under every
  traversal.  (The recorded rays run through test_host.py's and test_oracle.py's batteries
  over manifest["trav"], the images through theirs over manifest["images"].)
"""
import numpy as np
import pytest

import _material_scenes as MS
import _util as U

M = U.manifest()
pt = U.ptrace()

FIXTURE = {"matrix": "mat_matrix_24x24x8", "inside": "mat_inside_24x24x8", "camera": "mat_camera_23x17x8"}
TRAVERSALS = {"replay": 0, "exact": 1, "replay_div": 2}
NEED = 8          # events per census cell
EV = {e: k for k, e in enumerate(U.CENSUS_EVENTS)}
OUT, IN = 0, 1


@pytest.mark.parametrize("name", sorted(FIXTURE) + ["edges"])
def test_scene_text_is_the_one_recorded(name):
    text = MS.scene_text(name).encode()
    entry = M["trav"]["edges"] if name == "edges" else M["images"][FIXTURE[name]]
    assert entry["scene"] == MS.PREFIX + name
    assert U.md5(text) == entry["scene_md5"]
    with open(U.scene_path(MS.PREFIX + name), "rb") as f:
        assert f.read() == text
    if name == "edges":
        rays = MS.edge_rays()
        assert rays.shape == (4096, 6) and U.md5(rays.tobytes()) == entry["rays_md5"]
        assert np.array_equal(U.read_trav("edges")[0].view(np.uint32), rays.view(np.uint32))
    else:
        o = U.OracleScene(U.scene_path(MS.PREFIX + name))
        assert o.W <= 24 and o.H <= 24 and o.samples <= 8 and o.depth == 8


_census = {}


def census(name):
    """the oracle's render of a scene with the vertex census; rendered once, read only"""
    if name not in _census:
        o = U.OracleScene(U.scene_path(MS.PREFIX + name))
        rgb, rad, ctr = o.render(census=True)
        _census[name] = (o.prim_info(), rgb, rad, ctr)
    return _census[name]


@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_census_leaves_the_render_as_it_was(name):
    """With the census the oracle's image, radiance and four counters are the fixture's and
    those of a render without it; the counts do not depend on the number of threads, and
    no ray is counted twice (a ray that hits is one vertex event, a ray that misses none)."""
    m, img, rad = U.golden_image(FIXTURE[name])
    info, rgb, r, ctr = census(name)
    assert r.view(np.uint32).tolist() == rad.view(np.uint32).tolist()
    assert np.array_equal(rgb, img)
    o = U.OracleScene(U.scene_path(MS.PREFIX + name))
    rgb0, r0, ctr0 = o.render()
    assert np.array_equal(r0.view(np.uint32), r.view(np.uint32)) and np.array_equal(rgb0, rgb)
    assert ctr0 == {k: v for k, v in ctr.items() if k != "census"}
    _, _, one = o.render(census=True, threads=1)
    assert np.array_equal(one["census"], ctr["census"])
    assert ctr["census"].shape == (o.n_prims, 5, 2) and 0 < ctr["census"].sum() <= ctr["rays"]


def _cells():
    """(label, events) for every cell of the gate, from the matrix and inside scenes together"""
    rows = []   # (primitive info, census (5, 2))
    for name in ("matrix", "inside"):
        info, _, _, ctr = census(name)
        rows += list(zip(info, ctr["census"]))

    def total(event, side, pred):
        sides = (OUT, IN) if side is None else (side,)
        return int(sum(c[EV[event], s] for p, c in rows if pred(p) for s in sides))

    kinds = {"box": lambda p: p["type"] == "box", "ellipsoid": lambda p: p["type"] == "ellipsoid",
             "transformed triangle": lambda p: p["type"] == "triangle" and (p["moved"] or p["rotated"]),
             "plane": lambda p: p["type"] == "plane"}
    cells = []
    for kind, is_kind in kinds.items():
        cells.append((kind + ": refraction outside", total("refract", OUT, is_kind)))
        cells.append((kind + ": refraction interior", total("refract", IN, is_kind)))
        cells.append((kind + ": Fresnel reflection outside", total("fresnel", OUT, is_kind)))
        if kind in ("box", "ellipsoid"):
            cells.append((kind + ": total internal reflection interior", total("tir", IN, is_kind)))
        else:   # the flat kinds' cell: the outside face of an instance of IOR < 1
            cells.append((kind + ": total internal reflection outside, IOR < 1",
                          total("tir", OUT, lambda p: is_kind(p) and 0 < p["ior"] < 1)))
        cells.append((kind + ": metallic", total("metallic", None, is_kind)))
    cells.append(("IOR < 1: total internal reflection outside", total("tir", OUT, lambda p: 0 < p["ior"] < 1)))
    cells.append(("IOR 1.0: refraction", total("refract", None, lambda p: p["material"] == "dielectric" and p["ior"] == 1.0)))
    cells.append(("emitter: metallic", total("metallic", None, lambda p: p["emissive"])))
    cells.append(("plane or triangle: metallic interior",
                  total("metallic", IN, lambda p: p["type"] in ("plane", "triangle"))))
    return cells


def test_census_gate():
    cells = _cells()
    for label, n in cells:
        print("%-60s %6d" % (label, n))
    assert len(cells) == 24
    short = [(label, n) for label, n in cells if n < NEED]
    assert not short, short
    # what the scenes are written to hold, on the oracle's own reading of them
    info = census("matrix")[0]
    iors = {p["ior"] for p in info if p["material"] == "dielectric"}
    assert {round(v, 4) for v in iors} == {0.7, 1.0, 1.5, 2.4}
    assert any(p["type"] == "plane" and p["material"] == "metallic" and p["rotated"] for p in info)
    assert any(p["type"] == "plane" and p["material"] == "dielectric" for p in info)
    assert any(p["type"] == "triangle" and p["material"] == "dielectric" and not p["moved"] and not p["rotated"]
               for p in info)
    for mat in ("dielectric", "metallic"):
        for kind in ("box", "ellipsoid"):
            assert any(p["type"] == kind and p["material"] == mat and p["rotated"] for p in info)
        assert any(p["type"] == "triangle" and p["material"] == mat and p["moved"] and not p["rotated"] for p in info)
        assert any(p["type"] == "triangle" and p["material"] == mat and p["moved"] and p["rotated"] for p in info)
    # the camera of `inside` is inside: its first hits are interior ones
    info, _, _, ctr = census("inside")
    assert ctr["census"][:, :, IN].sum() > ctr["census"][:, :, OUT].sum()


def test_the_triangle_as_written_is_hit():
    """the glass triangle as written is hit (the reference hits a triangle's copy on the plane
    through the origin: this one lies in such a plane)"""
    info, _, _, ctr = census("matrix")
    plain = [i for i, p in enumerate(info) if p["type"] == "triangle" and not p["moved"] and not p["rotated"]]
    assert len(plain) == 1 and ctr["census"][plain[0]].sum() >= 8 * NEED


def test_edge_rays_reach_what_they_aim_at():
    """Conditions on the reference's recorded answers to the edge rays."""
    rays, ((ids, f, inter), (bids, bf, _)) = U.read_trav("edges")
    o = U.OracleScene(U.scene_path(MS.PREFIX + "edges"))
    info = o.prim_info()
    hit = ids != -1
    per_prim = np.bincount(ids[hit], minlength=o.n_prims)
    print("hits per primitive", per_prim.tolist(), "interior", int(inter[hit].sum()), "misses", int((~hit).sum()))
    assert len(rays) == 4096
    assert per_prim.min() >= 64, per_prim.tolist()
    assert int(inter[hit].sum()) >= 500
    assert int((~hit).sum()) >= 200
    assert not np.isnan(f[hit]).any() and not np.isnan(bf[bids != -1]).any()
    # the plane test's limit: hits at the float 1e5 and at its neighbour below, none beyond
    planes = np.array([p["type"] == "plane" for p in info])
    tp = f[hit & planes[np.maximum(ids, 0)], 0]
    t5 = np.float32(1e5)
    assert (tp == t5).any() and (tp == np.nextafter(t5, np.float32(0))).any() and not (tp > t5).any()
    # rays in and parallel to the plane y = -4 (d.n = 0: t is 0 / 0 or x / 0) never hit it
    flat = rays[:, 4] == 0
    floor = [i for i, p in enumerate(info) if p["type"] == "plane" and not p["rotated"]]
    assert len(floor) == 1 and flat.sum() >= 300 and (rays[flat, 1] == -4).sum() >= 20
    assert not (ids[flat] == floor[0]).any()
    # rays with a zero direction component, rays starting on a surface
    assert (rays[:, 3:] == 0).any(axis=1).sum() >= 1000
    assert (f[hit, 0] < 1e-3).sum() >= 64
    # ties in the box normal: normals along an edge's or a corner's diagonal
    boxes = np.array([p["type"] == "box" for p in info])
    nb = f[hit & boxes[np.maximum(ids, 0)], 1:4]
    assert ((nb != 0).sum(axis=1) == 2).sum() >= 32 and ((nb != 0).sum(axis=1) == 3).sum() >= 32


@pytest.mark.parametrize("trav", sorted(TRAVERSALS))
@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_material_scene_on_host_bit_exact(name, trav):
    m, img, rad = U.golden_image(FIXTURE[name])
    with pt.Scene.load(U.scene_path(MS.PREFIX + name)) as s:
        s.prepare()
        got = s.selftest_render_host(0, 0, img.shape[1], img.shape[0], traversal=TRAVERSALS[trav])
    assert got.view(np.uint32).tolist() == rad.view(np.uint32).tolist()
    assert np.array_equal(U.oracle_tonemap(got).reshape(img.shape), img)
