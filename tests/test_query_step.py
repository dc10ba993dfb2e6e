"""The query step (pt_query.h: q_step, q_exec, q_exec_aux) after its hit list got one edit
point and its aux entries lost their branches: the same answers, bit for bit, and the same
work counters as before.

Four seeded ray sets, each aimed at one part of the step:
  * stack: rays across 60 stacked triangles -- adds into a partly entered list, rejects
    that shift the list above entered hits, overflow passes, the exact-DFS hand-over;
  * zero:  rays with one or two direction components +-0 (the aux step's robust `par` form);
  * wide:  rays that are not `par` but whose certification margin dl overflows to +inf
    (the aux step then tests the entries' own boxes only);
  * bulk:  tests/_rays.py's two sets on the dragon fixture scene, for volume.

Answers come from the CPU oracle (U.OracleScene.ray_intersection; it returns no work
counters for single rays).  The work counters (reference node records, primitive tests, aux
node visits, exact-DFS fallbacks) are constants recorded from the build of the commit before
this file was added (e21e197), through the host execution of the same state machine
(selftest_ray_intersection(traversal=0)): a change of the step that visits, tests or hands
over anything else moves one of them.  The GPU tests run the same rays through k_rays /
k_rays_exact and compare with the same answers and the host's counters, and render the
dragon fixture on the path engine alone (k_wpath).

The other query forms (bvh_exact, both forms of bvh_replay, qc_run) share the reference rules
with the state machine, each rule one function: the same rays go through
them too, with their own recorded counters (FORM_COUNTERS), and the megakernel renders the
stack scene on the GPU.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _rays as R
import _util as U

DRAGON = "dragon_64x64x16"

# {set: (nodes, prim_tests, aux, fallbacks)} of selftest_ray_intersection(traversal=0), recorded
# from the parent commit's build (e21e197) on the rays below
PARENT_COUNTERS = {
    "stack": (37544, 28326, 15969, 151),
    "stack_few": (158, 1838, 1122, 0),
    "zero": (68, 84, 384, 0),
    "wide": (135, 928, 3036, 0),
    "bulk1": (461, 4075, 93824, 0),
    "bulk2": (385318, 166168, 46174, 32),
}


def _stack_scene(n=60, seed=7):
    """n small triangles stacked along z above the plane z = 0, with small tilts (the
    generator of tests/test_host.py): IntersectTriangle hits the plane through the origin,
    so their hit regions all overlap near (0, 0, 0) while their own boxes are spread along
    z -- a ray crossing the stack has dozens of hitting leaves."""
    rng = np.random.default_rng(seed)
    lines = ["DIMENSIONS 8 8", "SAMPLES 1", "RAY_DEPTH 1",
             "CAMERA_POSITION 0 0 5", "CAMERA_RIGHT 1 0 0", "CAMERA_UP 0 1 0", "CAMERA_FORWARD 0 0 -1",
             "CAMERA_FOV_X 1.0"]
    tris = []
    for k in range(n):
        z = 0.5 + 0.05 * k
        v = np.array([[-0.3, -0.3, z], [0.3, -0.3, z], [0.0, 0.3, z]]) + rng.normal(0, 0.02, (3, 3))
        txt = ["%.5f" % x for x in v.ravel()]
        tris.append(np.array([float(x) for x in txt]).reshape(3, 3))
        lines += ["NEW_PRIMITIVE", "TRIANGLE " + " ".join(txt), "COLOR 0.5 0.5 0.5"]
    return "\n".join(lines) + "\n", np.array(tris)


def _stack_rays(n=600, seed=11):
    rng = np.random.default_rng(seed)
    o = np.concatenate([rng.uniform(-0.4, 0.4, (n, 2)), rng.choice([-2.0, 6.0], (n, 1))], axis=1)
    tgt = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), rng.uniform(-0.5, 3.5, (n, 1))], axis=1)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1).astype(np.float32)


def _triangles_hit(rays, tris):
    """per ray, how many of the triangles its query's primitive test accepts, and how close
    the closest call was: the reference's test (the plane through the ORIGIN with the
    triangle's normal, then three edge tests at that point) in float64"""
    o, d = rays[:, None, :3].astype(np.float64), rays[:, None, 3:].astype(np.float64)
    a, b, c = tris[None, :, 0], tris[None, :, 1], tris[None, :, 2]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    dn = (d * n).sum(-1)
    t = -(o * n).sum(-1) / dn
    p = o + t[..., None] * d
    e = np.stack([(np.cross(b - a, p - a) * n).sum(-1), (np.cross(p - a, c - a) * n).sum(-1),
                  (np.cross(c - b, p - b) * n).sum(-1), t], axis=-1)
    ok = (e > 0).all(-1) & (t <= 1e5)
    return ok.sum(1), np.abs(e).min(axis=(1, 2))


def _zero_component_rays(scene, n=384, seed=5):
    """BVH-heavy rays with one (even rows) or two (odd rows) direction components set to +-0"""
    rng = np.random.default_rng(seed)
    r = R.bvh_rays(scene, n, rng)
    for i in range(n):
        for c in rng.choice(3, 1 + i % 2, replace=False):
            r[i, 3 + c] = 0.0 if rng.integers(2) else -0.0
    return r


WIDE_TINY, WIDE_FAR = 1e-29, 1e16


def _wide_margin_rays(scene, n=384, seed=9):
    """Rays that run along one axis from about 1e16 away: that axis' direction component is
    +-1, a second one is near 1e-29 (above the 1e-30 under which a ray is `par`), the third
    is tiny in the first half (the ray crosses the scene's box; its other origin components
    lie inside it) and ordinary in the second half (it passes far from the scene)."""
    rng = np.random.default_rng(seed)
    nodes, _ = scene.dump_bvh()
    root = np.frombuffer(nodes, np.float32, 6).astype(np.float64)
    r = np.zeros((n, 6))
    for i in range(n):
        a, b, c = rng.permutation(3)
        sgn = rng.choice([-1.0, 1.0])
        r[i, :3] = rng.uniform(root[0:3], root[3:6])
        r[i, a] = -sgn * WIDE_FAR * rng.uniform(0.5, 2.0)
        r[i, 3 + a] = sgn
        r[i, 3 + b] = rng.choice([-1.0, 1.0]) * WIDE_TINY * rng.uniform(1.0, 5.0)
        r[i, 3 + c] = rng.choice([-1.0, 1.0]) * (10.0 ** rng.uniform(-28, -20) if i < n // 2 else rng.uniform(0.05, 0.5))
    return r.astype(np.float32)


def _oracle(path, rays):
    """the CPU oracle's (ids, hits) (its ray loop is serial: the rays in parallel pieces)"""
    o = U.OracleScene(path)
    parts = np.array_split(np.arange(len(rays)), 16)
    with ThreadPoolExecutor(16) as ex:
        res = list(ex.map(lambda p: o.ray_intersection(rays[p]), parts))
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


_sets = {}


def ray_set(name, tmp_root):
    """(scene path, rays, oracle ids, oracle hits) of a set; computed once, shared, read-only"""
    if not _sets:
        pt = U.ptrace()
        stack = str(tmp_root / "stack.txt")
        text, tris = _stack_scene()
        with open(stack, "w") as f:
            f.write(text)
        srays = _stack_rays()
        cnt, closest = _triangles_hit(srays, tris)
        few = srays[(cnt >= 2) & (cnt <= 6) & (closest > 1e-4)]
        dragon = U.golden_scene_path(DRAGON)
        with pt.Scene.load(dragon) as s:
            s.prepare()
            bulk1, bulk2 = R.ray_sets(s)
            wide = _wide_margin_rays(s)
        p51 = U.scene_path("practice5_1.txt")
        with pt.Scene.load(p51) as s:
            s.prepare()
            zero = _zero_component_rays(s)
        for k, (path, rays) in {"stack": (stack, srays), "stack_few": (stack, few), "zero": (p51, zero),
                                "wide": (dragon, wide), "bulk1": (dragon, bulk1), "bulk2": (dragon, bulk2)}.items():
            rays = np.ascontiguousarray(rays)
            ids, hits = _oracle(path, rays)
            for a in (rays, ids, hits):
                a.setflags(write=False)
            _sets[k] = (path, rays, ids, hits)
    return _sets[name]


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("query_step")


def host_query(name, tmp_root, traversal=0, check=True):
    pt = U.ptrace()
    path, rays, oids, ohits = ray_set(name, tmp_root)
    with pt.Scene.load(path) as s:
        s.prepare()
        ids, hits, ctr = s.selftest_ray_intersection(rays, traversal=traversal, check=check)
    print("%s: %d rays, %d hits, counters %r" % (name, len(rays), int((oids != -1).sum()),
                                               (ctr["nodes"], ctr["prim_tests"], ctr["aux"], ctr["fallbacks"])))
    assert np.array_equal(ids, oids)
    hit = oids != -1
    assert np.array_equal(hits[hit].view(np.uint32), ohits[hit].view(np.uint32))
    return rays, oids, ctr


def assert_parent_counters(name, ctr):
    assert (ctr["nodes"], ctr["prim_tests"], ctr["aux"], ctr["fallbacks"]) == PARENT_COUNTERS[name]


# ---- host: the state machine itself --------------------------------------------------------
def test_stacked_triangles_adds_rejects_overflow_and_exact_handover(tmp_root):
    rays, oids, ctr = host_query("stack", tmp_root)
    assert len(rays) == 600 and (oids >= 0).sum() > len(rays) // 2
    assert ctr["fallbacks"] > 0          # lists full of entered hits with another hit to add
    assert_parent_counters("stack", ctr)
    # rays whose primitive test accepts 2-6 of the triangles (at most 6 hitting leaves: the
    # list holds them all) finish in the state machine: several adds, then each hitting leaf
    # entered or rejected (its own box may be missed: not every such ray has a hit), no hand-over
    few, fids, fctr = host_query("stack_few", tmp_root)
    assert len(few) >= 20 and (fids >= 0).any() and (fids == -1).any()
    assert fctr["fallbacks"] == 0 and fctr["prim_tests"] >= 2 * len(few)
    assert_parent_counters("stack_few", fctr)


def test_zero_direction_components_take_the_robust_aux_boxes(tmp_root):
    rays, oids, ctr = host_query("zero", tmp_root)
    zeros = (rays[:, 3:] == 0).sum(1)
    assert len(rays) == 384 and (zeros == 1).sum() == 192 and (zeros == 2).sum() == 192
    assert (np.signbit(rays[:, 3:]) & (rays[:, 3:] == 0)).any()       # -0 among them
    assert (oids >= 0).sum() >= 96
    assert_parent_counters("zero", ctr)


def test_infinite_margin_rays_that_are_not_par(tmp_root):
    rays, oids, ctr = host_query("wide", tmp_root)
    o, d = np.abs(rays[:, :3]), np.abs(rays[:, 3:])
    om, dm = o.max(1), d.min(1)
    # not par (replay_ok_ray: every |d| component in (1e-30, 3e38), the origin finite) ...
    assert (dm > np.float32(1e-30)).all() and (d < np.float32(3e38)).all() and (o < np.float32(3e38)).all()
    # ... and q_prep's dl = 2^-18 (X + |o|max) / |d|min overflows in f32 whatever the scene's
    # extent X >= 0 is, so PT_LEAF_MARGIN x dl is +inf too
    with np.errstate(over="ignore"):
        dl = np.float32(2.0 ** -18) * (np.float32(0.0) + om) / dm
    assert dl.dtype == np.float32 and np.isinf(dl).all()
    assert ctr["aux"] > 2 * len(rays)    # the crossing half goes down the aux tree
    assert_parent_counters("wide", ctr)


@pytest.mark.parametrize("name", ["bulk1", "bulk2"])
def test_bulk_rays_on_the_dragon_fixture(tmp_root, name):
    rays, oids, ctr = host_query(name, tmp_root)
    assert len(rays) == (R.N_FIRST if name == "bulk1" else R.N_SECOND) and (oids >= 0).sum() >= 600
    assert_parent_counters(name, ctr)


# ---- host: the other query forms on the same rays ------------------------------------------
# form: (traversal, PT_TUNE).  exact = bvh_exact alone; replay_div = bvh_replay<false> (+ bvh_exact
# for the rays it hands over); coop = the cooperative engine's qc_run; mega = bvh_replay<true>,
# the megakernel's query with the filtered node tests
FORMS = {"exact": (1, None), "replay_div": (2, None), "coop": (0, "qengine=coop"), "mega": (0, "qengine=mega")}

# {form: {set: (nodes, prim_tests, aux, fallbacks)}} of selftest_ray_intersection in that form,
# recorded from the build of commit 2ca9185 (the parent of the commit that made each reference
# rule of the query code one function) plus that commit's qengine=mega hook and nothing else.
# mega has no row: it makes the decisions of replay_div (the filtered node test decides what the
# division form decides), so its counters must equal replay_div's.
FORM_COUNTERS = {
    "exact": {
        "stack": (36852, 16607, 0, 0),
        "stack_few": (5668, 2644, 0, 0),
        "zero": (384, 75, 0, 0),
        "wide": (307464, 916, 0, 0),
        "bulk1": (20932326, 27558, 0, 0),
        "bulk2": (9348892, 172941, 0, 0),
    },
    "replay_div": {
        "stack": (133774, 19789, 59155, 151),
        "stack_few": (23196, 2644, 8256, 0),
        "zero": (384, 75, 0, 384),
        "wide": (17496, 916, 6295, 0),
        "bulk1": (558539, 27558, 250713, 0),
        "bulk2": (3251292, 172941, 74157, 816),
    },
    "coop": {
        "stack": (72106, 19658, 10242, 0),
        "stack_few": (3217, 1834, 1122, 0),
        "zero": (119, 82, 384, 0),
        "wide": (1036, 916, 3036, 0),
        "bulk1": (13676, 4062, 93824, 0),
        "bulk2": (394189, 166140, 46174, 32),
    },
}
FORM_COUNTERS["mega"] = FORM_COUNTERS["replay_div"]


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["stack", "stack_few", "zero", "wide", "bulk1", "bulk2"])
def test_other_query_forms_same_answers_and_parent_counters(tmp_root, monkeypatch, name, form):
    """bvh_exact, both forms of bvh_replay and qc_run share the leaf result (leaf_first_min),
    the carried bound (bound_between) and the node tests with the state machine: the oracle's
    answers (checked in host_query) and, per form, the work the parent commit's copies did.
    The stack set's rays with more than six hitting leaves take bvh_replay's hand-over and
    the exact DFS.  On 32 of them seven leaf hits in a row are each farther than the last:
    the six-entry list bvh_exact once kept its bounds in lost one there and counted it
    ("hit list overflow", pinned here as expected until the overlap scenes showed an answer
    it changes: tests/test_overlap_host.py).  bvh_exact now carries every bound, so every
    form reports errors == 0 -- with the same oracle answers and the same work: on this set
    the lost bounds pruned nothing the kept ones do not."""
    traversal, tune = FORMS[form]
    if tune:
        monkeypatch.setenv("PT_TUNE", tune)
    _, _, ctr = host_query(name, tmp_root, traversal)
    assert ctr["errors"] == 0
    if name == "stack" and form in ("replay_div", "mega"):
        assert ctr["fallbacks"] > 0
    assert (ctr["nodes"], ctr["prim_tests"], ctr["aux"], ctr["fallbacks"]) == FORM_COUNTERS[form][name]


# ---- GPU: the same rays through k_rays / k_rays_exact, and the path engine --------------------
@pytest.fixture(scope="module")
def gpu_pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stack", "stack_few", "zero", "wide", "bulk1", "bulk2"])
def test_ray_queries_match_the_oracle_and_the_host_counters(gpu_pt, tmp_root, name):
    pt = gpu_pt
    path, rays, oids, ohits = ray_set(name, tmp_root)
    want = R.expected_hits(pt, oids, ohits[:, :4], ohits[:, 4])
    with pt.Scene.load(path) as s:
        s.prepare()
        _, _, host = s.selftest_ray_intersection(rays, traversal=0)
        got, st = s.intersect(rays)
        n_planes = s.info["n_planes"]
    assert got.dtype == pt.HIT_DTYPE and got.shape == want.shape
    assert np.array_equal(got["id"], want["id"])
    hit = want["id"] != -1
    assert np.array_equal(got["t"][hit].view(np.uint32), want["t"][hit].view(np.uint32))
    assert np.array_equal(got["n"][hit].view(np.uint32), want["n"][hit].view(np.uint32))
    assert np.array_equal(got["interior"][hit], want["interior"][hit])
    miss = np.ascontiguousarray(got[~hit]).view(np.uint32).reshape(-1, 6)
    assert np.array_equal(miss[:, 0], np.full(len(miss), 0xFFFFFFFF, np.uint32)) and not miss[:, 1:].any()
    n = len(rays)
    assert st["errors"] == 0 and st["rays"] == n and st["plane_tests"] == n * n_planes
    assert (st["node_visits"], st["prim_tests"], st["aux_visits"], st["fallbacks"]) == \
        (host["nodes"], host["prim_tests"], host["aux"], host["fallbacks"])
    assert_parent_counters(name, host)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["engine_mega", "replay_div"])
def test_megakernel_renders_the_stack_scene_through_the_handover(gpu_pt, tmp_root, monkeypatch, form):
    """The stack scene itself (8x8 pixels, 1 spp, depth 1) on the megakernel: k_trace<true>
    (PT_TUNE engine=mega, traversal 0) and k_trace<false> (traversal 2).  It is the smallest
    shape on which bvh_replay's one loop hands rays over to bvh_exact on the device (more
    than six hitting leaves).  The scene has no light, so the oracle's image is black: what
    the case shows is that the hand-over runs, ends and counts every ray, with errors == 0
    (bvh_exact carries every bound: the six-entry list that lost one on camera rays down
    the stack, and tripped the render's exactness guard here, is gone)."""
    pt = gpu_pt
    path = ray_set("stack", tmp_root)[0]
    if form == "engine_mega":
        monkeypatch.setenv("PT_TUNE", "engine=mega")
    orgb, orad, octr = U.OracleScene(path).render()
    with pt.Scene.load(path) as s:
        s.prepare()
        rgb, r, st = s.render(radiance=True, traversal=0 if form == "engine_mega" else 2)
    print("stack scene, %s: %r" % (form, {k: st[k] for k in ("rays", "node_visits", "prim_tests", "aux_visits",
                                                             "fallbacks", "errors", "rounds")}))
    assert rgb.shape == (8, 8, 3) and st["rounds"] == 0 and st["short_pixels"] == 0
    assert st["fallbacks"] > 0
    assert st["errors"] == 0
    assert np.array_equal(r.view(np.uint32), orad.view(np.uint32))
    assert np.array_equal(rgb, orgb)
    assert st["rays"] == octr["rays"]


@pytest.mark.gpu
def test_path_engine_renders_the_dragon_fixture(gpu_pt, monkeypatch):
    """k_wpath alone (coop=0) at the fixture's 16 spp: the golden image and radiance, and the
    reference's ray count (the golden files hold none: the oracle's render counts them)."""
    pt = gpu_pt
    monkeypatch.setenv("PT_TUNE", "coop=0")
    m, img, rad = U.golden_image(DRAGON)
    path = U.golden_scene_path(DRAGON)
    with pt.Scene.load(path) as s:
        s.prepare()
        rgb, r, st = s.render(radiance=True, traversal=0)
    _, orad, octr = U.OracleScene(path).render()
    assert np.array_equal(orad.view(np.uint32), rad.view(np.uint32))
    assert st["errors"] == 0 and st["short_pixels"] == 0
    assert np.array_equal(r.view(np.uint32), rad.view(np.uint32))
    assert np.array_equal(rgb, img)
    assert st["rays"] == octr["rays"]
