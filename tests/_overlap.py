"""Seeded scene families of mutually overlapping primitives, and their ray sets (tests/test_overlap_host.py on
the CPU, tests/test_overlap.py on the GPU, tests/golden/make_golden.py for the recorded fixtures).

Every generator is a pure function of (family, seed, n) that returns scene text; every primitive carries a
POSITION.  A source string is "overlap:<family>:<seed>[:<n>]":

blob      n boxes, ellipsoids and triangles of scale 10^U(-0.7, 0.6) around the origin, all diffuse: a ray
          crosses dozens of them, most of its hitting leaves farther than the one before (the case the exact
          DFS's bounds have to survive: seed 306, n 96, ray 892 of its set is the ray on which a six-entry
          hit list lost one).  n in BLOB_N.
blob_lit  the same geometry with materials and one box emitter, for the rendered cases.
shells    n concentric, randomly rotated shells, alternately ELLIPSOID and BOX dielectrics (IOR 1.5, 1.1,
          0.8 in turn), half-size 0.3 + 0.3 i, centres jittered by N(0, 0.02), a small emitter in the
          middle; rays start inside, around the centre, and leave through every shell.  n = 300 is for
          the ray tests only (hundreds of hitting leaves on one ray).
voxels    a 5 x 5 x 3 lattice of unit boxes, 60 % filled, mixed materials: faces touch exactly.
dups      every primitive twice in a row, same geometry, other colour and material: equal t, the order decides.
mixed     n = 300 boxes, ellipsoids and triangles of scale 10^U(-1.3, 0.2), 70 % with a non-unit ROTATION,
          mixed materials and IORs, every ninth non-triangle primitive an emitter.
flat      boxes and ellipsoids with one half-size of 0, 1e-6 or 1e-20, collinear and repeated-vertex
          triangles, a zero-thickness box emitter.  The reference's radiance has NaN pixels here.
"""
import os

import numpy as np

PREFIX = "overlap:"
BLOB_N = (24, 48, 96, 160)
N_FAMILY_RAYS = 2000

HEAD = ["DIMENSIONS 16 12", "RAY_DEPTH 5", "SAMPLES 2", "BG_COLOR 0.05 0.07 0.1", "CAMERA_POSITION 0.1 0.2 6",
        "CAMERA_RIGHT 1 0 0", "CAMERA_UP 0 1 0", "CAMERA_FORWARD 0 0 -1", "CAMERA_FOV_X 1.1", "",
        "NEW_PRIMITIVE", "PLANE 0 1 0", "POSITION 0 -3 0", "COLOR 0.7 0.7 0.7", "",
        "NEW_PRIMITIVE", "PLANE 0 0 1", "POSITION 0 0 -4", "COLOR 0.7 0.6 0.7", ""]


def prim(kind, size, pos, rot=None, extra=()):
    L = ["NEW_PRIMITIVE", "%s %s" % (kind, " ".join("%.7g" % x for x in size)), "POSITION %.7g %.7g %.7g" % tuple(pos)]
    if rot is not None:
        L.append("ROTATION %.7g %.7g %.7g %.7g" % tuple(rot))
    return L + list(extra) + [""]


def _material(i):
    """a material by index: diffuse, metallic, glass of three IORs"""
    return [["COLOR 0.9 0.9 0.9"], ["METALLIC", "COLOR 0.9 0.8 0.6"], ["DIELECTRIC", "IOR 1.5", "COLOR 0.9 0.9 0.9"],
            ["COLOR 0.3 0.8 0.4"], ["DIELECTRIC", "IOR 1.1", "COLOR 0.8 0.9 0.9"],
            ["DIELECTRIC", "IOR 0.8", "COLOR 0.9 0.9 0.8"]][i % 6]


def blob(seed, n, lit=False):
    r = np.random.default_rng(seed)
    L = list(HEAD)
    for i in range(n):
        k = r.integers(0, 3)
        s = 10 ** r.uniform(-0.7, 0.6)
        pos = r.normal(0, 0.6, 3)
        extra = _material(i) if lit else ["COLOR 0.9 0.9 0.9"]
        if k < 2:
            L += prim(["ELLIPSOID", "BOX"][k], s * r.uniform(0.5, 1, 3), pos, r.normal(size=4), extra)
        else:
            L += prim("TRIANGLE", s * r.normal(0, 1, 9), pos * 0.2, r.normal(size=4), extra)
    if lit:
        L += prim("BOX", (0.6, 0.1, 0.6), (0.3, 2.5, 1.0), None, ["COLOR 0 0 0", "EMISSION 6 6 5"])
    return "\n".join(L) + "\n"


def shells(seed, n):
    r = np.random.default_rng(seed)
    L = list(HEAD)
    L += prim("BOX", (0.05, 0.05, 0.05), (0, 0, 0), None, ["COLOR 0 0 0", "EMISSION 20 18 15"])
    for i in range(n):
        h = 0.3 + 0.3 * i
        ior = (1.5, 1.1, 0.8)[i % 3]
        L += prim(["ELLIPSOID", "BOX"][i % 2], (h, h, h), r.normal(0, 0.02, 3), r.normal(size=4),
                  ["DIELECTRIC", "IOR %g" % ior, "COLOR 0.95 0.95 0.95"])
    return "\n".join(L) + "\n"


def voxels(seed):
    r = np.random.default_rng(seed)
    L = list(HEAD)
    k = 0
    for x in range(5):
        for y in range(5):
            for z in range(3):
                if r.uniform() >= 0.6:
                    continue
                L += prim("BOX", (0.5, 0.5, 0.5), (x - 2, y - 2, z - 1), None, _material(int(r.integers(0, 6))))
                k += 1
    L += prim("BOX", (0.5, 0.05, 0.5), (0, 3.05, 0), None, ["COLOR 0 0 0", "EMISSION 8 8 8"])
    return "\n".join(L) + "\n"


def dups(seed, n=24):
    r = np.random.default_rng(seed)
    L = list(HEAD)
    for i in range(n):
        k = int(r.integers(0, 3))
        s = 10 ** r.uniform(-0.5, 0.3)
        pos = r.normal(0, 0.8, 3)
        rot = r.normal(size=4)
        size = s * r.uniform(0.5, 1, 3) if k < 2 else s * r.normal(0, 1, 9)
        for twin in range(2):
            extra = list(_material(2 * i + 3 * twin)) + ([] if i != 5 else ["EMISSION 5 5 5"])
            L += prim(["ELLIPSOID", "BOX", "TRIANGLE"][k], size, pos, rot, extra)
    return "\n".join(L) + "\n"


def mixed(seed, n=300):
    r = np.random.default_rng(seed)
    L = list(HEAD)
    solid = 0
    for i in range(n):
        k = int(r.integers(0, 3))
        s = 10 ** r.uniform(-1.3, 0.2)
        pos = r.normal(0, 1.0, 3)
        rot = r.normal(size=4) if r.uniform() < 0.7 else None
        extra = list(_material(int(r.integers(0, 6))))
        if k < 2:
            solid += 1
            if solid % 9 == 0:
                extra.append("EMISSION 3 3 3")
            L += prim(["ELLIPSOID", "BOX"][k], s * r.uniform(0.5, 1, 3), pos, rot, extra)
        else:
            L += prim("TRIANGLE", s * r.normal(0, 1, 9), pos, rot, extra)
    return "\n".join(L) + "\n"


def flat(seed):
    r = np.random.default_rng(seed)
    L = list(HEAD)
    thin = (0.0, 1e-6, 1e-20)
    for i in range(18):
        size = r.uniform(0.3, 1.2, 3)
        size[i % 3] = thin[(i // 3) % 3]
        L += prim(["BOX", "ELLIPSOID"][i % 2], size, r.normal(0, 0.8, 3), r.normal(size=4) if i % 4 else None,
                  _material(i))
    for i in range(6):
        a, e = r.normal(0, 1, 3), r.normal(0, 1, 3)
        if i % 2:
            v = np.concatenate([a, a + e, a + 2.5 * e])          # collinear
        else:
            v = np.concatenate([a, a, a + e])                    # a repeated vertex
        L += prim("TRIANGLE", v, r.normal(0, 0.3, 3), None, _material(i))
    L += prim("BOX", (0.8, 0.0, 0.8), (0, 2.0, 0), None, ["COLOR 0 0 0", "EMISSION 6 6 6"])
    return "\n".join(L) + "\n"


def parse(src):
    """("family", seed, n or None) of a source string "overlap:<family>:<seed>[:<n>]" """
    assert src.startswith(PREFIX), src
    f = src[len(PREFIX):].split(":")
    return f[0], int(f[1]), int(f[2]) if len(f) > 2 else None


def scene_text(src):
    fam, seed, n = parse(src)
    if fam == "blob":
        return blob(seed, n)
    if fam == "blob_lit":
        return blob(seed, n, lit=True)
    if fam == "shells":
        return shells(seed, n)
    if fam in ("dups", "mixed"):
        return {"dups": dups, "mixed": mixed}[fam](seed, *([] if n is None else [n]))
    assert n is None, src
    return {"voxels": voxels, "flat": flat}[fam](seed)


def family_rays(src, count=N_FAMILY_RAYS):
    """The family's own rays, the first `count` of N_FAMILY_RAYS from default_rng(5000 + seed): origins
    N(0, 1) x U(0, 4) (shells: N(0, 0.15), inside the innermost shell), directions uniform on the sphere,
    normalised in float64, stored as float32"""
    fam, seed, _ = parse(src)
    r = np.random.default_rng(5000 + seed)
    N = N_FAMILY_RAYS
    o = r.normal(0, 1, (N, 3)) * r.uniform(0, 4, (N, 1))
    d = r.normal(size=(N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if fam == "shells":
        o = o / np.maximum(np.linalg.norm(o, axis=1, keepdims=True), 1e-9) * np.abs(r.normal(0, 0.15, (N, 1)))
    return np.concatenate([o, d], axis=1).astype(np.float32)[:count]


class _TreeOf:
    """what _rays.special_rays reads of a scene, from the oracle's"""
    def __init__(self, o):
        self.info = {"n_bvh_prims": o.n_bvh}
        self.dump_bvh = o.dump_bvh


def ray_set(src, oracle_scene, n_family, n_special):
    """A recorded ray set: the family's first n_family rays, then n_special of _rays.special_rays on the
    scene's tree (the oracle's dump): BVH-heavy rays with +-0 direction components, and non-finite rays"""
    import _rays
    _, seed, _ = parse(src)
    own = family_rays(src, n_family)
    special = _rays.special_rays(_TreeOf(oracle_scene), n_special, np.random.default_rng(7000 + seed))
    return np.concatenate([own, special], axis=0)


def same_but_nan_signs(a, b):
    """The rule for scenes whose reference radiance has NaNs (flat): NaN at the same positions, every other
    float bit-equal.  A NaN's sign and payload are not pinned."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


# ---- the recorded fixtures (tests/golden/make_golden.py --rays / --images) ---------------------------
# ray source -> (family rays, special rays); blob:306:96's family rays include ray 892
RAY_FIXTURES = {
    "overlap:blob:306:96": (1920, 128),
    "overlap:blob:11:160": (768, 256),
    "overlap:shells:7:14": (1536, 512),
    "overlap:shells:2:30": (768, 256),
    "overlap:shells:3:300": (384, 128),
    "overlap:voxels:1": (768, 256),
    "overlap:dups:1": (768, 256),
    "overlap:mixed:1": (768, 256),
    "overlap:flat:1": (768, 256),
}
IMAGE_FIXTURES = ["overlap:blob_lit:306:96", "overlap:blob_lit:11:160", "overlap:shells:7:14", "overlap:shells:2:30",
                  "overlap:voxels:1", "overlap:dups:1", "overlap:mixed:1", "overlap:flat:1"]
BLOB_306, RAY_892 = "overlap:blob:306:96", 892


def centres():
    """the pixel centres of the 16 x 12 frame, row-major: (192, 2) float32"""
    ys, xs = np.mgrid[0:12, 0:16]
    return np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float32)


def fixture_name(src):
    """the fixture's file stem: overlap:blob:306:96 -> overlap_blob_306_96"""
    return src.replace(":", "_")


# ---- inputs reach the case: a float64 restatement of the primitive tests -----------------------------
def _qrot(q, v):
    """q * v as the reference computes it for q = (x, y, z, w): v + 2 (w u x v + u x (u x v)), the quaternion
    used as written (a ROTATION that is no unit quaternion is a linear map, not a rotation), in float64"""
    q = np.asarray(q, np.float64)
    u, w = q[:3], q[3]
    uv = np.cross(u, v)
    return v + 2.0 * (w * uv + np.cross(u, uv))


def prim_hits64(text, rays, planes=False):
    """(n_rays, n_prims) float64: the nearest t >= 0 at which each ray meets each BOX / ELLIPSOID / TRIANGLE
    of the scene text (planes=True: each of its PLANEs instead), inf where it does not -- plain geometry in float64, independent
    of the code under test, for counting the rays that reach a case."""
    rays = np.asarray(rays, np.float64)
    blocks, cur = [], None
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "NEW_PRIMITIVE":
            cur = {"rot": (0.0, 0.0, 0.0, 1.0), "pos": (0.0, 0.0, 0.0)}
            blocks.append(cur)
        elif cur is not None and w[0] in ("BOX", "ELLIPSOID", "TRIANGLE", "PLANE"):
            cur["kind"], cur["size"] = w[0], np.array([float(x) for x in w[1:]])
        elif cur is not None and w[0] == "POSITION":
            cur["pos"] = tuple(float(x) for x in w[1:4])
        elif cur is not None and w[0] == "ROTATION":
            cur["rot"] = tuple(float(x) for x in w[1:5])
    blocks = [b for b in blocks if (b["kind"] == "PLANE") == planes]
    out = np.full((len(rays), len(blocks)), np.inf)
    with np.errstate(all="ignore"):
        for j, b in enumerate(blocks):
            qc = np.array(b["rot"]) * (-1, -1, -1, 1)                # the inverse rotation
            o = _qrot(qc, rays[:, :3] - np.array(b["pos"]))
            d = _qrot(qc, rays[:, 3:])
            s = b["size"]
            if b["kind"] == "PLANE":
                t = -(o @ s) / (d @ s)
                ok = (t > 0) & (t <= 1e5)
            elif b["kind"] == "BOX":
                a, c = (-s - o) / d, (s - o) / d
                t1, t2 = np.minimum(a, c).max(1), np.maximum(a, c).min(1)
                ok = (t1 <= t2) & (t2 >= 0)
                t = np.where(t1 < 0, t2, t1)
            elif b["kind"] == "ELLIPSOID":
                od, dd = o / s, d / s
                A, B, Cc = (dd * dd).sum(1), (od * dd).sum(1), (od * od).sum(1) - 1.0
                disc = B * B - A * Cc
                sq = np.sqrt(np.maximum(disc, 0))
                t1, t2 = (-B - sq) / A, (-B + sq) / A
                ok = (disc > 0) & (t2 >= 0)
                t = np.where(t1 < 0, t2, t1)
            else:
                # the reference's triangle: the plane through the LOCAL ORIGIN with the triangle's normal,
                # then three orientation tests of the point against the edges (src/primitives.cpp:155-174)
                va, vb, vc = s[0:3], s[3:6], s[6:9]
                n = np.cross(vb - va, vc - va)
                n = n / np.linalg.norm(n)
                t = -(o @ n) / (d @ n)
                pt_ = o + t[:, None] * d
                ok = (t > 0) & (t <= 1e5)
                for e, q in ((vb - va, pt_ - va), (None, None), (vc - vb, pt_ - vb)):
                    if e is None:
                        ok &= (np.cross(pt_ - va, vc - va) @ n) > 0
                    else:
                        ok &= (np.cross(e, q) @ n) > 0
            out[:, j] = np.where(ok & np.isfinite(t), t, np.inf)
    return out


def leaves_in_order(oracle_scene, text):
    """The reference tree's leaves in the order BVH_t::Intersect_ visits them (left first), each (the id of its first
    primitive, its primitives' indices into prim_hits64's columns): the oracle's dump of the tree, its primitives matched to the
    text's by type, float32 size and position (twins of equal geometry are interchangeable here)."""
    nodes, prims = oracle_scene.dump_bvh()
    nd = np.frombuffer(nodes, np.uint8).reshape(-1, 40)[:, 24:40].copy().view(np.uint32).reshape(-1, 4)
    pr = np.frombuffer(prims, np.uint8).reshape(-1, 52)
    kinds = {"BOX": 2, "ELLIPSOID": 4, "TRIANGLE": 8}
    keys, col = {}, 0
    cur = None
    for line in text.split("\n"):
        w = line.split()
        if w and w[0] in ("BOX", "ELLIPSOID", "TRIANGLE", "PLANE"):
            cur = None if w[0] == "PLANE" else [kinds[w[0]], np.array([float(x) for x in w[1:]], np.float32)]
        elif w and w[0] == "POSITION" and cur is not None:
            size = np.zeros(9, np.float32)
            size[:len(cur[1])] = cur[1]
            k = (cur[0], size.tobytes(), np.array([float(x) for x in w[1:4]], np.float32).tobytes())
            keys.setdefault(k, []).append(col)
            col += 1
            cur = None
    def column(i):
        rec = pr[i]
        k = (int(rec[0:4].copy().view(np.uint32)[0]), rec[4:40].tobytes(), rec[40:52].tobytes())
        return keys[k][0]
    out, stack = [], [0]
    while stack:
        v = stack.pop()
        left, right, first, count = (int(x) for x in nd[v])
        if left == 0xFFFFFFFF:
            out.append((first, [column(i) for i in range(first, first + count)]))
        else:
            stack += [right, left]
    assert sum(len(x) for _, x in out) == col, "the dump's leaves do not cover the text's primitives"
    return out


def reference_walk(oracle_scene, text, rays):
    """BVH_t::Intersect_ (src/bvh.cpp:185-225) restated in float64 over the oracle's dump of the tree: per
    ray (id or -1 of Scene::RayIntersection's answer, hitting leaves visited, ascending, carried).  A
    visited leaf is one the recursion enters (its box hit, not pruned by the bound it was handed).
    ascending: the most of the visited hitting leaves that lie in ascending order of t, in visiting
    order (the longest strictly ascending subsequence).  carried: the length a suffix-minimum list of
    the visited leaf hits reaches -- the recorded hits, each nearer than every later one, that some right
    child's bound may still have to come from; seven is what a six-entry list cannot hold.  Independent
    of the product: for counting the rays that reach the case, and right about the answer wherever
    float64 and float32 agree on every decision."""
    import bisect
    import sys
    rays = np.asarray(rays, np.float64)
    t = prim_hits64(text, rays)
    tp = prim_hits64(text, rays, planes=True).min(axis=1)
    nodes, _ = oracle_scene.dump_bvh()
    raw = np.frombuffer(nodes, np.uint8).reshape(-1, 40)
    box = raw[:, :24].copy().view(np.float32).reshape(-1, 6).astype(np.float64)
    nd = raw[:, 24:40].copy().view(np.uint32).reshape(-1, 4).tolist()
    col_of = {}
    for first, cols in leaves_in_order(oracle_scene, text):
        for k, c in enumerate(cols):
            col_of[first + k] = c
    centre, half = (box[:, :3] + box[:, 3:]) / 2, (box[:, 3:] - box[:, :3]) / 2
    with np.errstate(all="ignore"):
        o = rays[:, None, :3] - centre[None]
        a, c = (-half[None] - o) / rays[:, None, 3:], (half[None] - o) / rays[:, None, 3:]
        t1, t2 = np.minimum(a, c).max(axis=2), np.maximum(a, c).min(axis=2)
        entered = ~(t1 > t2) & ~(t2 < 0)
        t_in = np.where(t1 < 0, -np.inf, t1)      # interior: never pruned
    ids = np.full(len(rays), -1)
    visited = np.zeros(len(rays), np.int64)
    longest = np.zeros(len(rays), np.int64)
    ascending = np.zeros(len(rays), np.int64)
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * len(nd) + 100))
    for r in range(len(rays)):
        ent, tin, tr = entered[r].tolist(), t_in[r].tolist(), t[r].tolist()
        run, state, seq = [], [0, 0], []

        def walk(v, bound):
            if not ent[v] or bound < tin[v]:
                return np.inf, -1
            left, right, first, count = nd[v]
            if left == 0xFFFFFFFF:
                best, bid = np.inf, -1
                for i in range(first, first + count):
                    if tr[col_of[i]] < best:
                        best, bid = tr[col_of[i]], i
                if bid >= 0:
                    while run and run[-1] >= best:
                        run.pop()
                    run.append(best)
                    seq.append(best)
                    state[0] += 1
                    state[1] = max(state[1], len(run))
                return best, bid
            lt, lid = walk(left, bound)
            if lid != -1:
                bound = lt
            rt, rid = walk(right, bound)
            return (rt, rid) if rid != -1 and rt < lt else (lt, lid)

        bt, bid = walk(0, tp[r])
        ids[r] = bid if bid != -1 and bt < tp[r] else (-2 if np.isfinite(tp[r]) else -1)   # -2: a plane
        visited[r], longest[r] = state
        tails = []
        for x in seq:
            k = bisect.bisect_left(tails, x)
            tails[k:k + 1] = [x]
        ascending[r] = len(tails)
    return ids, visited, ascending, longest


# ---- the recorded cases, loaded once and shared (read-only) ------------------------------------------
_cases = {}


def case(src):
    """{"path", "text", "oracle", "rays", "ids", "hits" (n, 4: t, n.xyz), "interior"} of a ray fixture: the
    scene written under scenes/gen, its recorded rays and the reference's RayIntersection answers; the
    files are checked against the manifest, and the generators against what the fixture was recorded from"""
    if src not in _cases:
        import _util as U
        name = fixture_name(src)
        m = U.manifest()["overlap"]["rays"][name]
        text = scene_text(src)
        assert U.md5(text.encode()) == m["scene_md5"], src + ": the generator no longer writes the recorded scene"
        path = U.scene_path(src)
        with open(os.path.join(U.GOLDEN, "trav_%s.bin" % name), "rb") as f:
            assert U.md5(f.read()) == m["md5"]
        rays, ((ids, f, inter), _) = U.read_trav(name)
        o = U.OracleScene(path)
        want = ray_set(src, o, *RAY_FIXTURES[src])
        assert U.md5(want.tobytes()) == m["rays_md5"] and np.array_equal(want.view(np.uint32), rays.view(np.uint32))
        for a in (rays, ids, f, inter):
            a.setflags(write=False)
        _cases[src] = {"path": path, "text": text, "oracle": o, "rays": rays, "ids": ids, "hits": f, "interior": inter}
    return _cases[src]


def image(src):
    """{"path", "rgb" (12, 16, 3) u8, "rad" (12, 16, 3) f32, "rays"} of an image fixture, md5-checked"""
    key = ("image", src)
    if key not in _cases:
        import _util as U
        name = fixture_name(src)
        m = U.manifest()["overlap"]["images"][name]
        assert U.md5(scene_text(src).encode()) == m["scene_md5"], src + ": the generator no longer writes the recorded scene"
        raw = [open(os.path.join(U.GOLDEN, f % name), "rb").read() for f in ("img_%s.ppm", "rad_%s.f32")]
        assert [U.md5(b) for b in raw] == [m["ppm_md5"], m["rad_md5"]]
        rgb = U.read_ppm(os.path.join(U.GOLDEN, "img_%s.ppm" % name))
        rad = np.frombuffer(raw[1], np.float32).reshape(rgb.shape)
        assert rgb.shape == (12, 16, 3)
        _cases[key] = {"path": U.scene_path(src), "rgb": rgb, "rad": rad, "rays": m["rays"]}
    return _cases[key]


def assert_radiance(src, got, want, what):
    """bit for bit; a flat scene by the NaN rule (same_but_nan_signs)"""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    if parse(src)[0] == "flat":
        ng, nw = np.isnan(got), np.isnan(want)
        bad = np.flatnonzero((ng != nw) | (~ng & ~nw & (got.view(np.uint32) != want.view(np.uint32))))
        assert same_but_nan_signs(got, want), "%s, %s: differs beyond the signs of NaNs at %d floats %r: got %r, want %r" % (
            src, what, len(bad), bad[:12].tolist(), got[bad[:12]].tolist(), want[bad[:12]].tolist())
    else:
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, "%s, %s: %d floats differ, first %d: %r != %r" % (src, what, len(bad), bad[0], got[bad[0]],
                                                                                want[bad[0]])


def assert_hits(src, ids, t, n, interior, c, what):
    """ids, and on the hits the bits of t and n and the interior flag, against the recorded answers (a flat
    scene's NaN normals by the NaN rule); the first differing ray is named"""
    bad = np.flatnonzero(np.asarray(ids) != c["ids"])
    assert len(bad) == 0, "%s, %s: %d ids differ, first at ray %d: got %d, recorded %d" % (
        src, what, len(bad), bad[0], ids[bad[0]], c["ids"][bad[0]])
    hit = c["ids"] != -1
    got = np.concatenate([np.asarray(t, np.float32).reshape(-1, 1), np.asarray(n, np.float32).reshape(-1, 3)], axis=1)[hit]
    want = np.ascontiguousarray(c["hits"][hit])
    differ = got.view(np.uint32) != want.view(np.uint32)
    if parse(src)[0] == "flat":
        differ &= ~(np.isnan(got) & np.isnan(want))     # the NaN rule: a NaN's sign and payload are not pinned
    bad = np.flatnonzero(differ.any(axis=1))
    assert len(bad) == 0, "%s, %s: %d hits differ in t or n, first at ray %d: got %r, recorded %r" % (
        src, what, len(bad), np.flatnonzero(hit)[bad[0]], got[bad[0]].tolist(), want[bad[0]].tolist())
    assert np.array_equal(np.asarray(interior)[hit] != 0, c["interior"][hit] != 0), "%s, %s: interior flags" % (src, what)


def expected_features(pt, src, path, xy):
    """The FEATURE_DTYPE records Scene.features owes for the positions xy: tests/_features.py's, built from
    the oracle's closest hits and the scene text.  Two families are beyond its text matching -- dups (twins
    of equal geometry: the text cannot tell which of them a prepared-order id names) and flat (a recorded
    hit may have a NaN normal) -- and take the hit from the oracle all the same, the type from the oracle's
    prim_info and the shade words from the scene's own table (Scene.shade: the loader's, not the query's)."""
    import _features as F
    import _util as U
    if parse(src)[0] not in ("dups", "flat"):
        return F.expected(pt, path, xy)[0]
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    o = U.OracleScene(path)
    # (the camera is the common head's: _features reads it from a scene of the head alone)
    import _ladder as L
    ids, hits = o.ray_intersection(F.camera_rays(L.write_scene("overlap_head", "\n".join(HEAD) + "\n"), xy))
    info = o.prim_info()
    with pt.Scene.load(path) as s:
        s.prepare()
        tab, bg = s.shade(), s.background
    for i, p in enumerate(info):      # the loader's table against the oracle's view of the same primitives
        assert U.MATERIALS[int(tab["material"][i])] == p["material"] and bool(tab["emission"][i].any()) == p["emissive"]
        assert tab["ior"][i] == np.float32(p["ior"])
    out = np.zeros(len(xy), pt.FEATURE_DTYPE)
    hit = ids >= 0
    out["id"] = np.where(hit, ids, -1)
    out["t"][hit] = hits[hit, 0]
    out["n"][hit] = hits[hit, 1:4]
    out["interior"][hit] = (hits[hit, 4] != 0).astype(np.uint32)
    for k in ("albedo", "ior", "emission", "material"):
        out[k][hit] = tab[k][ids[hit]]
    code = {v: k for k, v in U.PRIM_TYPES.items()}
    out["type"][hit] = [code[info[i]["type"]] for i in ids[hit]]
    out["emission"][~hit] = bg
    return out


def assert_features(src, got, want):
    """word for word; a flat scene's t and n by the NaN rule (NaN where the expected record has one)"""
    g = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), 16)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(len(want), 16)
    same = g == w
    if parse(src)[0] == "flat":
        gf, wf = g[:, 1:5].view(np.float32), w[:, 1:5].view(np.float32)
        same[:, 1:5] |= np.isnan(gf) & np.isnan(wf)
    bad = np.flatnonzero(~same.all(axis=1))
    assert len(bad) == 0, "%s: %d of %d records differ; first %d: got %s want %s" % (src, len(bad), len(w), bad[0],
                                                                                   got[bad[0]], want[bad[0]])
