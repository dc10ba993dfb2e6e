"""Expected first-hit feature records for tests/test_features_host.py and tests/test_features.py.

Nothing here comes from the code under test.  A record is put together from three sources:
  the ray          Camera::GetToRay restated in numpy float32, the camera parsed from the scene text
  id, t, n, side   the oracle's ray_intersection on those rays
  material, ior,   the oracle's prim_info
  type
  albedo,          a small parser of the scene text's NEW_PRIMITIVE blocks; a block is matched to
  emission,        a prepared-order id through the oracle's dump_bvh record of that id (type, a, b,
  BG_COLOR         c, position), and two blocks that share that key but differ in what the record
                   copies are an error, never a guess
"""
import functools

import numpy as np

import _util as U

SCENES = ("dragon_64x64x16", "dragon_metal_64x64x8", "dragon_glass_40x24x7", "standin_48x32x4", "rabbid_48x48x4",
          "hw3s6_48x48x8", "mat_matrix_24x24x8", "mat_inside_24x24x8", "mat_camera_23x17x8")
SEED = 20261020
N_SUB = 4096
TYPE_CODE = {v: k for k, v in U.PRIM_TYPES.items()}
MATERIAL_CODE = {v: k for k, v in U.MATERIALS.items()}
SHAPES = {"PLANE": 1, "BOX": 2, "ELLIPSOID": 4, "TRIANGLE": 8}
_f32 = np.float32


def _floats(words):
    return np.array([float(w) for w in words], _f32)


@functools.lru_cache(maxsize=None)
def scene_text(path):
    """the scene text's top-level values and its primitive blocks:
    ({"BG_COLOR", "CAMERA_*", "DIMENSIONS"}, {key: (albedo, emission, material, ior)})"""
    top, blocks = {}, {}
    cur = None

    def close():
        if cur is None:
            return
        if cur["shape"] is None:
            raise AssertionError("%s: a NEW_PRIMITIVE block without a shape line" % path)
        key = (cur["shape"], cur["geom"].tobytes(), cur["pos"].tobytes())
        val = (cur["col"].tobytes(), cur["emis"].tobytes(), cur["mat"], cur["ior"].tobytes())
        if blocks.setdefault(key, val) != val:
            raise AssertionError("%s: two blocks share type, geometry and position but differ in colour, emission, "
                                 "material or IOR: their prepared-order ids cannot be told apart" % path)

    with open(path) as f:
        for line in f:
            w = line.split()
            if not w:
                close()
                cur = None
                continue
            if w[0] == "NEW_PRIMITIVE":
                close()
                cur = {"shape": None, "geom": np.zeros(9, _f32), "pos": np.zeros(3, _f32), "col": np.zeros(3, _f32),
                       "emis": np.zeros(3, _f32), "mat": 0, "ior": np.zeros(1, _f32)}
                continue
            if cur is None:
                if w[0] in ("BG_COLOR", "DIMENSIONS", "CAMERA_POSITION", "CAMERA_RIGHT", "CAMERA_UP", "CAMERA_FORWARD",
                            "CAMERA_FOV_X"):
                    top[w[0]] = _floats(w[1:])
                continue
            if w[0] in SHAPES:
                # (the reference starts the primitive afresh at its shape line: nothing may come before it)
                if cur["shape"] is not None or cur["col"].any() or cur["emis"].any() or cur["mat"] or cur["pos"].any():
                    raise AssertionError("%s: a block with two shape lines, or with values before its shape line" % path)
                cur["shape"] = SHAPES[w[0]]
                k = 9 if w[0] == "TRIANGLE" else 3
                cur["geom"][:k] = _floats(w[1:1 + k])
            elif w[0] == "COLOR":
                cur["col"] = _floats(w[1:4])
            elif w[0] == "EMISSION":
                cur["emis"] = _floats(w[1:4])
            elif w[0] == "POSITION":
                cur["pos"] = _floats(w[1:4])
            elif w[0] == "METALLIC":
                cur["mat"] = 1
            elif w[0] == "DIELECTRIC":
                cur["mat"] = 2
            elif w[0] == "IOR":
                cur["ior"] = _floats(w[1:2])
            elif w[0] != "ROTATION":
                # a top-level command ends the block (and is one)
                close()
                cur = None
                if w[0] in ("BG_COLOR", "DIMENSIONS", "CAMERA_POSITION", "CAMERA_RIGHT", "CAMERA_UP", "CAMERA_FORWARD",
                            "CAMERA_FOV_X"):
                    top[w[0]] = _floats(w[1:])
        close()
    return top, blocks


@functools.lru_cache(maxsize=None)
def oracle_scene(path):
    return U.OracleScene(path)


@functools.lru_cache(maxsize=None)
def shade_table(path):
    """per prepared-order id, an array of (albedo 3 f32, ior f32, emission 3 f32, material u32, type u32):
    albedo and emission from the scene text, the rest from the oracle's prim_info; and BG_COLOR"""
    top, blocks = scene_text(path)
    o = oracle_scene(path)
    info = o.prim_info()
    prims = np.frombuffer(o.dump_bvh()[1], np.uint8).reshape(-1, 52)
    tab = np.zeros(o.n_prims, np.dtype([("albedo", _f32, (3,)), ("ior", _f32), ("emission", _f32, (3,)),
                                        ("material", np.uint32), ("type", np.uint32)]))
    for i in range(o.n_prims):
        rec = prims[i]
        typ = int(rec[0:4].view(np.uint32)[0])
        key = (typ, rec[4:40].tobytes(), rec[40:52].tobytes())
        if key not in blocks:
            raise AssertionError("%s: primitive %d of the oracle's prepared order matches no block of the text" % (path, i))
        col, emis, mat, ior = blocks[key]
        pi = info[i]
        assert TYPE_CODE[pi["type"]] == typ and MATERIAL_CODE[pi["material"]] == mat, (path, i)
        assert _f32(pi["ior"]).tobytes() == ior, (path, i)
        assert pi["emissive"] == bool(np.frombuffer(emis, _f32).any()), (path, i)
        tab[i] = (np.frombuffer(col, _f32), _f32(pi["ior"]), np.frombuffer(emis, _f32), MATERIAL_CODE[pi["material"]],
                  TYPE_CODE[pi["type"]])
    return tab, top["BG_COLOR"][:3].copy()


def camera(path):
    top, _ = scene_text(path)
    W, H = _f32(top["DIMENSIONS"][0]), _f32(top["DIMENSIONS"][1])
    tx = _f32(np.tan(np.float64(top["CAMERA_FOV_X"][0] / _f32(2))))
    return {"W": W, "H": H, "tx": tx, "ty": tx * H / W, "pos": top["CAMERA_POSITION"][:3], "right": top["CAMERA_RIGHT"][:3],
            "up": top["CAMERA_UP"][:3], "fwd": top["CAMERA_FORWARD"][:3]}


def camera_rays(path, xy):
    """Camera::GetToRay (src/scene.cpp:180-187) for (n, 2) float32 positions, in float32 and in
    GetToRay's order, vectorised: (n, 6) float32"""
    c = camera(path)
    xy = np.ascontiguousarray(xy, _f32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        nx = ((_f32(2) * xy[:, 0] / c["W"] - _f32(1)) * c["tx"])[:, None]
        ny = (_f32(-1) * (_f32(2) * xy[:, 1] / c["H"] - _f32(1)) * c["ty"])[:, None]
        d = nx * c["right"][None, :] + ny * c["up"][None, :] + _f32(1) * c["fwd"][None, :]
    assert nx.dtype == _f32 and d.dtype == _f32
    return np.concatenate([np.broadcast_to(c["pos"], d.shape), d], axis=1).astype(_f32)


def dims(path):
    c = camera(path)
    return int(c["W"]), int(c["H"])


def centres(path):
    """the pixel centres of the whole frame, row-major: (W * H, 2) float32"""
    W, H = dims(path)
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(_f32)


def pixel_centres(xy_u32):
    """(x + 0.5, y + 0.5) in float32 for (n, 2) integer pixels"""
    p = np.asarray(xy_u32)
    return (p.astype(_f32) + _f32(0.5)).astype(_f32)


NONFINITE = 32


def subpixel_set(path):
    """N_SUB seeded positions uniform in [-0.25 W, 1.25 W) x [-0.25 H, 1.25 H), then 4 x 8 non-finite
    ones: x = NaN, y = NaN, y = +inf, x = -inf"""
    W, H = dims(path)
    rng = np.random.default_rng(SEED)
    xy = np.stack([rng.uniform(-0.25 * W, 1.25 * W, N_SUB), rng.uniform(-0.25 * H, 1.25 * H, N_SUB)], axis=1).astype(_f32)
    bad = np.stack([rng.uniform(0, W, NONFINITE), rng.uniform(0, H, NONFINITE)], axis=1).astype(_f32)
    bad[0:8, 0] = np.nan
    bad[8:16, 1] = np.nan
    bad[16:24, 1] = np.inf
    bad[24:32, 0] = -np.inf
    return np.concatenate([xy, bad]).astype(_f32)


def expected(pt, path, xy):
    """the expected FEATURE_DTYPE records of the positions xy, with the rays they were made from"""
    xy = np.ascontiguousarray(xy, _f32).reshape(-1, 2)
    rays = camera_rays(path, xy)
    ids, hits = oracle_scene(path).ray_intersection(rays)
    tab, bg = shade_table(path)
    out = np.zeros(len(xy), pt.FEATURE_DTYPE)
    hit = ids >= 0
    out["id"] = np.where(hit, ids, -1)
    out["t"][hit] = hits[hit, 0]
    out["n"][hit] = hits[hit, 1:4]
    out["interior"][hit] = (hits[hit, 4] != 0).astype(np.uint32)
    row = tab[ids[hit]]
    for k in ("albedo", "ior", "emission", "material", "type"):
        out[k][hit] = row[k]
    out["emission"][~hit] = bg
    # (a condition of every comparison: a NaN would compare on its payload)
    assert not np.isnan(out["t"][hit]).any() and not np.isnan(out["n"][hit]).any(), "an expected t or n is NaN on a hit row"
    return out, rays


@functools.lru_cache(maxsize=None)
def _expected_centres(path):
    pt = U.ptrace()
    out, rays = expected(pt, path, centres(path))
    out.setflags(write=False)
    rays.setflags(write=False)
    return out, rays


def expected_centres(name):
    """(path, read-only expected records of the frame's pixel centres, their rays), computed once"""
    path = U.golden_scene_path(name)
    out, rays = _expected_centres(path)
    return path, out, rays


@functools.lru_cache(maxsize=None)
def _expected_sub(path):
    pt = U.ptrace()
    xy = subpixel_set(path)
    out, rays = expected(pt, path, xy)
    for a in (xy, out, rays):
        a.setflags(write=False)
    return xy, out, rays


def expected_subpixel(name):
    path = U.golden_scene_path(name)
    return (path,) + _expected_sub(path)


def census(rec):
    """what the oracle's records hold, for the tests' conditions and their printed counts"""
    hit = rec["id"] >= 0
    c = {"n": len(rec), "misses": int((~hit).sum()), "interior": int(rec["interior"][hit].sum()),
         "emissive": int(rec["emission"][hit].any(axis=1).sum()), "ids": int(len(np.unique(rec["id"][hit])))}
    for code, name in U.PRIM_TYPES.items():
        c[name] = int((rec["type"][hit] == code).sum())
    for code, name in U.MATERIALS.items():
        c[name] = int((rec["material"][hit] == code).sum())
    return c


def print_census(name, c):
    print("%s: %s" % (name, " ".join("%s=%d" % kv for kv in sorted(c.items()))))


def check_conditions(name, rec):
    """what the issue asks of the oracle's answers, before anything is compared with them"""
    c = census(rec)
    print_census(name, c)
    if name == "dragon_64x64x16":
        assert c["triangle"] >= 128 and c["emissive"] >= 64 and c["interior"] >= 16
    if name == "mat_matrix_24x24x8":
        assert min(c["diffuse"], c["metallic"], c["dielectric"]) >= 64
        assert min(c["plane"], c["box"], c["ellipsoid"], c["triangle"]) >= 32
        assert c["emissive"] >= 16
    if name == "mat_inside_24x24x8":
        assert c["interior"] >= 256
    if name == "hw3s6_48x48x8":
        assert c["misses"] >= 32
    return c


def assert_records(got, want):
    """byte for byte, with the first differing record named"""
    assert got.dtype.itemsize == want.dtype.itemsize == 64 and len(got) == len(want)
    g = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), 16)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(len(want), 16)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert len(bad) == 0, "%d of %d records differ; first %d: got %s want %s" % (len(bad), len(w), bad[0], got[bad[0]],
                                                                              want[bad[0]])
