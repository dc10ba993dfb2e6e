"""The guided filter (include/pt.h "guided filter") restated in numpy float32, for tests/test_filter_host.py
and tests/test_filter.py.

Nothing here comes from the code under test: the features are tests/_features.py's (oracle, camera
restatement, scene-text parser), the radiance is tests/golden/rad_<name>.f32.  Every scalar is a
np.float32 and every numpy operation is one rounded float32 operation, in the definition's order; the 25
taps are visited dy outer, dx inner.  A tap the definition skips enters with the weight 0 and the colour 0,
which adds nothing, bit for bit.
"""
import functools
import os

import numpy as np

import _features as F
import _util as U

_f32 = np.float32
K = (_f32(1 / 16), _f32(1 / 4), _f32(3 / 8), _f32(1 / 4), _f32(1 / 16))
DEFAULTS = {"levels": 3, "sigma_c": 1.0, "sigma_z": 0.05, "sigma_a": 0.1, "normal_pow2": 5}
CENSUS_KEYS = ("outside", "class", "nonfinite", "wn0", "ez", "ea", "ec", "kept")
SCENES = ("dragon_64x64x16", "hw3s6_48x48x8", "mat_matrix_24x24x8", "mat_camera_23x17x8", "dragon_glass_40x24x7")
LEVELS = (1, 3, 5)
SYNTH_SIZES = ((1, 1), (1, 7), (5, 1), (33, 9), (70, 37))   # (w, h)
SEED = 20261021


def options(**changes):
    o = dict(DEFAULTS)
    for k in changes:
        assert k in o, k
    o.update(changes)
    return o


def guides(feat):
    """(n (.., 3), t, a (.., 3), cls) of FEATURE_DTYPE records"""
    hit = feat["id"] >= 0
    with np.errstate(invalid="ignore"):
        emits = (feat["emission"] != _f32(0)).any(axis=-1)
    cls = np.where(hit, np.uint32(1) + feat["material"] + np.uint32(4) * emits.astype(np.uint32), np.uint32(0))
    return feat["n"], feat["t"], feat["albedo"], cls.astype(np.uint32)


def _inv(g):
    with np.errstate(all="ignore"):
        return np.where(g > _f32(0), _f32(1) / g, _f32(0)).astype(_f32)


def _sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def filtered(feat, rad, **opts):
    """(the filtered (h, w, 3) float32, the census of the run) for (h, w) records and (h, w, 3) radiance"""
    o = options(**opts)
    rad = np.asarray(rad, _f32)
    h, w = rad.shape[:2]
    feat = np.asarray(feat).reshape(h, w)
    n, t, a, cls = guides(feat)
    sigma_c, sigma_z, sigma_a = _f32(o["sigma_c"]), _f32(o["sigma_z"]), _f32(o["sigma_a"])
    ia = _inv(np.asarray(sigma_a * sigma_a, _f32))
    Y, X = np.mgrid[0:h, 0:w]
    census = dict.fromkeys(CENSUS_KEYS, 0)
    c = rad.copy()
    with np.errstate(all="ignore"):
        gz = sigma_z * t
        gz = gz * gz
        iz = _inv(gz)
        for L in range(o["levels"]):
            s = 1 << L
            sc = sigma_c * _f32(2.0 ** -L)
            ic = _inv(np.asarray(sc * sc, _f32))
            fin = np.isfinite(c).all(axis=2)
            acc = np.zeros((h, w, 3), _f32)
            ws = np.zeros((h, w), _f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if dx == 0 and dy == 0:
                        wc = _f32(9 / 64)
                        acc = acc + wc * c
                        ws = ws + wc
                        continue
                    qx, qy = X + dx * s, Y + dy * s
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    lx, ly = np.where(inside, qx, X), np.where(inside, qy, Y)
                    nq, tq, aq, clsq, cq, finq = n[ly, lx], t[ly, lx], a[ly, lx], cls[ly, lx], c[ly, lx], fin[ly, lx]
                    d = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    d = np.where(d > _f32(0), d, _f32(0)).astype(_f32)
                    for _ in range(o["normal_pow2"]):
                        d = d * d
                    wn = np.where(cls == 0, _f32(1), d).astype(_f32)
                    dz = t - tq
                    ez = dz * dz
                    ea = _sq3(a - aq)
                    ec = _sq3(c - cq)
                    tz, ta, tc = ez * iz, ea * ia, ec * ic
                    D = ((_f32(1) + tz) * (_f32(1) + ta)) * (_f32(1) + tc)
                    wt = (K[dy + 2] * K[dx + 2] * wn) / D
                    wt = np.where(wt > _f32(0), wt, _f32(0)).astype(_f32)
                    same = clsq == cls
                    keep = inside & same & finq
                    wt = np.where(keep, wt, _f32(0)).astype(_f32)
                    acc = acc + wt[..., None] * np.where(keep[..., None], cq, _f32(0)).astype(_f32)
                    ws = ws + wt
                    assert d.dtype == D.dtype == wt.dtype == acc.dtype == ws.dtype == _f32
                    # the census, over the taps of finite centre pixels; a tap is counted under the first
                    # rule that skips it, a tap no rule skips under every stopping term that applies to it
                    census["outside"] += int((fin & ~inside).sum())
                    census["class"] += int((fin & inside & ~same).sum())
                    census["nonfinite"] += int((fin & inside & same & ~finq).sum())
                    live = fin & keep
                    census["wn0"] += int((live & (wn == 0)).sum())
                    census["ez"] += int((live & (tz > 1)).sum())
                    census["ea"] += int((live & (ta > 1)).sum())
                    census["ec"] += int((live & (tc > 1)).sum())
                    census["kept"] += int((live & (wt > 0)).sum())
            inv = _f32(1) / ws
            out = acc * inv[..., None]
            assert (ws[fin] >= _f32(9 / 64)).all()
            c = np.where(fin[..., None], out, c).astype(_f32)
    return c, census


def print_census(name, c):
    print("%s: %s" % (name, " ".join("%s=%d" % (k, c[k]) for k in CENSUS_KEYS)))


def radiance(name):
    path = U.golden_scene_path(name)
    w, h = F.dims(path)
    return np.fromfile(os.path.join(U.GOLDEN, "rad_%s.f32" % name), _f32).reshape(h, w, 3)


def poisoned(name):
    """the fixture's radiance with three pixels made non-finite: NaN at flat index 7, +inf in channel 1 at
    W + 3, -inf at W * H / 2 + 5"""
    rad = radiance(name).copy()
    h, w = rad.shape[:2]
    flat = rad.reshape(-1, 3)
    flat[7 % (w * h)] = np.nan
    flat[(w + 3) % (w * h), 1] = np.inf
    flat[(w * h // 2 + 5) % (w * h)] = -np.inf
    return rad


def scene_features(name):
    """(path, the (h, w) expected feature records of the fixture's pixel centres)"""
    path, rec, _ = F.expected_centres(name)
    w, h = F.dims(path)
    return path, rec.reshape(h, w)


@functools.lru_cache(maxsize=None)
def _expected_scene(name, items):
    _, feat = scene_features(name)
    out, census = filtered(feat, poisoned(name), **dict(items))
    out.setflags(write=False)
    return out, census


def expected_scene(name, **opts):
    """(expected output, census) for the fixture with its three poisoned pixels, computed once per option set"""
    return _expected_scene(name, tuple(sorted(opts.items())))


def synthetic(pt, w, h):
    """a seeded frame with guides over all classes and special values in guides and colours:
    ((h, w) FEATURE_DTYPE records, (h, w, 3) float32 radiance)"""
    rng = np.random.default_rng(SEED + 1000 * w + h)
    n = w * h
    feat = np.zeros(n, pt.FEATURE_DTYPE)
    feat["id"] = rng.integers(-1, 6, n)
    # (a few orientations and depths, so that neighbours often share them)
    dirs = rng.normal(size=(5, 3)).astype(_f32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True).astype(_f32)
    feat["n"] = dirs[rng.integers(0, 5, n)]
    feat["t"] = (rng.integers(1, 4, n) + rng.uniform(0, 0.05, n)).astype(_f32)
    feat["albedo"] = rng.choice(np.array([0.1, 0.15, 0.8], _f32), (n, 3))
    feat["material"] = rng.integers(0, 3, n)
    feat["emission"][:, 1] = np.where(rng.random(n) < 0.3, rng.choice(np.array([2.0, -0.0, np.nan], _f32), n), 0)
    feat["ior"] = 1.5
    feat["type"] = 2
    miss = feat["id"] < 0
    for k in ("t", "n", "albedo", "ior", "type", "material", "interior"):
        feat[k][miss] = 0
    rad = rng.gamma(0.7, 1.0, (n, 3)).astype(_f32)
    if n >= 40:
        pick = rng.choice(n, 16, replace=False)
        feat["t"][pick[0:2]] = np.inf
        feat["n"][pick[2:4], 0] = np.nan
        feat["albedo"][pick[4:6], 2] = np.nan
        feat["n"][pick[6:8]] = -0.0
        feat["t"][pick[8]] = -0.0
        rad[pick[9]] = np.nan
        rad[pick[10], 2] = np.inf
        rad[pick[11], 0] = -np.inf
        rad[pick[12]] = -0.0
        rad[pick[13]] = 3.0e38   # sums of it overflow: a pixel that becomes non-finite at a later level
        rad[pick[14]] = 1.0e-40
    elif n > 1:
        rad[n // 2, 1] = np.nan
    return feat.reshape(h, w), rad.reshape(h, w, 3)


def assert_frames(got, want, what=""):
    """byte for byte, with the first differing pixel named"""
    got, want = np.ascontiguousarray(got, _f32), np.ascontiguousarray(want, _f32)
    assert got.shape == want.shape, (got.shape, want.shape)
    g, w = got.view(np.uint32).reshape(-1, 3), want.view(np.uint32).reshape(-1, 3)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert len(bad) == 0, "%s: %d of %d pixels differ; first %d: got %s want %s" % (
        what, len(bad), len(w), bad[0], got.reshape(-1, 3)[bad[0]], want.reshape(-1, 3)[bad[0]])
