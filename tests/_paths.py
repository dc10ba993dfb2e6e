"""Batch radiance records and their expected values (tests/test_paths_host.py, tests/test_paths.py).

Expected values never come from the code under test.  A record is built so that it IS the first
sample of a pixel of the scene's own camera, and the CPU oracle's one-sample render of that pixel
is then what the record must return:

  pixel (x, y) of a scene of width W has the stream seed i = y * W + x; its first sample draws two
  uniforms u1, u2 (U.oracle_rng), the ray is Camera::GetToRay(float32(x) + u1, float32(y) + u2)
  (Scene.camera_rays), and RayTrace goes on with the stream's state after those two draws --
  minstd_rand steps twice: seed' = (i % m or 1) * 48271**2 % m, m = 2**31 - 1, in Python integers.
  The oracle's radiance at 1 spp is (1.f / 1) * (0 + RayTrace), so it equals got + float32(0).
"""
import os

import numpy as np

import _util as U

M31 = 2 ** 31 - 1
# whole frames, and a window of a benchmark configuration
FRAMES = ["mat_matrix_24x24x8", "mat_inside_24x24x8", "mat_camera_23x17x8", "dragon_glass_64x64x8", "hw3s3_48x48x8",
          "rabbid_48x48x4", "many_lights_48x48x8", "dragon_d10_glass_48x48x16"]
WINDOWS = ["c4glass_s4_win_900_560_16x16"]
# the SAMPLES-1 variants recorded from the untouched reference (tests/golden/make_golden_paths.py):
# name -> (scene source, generator args or None)
S1 = {
    "dragon_glass_64x64": ("practice5_dragon_10k.txt", (64, 64, 1, False, "glass")),
    "hw3s3_48x48": ("hw3_sample3.txt", (48, 48, 1, False, "diffuse")),
    "mat_matrix_24x24": ("material:matrix", None),
}


def fixture(name):
    m = U.manifest()
    return m["images"].get(name) or m["deep"][name]


def fixture_scene(name):
    e = fixture(name)
    return U.scene_path(e["scene"], tuple(e["gen"]) if e["gen"] else None)


def s1_scene_text(src):
    """a material scene's text with its SAMPLES line set to 1"""
    text = U._material_scenes.scene_text(src[len(U._material_scenes.PREFIX):])
    lines = ["SAMPLES 1" if ln.split()[:1] == ["SAMPLES"] else ln for ln in text.split("\n")]
    assert lines.count("SAMPLES 1") == 1
    return "\n".join(lines)


def s1_scene(name):
    """the scene file of a SAMPLES-1 variant"""
    src, gen = S1[name]
    if gen is not None:
        return U.scene_path(src, gen)
    text = s1_scene_text(src)
    os.makedirs(U.GEN, exist_ok=True)
    out = os.path.join(U.GEN, "%s_s1_%s.txt" % (src.replace(":", "_"), U.md5(text.encode())[:8]))
    if not os.path.exists(out):
        with open(out + ".tmp%d" % os.getpid(), "w") as f:
            f.write(text)
        os.replace(out + ".tmp%d" % os.getpid(), out)
    return out


def paths_manifest():
    import json
    with open(os.path.join(U.GOLDEN, "paths_manifest.json")) as f:
        return json.load(f)


def seed_after_two_draws(i):
    return (i % M31 or 1) * 48271 ** 2 % M31


def pixel_records(pt, scene, W, window):
    """the records of the first sample of every pixel of window = (x0, y0, w, h), row-major"""
    x0, y0, w, h = window
    rec = np.zeros(w * h, pt.PATH_DTYPE)
    xy = np.zeros((w * h, 2), np.float32)
    for k in range(w * h):
        x, y = x0 + k % w, y0 + k // w
        i = y * W + x
        u = U.oracle_rng(i, 2)[:2]
        xy[k] = (np.float32(x) + u[0], np.float32(y) + u[1])
        rec["seed"][k] = seed_after_two_draws(i)
    rays = scene.camera_rays(xy)
    rec["o"], rec["d"] = rays[:, :3], rays[:, 3:]
    return rec


_expected = {}


def expected(pt, name, path=None, window=None, census=False):
    """The records of a fixture's pixels (its whole frame, or its window) and the oracle's answers at
    one sample per pixel: {"path", "records", "rad" (n, 3) f32, "rays", "census"}.  Computed once
    and shared (read-only).  The conditions every test needs of its inputs are asserted here, on the
    oracle's answers."""
    if name in _expected:
        return _expected[name]
    if path is None:
        path = fixture_scene(name)
        window = fixture(name)["window"]
    o = U.OracleScene(path)
    win = tuple(window) if window else (0, 0, o.W, o.H)
    _, rad, ctr = o.render(*win, spp=1, census=census or name.startswith("mat_matrix"))
    with pt.Scene.load(path) as s:
        rec = pixel_records(pt, s, o.W, win)
    rad = np.ascontiguousarray(rad.reshape(-1, 3))
    n = len(rec)
    assert ctr["rays"] > n, "%s: the oracle traced no path beyond its first ray" % name
    assert (rad != 0).any(axis=1).sum() * 2 >= n, "%s: fewer than half of the oracle's pixels are non-zero" % name
    assert np.isfinite(rad).all()
    if "census" in ctr:
        cen = ctr["census"].sum(axis=0)   # (event, outside / interior)
        if name.startswith("mat_matrix"):
            for e, ev in enumerate(U.CENSUS_EVENTS):
                for side in (0, 1):
                    if (ev, side) != ("diffuse", 1):
                        assert cen[e, side] >= 30, "%s: %s (interior %d) reached %d times" % (name, ev, side, cen[e, side])
    for a in (rec, rad):
        a.setflags(write=False)
    _expected[name] = {"path": path, "records": rec, "rad": rad, "rays": ctr["rays"], "census": ctr.get("census")}
    return _expected[name]


def assert_radiance(got, want_rad):
    """the bits of got + float32(0) against the oracle's one-sample mean"""
    g = (got["rgb"] + np.float32(0)).astype(np.float32)
    assert g.shape == want_rad.shape
    bad = np.flatnonzero((g.view(np.uint32) != want_rad.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, "%d of %d paths differ, first %d: %r != %r" % (len(bad), len(g), bad[0], g[bad[0]], want_rad[bad[0]])


def host_run(pt, name, path, records):
    """the host execution's outputs and counters of `records` on the scene at `path` (cached)"""
    key = ("host", name)
    if key not in _expected:
        with pt.Scene.load(path) as s:
            out, ctr = s.selftest_paths_host(records)
        out.setflags(write=False)
        _expected[key] = (out, ctr)
    return _expected[key]
