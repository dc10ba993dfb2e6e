"""Pixel-sample states, the cases both test files run and their expected values
(tests/test_pixels_host.py on the host twin, tests/test_pixels.py on the GPU).

Expected values never come from the code under test.  They are the CPU oracle's render of the
record's pixel at SAMPLES = the record's total (U.OracleScene.render(window, spp=S): the oracle's
mean is 1.f / S * sum of the very loop a record restates), and the committed radiance and images
recorded from the untouched reference.  Comparisons are on f32 bits.

A case takes `run(scene, state, counts=None, spp=0) -> (state after, stats)`: the host twin
(Scene.selftest_pixels_host) or a GPU path (Scene.sample_pixels, PixelQuery).
"""
import os

import numpy as np

import _paths as P
import _util as U

M31 = 2 ** 31 - 1
# the fixtures recorded at odd SAMPLES (3, 5, 7) and the material matrix at 8
WHOLE_FRAMES = ["p51_40x24x3", "hw3s4_24x40x5", "dragon_glass_40x24x7", "mat_matrix_24x24x8"]
DRAGON = "dragon_glass_64x64x8"
DEPTH0 = ("DIMENSIONS 8 6\nRAY_DEPTH 0\nSAMPLES 1\nBG_COLOR 0.2 0.3 0.4\nCAMERA_POSITION 0 0 4\nCAMERA_RIGHT 1 0 0\n"
          "CAMERA_UP 0 1 0\nCAMERA_FORWARD 0 0 -1\nCAMERA_FOV_X 1.2\nNEW_PRIMITIVE\nBOX 0.5 0.5 0.5\nCOLOR 1 0 0\n"
          "NEW_PRIMITIVE\nELLIPSOID 0.3 0.3 0.3\nPOSITION 1 0 0\nEMISSION 2 2 2\n")
SAVED_BIT = 1 << 31

_cache = {}


def golden(name):
    """a fixture's manifest entry, scene path, image (h, w, 3) u8 and radiance (h, w, 3) f32, md5-checked"""
    if ("golden", name) not in _cache:
        m = P.fixture(name)
        raw_img = open(os.path.join(U.GOLDEN, "img_%s.ppm" % name), "rb").read()
        raw_rad = open(os.path.join(U.GOLDEN, "rad_%s.f32" % name), "rb").read()
        assert U.md5(raw_img) == m["ppm_md5"] and U.md5(raw_rad) == m["rad_md5"]
        img = U.read_ppm(os.path.join(U.GOLDEN, "img_%s.ppm" % name))
        rad = np.frombuffer(raw_rad, np.float32).reshape(img.shape)
        _cache["golden", name] = (m, P.fixture_scene(name), img, rad)
    return _cache["golden", name]


def oracle_render(path, window, spp):
    """the oracle's (rgb (n, 3), radiance (n, 3), counters) of window = (x0, y0, w, h) at spp, row-major,
    computed once and shared (read-only)"""
    key = ("oracle", path, tuple(window), spp)
    if key not in _cache:
        rgb, rad, ctr = U.OracleScene(path).render(*window, spp=spp)
        rgb, rad = np.ascontiguousarray(rgb.reshape(-1, 3)), np.ascontiguousarray(rad.reshape(-1, 3))
        assert np.isfinite(rad).all()
        rgb.setflags(write=False)
        rad.setflags(write=False)
        _cache[key] = (rgb, rad, ctr)
    return _cache[key]


def window_xy(window):
    x0, y0, w, h = window
    k = np.arange(w * h)
    return np.stack([x0 + k % w, y0 + k // w], axis=1).astype(np.uint32)


def assert_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(len(got), -1).any(axis=1))
    assert len(bad) == 0, "%s: %d of %d records differ, first %d: %r != %r" % (
        what, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]])


def assert_pixels_kept(before, after):
    assert np.array_equal(before["x"], after["x"]) and np.array_equal(before["y"], after["y"])


def minstd_steps(seed, k):
    """minstd_rand(seed)'s state after k draws, in Python integers"""
    return (seed % M31 or 1) * pow(48271, k, M31) % M31


# ---- 1. whole frames at the reference's sample count ---------------------------------------------
def case_whole_frame(pt, run, name):
    m, path, img, rad = golden(name)
    with pt.Scene.load(path) as s:
        inf = s.info
        W, H, S = inf["width"], inf["height"], inf["samples"]
        assert (H, W, 3) == img.shape and name.endswith("x%d" % S)
        window = (0, 0, W, H)
        state = s.pixel_init(window_xy(window))
        assert state["rng"][0] == 1 and state["rng"][W + 1] == W + 1 and not state["samples"].any()
        out, st = run(s, state, spp=S)
        mean, rgb = s.pixel_resolve(out)
    _, orad, octr = oracle_render(path, window, S)
    assert (rad.reshape(-1, 3) != 0).any(axis=1).sum() * 2 >= W * H, "fewer than half of the fixture's pixels are non-zero"
    assert_bits(mean, rad.reshape(-1, 3), name + " against the reference's recorded radiance")
    assert_bits(mean, orad, name + " against the oracle")
    assert np.array_equal(rgb, img.reshape(-1, 3))
    assert (out["samples"] == S).all()
    assert_pixels_kept(state, out)
    assert st["errors"] == 0 and st["rays"] == octr["rays"] and st["samples"] == W * H * S
    return out, st


# ---- 2. resume ----------------------------------------------------------------------------------------
def case_resume(pt, run, name, splits):
    """every way of `splits` (tuples of run lengths with one total) gives the same 32-byte states,
    which resolve to the fixture; returns the states after the first run of splits[0]"""
    m, path, img, rad = golden(name)
    ends, first = [], None
    with pt.Scene.load(path) as s:
        inf = s.info
        state0 = s.pixel_init(window_xy((0, 0, inf["width"], inf["height"])))
        for parts in splits:
            assert sum(parts) == inf["samples"]
            state = state0
            for k, a in enumerate(parts):
                state, st = run(s, state, spp=a)
                assert st["errors"] == 0 and st["samples"] == a * len(state)
                if first is None and k == 0:
                    first = state
            ends.append(state)
        mean, rgb = s.pixel_resolve(ends[0])
    for parts, e in zip(splits[1:], ends[1:]):
        assert e.tobytes() == ends[0].tobytes(), "runs of %r and of %r end in different states" % (splits[0], parts)
    assert_bits(mean, rad.reshape(-1, 3), name)
    assert np.array_equal(rgb, img.reshape(-1, 3))
    return first


# ---- 3. per-pixel counts ------------------------------------------------------------------------------
def case_counts(pt, run, name, window):
    m, path, img, rad = golden(name)
    x0, y0, w, h = window
    n = w * h
    counts = (1 + (np.arange(n) * 7) % 8).astype(np.uint32)
    assert set(counts.tolist()) == set(range(1, 9))
    want = np.zeros((n, 3), np.float32)
    for c in range(1, 9):
        _, orad, _ = oracle_render(path, window, c)
        want[counts == c] = orad[counts == c]
    with pt.Scene.load(path) as s:
        assert s.info["samples"] == 8
        state = s.pixel_init(window_xy(window))
        mid, st1 = run(s, state, counts=counts)
        mean, _ = s.pixel_resolve(mid)
        assert_bits(mean, want, name + " at 1 + (k * 7) % 8 samples")
        assert np.array_equal(mid["samples"], counts) and st1["samples"] == int(counts.sum()) and st1["errors"] == 0
        rest = (8 - counts).astype(np.uint32)
        assert (rest == 0).sum() >= n // 8 - 1
        end, st2 = run(s, mid, counts=rest)
        mean, rgb = s.pixel_resolve(end)
    assert end[rest == 0].tobytes() == mid[rest == 0].tobytes(), "a count of 0 changed its record"
    assert (end["samples"] == 8).all() and st2["samples"] == int(rest.sum()) and st2["errors"] == 0
    assert_bits(mean, rad[y0:y0 + h, x0:x0 + w].reshape(-1, 3), name + " brought to 8 samples")
    assert np.array_equal(rgb, img[y0:y0 + h, x0:x0 + w].reshape(-1, 3))
    _, _, octr = oracle_render(path, window, 8)
    assert st1["rays"] + st2["rays"] == octr["rays"]


# ---- 4. shapes ----------------------------------------------------------------------------------------
def dragon_expected():
    """(scene path, the oracle's radiance of the dragon frame's 64 x 64 pixels at 2 samples)"""
    path = golden(DRAGON)[1]
    return path, oracle_render(path, (0, 0, 64, 64), 2)[1]


def case_first_pixels(pt, run, n):
    path, orad = dragon_expected()
    with pt.Scene.load(path) as s:
        state = s.pixel_init(window_xy((0, 0, 64, 64))[:n])
        out, st = run(s, state, spp=2)
        mean, _ = s.pixel_resolve(out)
    assert_bits(mean, orad[:n], "the first %d pixels" % n)
    assert st["samples"] == 2 * n and st["errors"] == 0 and st["rays"] >= 2 * n
    return out, st


def case_scattered(pt, run):
    path, orad = dragon_expected()
    rng = np.random.default_rng(11)
    pix = rng.permutation(64 * 64)[:333]
    pix[200] = pix[17]   # one pixel twice
    assert len(set(pix.tolist())) == 332
    xy = np.stack([pix % 64, pix // 64], axis=1).astype(np.uint32)
    with pt.Scene.load(path) as s:
        out, st = run(s, s.pixel_init(xy), spp=2)
        mean, _ = s.pixel_resolve(out)
    assert_bits(mean, orad[pix], "scattered pixels")
    assert out[200].tobytes() == out[17].tobytes()
    assert st["samples"] == 2 * len(pix) and st["errors"] == 0


def case_one_long_record(pt, run):
    """one record with 200 samples among 300 with 1"""
    path = P.s1_scene("hw3s3_48x48")
    long_at, long_xy = 137, (29, 31)
    xy = window_xy((0, 0, 48, 48))[:301].copy()
    xy[long_at] = long_xy
    counts = np.ones(301, np.uint32)
    counts[long_at] = 200
    want = np.array(oracle_render(path, (0, 0, 48, 48), 1)[1][:301])
    want[long_at] = oracle_render(path, (long_xy[0], long_xy[1], 1, 1), 200)[1][0]
    assert want[long_at].any()
    with pt.Scene.load(path) as s:
        out, st = run(s, s.pixel_init(xy), counts=counts)
        mean, _ = s.pixel_resolve(out)
    assert_bits(mean, want, "one long record")
    assert np.array_equal(out["samples"], counts) and st["samples"] == 500 and st["errors"] == 0
    return out


# ---- 5. depth -----------------------------------------------------------------------------------------
def case_depth_1(pt, run):
    """override(ray_depth=1) against the oracle on the same scene written with RAY_DEPTH 1"""
    gen = (40, 24, 7, False, "glass")
    src = "practice5_dragon_10k.txt"
    window = (0, 0, 40, 24)
    _, orad, octr = oracle_render(U.scene_path(src, gen + (1,)), window, 3)
    assert orad.any() and octr["rays"] == 40 * 24 * 3
    with pt.Scene.load(U.scene_path(src, gen)) as s:
        s.override(ray_depth=1)
        out, st = run(s, s.pixel_init(window_xy(window)), spp=3)
        mean, _ = s.pixel_resolve(out)
    assert_bits(mean, orad, "RAY_DEPTH 1")
    assert st["rays"] == octr["rays"] and st["errors"] == 0


def case_depth_10(pt, run):
    """the depth-10 glass dragon, a 16 x 16 window at 4 samples"""
    path = P.fixture_scene("dragon_d10_glass_48x48x16")
    window = (16, 16, 16, 16)
    _, orad, octr = oracle_render(path, window, 4)
    assert octr["rays"] > 3 * 256 * 4, "the window's paths are not deep"
    with pt.Scene.load(path) as s:
        assert s.info["ray_depth"] == 10
        out, st = run(s, s.pixel_init(window_xy(window)), spp=4)
        mean, _ = s.pixel_resolve(out)
    assert_bits(mean, orad, "RAY_DEPTH 10")
    assert st["rays"] == octr["rays"] and st["errors"] == 0


def case_depth_0(pt, run):
    with pt.Scene.loads(DEPTH0) as s:
        assert s.info["ray_depth"] == 0
        state = s.pixel_init(window_xy((0, 0, 8, 6)))
        counts = (np.arange(48) % 7).astype(np.uint32)
        out, st = run(s, state, counts=counts)
        out2, st2 = run(s, out, spp=3)
    for o, total in ((out, counts), (out2, counts + 3)):
        assert not o["sum"].view(np.uint32).any() and not o["saved"].view(np.uint32).any()
        assert np.array_equal(o["samples"], total)
        assert o["rng"].tolist() == [minstd_steps(i, 2 * int(t)) for i, t in enumerate(total)]
    assert st["rays"] == 0 and st["samples"] == int(counts.sum()) and st2["samples"] == 3 * 48
    assert st["errors"] == 0 and st["plane_tests"] == 0


# ---- 6. seeds -----------------------------------------------------------------------------------------
def case_seed_reduction(pt, run):
    name = "p51_40x24x3"
    m, path, img, rad = golden(name)
    xy = window_xy((0, 0, 40, 24))
    i = np.arange(40 * 24, dtype=np.uint64)
    with pt.Scene.load(path) as s:
        a = s.pixel_init(xy)
        b = s.pixel_init(xy, seeds=(xy[:, 1] * 40 + xy[:, 0]))
        c = s.pixel_init(xy, seeds=(i + M31).astype(np.uint32))
        d = s.pixel_init(xy[:1], seeds=[M31])
        assert a.tobytes() == b.tobytes() == c.tobytes() and d.tobytes() == a[:1].tobytes()
        assert a["rng"][0] == 1 and a["rng"][1] == 1 and a["rng"][2] == 2   # seeds 0 and 1 are one stream
        out, st = run(s, c, spp=3)
        mean, _ = s.pixel_resolve(out)
    assert_bits(mean, rad.reshape(-1, 3), "seeds i + (2^31 - 1)")


def arbitrary_records(pt, s, W, H, n=400):
    """n pixels and seeds drawn at random, and the batch radiance records of their first samples as
    tests/_paths.py builds them: the two jitter draws from the oracle's stream, the camera ray, and
    the stream's state after two draws in Python integers"""
    rng = np.random.default_rng(23)
    xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], axis=1).astype(np.uint32)
    seeds = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    seeds[:3] = (0, M31, 2 ** 32 - 1)
    rec = np.zeros(n, pt.PATH_DTYPE)
    fxy = np.zeros((n, 2), np.float32)
    for k in range(n):
        u = U.oracle_rng(int(seeds[k]), 2)[:2]
        fxy[k] = (np.float32(xy[k, 0]) + u[0], np.float32(xy[k, 1]) + u[1])
        rec["seed"][k] = P.seed_after_two_draws(int(seeds[k]))
    rays = s.camera_rays(fxy)
    rec["o"], rec["d"] = rays[:, :3], rays[:, 3:]
    return xy, seeds, rec


def case_arbitrary_seeds_cross_engine(pt, run, radiance):
    """A CROSS-ENGINE check, not an oracle one: a record's first sample against the batch radiance
    engine's value of the same ray and stream (`radiance(scene, records)`: Scene.radiance on the GPU,
    selftest_paths_host on the host), whose own tests hold it to the oracle."""
    path = golden(DRAGON)[1]
    with pt.Scene.load(path) as s:
        xy, seeds, rec = arbitrary_records(pt, s, 64, 64)
        want, wst = radiance(s, rec)
        out, st = run(s, s.pixel_init(xy, seeds=seeds), spp=1)
    assert_bits(out["sum"], (np.float32(0) + want["rgb"]).astype(np.float32), "arbitrary seeds, one sample")
    assert st["rays"] == wst["rays"] == int(want["rays"].sum()) and st["errors"] == 0
    assert (out["samples"] == 1).all()
