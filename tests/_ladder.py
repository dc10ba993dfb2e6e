"""Generated scenes that force the launch shapes the fixtures never reach (tests/test_shapes_host.py
on the CPU, tests/test_shapes.py on the GPU).  Nothing here is committed but the generator.

ladder(emitters)   a "scale ladder": N_PRIMS primitives, alternately BOX and ELLIPSOID, primitive k of
                   scale s = 1e-7 x 1.1^k (up to about 1e7), half-size 0.25 s, at
                   (+-(0.2..0.5) s, +-(0.1..0.4) s, -s), seen from (0, 0, 0.5) down -z.  The SAH build
                   cannot balance fourteen decades of scale: the wide aux tree comes out more than 21
                   levels deep, so a batch lane's aux stack no longer fits a 256-thread workgroup's LDS
                   (block 128), and the cooperative engine's teams of 8 and 16 no longer hold a descent.
                   Only primitives of scale in (1e-2, 1e2) carry EMISSION: an emitter of extreme scale
                   stalls Scene::RayTrace's emitter sampling ("Known stall").
                   "few": 8 emitters (the plan's LDS tables hold them, big = 0); "many": every fifth
                   primitive of that band and every one of its boxes besides (> QC_NEM, big = 1).
                   "stall": every fifth primitive whatever its scale -- the input of the stall,
                   for the CPU tests that pin it down; never rendered beyond the rows known to end.
mirror_box(depth)  test_gpu.py's mirror box (imported, not copied) at RAY_DEPTH `depth`.

guarded(text, ...) is the rule for every scene that reaches a GPU test: the oracle renders it first, at
the test's own size and sample count, in a child process with a 30 s limit; a timeout is a failure.
The CPU suite runs the same guard on the same scenes (test_shapes_host.py), so a scene whose
sampling never ends fails there, before any GPU test imports it.
"""
import os
import subprocess
import sys

import numpy as np

import _util as U

N_PRIMS = 338
W, H, SPP = 24, 16, 2
GUARD_SECONDS = 30
EMISSIVE_BAND = (1e-2, 1e2)   # scales whose primitives may carry EMISSION
QC_NEM = 8                    # (pt_kernels.h: emitter records the cooperative engine keeps in LDS)
PT_QUERY_SP_MAX = 127         # (pt_query.h: the aux stack's 7-bit counter)

HEAD = """DIMENSIONS %d %d
RAY_DEPTH 4
SAMPLES %d

BG_COLOR 0.1 0.2 0.3

CAMERA_POSITION 0 0 0.5
CAMERA_RIGHT 1 0 0
CAMERA_UP 0 1 0
CAMERA_FORWARD 0 0 -1
CAMERA_FOV_X 1.2
"""


def scale(k):
    return 1e-7 * 1.1 ** k


def in_band(k):
    return EMISSIVE_BAND[0] < scale(k) < EMISSIVE_BAND[1]


def emissive(emitters, k):
    if emitters == "stall":
        return k % 5 == 0
    if not in_band(k):
        return False
    if emitters == "few":
        # the band's every fifth primitive, the first 8 of them
        first = [j for j in range(N_PRIMS) if j % 5 == 0 and in_band(j)][:QC_NEM]
        return k in first
    assert emitters == "many"
    return k % 5 == 0 or k % 2 == 0   # (even k: the boxes)


def ladder_text(emitters, width=W, height=H, spp=SPP):
    rng = np.random.default_rng(338)
    out = [HEAD % (width, height, spp)]
    for k in range(N_PRIMS):
        s = scale(k)
        sx, sy = rng.choice([-1.0, 1.0], 2)
        x, y = sx * rng.uniform(0.2, 0.5) * s, sy * rng.uniform(0.1, 0.4) * s
        out.append("\nNEW_PRIMITIVE\n%s %.9g %.9g %.9g\nPOSITION %.9g %.9g %.9g\nCOLOR %.3f %.3f %.3f\n" % (
            "BOX" if k % 2 == 0 else "ELLIPSOID", 0.25 * s, 0.25 * s, 0.25 * s, x, y, -s,
            0.5 + 0.4 * (k % 3 == 0), 0.5 + 0.4 * (k % 3 == 1), 0.5 + 0.4 * (k % 3 == 2)))
        if emissive(emitters, k):
            out.append("EMISSION 2 2 2\n")
        elif k % 2:
            out.append("DIELECTRIC\nIOR 1.5\n")
        else:
            out.append("METALLIC\n")
    return "".join(out)


def n_emitters(emitters):
    return sum(emissive(emitters, k) for k in range(N_PRIMS))


def mirror_box_text(depth):
    import test_gpu
    return test_gpu.MIRROR_BOX % depth


def write_scene(name, text):
    """the scene's file under scenes/gen (ignored by git), named by its text"""
    os.makedirs(U.GEN, exist_ok=True)
    out = os.path.join(U.GEN, "%s_%s.txt" % (name, U.md5(text.encode())[:8]))
    if not os.path.exists(out):
        tmp = out + ".tmp%d" % os.getpid()
        with open(tmp, "w") as f:
            f.write(text)
        os.replace(tmp, out)
    return out


# ---- the guard: the oracle's render in a child process under a time limit ---------------------------
_GUARD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import _util as U
o = U.OracleScene(sys.argv[1])
win = tuple(int(v) for v in sys.argv[2:6])
rgb, rad, ctr = o.render(*win, spp=int(sys.argv[6]))
np.savez(sys.argv[7], rgb=rgb, rad=rad, rays=np.uint64(ctr["rays"]))
"""
_guarded = {}


def guarded(path, window=None, spp=0, seconds=GUARD_SECONDS, finite=True):
    """The oracle's (rgb, radiance, {"rays"}) of the scene at `path` -- of its whole frame at its own
    SAMPLES, or of window = (x0, y0, w, h) at spp --, rendered in a child process that is killed after
    `seconds`: an AssertionError then, and no caller goes on to a device with that scene.  Computed
    once per (scene, window, spp) and shared, read-only.  finite=False: for a scene whose reference
    radiance is known to hold NaNs (tests/_overlap.py "flat")."""
    key = (path, window, spp)
    if key in _guarded:
        return _guarded[key]
    o = U.OracleScene(path)   # (builds the oracle if need be; loading never samples)
    win = tuple(window) if window else (0, 0, o.W, o.H)
    out = "%s.guard_%d_%d_%d_%d_%d_%d.npz" % ((path,) + win + (spp, os.getpid()))
    try:
        try:
            subprocess.run([sys.executable, "-c", _GUARD % os.path.dirname(os.path.abspath(__file__)), path] +
                           [str(v) for v in win] + [str(spp), out], check=True, timeout=seconds,
                           stdout=subprocess.DEVNULL)
        except subprocess.TimeoutExpired:
            raise AssertionError("the oracle did not render %s %r x %d within %d s: the scene must not reach a GPU"
                                 % (os.path.basename(path), win, spp, seconds))
        with np.load(out) as z:
            rgb, rad, rays = z["rgb"], z["rad"], int(z["rays"])
    finally:
        if os.path.exists(out):
            os.remove(out)
    assert not finite or np.isfinite(rad).all()
    for a in (rgb, rad):
        a.setflags(write=False)
    _guarded[key] = (rgb, rad, {"rays": rays})
    return _guarded[key]


def ladder(emitters, width=W, height=H, spp=SPP):
    """the ladder scene's path; "few" and "many" are guarded at the size they are written with"""
    assert emitters in ("few", "many", "stall")
    path = write_scene("ladder_%s_%dx%dx%d" % (emitters, width, height, spp), ladder_text(emitters, width, height, spp))
    if emitters != "stall":
        guarded(path)
    return path


def mirror_box(depth):
    """the mirror box's path at RAY_DEPTH depth (8 x 8, 2 samples), guarded"""
    path = write_scene("mirror_box_d%d" % depth, mirror_box_text(depth))
    guarded(path)
    return path


_path_cases = {}


def path_case(pt, path):
    """The batch radiance records of the first sample of every pixel of the scene's frame (tests/_paths.py)
    and the oracle's guarded one-sample answers: {"records", "rad" (n, 3) f32, "rays", "size" (W, H), "nonzero" pixels};
    computed once and shared, read-only."""
    if path not in _path_cases:
        import _paths as P
        o = U.OracleScene(path)
        _, rad, ctr = guarded(path, (0, 0, o.W, o.H), 1)
        with pt.Scene.load(path) as s:
            rec = P.pixel_records(pt, s, o.W, (0, 0, o.W, o.H))
        rad = np.ascontiguousarray(rad.reshape(-1, 3))
        assert ctr["rays"] > len(rec), "the oracle traced no path beyond its first ray"
        for a in (rec, rad):
            a.setflags(write=False)
        _path_cases[path] = {"records": rec, "rad": rad, "rays": ctr["rays"], "size": (o.W, o.H),
                             "nonzero": int((rad != 0).any(axis=1).sum())}
    return _path_cases[path]


def check_tree(info):
    """the tree facts that make a ladder scene useful: a builder change that flattens the tree fails here"""
    assert info["aux_depth"] >= 21, "3 x aux_depth + 1 >= 64 needs a wide aux tree 21 deep, got %d" % info["aux_depth"]
    assert info["aux_depth"] <= 42, "pt_scene_prepare accepts aux stacks of at most 127 words"
    return info
