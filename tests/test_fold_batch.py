"""The end-of-path fold (fold_path, pt_devutil.h) loads a path's fold records in chunks of
PT_FOLD_CH vertices, deepest first, every record of a chunk at once, then the shading
records they name.  These cases walk it through vertex counts from 0 to RAY_DEPTH, at
depths on both sides of any chunk size from 4 to 8, in each engine that folds with it
(the path engine's end_item, k_wshade's shade_item) and in the default engine choice,
against the CPU oracle: image bytes, f32 radiance bits and ray count.

Two scenes, both test_gpu.py's mirror box with planes taken out, 4 samples, and a lattice
of small mirror balls added (without them no query outgrows a one-word aux stack, and
the `exact` setting would send nothing through k_wshade):
  box4    its ceiling (y = 3) and the wall behind the camera (z = 3) removed.  A PLANE is
          infinite, so the two parallel walls that are left still hold nearly every path
          until RAY_DEPTH cuts it (leaf 0, RAY_DEPTH vertices: full chunks and the
          remainder chunk); a few paths end early, at the emitter or through an opening.
  corner  only the floor, the left wall and the far wall left, no two of them parallel:
          paths leave after 0 to about 7 vertices with the background as their leaf.
"""
import numpy as np
import pytest

import _util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


W, H, SPP = 8, 8, 4
BG = (0.1, 0.2, 0.3)

HEAD = """DIMENSIONS %d %d
RAY_DEPTH %%d
SAMPLES %d

BG_COLOR %g %g %g

CAMERA_POSITION 0 0 0
CAMERA_RIGHT 1 0 0
CAMERA_UP 0 1 0
CAMERA_FORWARD 0 0 %%d
CAMERA_FOV_X 1.2
""" % ((W, H, SPP) + BG)

PLANES = {"floor": ("0 1 0", "0 -3 0"), "ceiling": ("0 -1 0", "0 3 0"), "left": ("1 0 0", "-3 0 0"),
          "right": ("-1 0 0", "3 0 0"), "far": ("0 0 1", "0 0 -3"), "behind": ("0 0 -1", "0 0 3")}
SCENES = {"box4": ["floor", "left", "right", "far"], "corner": ["floor", "left", "far"]}

# The box's four objects, and a lattice of small mirror balls in front of the camera: with
# them the auxiliary tree is deep enough for a query to outgrow a one-word aux stack
# (PT_TUNE lstack=1), which is what sends rays through k_wexact / k_wshade.
N_BALLS = 32
OBJECTS = """
NEW_PRIMITIVE
ELLIPSOID 0.15 0.15 0.15
POSITION 1 1 -2
COLOR 0 0 0
EMISSION 40 40 40

NEW_PRIMITIVE
ELLIPSOID 0.6 0.4 0.5
POSITION -1 -1 -2
COLOR 0.9 0.9 0.9
DIELECTRIC
IOR 1.5

NEW_PRIMITIVE
TRIANGLE 0 0 0 1 0 0 0 1 0
POSITION -0.5 0.5 -2.5
ROTATION 0 0.3826834 0 0.9238795
COLOR 0.8 0.6 0.4
METALLIC

NEW_PRIMITIVE
BOX 0.3 0.2 0.4
POSITION 0.8 -1.2 -1.5
COLOR 0.5 0.5 1.0
METALLIC
""" + "".join("""
NEW_PRIMITIVE
ELLIPSOID 0.14 0.14 0.14
POSITION %g %g %g
COLOR 0.9 0.9 0.9
METALLIC
""" % (-0.45 + 0.3 * (i % 4), -0.45 + 0.3 * (i // 4 % 4), -1.6 - 0.3 * (i // 16)) for i in range(N_BALLS))


def scene_text(scene, depth, forward_z):
    return HEAD % (depth, forward_z) + "".join("""
NEW_PRIMITIVE
PLANE %s
POSITION %s
COLOR 0.99 0.98 0.97
METALLIC
""" % PLANES[p] for p in SCENES[scene]) + OBJECTS


ENGINES = {"default": None, "path": "coop=0", "exact": "coop=0,lstack=1"}

_oracle = {}   # scene text -> the oracle's (image, radiance, counters): rendered once, read only


def render_vs_oracle(pt, tmp_path, scene, depth, forward_z):
    text = scene_text(scene, depth, forward_z)
    path = str(tmp_path / ("%s_d%d.txt" % (scene, depth)))
    with open(path, "w") as f:
        f.write(text)
    if text not in _oracle:
        _oracle[text] = U.OracleScene(path).render()
    orgb, orad, octr = _oracle[text]
    with pt.Scene.load(path) as s:
        rgb, rad, st = s.render(radiance=True)
    assert st["errors"] == 0
    assert rad.view(np.uint32).tolist() == orad.view(np.uint32).tolist()
    assert np.array_equal(rgb, orgb)
    assert st["rays"] == octr["rays"]
    return orad, octr, st


CASES = [("box4", d) for d in [1, 2, 5, 6, 7, 8, 9, 13, 17]] + [("corner", d) for d in [2, 6, 7]]


@pytest.mark.parametrize("engine", sorted(ENGINES))
@pytest.mark.parametrize("scene,depth", CASES)
def test_fold_every_vertex_count(pt, tmp_path, scene, depth, engine, monkeypatch):
    if ENGINES[engine]:
        monkeypatch.setenv("PT_TUNE", ENGINES[engine])
    _, octr, st = render_vs_oracle(pt, tmp_path, scene, depth, -1)
    # the scene does what it is for: some paths end before the depth cut ...
    if depth > 1:
        assert octr["rays"] < W * H * SPP * depth
    else:
        assert octr["rays"] == W * H * SPP   # (RAY_DEPTH 1: one ray per path, however it ends)
    # ... and some go on
    if depth >= 6:
        assert octr["rays"] > W * H * SPP
    if engine == "exact":
        # rays through k_wexact / k_wshade, and so through shade_item's fold
        assert st["handoff"]["exact"] > 0, st["handoff"]


@pytest.mark.parametrize("engine", sorted(ENGINES))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_fold_first_path_without_vertices(pt, tmp_path, scene, engine, monkeypatch):
    """The camera turned round (CAMERA_FORWARD 0 0 1), RAY_DEPTH 6, a fresh session: in
    `corner` nothing lies up and to the right of it, so a quarter of the pixels' paths all
    end with no vertex -- the fold of a slot whose fold records have never been written."""
    if ENGINES[engine]:
        monkeypatch.setenv("PT_TUNE", ENGINES[engine])
    orad, octr, _ = render_vs_oracle(pt, tmp_path, scene, 6, 1)
    if scene == "corner":
        # pixels that only ever saw the background (4 paths of no vertex each)
        only_bg = np.all(np.abs(orad.reshape(-1, 3) - np.array(BG, np.float32)) < 1e-6, axis=1)
        assert only_bg.sum() >= W * H // 4
