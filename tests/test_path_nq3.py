"""The path engine's full rounds in their second shape: k_wpath<3, false>, three query
waves and three done rings per shade wave, 3 workgroups per CU (PT_TUNE nq=3; DESIGN.md
§4.4).  Everything is compared with the CPU oracle: image bytes, f32 radiance bits and
ray count.

Scenes: test_fold_batch.py's two (the lattice of mirror balls in the open box, and the
corner) at 96 x 64, 4 samples, RAY_DEPTH 6.  With one workgroup per CU (wg_per_cu=1) that
is 6,144 chains over 768 query waves on the 256-CU part, so every workgroup's three query
waves and three done rings carry chains.  A pass this small would otherwise go to the
cooperative engine at once, or run low-chain rounds (NQ = 2) or the end-of-pass kernel
(NQ = 2): FULL switches those off, and the round log (roundlog=2) names each round's shape,
which the tests that mean the new kernel check.
"""
import numpy as np
import pytest

import _util as U
import test_fold_batch as FB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


W, H, SPP, DEPTH = 96, 64, 4, 6
# every round a full one: no cooperative hand-over, no low-chain rounds, no end-of-pass kernel
FULL = "coop=0,lowq=0,sparse=0,wg_per_cu=1"

_oracle = {}   # scene name -> (path, the oracle's image, radiance, counters): rendered once, read only


def scene(tmp_path_factory, name):
    if name not in _oracle:
        text = FB.scene_text(name, DEPTH, -1).replace("DIMENSIONS %d %d" % (FB.W, FB.H), "DIMENSIONS %d %d" % (W, H))
        assert "DIMENSIONS %d %d" % (W, H) in text and "SAMPLES %d" % SPP in text
        path = str(tmp_path_factory.mktemp("nq3") / (name + ".txt"))
        with open(path, "w") as f:
            f.write(text)
        _oracle[name] = (path,) + U.OracleScene(path).render()
    return _oracle[name]


def shapes(err):
    """The shapes ("nq N") of the path rounds in a roundlog=2 log."""
    return {ln.split(", nq ")[1].split(" ")[0] for ln in err.splitlines() if ln.startswith("round ") and ", nq " in ln}


def check(rgb, rad, st, orgb, orad, octr):
    assert st["errors"] == 0 and st["short_pixels"] == 0
    assert rad.view(np.uint32).tolist() == orad.view(np.uint32).tolist()
    assert np.array_equal(rgb, orgb)
    assert st["rays"] == octr["rays"]


# tune, and the shape its path rounds must report (None: whatever the default engine choice runs)
ENGINES = {
    "nq3": ("nq=3,wg_per_cu=1", None),
    "nq3_coop0": ("nq=3,coop=0,wg_per_cu=1", None),
    "nq3_full": ("nq=3," + FULL, "3"),
    "nq2_full": ("nq=2," + FULL, "2"),   # the control
}


@pytest.mark.parametrize("engine", sorted(ENGINES))
@pytest.mark.parametrize("name", sorted(FB.SCENES))
def test_nq3_scenes_vs_oracle(pt, tmp_path_factory, name, engine, monkeypatch, capfd):
    tune, shape = ENGINES[engine]
    monkeypatch.setenv("PT_TUNE", tune + ",roundlog=2")
    path, orgb, orad, octr = scene(tmp_path_factory, name)
    with pt.Scene.load(path) as s:
        rgb, rad, st = s.render(radiance=True)
    check(rgb, rad, st, orgb, orad, octr)
    assert octr["rays"] > W * H * SPP   # (paths go on past their first vertex)
    if shape:
        assert shapes(capfd.readouterr().err) == {shape}


def test_nq3_golden_window(pt, monkeypatch, capfd):
    name = "c2_win_240_200_24x24"
    monkeypatch.setenv("PT_TUNE", "nq=3," + FULL + ",roundlog=2")
    m, img, rad = U.golden_image(name)
    with pt.Scene.load(U.golden_scene_path(name)) as s:
        rgb, r, st = s.render(radiance=True, window=tuple(m["window"]))
    assert st["errors"] == 0 and st["short_pixels"] == 0
    assert r.view(np.uint32).tolist() == rad.view(np.uint32).tolist()
    assert np.array_equal(rgb, img)
    assert shapes(capfd.readouterr().err) == {"3"}


# the path engine's hand-off sites with the settings that force them, in the NQ = 3 shape
NQ3 = "nq=3,lowq=0,sparse=0,wg_per_cu=1,"
HANDOFF_FORCE = {
    "suspend": NQ3 + "coop=0,runend=0,budget=2",
    "flush": NQ3 + "coop=0,runend=0,budget=2,shade_hold=1",
    "ringout": NQ3 + "coop=0,runend=0,budget=2",
    "exact": NQ3 + "coop=0,lstack=1",
}


@pytest.mark.parametrize("site", sorted(HANDOFF_FORCE))
def test_nq3_handoff_site_runs_and_keeps_every_sample(pt, tmp_path_factory, site, monkeypatch, capfd):
    monkeypatch.setenv("PT_TUNE", HANDOFF_FORCE[site] + ",roundlog=2")
    path, orgb, orad, octr = scene(tmp_path_factory, "box4")
    with pt.Scene.load(path) as s:
        rgb, rad, st = s.render(radiance=True)
    assert st["handoff"][site] > 0, st["handoff"]
    check(rgb, rad, st, orgb, orad, octr)
    assert shapes(capfd.readouterr().err) == {"3"}


def test_nq3_suspend_dropped_fails_the_resolve(pt, tmp_path_factory, monkeypatch):
    monkeypatch.setenv("PT_TUNE", HANDOFF_FORCE["suspend"] + ",drop=suspend")
    path = scene(tmp_path_factory, "box4")[0]
    with pt.Scene.load(path) as s:
        with pytest.raises(pt.PTError, match="did not take exactly"):
            s.render()


def test_nq3_two_tile_shards(pt, tmp_path_factory, monkeypatch, capfd):
    """Ranks 0 and 1 of 2 on one device, each the NQ = 3 shape over its tiles, the samples in
    two chunks (two passes per session): stitched, the oracle's image."""
    monkeypatch.setenv("PT_TUNE", "nq=3," + FULL + ",roundlog=2")
    path, orgb, _, _ = scene(tmp_path_factory, "corner")
    out = np.zeros_like(orgb)
    with pt.Scene.load(path) as s:
        s.prepare()
        for r in range(2):
            ss = pt.Session(s, rank=r, world=2)
            ss.trace(3)
            ss.sync()
            ss.trace(1)
            ss.resolve()
            ss.sync()
            pt.unpack_tiles(ss.read_packed(), W, H, r, 2, out=out)
            ss.close()
    assert np.array_equal(out, orgb)
    assert shapes(capfd.readouterr().err) == {"3"}


@pytest.mark.parametrize("bad", ["4", "1", "0", "three", "3x"])
def test_nq_values_are_checked(pt, bad, monkeypatch):
    monkeypatch.setenv("PT_TUNE", "nq=" + bad)
    with pt.Scene.load(U.golden_scene_path("dragon_64x64x16")) as s:
        with pytest.raises(pt.PTError, match="no such shape"):
            s.render()
