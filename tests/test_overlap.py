"""Generated scenes of mutually overlapping primitives (tests/_overlap.py) on the GPU: every engine and every
batch API against the fixtures recorded from the untouched reference (tests/test_overlap_host.py runs the
same fixtures through the host forms, and says what the families are for).

Every scene is guarded first (_ladder.guarded: the oracle renders it in a child process under a time limit).
All frames are 16 x 12 at 2 spp and the ray sets hold at most 2,048 rays.  flat is compared by the NaN rule:
NaNs by position, every other float by its bits.
"""
import numpy as np
import pytest

import _ladder as L
import _overlap as O
import _paths as P
import _util as U

pytestmark = pytest.mark.gpu

W, H, SPP = 16, 12, 2
RENDER_TUNES = ["", "coop=0", "coop=100000000,coop_team=8", "coop=100000000,coop_team=64", "engine=mega", "lstack=1,coop=0"]
STATE_MACHINE_TUNES = ("coop=0", "lstack=1,coop=0")     # k_wpath alone, and every query through k_wexact
LONG = ("blob", "blob_lit", "shells")


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


def finite(src):
    return O.parse(src)[0] != "flat"


def guarded_image(src):
    """the fixture, after the guard has rendered the scene (and found the fixture's frame)"""
    im = O.image(src)
    rgb, rad, ctr = L.guarded(im["path"], finite=finite(src))
    O.assert_radiance(src, rad, im["rad"], "the oracle")
    assert ctr["rays"] == im["rays"]
    return im


def guarded_case(src):
    c = O.case(src)
    L.guarded(c["path"], finite=finite(src))
    return c


_host = {}


def host_pixels(pt, src):
    """the host state machine's counters of the frame's two samples (Scene.sample_pixels' host form)"""
    if src not in _host:
        im = O.image(src)
        with pt.Scene.load(im["path"]) as s:
            st, c = s.selftest_pixels_host(s.pixel_init(pt.rank_pixels(W, H, 0, 1)), spp=SPP)
        assert c["errors"] == 0 and c["rays"] == im["rays"]
        _host[src] = c
    return _host[src]


# ---- the recorded rays: k_rays and k_rays_exact ------------------------------------------------------
@pytest.mark.parametrize("src", sorted(O.RAY_FIXTURES))
def test_intersect_recorded_rays(pt, src):
    c = guarded_case(src)
    with pt.Scene.load(c["path"]) as s:
        s.prepare()
        _, _, host = s.selftest_ray_intersection(c["rays"], traversal=0)
        got, st = s.intersect(c["rays"])
        n_planes = s.info["n_planes"]
    print("%s: %r" % (src, {k: st[k] for k in ("rays", "node_visits", "prim_tests", "aux_visits", "fallbacks", "errors")}))
    assert got.dtype == pt.HIT_DTYPE and len(got) == len(c["rays"])
    O.assert_hits(src, got["id"], got["t"], got["n"], got["interior"], c, "Scene.intersect")
    miss = np.ascontiguousarray(got[c["ids"] == -1]).view(np.uint32).reshape(-1, 6)
    assert np.array_equal(miss[:, 0], np.full(len(miss), 0xFFFFFFFF, np.uint32)) and not miss[:, 1:].any()
    n = len(c["rays"])
    assert st["errors"] == 0 and st["rays"] == n and st["plane_tests"] == n * n_planes
    assert (st["node_visits"], st["prim_tests"], st["aux_visits"], st["fallbacks"]) == \
        (host["nodes"], host["prim_tests"], host["aux"], host["fallbacks"])
    if O.parse(src)[0] in LONG:
        assert st["fallbacks"] > 0      # k_rays_exact really ran
    if src == O.BLOB_306:
        assert got["id"][O.RAY_892] == 11


# ---- the recorded frames -----------------------------------------------------------------------------
@pytest.mark.parametrize("src", O.IMAGE_FIXTURES)
def test_features_on_the_pixel_centres(pt, src):
    im = guarded_image(src)
    xy = O.centres()
    want = O.expected_features(pt, src, im["path"], xy)
    with pt.Scene.load(im["path"]) as s:
        got, st = s.features(xy)
    assert st["errors"] == 0 and st["rays"] == len(xy)
    O.assert_features(src, got, want)


@pytest.mark.parametrize("src", O.IMAGE_FIXTURES)
def test_radiance_on_camera_rays_with_the_pixel_seeds(pt, src):
    im = guarded_image(src)
    _, orad, octr = L.guarded(im["path"], (0, 0, W, H), 1, finite=finite(src))
    with pt.Scene.load(im["path"]) as s:
        rec = P.pixel_records(pt, s, W, (0, 0, W, H))
        out, st = s.radiance(rec)
    assert st["errors"] == 0 and st["short_pixels"] == 0
    assert st["rays"] == octr["rays"] == int(out["rays"].sum())
    O.assert_radiance(src, out["rgb"] + np.float32(0), orad, "Scene.radiance")
    if O.parse(src)[0] in LONG:
        assert st["fallbacks"] > 0


@pytest.mark.parametrize("src", O.IMAGE_FIXTURES)
def test_sample_pixels_in_runs_of_one_and_one(pt, src):
    im = guarded_image(src)
    host = host_pixels(pt, src)
    with pt.Scene.load(im["path"]) as s:
        st0 = s.pixel_init(pt.rank_pixels(W, H, 0, 1))
        st1, a = s.sample_pixels(st0, spp=1)
        st2, b = s.sample_pixels(st1, spp=1)
        mean, rgb = s.pixel_resolve(st2)
    assert a["errors"] == 0 and b["errors"] == 0 and a["short_pixels"] == 0 and b["short_pixels"] == 0
    assert a["rays"] + b["rays"] == im["rays"] and (st2["samples"] == SPP).all()
    assert a["fallbacks"] + b["fallbacks"] == host["fallbacks"]
    at = st2["y"].astype(np.int64) * W + st2["x"]
    O.assert_radiance(src, mean, im["rad"].reshape(-1, 3)[at], "Scene.sample_pixels")
    assert np.array_equal(rgb, im["rgb"].reshape(-1, 3)[at])
    if O.parse(src)[0] in LONG:
        assert host["fallbacks"] > 0


@pytest.mark.parametrize("tune", RENDER_TUNES)
@pytest.mark.parametrize("src", O.IMAGE_FIXTURES)
def test_render_every_engine(pt, monkeypatch, src, tune):
    im = guarded_image(src)
    if tune:
        monkeypatch.setenv("PT_TUNE", tune)
    with pt.Scene.load(im["path"]) as s:
        s.prepare()
        rgb, rad, st = s.render(radiance=True, traversal=0)
    print("%s [%s]: %r" % (src, tune, {k: st[k] for k in ("rays", "node_visits", "prim_tests", "aux_visits", "fallbacks",
                                                          "errors", "rounds")}))
    assert st["errors"] == 0 and st["short_pixels"] == 0 and st["rays"] == im["rays"]
    O.assert_radiance(src, rad, im["rad"], "Scene.render [%s]" % tune)
    assert np.array_equal(rgb, im["rgb"])
    if tune in STATE_MACHINE_TUNES and O.parse(src)[0] in LONG:
        assert st["fallbacks"] > 0      # the exact hand-over really ran


@pytest.mark.parametrize("src", O.IMAGE_FIXTURES)
def test_session_states_through_a_fresh_session(pt, src):
    """trace(1), export, import into a fresh session, trace(1), resolve: the recorded frame"""
    import torch
    im = guarded_image(src)
    with pt.Scene.load(im["path"]) as s:
        s.prepare()
        a = pt.Session(s)
        a.trace(1)
        states = a.export_states()
        sa = a.stats()
        a.close()
        b = pt.Session(s)
        assert b.import_states(states) == W * H
        b.trace(1)
        drad = torch.empty(max(b.n_tiles, 1) * 256 * 3, dtype=torch.float32, device="cuda")
        b.resolve(dev_rad=drad.data_ptr())
        b.sync()
        sb = b.stats()
        rgb = pt.unpack_tiles(b.read_packed(), W, H, 0, 1)
        rad = pt.unpack_tiles_f32(drad.cpu().numpy(), W, H, 0, 1)
        b.close()
    assert sa["errors"] == 0 and sb["errors"] == 0 and sa["short_pixels"] == 0 and sb["short_pixels"] == 0
    assert sa["rays"] + sb["rays"] == im["rays"]
    O.assert_radiance(src, rad, im["rad"], "two sessions")
    assert np.array_equal(rgb, im["rgb"])
