"""First-hit features without a GPU: the record layouts, the scene accessors, and the host mirror
(camera_ray, the query state machine, the shade lookup -- the inline functions k_feats runs)
against records put together from the oracle and the scene text (tests/_features.py)."""
import ctypes as C

import numpy as np
import pytest

import _features as F
import _util as U

pt = U.ptrace()
PT_E_INVALID = -1


def test_record_layouts():
    f, s = pt.FEATURE_DTYPE, pt.SHADE_DTYPE
    assert f.itemsize == 64 and s.itemsize == 32
    assert [f.fields[k][1] for k in ("id", "t", "n", "interior", "albedo", "ior", "emission", "material", "type",
                                     "reserved")] == [0, 4, 8, 20, 24, 36, 40, 52, 56, 60]
    assert [s.fields[k][1] for k in ("albedo", "ior", "emission", "material")] == [0, 12, 16, 28]
    # bytes 0..23 are the pt_ray_hit
    assert [f.fields[k][1] for k in ("id", "t", "n", "interior")] == [pt.HIT_DTYPE.fields[k][1] for k in
                                                                     ("id", "t", "n", "interior")]
    assert pt.FEATS_CHUNK == 1 << 22
    for sym in ("pt_featq_create", "pt_featq_run", "pt_featq_stats", "pt_featq_free", "pt_features", "pt_session_features",
                "pt_session_features_host", "pt_scene_shade", "pt_scene_background", "pt_selftest_features_host"):
        assert sym in pt.EXPORTED


@pytest.mark.parametrize("name", ["mat_matrix_24x24x8", "mat_inside_24x24x8", "hw3s6_48x48x8", "practice5_dragon_10k"])
def test_shade_and_background_are_the_scene_text(name):
    path = U.scene_path(name + ".txt") if name.startswith("practice5") else U.golden_scene_path(name)
    tab, bg = F.shade_table(path)
    info = F.oracle_scene(path).prim_info()
    with pt.Scene.load(path) as s:
        with pytest.raises(pt.PTError):   # before prepare
            s.shade()
        assert np.array_equal(s.background.view(np.uint32), bg.view(np.uint32))   # (needs no prepare)
        s.prepare()
        got = s.shade()
        assert np.array_equal(s.background.view(np.uint32), bg.view(np.uint32))
    assert len(got) == len(tab) == len(info)
    for k in ("albedo", "ior", "emission"):
        assert np.array_equal(got[k].view(np.uint32), tab[k].view(np.uint32)), k
    assert np.array_equal(got["material"], tab["material"])
    assert [U.MATERIALS[int(m)] for m in got["material"]] == [p["material"] for p in info]
    assert np.array_equal(got["ior"].view(np.uint32), np.array([p["ior"] for p in info], np.float32).view(np.uint32))


def _host_counters(s, rays):
    return s.selftest_ray_intersection(rays, traversal=pt.TRAVERSAL_REPLAY)[2]


@pytest.mark.parametrize("name", F.SCENES)
def test_host_mirror_on_the_pixel_centres(name):
    path, want, rays = F.expected_centres(name)
    F.check_conditions(name, want)
    with pt.Scene.load(path) as s:
        got, ctr = s.selftest_features(F.centres(path))
        ref = _host_counters(s, rays)
        n_planes = s.info["n_planes"]
    F.assert_records(got, want)
    assert ctr["rays"] == len(want) and ctr["errors"] == 0 and ctr["fallbacks_ray"] == 0
    assert ctr["plane_tests"] >= len(want) * n_planes
    assert (ctr["node_visits"], ctr["prim_tests"], ctr["aux_visits"], ctr["fallbacks"], ctr["errors"]) == \
        (ref["nodes"], ref["prim_tests"], ref["aux"], ref["fallbacks"], ref["errors"])


@pytest.mark.parametrize("name", F.SCENES)
def test_host_mirror_on_subpixel_and_nonfinite_positions(name):
    path, xy, want, rays = F.expected_subpixel(name)
    c = F.census(want)
    F.print_census(name + " sub-pixel", c)
    assert len(xy) == F.N_SUB + F.NONFINITE and not np.isfinite(xy[F.N_SUB:]).all(axis=1).any()
    if name == "hw3s6_48x48x8":
        assert c["misses"] >= 32
    with pt.Scene.load(path) as s:
        got, ctr = s.selftest_features(xy)
        ref = _host_counters(s, rays)
    F.assert_records(got, want)
    assert ctr["rays"] == len(want) and ctr["errors"] == 0
    assert ctr["fallbacks_ray"] == F.NONFINITE == 32
    assert ctr["fallbacks"] >= F.NONFINITE
    assert (ctr["node_visits"], ctr["prim_tests"], ctr["aux_visits"], ctr["fallbacks"], ctr["errors"]) == \
        (ref["nodes"], ref["prim_tests"], ref["aux"], ref["fallbacks"], ref["errors"])


def test_refusals_leave_the_output_untouched():
    lib = pt._lib
    path = U.golden_scene_path("mat_matrix_24x24x8")
    with pt.Scene.load(path) as s:
        n = s.info["n_prims"]
        guard = np.full(n + 1, 0xA5, np.uint8).repeat(32).view(pt.SHADE_DTYPE)
        out = guard.copy()
        # before prepare
        assert lib.pt_scene_shade(s._h, pt._ptr(out), n) == PT_E_INVALID
        s.prepare()
        # a count that does not match, either way; null arguments
        for m in (n - 1, n + 1, 0):
            assert lib.pt_scene_shade(s._h, pt._ptr(out), m) == PT_E_INVALID
        assert lib.pt_scene_shade(s._h, None, n) == PT_E_INVALID
        assert lib.pt_scene_shade(None, pt._ptr(out), n) == PT_E_INVALID
        assert out.tobytes() == guard.tobytes()
        assert lib.pt_scene_shade(s._h, pt._ptr(out), n) == pt.PT_OK
        assert out[n:].tobytes() == guard[n:].tobytes() and out[:n].tobytes() != guard[:n].tobytes()
        rgb = np.full(3, 7.0, np.float32)
        assert lib.pt_scene_background(None, pt._ptr(rgb)) == PT_E_INVALID
        assert lib.pt_scene_background(s._h, None) == PT_E_INVALID
        assert (rgb == 7.0).all()

        xy = F.centres(path)[:5].copy()
        fguard = np.full(6 * 64, 0xA5, np.uint8).view(pt.FEATURE_DTYPE)
        fout = fguard.copy()
        ctr = np.full(8, 99, np.uint64)
        assert lib.pt_selftest_features_host(None, 5, pt._ptr(xy), pt._ptr(fout), pt._ptr(ctr)) == PT_E_INVALID
        assert lib.pt_selftest_features_host(s._h, 5, None, pt._ptr(fout), pt._ptr(ctr)) == PT_E_INVALID
        assert lib.pt_selftest_features_host(s._h, 5, pt._ptr(xy), None, pt._ptr(ctr)) == PT_E_INVALID
        assert fout.tobytes() == fguard.tobytes() and (ctr == 99).all()
        # n = 0 is fine, with or without buffers, and writes no record
        assert lib.pt_selftest_features_host(s._h, 0, None, None, None) == pt.PT_OK
        assert lib.pt_selftest_features_host(s._h, 0, pt._ptr(xy), pt._ptr(fout), pt._ptr(ctr)) == pt.PT_OK
        assert fout.tobytes() == fguard.tobytes() and not ctr.any()
        # the counters are optional; nothing is written past n records
        assert lib.pt_selftest_features_host(s._h, 5, pt._ptr(xy), pt._ptr(fout), None) == pt.PT_OK
        assert fout[5:].tobytes() == fguard[5:].tobytes()
        got, _ = s.selftest_features(np.zeros((0, 2), np.float32))
        assert len(got) == 0
    # the GPU entry points refuse null arguments before they touch a device
    assert lib.pt_featq_create(None, 0, 16, C.byref(pt._P())) == PT_E_INVALID
    assert lib.pt_featq_run(None, None, 1, None, None) == PT_E_INVALID
    assert lib.pt_featq_stats(None, None) == PT_E_INVALID
    assert lib.pt_features(None, 0, 1, None, None, None) == PT_E_INVALID
    assert lib.pt_session_features(None, None, 0, None) == PT_E_INVALID
    assert lib.pt_session_features_host(None, None, 0, None) == PT_E_INVALID
    lib.pt_featq_free(None)
