"""The guided filter without a GPU (include/pt.h "guided filter"): the host mirror -- the guide packer and
the per-pixel level function that k_filter_guides and k_filter run, compiled for the host -- against the
numpy float32 restatement of the definition (tests/_filter.py), on bytes."""
import ctypes as C

import numpy as np
import pytest

import _filter as FL
import _util as U

pt = U.ptrace()
PT_E_INVALID = -1

# what the definition's rules must be exercised by on dragon_64x64x16 at levels 3, before anything is compared
DRAGON_FLOORS = {"outside": 13000, "class": 4000, "wn0": 19000, "ec": 1500, "ea": 20000, "nonfinite": 70, "kept": 100000}


def test_layouts_and_defaults():
    assert C.sizeof(pt.FilterOpts) == 24
    assert [getattr(pt.FilterOpts, k).offset for k in ("levels", "sigma_c", "sigma_z", "sigma_a", "normal_pow2",
                                                       "layout")] == [0, 4, 8, 12, 16, 20]
    assert (pt.FILTER_ROWMAJOR, pt.FILTER_TILES) == (0, 1)
    d = pt.FilterOpts.default()
    assert (d.levels, d.normal_pow2, d.layout) == (3, 5, pt.FILTER_ROWMAJOR)
    assert [np.float32(v).tobytes() for v in (d.sigma_c, d.sigma_z, d.sigma_a)] == \
        [np.float32(v).tobytes() for v in (1.0, 0.05, 0.1)]
    assert {k: FL.DEFAULTS[k] for k in FL.DEFAULTS} == {"levels": 3, "sigma_c": 1.0, "sigma_z": 0.05, "sigma_a": 0.1,
                                                        "normal_pow2": 5}
    for sym in ("pt_filter_opts_default", "pt_filtq_create", "pt_filtq_set_features", "pt_filtq_run", "pt_filtq_stats",
                "pt_filtq_free", "pt_filter", "pt_selftest_filter_host"):
        assert sym in pt.EXPORTED and hasattr(pt._lib, sym)
    pt._lib.pt_filter_opts_default(None)   # (ignored)


def check_census(name, levels, census, feat):
    FL.print_census("%s levels %d" % (name, levels), census)
    classes = np.unique(FL.guides(feat)[3])
    print("%s: classes %s" % (name, classes.tolist()))
    if name == "dragon_64x64x16" and levels == 3:
        for k, floor in DRAGON_FLOORS.items():
            assert census[k] >= floor, (k, census[k], floor)
    if name == "hw3s6_48x48x8":
        assert 0 in classes and 1 in classes
    if name == "mat_matrix_24x24x8":
        assert len(classes) >= 5
    if levels == 5:
        assert census["outside"] > 0   # (the taps reach +-32 pixels)
    assert census["kept"] > 0


@pytest.mark.parametrize("levels", FL.LEVELS)
@pytest.mark.parametrize("name", FL.SCENES)
def test_host_mirror_on_the_fixtures(name, levels):
    _, feat = FL.scene_features(name)
    want, census = FL.expected_scene(name, levels=levels)
    check_census(name, levels, census, feat)
    rad = FL.poisoned(name)
    h, w = rad.shape[:2]
    got = pt.selftest_filter_host(feat, rad, w, h, levels=levels)
    FL.assert_frames(got, want, "%s levels %d" % (name, levels))
    # finite where the input is, and the three poisoned pixels keep their words
    bad = ~np.isfinite(rad).all(axis=2)
    assert bad.sum() == 3 and np.isfinite(got[~bad]).all()
    assert got[bad].tobytes() == rad[bad].tobytes()


@pytest.mark.parametrize("off", ["sigma_c", "sigma_z", "sigma_a", "normal_pow2"])
def test_each_option_matters(off):
    name = "dragon_64x64x16"
    base, _ = FL.expected_scene(name, levels=3)
    want, _ = FL.expected_scene(name, levels=3, **{off: 0})
    changed = int((base.view(np.uint32) != want.view(np.uint32)).any(axis=2).sum())
    print("%s = 0: %d pixels change" % (off, changed))
    assert changed >= 500
    _, feat = FL.scene_features(name)
    rad = FL.poisoned(name)
    got = pt.selftest_filter_host(feat, rad, 64, 64, levels=3, **{off: 0})
    FL.assert_frames(got, want, off)


@pytest.mark.parametrize("size", FL.SYNTH_SIZES)
def test_synthetic_frames(size):
    w, h = size
    feat, rad = FL.synthetic(pt, w, h)
    classes = np.unique(FL.guides(feat)[3])
    if w * h >= 40:
        assert len(classes) >= 6 and 0 in classes
        assert np.isinf(feat["t"]).any() and np.isnan(feat["n"]).any() and np.isnan(feat["albedo"]).any()
        assert (~np.isfinite(rad)).any(axis=2).sum() == 3
    for o in ({"levels": 1}, {"levels": 4}, {"levels": 8, "sigma_c": 2.5, "normal_pow2": 1}, {"levels": 2, "sigma_z": 0.0,
                                                                                            "normal_pow2": 8}):
        want, census = FL.filtered(feat, rad, **o)
        FL.print_census("synthetic %dx%d %s" % (w, h, o), census)
        got = pt.selftest_filter_host(feat, rad, w, h, **o)
        FL.assert_frames(got, want, "%dx%d %s" % (w, h, o))
    if (w, h) == (70, 37):
        # every rule is met on this frame too
        assert min(census[k] for k in ("outside", "class", "nonfinite", "wn0", "ea", "ec", "kept")) > 0


def pack_tiles(rad):
    """a frame as a world-1 session packs it (16 x 16 tiles, padded), written from the layout's definition"""
    h, w = rad.shape[:2]
    tx, ty = (w + 15) // 16, (h + 15) // 16
    pad = np.full((ty * 16, tx * 16, 3), 0xA5A5A5A5, np.uint32).view(np.float32)
    pad[:h, :w] = rad
    return np.ascontiguousarray(pad.reshape(ty, 16, tx, 16, 3).transpose(0, 2, 1, 3, 4)).reshape(-1)


@pytest.mark.parametrize("name", ["dragon_64x64x16", "mat_camera_23x17x8"])
def test_tile_layout(name):
    _, feat = FL.scene_features(name)
    rad = FL.poisoned(name)
    h, w = rad.shape[:2]
    packed = pack_tiles(rad)
    # the packing is what pt_unpack_tiles_f32 reads
    assert pt.unpack_tiles_f32(packed, w, h, 0, 1).tobytes() == rad.tobytes()
    want, _ = FL.expected_scene(name, levels=3)
    got = pt.selftest_filter_host(feat, packed, w, h, levels=3, layout=pt.FILTER_TILES)
    FL.assert_frames(got, want, name + " tiles")


def test_refusals_leave_the_output_untouched():
    lib = pt._lib
    feat, rad = FL.synthetic(pt, 5, 1)
    feat = np.ascontiguousarray(feat)
    guard = np.full((1, 5, 3), 0xA5A5A5A5, np.uint32).view(np.float32)
    out = guard.copy()

    def call(o, f=feat, i=rad, r=out, w=5, h=1):
        return lib.pt_selftest_filter_host(w, h, pt._ptr(f), C.byref(o) if o is not None else None, pt._ptr(i), pt._ptr(r))

    bad = [pt.FilterOpts.default(levels=0), pt.FilterOpts.default(levels=9), pt.FilterOpts.default(sigma_c=-1.0),
           pt.FilterOpts.default(sigma_z=float("nan")), pt.FilterOpts.default(sigma_a=float("inf")),
           pt.FilterOpts.default(sigma_a=-0.5), pt.FilterOpts.default(normal_pow2=9), pt.FilterOpts.default(layout=2)]
    for o in bad:
        assert call(o) == PT_E_INVALID, o.as_dict()
    ok = pt.FilterOpts.default()
    assert call(None) == PT_E_INVALID
    assert call(ok, f=None) == PT_E_INVALID and call(ok, i=None) == PT_E_INVALID and call(ok, r=None) == PT_E_INVALID
    assert call(ok, w=0) == PT_E_INVALID and call(ok, h=0) == PT_E_INVALID
    assert out.tobytes() == guard.tobytes()
    assert call(ok) == pt.PT_OK and out.tobytes() != guard.tobytes()
    # sigmas of 0 and the extreme levels and powers are options like any other
    for o in (pt.FilterOpts.default(sigma_c=0.0, sigma_z=0.0, sigma_a=0.0, normal_pow2=0, levels=8),
              pt.FilterOpts.default(levels=1, normal_pow2=8)):
        assert call(o) == pt.PT_OK
    with pytest.raises(TypeError):
        pt.FilterOpts.default(sigma=1.0)
    # the GPU entry points refuse null arguments before they touch a device
    assert lib.pt_filtq_create(None, 0, 0, 0, 0, 0, C.byref(pt._P())) == PT_E_INVALID
    assert lib.pt_filtq_set_features(None, None, None) == PT_E_INVALID
    assert lib.pt_filtq_run(None, None, C.byref(ok), None, None, None) == PT_E_INVALID
    assert lib.pt_filtq_stats(None, None) == PT_E_INVALID
    assert lib.pt_filter(None, 0, 0, 0, 0, 0, C.byref(ok), None, None, None) == PT_E_INVALID
    lib.pt_filtq_free(None)
