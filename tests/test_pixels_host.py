"""CPU tests of the pixel-sample interface (include/pt.h pt_pixel_init, pt_pixel_resolve, pt_pixq_*,
pt_sample_pixels; ptrace.PixelQuery, Scene.pixel_init / sample_pixels / pixel_resolve) -- no GPU
needed: the host-only calls, the argument checks that come before the device check, the record's
layout, and the host twin (selftest_pixels_host: camera_ray and trace_path_with over the query state
machine, on each record's stream) on the cases of tests/_pixels.py, whose expected values are the
CPU oracle's renders and the reference's recorded radiance.  tests/test_pixels.py runs the same
cases on the GPU.
"""
import ctypes as C

import numpy as np
import pytest

import _pixels as X
import _util as U

pt = U.ptrace()


def run(s, state, counts=None, spp=0):
    return s.selftest_pixels_host(state, counts=counts, spp=spp)


@pytest.fixture(scope="module")
def scene():
    with pt.Scene.load(U.scene_path("practice5_1.txt")) as s:
        yield s


# ---- 1. whole frames ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.WHOLE_FRAMES)
def test_whole_frames_at_the_reference_sample_count(name):
    X.case_whole_frame(pt, run, name)


# ---- 2. resume ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,splits", [("dragon_glass_40x24x7", ((3, 4), (1,) * 7, (7,))),
                                         ("hw3s4_24x40x5", ((2, 3), (5,)))])
def test_a_run_of_a_then_b_is_a_run_of_a_plus_b(name, splits):
    at_split = X.case_resume(pt, run, name, splits)
    # the condition without which the case does not show that the saved value travels: at the
    # split, a fair part of the records carry one and a fair part carry none
    saved = (at_split["rng"] & X.SAVED_BIT) != 0
    print("%s: %d of %d records carry a saved value after %d samples" % (name, saved.sum(), len(saved), splits[0][0]))
    assert saved.sum() * 10 >= len(saved) and (~saved).sum() * 10 >= len(saved)
    assert (at_split["saved"][saved] != 0).all() and not at_split["saved"][~saved].view(np.uint32).any()
    assert (at_split["rng"] & ~np.uint32(X.SAVED_BIT)).min() >= 1


# ---- 3. per-pixel counts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,window", [("mat_matrix_24x24x8", (0, 0, 24, 24)), ("many_lights_48x48x8", (0, 0, 24, 24))])
def test_per_pixel_counts_and_a_second_run_with_zeros(name, window):
    X.case_counts(pt, run, name, window)


# ---- 4. shapes ----------------------------------------------------------------------------------------------
# (1,000 records are four workgroups, whose waves pull 64 records at a time: no multiple of the batch)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_first_pixels(n):
    X.case_first_pixels(pt, run, n)


def test_scattered_pixels_with_one_twice():
    X.case_scattered(pt, run)


def test_one_long_record_among_short_ones():
    X.case_one_long_record(pt, run)


# ---- 5. depth -----------------------------------------------------------------------------------------------
def test_ray_depth_1_by_override():
    X.case_depth_1(pt, run)


def test_ray_depth_10():
    X.case_depth_10(pt, run)


def test_ray_depth_0_draws_the_jitter_and_adds_zero():
    X.case_depth_0(pt, run)


# ---- 6. seeds -----------------------------------------------------------------------------------------------
def test_seeds_are_reduced_as_minstd_rand_reduces_them():
    X.case_seed_reduction(pt, run)


def test_arbitrary_seeds_against_the_batch_radiance_twin():
    # a cross-engine check, not an oracle one (tests/_pixels.py)
    X.case_arbitrary_seeds_cross_engine(pt, run, lambda s, rec: s.selftest_paths_host(rec))


# ---- 8. arguments ---------------------------------------------------------------------------------------------
def test_record_layout():
    assert pt.PIXEL_DTYPE.itemsize == 32
    assert [pt.PIXEL_DTYPE.fields[k][1] for k in ("rng", "saved", "x", "y", "sum", "samples")] == [0, 4, 8, 12, 16, 28]
    assert pt.PIXELS_CHUNK == 1 << 22
    for name in ("pt_pixel_init", "pt_pixq_create", "pt_pixq_run", "pt_pixq_stats", "pt_pixq_free", "pt_sample_pixels",
                 "pt_pixel_resolve", "pt_selftest_pixels_host"):
        assert name in pt.EXPORTED
    assert pt.abi_version() == 6


def test_pixel_init_rejects_pixels_outside_the_image(scene):
    inf = scene.info
    W, H = inf["width"], inf["height"]
    ok = scene.pixel_init([[W - 1, H - 1], [0, 0]])
    assert ok["rng"].tolist() == [(H - 1) * W + W - 1, 1] and not ok["sum"].any() and not ok["samples"].any()
    assert ok["x"].tolist() == [W - 1, 0] and ok["y"].tolist() == [H - 1, 0]
    for bad in ([W, 0], [0, H], [2 ** 32 - 1, 0]):
        out = np.full(2, 0xA5, np.uint8).repeat(32).view(pt.PIXEL_DTYPE)
        with pytest.raises(pt.PTError) as e:
            scene.pixel_init([[0, 0], bad])
        assert e.value.code == pt.PT_E_INVALID
        xy = np.array([[0, 0], bad], np.uint32)
        assert pt._lib.pt_pixel_init(scene._h, 2, U._p(xy), None, U._p(out)) == pt.PT_E_INVALID
        assert (out.view(np.uint8) == 0xA5).all(), "a refused call wrote states"
    xy = np.zeros((1, 2), np.uint32)
    out = np.zeros(1, pt.PIXEL_DTYPE)
    assert pt._lib.pt_pixel_init(None, 1, U._p(xy), None, U._p(out)) == pt.PT_E_INVALID
    assert pt._lib.pt_pixel_init(scene._h, 1, None, None, U._p(out)) == pt.PT_E_INVALID
    assert pt._lib.pt_pixel_init(scene._h, 1, U._p(xy), None, None) == pt.PT_E_INVALID
    assert pt._lib.pt_pixel_init(scene._h, 0, None, None, None) == pt.PT_OK


def test_resolve_rejects_a_state_without_samples(scene):
    st = scene.pixel_init([[1, 2], [3, 4]])
    st["samples"] = (4, 0)
    with pytest.raises(pt.PTError) as e:
        scene.pixel_resolve(st)
    assert e.value.code == pt.PT_E_INVALID
    assert pt._lib.pt_pixel_resolve(None, 2, U._p(st), None, None) == pt.PT_E_INVALID
    assert pt._lib.pt_pixel_resolve(scene._h, 2, None, None, None) == pt.PT_E_INVALID
    assert pt._lib.pt_pixel_resolve(scene._h, 0, None, None, None) == pt.PT_OK


def test_resolve_is_the_reciprocal_product_and_the_oracle_tonemap(scene):
    """mean = 1.f / samples * sum in float32 (not sum / samples), rgb = the oracle's tonemap of it"""
    rng = np.random.default_rng(5)
    st = np.zeros(3000, pt.PIXEL_DTYPE)
    st["samples"] = rng.integers(1, 300, len(st))
    st["samples"][:4] = (1, 3, 7, 200)
    st["sum"] = (rng.random((len(st), 3)) * st["samples"][:, None] * 1.5).astype(np.float32)
    mean, rgb = scene.pixel_resolve(st)
    inv = (np.float32(1) / st["samples"].astype(np.float32)).astype(np.float32)
    want = (inv[:, None] * st["sum"]).astype(np.float32)
    X.assert_bits(mean, want, "mean")
    quot = (st["sum"] / st["samples"].astype(np.float32)[:, None]).astype(np.float32)
    assert (quot.view(np.uint32) != want.view(np.uint32)).any(), "the inputs do not tell the product from the quotient"
    assert np.array_equal(rgb, U.oracle_tonemap(want))
    # either output alone
    m2 = np.zeros((len(st), 3), np.float32)
    assert pt._lib.pt_pixel_resolve(scene._h, len(st), U._p(st), U._p(m2), None) == pt.PT_OK
    assert m2.tobytes() == mean.tobytes()


def test_create_run_and_stats_reject_bad_arguments(scene):
    h = C.c_void_p()
    assert pt._lib.pt_pixq_create(None, 0, 16, C.byref(h)) == pt.PT_E_INVALID
    assert pt._lib.pt_pixq_create(scene._h, 0, 16, None) == pt.PT_E_INVALID
    for bad in (0, 1 << 32, (1 << 64) - 1):
        assert pt._lib.pt_pixq_create(scene._h, 0, bad, C.byref(h)) == pt.PT_E_INVALID, bad
        assert "max_pixels" in pt.last_error()
    assert not h.value
    buf = np.zeros(32, np.uint8)
    assert pt._lib.pt_pixq_run(None, None, 1, U._p(buf), None, 1) == pt.PT_E_INVALID
    assert pt._lib.pt_pixq_stats(None, None) == pt.PT_E_INVALID
    pt._lib.pt_pixq_free(None)   # a no-op, like the other *_free
    assert pt._lib.pt_sample_pixels(None, 0, 1, U._p(buf), None, 1, None) == pt.PT_E_INVALID
    assert pt._lib.pt_sample_pixels(scene._h, 0, 1, None, None, 1, None) == pt.PT_E_INVALID
    st = pt.Stats()
    assert pt._lib.pt_sample_pixels(scene._h, 0, 0, None, None, 1, C.byref(st)) == pt.PT_OK and st.samples == 0
    assert pt._lib.pt_selftest_pixels_host(None, 1, U._p(buf), None, 1, None) == pt.PT_E_INVALID
    assert pt._lib.pt_selftest_pixels_host(scene._h, 1, None, None, 1, None) == pt.PT_E_INVALID
    with pytest.raises(ValueError):
        scene.selftest_pixels_host(scene.pixel_init([[0, 0], [1, 1]]), counts=[1])


def test_sample_pixels_without_gpu_fails_loudly(scene):
    if U.gpu_available():
        # (with a device the same calls succeed: tests/test_pixels.py)
        with pt.PixelQuery(scene, max_pixels=8) as q:
            assert q.stats()["samples"] == 0
        return
    with pytest.raises(pt.PTError) as e:
        scene.sample_pixels(scene.pixel_init([[0, 0]]), spp=1)
    assert e.value.code in (pt.PT_E_NO_GPU, pt.PT_E_HIP)
    with pytest.raises(pt.PTError) as e:
        pt.PixelQuery(scene, max_pixels=8)
    assert e.value.code in (pt.PT_E_NO_GPU, pt.PT_E_HIP)


def test_the_twin_leaves_its_argument_and_zero_count_records_alone(scene):
    st = scene.pixel_init([[5, 5], [6, 5], [7, 5]])
    before = st.tobytes()
    out, ctr = scene.selftest_pixels_host(st, counts=[2, 0, 1])
    assert st.tobytes() == before
    assert out[1].tobytes() == st[1].tobytes() and out["samples"].tolist() == [2, 0, 1] and ctr["samples"] == 3
