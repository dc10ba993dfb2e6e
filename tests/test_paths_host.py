"""CPU tests of the batch radiance interface (include/pt.h pt_pathq_*, pt_radiance, pt_camera_rays;
ptrace.PathQuery, Scene.radiance) -- no GPU needed: argument checks come before the device check,
the records' layouts, and the host execution of the engine's pieces (selftest_paths_host:
trace_path_with over the query state machine) against the CPU oracle, built as tests/_paths.py
describes: a record that is a pixel's first sample must return the oracle's one-sample radiance.
"""
import ctypes as C

import numpy as np
import pytest

import _paths as P
import _util as U

pt = U.ptrace()

DEPTH0 = ("DIMENSIONS 8 6\nRAY_DEPTH 0\nSAMPLES 1\nBG_COLOR 0.2 0.3 0.4\nCAMERA_POSITION 0 0 4\nCAMERA_RIGHT 1 0 0\n"
          "CAMERA_UP 0 1 0\nCAMERA_FORWARD 0 0 -1\nCAMERA_FOV_X 1.2\nNEW_PRIMITIVE\nBOX 0.5 0.5 0.5\nCOLOR 1 0 0\n"
          "NEW_PRIMITIVE\nELLIPSOID 0.3 0.3 0.3\nPOSITION 1 0 0\nEMISSION 2 2 2\n")


@pytest.fixture(scope="module")
def scene():
    with pt.Scene.load(U.scene_path("practice5_1.txt")) as s:
        yield s


def test_create_rejects_bad_arguments(scene):
    h = C.c_void_p()
    assert pt._lib.pt_pathq_create(None, 0, 16, C.byref(h)) == pt.PT_E_INVALID
    assert pt._lib.pt_pathq_create(scene._h, 0, 16, None) == pt.PT_E_INVALID
    for bad in (0, 1 << 32, (1 << 32) + 5, (1 << 64) - 1):
        assert pt._lib.pt_pathq_create(scene._h, 0, bad, C.byref(h)) == pt.PT_E_INVALID, bad
        assert "max_paths" in pt.last_error()
    assert not h.value


def test_run_and_stats_reject_a_null_context():
    buf = np.zeros(32, np.uint8)
    assert pt._lib.pt_pathq_run(None, None, 1, U._p(buf), U._p(buf)) == pt.PT_E_INVALID
    assert pt._lib.pt_pathq_run(None, None, 0, None, None) == pt.PT_E_INVALID
    assert pt._lib.pt_pathq_stats(None, None) == pt.PT_E_INVALID
    pt._lib.pt_pathq_free(None)   # a no-op, like the other *_free


def test_radiance_rejects_bad_arguments(scene):
    rec = np.zeros(2, pt.PATH_DTYPE)
    out = np.zeros(2, pt.RADIANCE_DTYPE)
    assert pt._lib.pt_radiance(None, 0, 2, U._p(rec), U._p(out), None) == pt.PT_E_INVALID
    assert pt._lib.pt_radiance(scene._h, 0, 2, None, U._p(out), None) == pt.PT_E_INVALID
    assert pt._lib.pt_radiance(scene._h, 0, 2, U._p(rec), None, None) == pt.PT_E_INVALID
    # n = 0 asks for nothing: no buffers, no device
    st = pt.Stats()
    assert pt._lib.pt_radiance(scene._h, 0, 0, None, None, C.byref(st)) == pt.PT_OK
    assert st.rays == 0
    got, st = scene.radiance(np.zeros(0, pt.PATH_DTYPE))
    assert len(got) == 0 and got.dtype == pt.RADIANCE_DTYPE and st["rays"] == 0


def test_camera_rays_rejects_bad_arguments(scene):
    xy = np.zeros((2, 2), np.float32)
    rays = np.zeros((2, 6), np.float32)
    assert pt._lib.pt_camera_rays(None, 2, U._p(xy), U._p(rays)) == pt.PT_E_INVALID
    assert pt._lib.pt_camera_rays(scene._h, 2, None, U._p(rays)) == pt.PT_E_INVALID
    assert pt._lib.pt_camera_rays(scene._h, 2, U._p(xy), None) == pt.PT_E_INVALID
    assert pt._lib.pt_camera_rays(scene._h, 0, None, None) == pt.PT_OK
    assert scene.camera_rays(np.zeros((0, 2))).shape == (0, 6)


def test_radiance_without_gpu_fails_loudly(scene):
    if U.gpu_available():
        # (with a device the same calls succeed: tests/test_paths.py)
        with pt.PathQuery(scene, max_paths=8) as q:
            assert q.stats()["rays"] == 0
        return
    with pytest.raises(pt.PTError) as e:
        scene.radiance(np.zeros(3, pt.PATH_DTYPE))
    assert e.value.code in (pt.PT_E_NO_GPU, pt.PT_E_HIP)
    with pytest.raises(pt.PTError) as e:
        pt.PathQuery(scene, max_paths=8)
    assert e.value.code in (pt.PT_E_NO_GPU, pt.PT_E_HIP)


def test_record_layouts():
    assert pt.PATH_DTYPE.itemsize == 32
    assert [pt.PATH_DTYPE.fields[k][1] for k in ("o", "d", "seed", "reserved")] == [0, 12, 24, 28]
    assert pt.RADIANCE_DTYPE.itemsize == 16
    assert [pt.RADIANCE_DTYPE.fields[k][1] for k in ("rgb", "rays")] == [0, 12]
    assert pt.PATHS_CHUNK == 1 << 22


def test_camera_rays_are_the_camera_of_the_scene_text(scene):
    """practice5_1's camera, restated here in float32 in Camera::GetToRay's order"""
    inf = scene.info
    W, H = np.float32(inf["width"]), np.float32(inf["height"])
    cam = {}
    with open(U.scene_path("practice5_1.txt")) as f:
        for line in f:
            w = line.split()
            if w and w[0].startswith("CAMERA_"):
                cam[w[0]] = np.array([float(v) for v in w[1:]], np.float32)
    tx = np.float32(np.tan(np.float64(cam["CAMERA_FOV_X"][0] / np.float32(2))))
    ty = tx * H / W
    xy = np.array([[0.0, 0.0], [3.25, 7.5], [float(W) - 0.5, float(H) - 0.25]], np.float32)
    got = scene.camera_rays(xy)
    for (x, y), r in zip(xy, got):
        nx = (np.float32(2) * x / W - np.float32(1)) * tx
        ny = np.float32(-1) * (np.float32(2) * y / H - np.float32(1)) * ty
        d = nx * cam["CAMERA_RIGHT"] + ny * cam["CAMERA_UP"] + np.float32(1) * cam["CAMERA_FORWARD"]
        assert np.array_equal(r[:3].view(np.uint32), cam["CAMERA_POSITION"].view(np.uint32))
        assert np.array_equal(r[3:].view(np.uint32), d.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("name", P.FRAMES + P.WINDOWS)
def test_host_execution_matches_the_oracle(name):
    e = P.expected(pt, name)
    rec = e["records"]
    if name in P.FRAMES:
        assert rec["seed"][0] == 48271 ** 2 % P.M31   # pixel 0: seed 0 -> state 1, then two draws
    got, ctr = P.host_run(pt, name, e["path"], rec)
    P.assert_radiance(got, e["rad"])
    assert int(got["rays"].sum()) == e["rays"] == ctr["rays"]
    assert (got["rays"] >= 1).all()
    assert ctr["errors"] == 0


def test_ray_depth_0_gives_zeros_and_no_rays():
    with pt.Scene.loads(DEPTH0) as s:
        assert s.info["ray_depth"] == 0
        rec = np.zeros(70, pt.PATH_DTYPE)
        rec["d"] = (0.0, 0.0, -1.0)
        rec["o"] = (0.0, 0.0, 4.0)
        rec["seed"] = np.arange(70)
        got, ctr = s.selftest_paths_host(rec)
    assert not got.view(np.uint32).any()
    assert ctr["rays"] == 0 and ctr["node_visits"] == 0 and ctr["plane_tests"] == 0


def test_a_record_is_a_function_of_its_ray_and_seed():
    e = P.expected(pt, "hw3s3_48x48x8")
    rec = np.array(e["records"][:512])
    twice = np.concatenate([rec, rec])
    with pt.Scene.load(e["path"]) as s:
        got, _ = s.selftest_paths_host(twice)
        other = rec.copy()
        other["seed"] = other["seed"] ^ np.uint32(0x5bd1e995)
        got2, _ = s.selftest_paths_host(other)
    assert got[:512].tobytes() == got[512:].tobytes()
    # the same rays with other seeds: a diffuse scene's paths differ somewhere
    assert (got2["rgb"].view(np.uint32) != got["rgb"][:512].view(np.uint32)).any()
