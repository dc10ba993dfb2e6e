"""CPU tests of the ray-query interface (include/pt.h pt_rayq_*, pt_intersect; ptrace.RayQuery,
Scene.intersect) -- no GPU needed: argument checks come before the device check, the hit
record's layout is the committed traversal fixtures', and without a GPU a query fails loudly.
"""
import ctypes as C

import numpy as np
import pytest

import _util as U

M = U.manifest()
pt = U.ptrace()


@pytest.fixture(scope="module")
def scene():
    with pt.Scene.load(U.scene_path("practice5_1.txt")) as s:
        yield s


def test_create_rejects_bad_arguments(scene):
    h = C.c_void_p()
    assert pt._lib.pt_rayq_create(None, 0, 16, C.byref(h)) == pt.PT_E_INVALID
    assert pt._lib.pt_rayq_create(scene._h, 0, 16, None) == pt.PT_E_INVALID
    for bad in (0, 1 << 32, (1 << 32) + 5, (1 << 64) - 1):
        assert pt._lib.pt_rayq_create(scene._h, 0, bad, C.byref(h)) == pt.PT_E_INVALID, bad
        assert "max_rays" in pt.last_error()
    assert not h.value


def test_run_and_stats_reject_a_null_context():
    buf = np.zeros(24, np.uint8)
    assert pt._lib.pt_rayq_run(None, None, 1, U._p(buf), U._p(buf)) == pt.PT_E_INVALID
    assert pt._lib.pt_rayq_run(None, None, 0, None, None) == pt.PT_E_INVALID
    assert pt._lib.pt_rayq_stats(None, None) == pt.PT_E_INVALID
    pt._lib.pt_rayq_free(None)   # a no-op, like the other *_free


def test_intersect_rejects_bad_arguments(scene):
    rays = np.zeros((2, 6), np.float32)
    hits = np.zeros(2, pt.HIT_DTYPE)
    assert pt._lib.pt_intersect(None, 0, 2, U._p(rays), U._p(hits), None) == pt.PT_E_INVALID
    assert pt._lib.pt_intersect(scene._h, 0, 2, None, U._p(hits), None) == pt.PT_E_INVALID
    assert pt._lib.pt_intersect(scene._h, 0, 2, U._p(rays), None, None) == pt.PT_E_INVALID
    # n = 0 asks for nothing: no buffers, no device
    st = pt.Stats()
    assert pt._lib.pt_intersect(scene._h, 0, 0, None, None, C.byref(st)) == pt.PT_OK
    assert st.rays == 0


def test_intersect_without_gpu_fails_loudly(scene):
    if U.gpu_available():
        pytest.skip("GPU present")
    with pytest.raises(pt.PTError) as e:
        scene.intersect(np.zeros((3, 6), np.float32))
    assert e.value.code in (pt.PT_E_NO_GPU, pt.PT_E_HIP)
    with pytest.raises(pt.PTError) as e:
        pt.RayQuery(scene, max_rays=8)
    assert e.value.code in (pt.PT_E_NO_GPU, pt.PT_E_HIP)


def test_hit_dtype_is_the_24_byte_record():
    assert pt.HIT_DTYPE.itemsize == 24
    assert [pt.HIT_DTYPE.fields[k][1] for k in ("id", "t", "n", "interior")] == [0, 4, 8, 20]
    assert pt.RAYS_CHUNK == 1 << 22


@pytest.mark.parametrize("name", sorted(M["trav"]))
def test_hit_dtype_reads_the_traversal_fixtures(name):
    rays, ((ids, f, inter), _) = U.read_trav(name)
    raw = np.fromfile(U.os.path.join(U.GOLDEN, "trav_%s.bin" % name), np.uint8).reshape(-1, 72)
    h = np.ascontiguousarray(raw[:, 24:48]).view(pt.HIT_DTYPE).reshape(-1)
    assert len(h) == len(rays)
    assert np.array_equal(h["id"], ids)
    assert np.array_equal(h["t"].view(np.uint32), f[:, 0].view(np.uint32))
    assert np.array_equal(h["n"].view(np.uint32), f[:, 1:4].view(np.uint32))
    assert np.array_equal(h["interior"], inter)
