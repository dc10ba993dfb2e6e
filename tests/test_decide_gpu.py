"""The aux step's short body on the GPU (pt_query.h q_exec_aux / q_aux_entries;
tests/test_decide_host.py has the host's side): the per-entry bookkeeping without the range
test, picked per wave by a scalar test, so a wave runs the general body as soon as one of its
lanes is in a later pass or holds a full list.

  * k_rays / k_rays_exact on the stack, stack_few, zero and bulk1 sets of test_query_step.py:
    the oracle's answers and the host state machine's work counters.  The stack set's waves mix
    lanes in later passes and with full lists (the range test decides for them) with lanes in
    their first pass; every wave of bulk1 stays on the short body.
  * k_wpath alone (PT_TUNE coop=0): the 8 x 8 stacked-triangle scene and the dragon fixture
    against the CPU oracle's render of the same scene text -- f32 radiance bits, image bytes,
    ray count, no exactness error, no pixel short of its samples -- with no extra aux-node
    step per trip and with two (the aux step is compiled into the trip twice: the step and
    path_aux_extra's).
"""
import numpy as np
import pytest

import _rays as R
import _util as U
import test_query_step as QS

pytestmark = pytest.mark.gpu

DRAGON = "dragon_64x64x16"


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("decide_gpu")


_oracle = {}   # scene path -> the oracle's (image, radiance, counters): rendered once, read only


def oracle(path):
    if path not in _oracle:
        rgb, rad, ctr = U.OracleScene(path).render()
        rgb.setflags(write=False)
        rad.setflags(write=False)
        _oracle[path] = (rgb, rad, ctr)
    return _oracle[path]


@pytest.mark.parametrize("name", ["stack", "stack_few", "zero", "bulk1"])
def test_ray_queries_match_the_oracle_and_the_host_counters(pt, tmp_root, name):
    path, rays, oids, ohits = QS.ray_set(name, tmp_root)
    want = R.expected_hits(pt, oids, ohits[:, :4], ohits[:, 4])
    with pt.Scene.load(path) as s:
        s.prepare()
        _, _, host = s.selftest_ray_intersection(rays, traversal=0)
        got, st = s.intersect(rays)
        n_planes = s.info["n_planes"]
    print("%s: %d rays, GPU counters %r" % (name, len(rays), (st["node_visits"], st["prim_tests"], st["aux_visits"],
                                                               st["fallbacks"])))
    assert np.array_equal(got["id"], want["id"])
    hit = want["id"] != -1
    assert np.array_equal(got["t"][hit].view(np.uint32), want["t"][hit].view(np.uint32))
    assert np.array_equal(got["n"][hit].view(np.uint32), want["n"][hit].view(np.uint32))
    assert np.array_equal(got["interior"][hit], want["interior"][hit])
    assert st["errors"] == 0 and st["rays"] == len(rays) and st["plane_tests"] == len(rays) * n_planes
    assert (st["node_visits"], st["prim_tests"], st["aux_visits"], st["fallbacks"]) == \
        (host["nodes"], host["prim_tests"], host["aux"], host["fallbacks"])
    QS.assert_parent_counters(name, host)
    if name == "stack":
        assert st["fallbacks"] > 0   # lists full of entered hits: lanes that need the general body


@pytest.mark.parametrize("aux_extra", [0, 2])
@pytest.mark.parametrize("scene", ["stack", "dragon"])
def test_path_engine_renders_match_the_oracle(pt, tmp_root, monkeypatch, scene, aux_extra):
    path = QS.ray_set("stack", tmp_root)[0] if scene == "stack" else U.golden_scene_path(DRAGON)
    monkeypatch.setenv("PT_TUNE", "coop=0,aux_extra=%d" % aux_extra)
    orgb, orad, octr = oracle(path)
    with pt.Scene.load(path) as s:
        s.prepare()
        rgb, rad, st = s.render(radiance=True, traversal=0)
    print("%s aux_extra=%d: rays %d (oracle %d), errors %d, short %d, fallbacks %d"
          % (scene, aux_extra, st["rays"], octr["rays"], st["errors"], st["short_pixels"], st["fallbacks"]))
    assert np.array_equal(rad.view(np.uint32), orad.view(np.uint32))
    assert np.array_equal(rgb, orgb)
    assert st["rays"] == octr["rays"]
    assert st["errors"] == 0
    assert st["short_pixels"] == 0
    if scene == "stack":
        assert st["rays"] == 64 and st["fallbacks"] > 0   # camera rays down the stack: full lists
