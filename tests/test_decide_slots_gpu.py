"""q_decide against its reference and the aux entries' ready-made words on the GPU (pt_query.h,
pt_wcoop.hip; tests/test_decide_slots_host.py has the host's side, and says which form of
q_decide the tree holds).

  * k_selftest_decide: q_decide on the seeded decision states of pt_selftest_decide, 64
    consecutive states to a wave, against the host's plain loop byte for byte.  The lanes of a
    wave sit at different slots: some waves have no live lane at a slot, some a single live lane
    at the last one, and the last wave is partial.
  * k_rays / k_rays_exact on the stack, stack_few, zero and bulk1 sets of test_query_step.py:
    the oracle's answers and that file's PARENT_COUNTERS.  The stack set (60 stacked triangles)
    is the smallest input with full lists, overflow passes and exact hand-overs.
  * the 8 x 8 stacked-triangle scene and the dragon fixture against the CPU oracle's render --
    f32 radiance bits, image bytes, ray count, no exactness error, no pixel short of its samples:
    on k_wpath alone (PT_TUNE coop=0) with no extra aux-node step per trip and with two, and on
    the cooperative engine alone (coop=100000000), whose expansion reads the entries' new words.
"""
import numpy as np
import pytest

import _rays as R
import _util as U
import test_query_step as QS

pytestmark = pytest.mark.gpu

DRAGON = QS.DRAGON
SEEDS = [1, 2, 3]
N = 100000


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("decide_slots_gpu")


_oracle = {}   # scene path -> the oracle's (image, radiance, counters): rendered once, read only


def oracle(path):
    if path not in _oracle:
        rgb, rad, ctr = U.OracleScene(path).render()
        rgb.setflags(write=False)
        rad.setflags(write=False)
        _oracle[path] = (rgb, rad, ctr)
    return _oracle[path]


@pytest.mark.parametrize("seed", SEEDS)
def test_device_decide_equals_the_host_loop(pt, seed):
    want, exits, slots = pt.selftest_decide_states(seed, N)
    got, _, _ = pt.selftest_decide_states(seed, N, device=0)
    differ = np.flatnonzero((want != got).any(axis=1))
    print("seed %d: %d states of %d bytes, %d differ, exits %r, deciding slots %r"
          % (seed, len(want), want.shape[1], len(differ), exits, slots))
    assert want.shape == got.shape and len(want) == N
    assert len(differ) == 0, "first differing states: %r" % differ[:8].tolist()
    assert all(v > 0 for v in exits.values()) and all(c > 0 for c in slots)


@pytest.mark.parametrize("name", ["stack", "stack_few", "zero", "bulk1"])
def test_ray_queries_match_the_oracle_and_the_parent_counters(pt, tmp_root, name):
    path, rays, oids, ohits = QS.ray_set(name, tmp_root)
    want = R.expected_hits(pt, oids, ohits[:, :4], ohits[:, 4])
    with pt.Scene.load(path) as s:
        s.prepare()
        got, st = s.intersect(rays)
        n_planes = s.info["n_planes"]
    ctr = {"nodes": st["node_visits"], "prim_tests": st["prim_tests"], "aux": st["aux_visits"],
           "fallbacks": st["fallbacks"]}
    print("%s: %d rays, GPU counters %r" % (name, len(rays), ctr))
    assert np.array_equal(got["id"], want["id"])
    hit = want["id"] != -1
    assert np.array_equal(got["t"][hit].view(np.uint32), want["t"][hit].view(np.uint32))
    assert np.array_equal(got["n"][hit].view(np.uint32), want["n"][hit].view(np.uint32))
    assert np.array_equal(got["interior"][hit], want["interior"][hit])
    assert st["errors"] == 0 and st["rays"] == len(rays) and st["plane_tests"] == len(rays) * n_planes
    QS.assert_parent_counters(name, ctr)


@pytest.mark.parametrize("engine", ["coop=0,aux_extra=0", "coop=0,aux_extra=2", "coop=100000000"])
@pytest.mark.parametrize("scene", ["stack", "dragon"])
def test_engine_renders_match_the_oracle(pt, tmp_root, monkeypatch, scene, engine):
    path = QS.ray_set("stack", tmp_root)[0] if scene == "stack" else U.golden_scene_path(DRAGON)
    monkeypatch.setenv("PT_TUNE", engine)
    orgb, orad, octr = oracle(path)
    with pt.Scene.load(path) as s:
        s.prepare()
        rgb, rad, st = s.render(radiance=True, traversal=0)
    print("%s %s: rays %d (oracle %d), errors %d, short %d, fallbacks %d, coop rays %d"
          % (scene, engine, st["rays"], octr["rays"], st["errors"], st["short_pixels"], st["fallbacks"],
             st.get("coop_rays", -1)))
    assert np.array_equal(rad.view(np.uint32), orad.view(np.uint32))
    assert np.array_equal(rgb, orgb)
    assert st["rays"] == octr["rays"]
    assert st["errors"] == 0
    assert st["short_pixels"] == 0
    if engine.startswith("coop=1"):
        assert st.get("coop_rays", 1) > 0   # the cooperative engine did the work
