"""The path engine's query trip on the GPU with one q_decide per trip, after the trip's steps
(pt_path.hip path_query_wave), and the parts of the trip around it that other cuts of the same
round touched and did not keep (profiles/r25_trip): the refill of a workgroup that is always at
its cap, and the done ring when it is full.

Every render here runs on k_wpath alone (PT_TUNE coop=0) and is compared with the CPU oracle's
render of the same scene text: f32 radiance bits, image bytes, ray count; no exactness error, no
pixel short of its samples.

  * the 60 stacked triangles of test_query_step.py (adds into a partly entered list, rejects,
    overflow passes, the exact hand-over) under the deferred decide;
  * the dragon fixture under other step mixes (no extra aux step, two, a probe every trip);
  * workgroups that are always full (cap=8,batch=4: a workgroup of 128 query lanes may hold 64
    chains -- the smallest cap there is -- so its waves always have idle lanes, refill every trip
    and find it full), once more with rounds that end after two trips (suspends and flushes);
  * done rings that are full: see test_done_ring_full.
"""
import re

import numpy as np
import pytest

import _util as U
import test_query_step as QS

pytestmark = pytest.mark.gpu

DRAGON = "dragon_64x64x16"
DQN = 48   # pt_kernels.h PT_DQN: a done ring's entries


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("trip_gpu")


_oracle = {}   # scene path -> the oracle's (image, radiance, counters): rendered once, read only


def oracle(path):
    if path not in _oracle:
        rgb, rad, ctr = U.OracleScene(path).render()
        rgb.setflags(write=False)
        rad.setflags(write=False)
        _oracle[path] = (rgb, rad, ctr)
    return _oracle[path]


def render_and_check(pt, path, tune, monkeypatch):
    monkeypatch.setenv("PT_TUNE", tune)
    orgb, orad, octr = oracle(path)
    with pt.Scene.load(path) as s:
        s.prepare()
        rgb, rad, st = s.render(radiance=True, traversal=0)
    print("%s: rays %d (oracle %d), errors %d, short %d, fallbacks %d, rounds %d, handoff %r"
          % (tune, st["rays"], octr["rays"], st["errors"], st["short_pixels"], st["fallbacks"], st["rounds"],
             st["handoff"]))
    assert np.array_equal(rad.view(np.uint32), orad.view(np.uint32))
    assert np.array_equal(rgb, orgb)
    assert st["rays"] == octr["rays"]
    assert st["errors"] == 0
    assert st["short_pixels"] == 0
    return st


def test_stacked_triangles_under_the_deferred_decide(pt, tmp_root, monkeypatch):
    path = QS.ray_set("stack", tmp_root)[0]
    st = render_and_check(pt, path, "coop=0", monkeypatch)
    assert st["rays"] == 64        # 8 x 8 pixels, 1 sample, RAY_DEPTH 1: the camera rays
    assert st["fallbacks"] > 0     # camera rays down the stack: full lists, the exact hand-over


@pytest.mark.parametrize("mix", ["aux_extra=0", "aux_extra=2", "probe_every=1"])
def test_step_mix_sweep(pt, mix, monkeypatch):
    render_and_check(pt, U.golden_scene_path(DRAGON), "coop=0," + mix, monkeypatch)


@pytest.mark.parametrize("rounds", ["", ",runend=0,budget=2"])
def test_workgroups_that_are_always_full(pt, rounds, monkeypatch):
    st = render_and_check(pt, U.golden_scene_path(DRAGON), "coop=0,cap=8,batch=4" + rounds, monkeypatch)
    if rounds:
        # rounds that end two trips after their work ran out: running queries are suspended,
        # and what the shade wave emits after the query waves left goes to the next round
        assert st["handoff"]["suspend"] > 0 and st["handoff"]["flush"] + st["handoff"]["ringout"] > 0, st["handoff"]


def test_done_ring_full(pt, tmp_root, monkeypatch, capfd):
    """Finished queries that do not fit their wave's done ring wait in their lanes, phase
    Q_DONE, through trips whose decide must leave them alone, and are suspended at the round's
    end (the path a done-ring head kept from trip to trip would have to get right).

    The arithmetic.  The fixture's scene at C x 128 pixels, 1 sample, on a device of C compute
    units: 128 C chains.  wg_per_cu=1 launches C workgroups of two query waves, all resident at
    once, and a wave takes the round's work in batches of min(batch, chains / waves) = min(32, 64)
    = 32 for as long as it has idle lanes: the 2 C waves take all 128 C chains at once, 64 per
    wave on average.  shade_hold=1 keeps every shade wave from reading its done rings until its
    workgroup's query waves have left, and they leave budget_us = 3 ms after the work ran out
    (runend=0: however few the chains) -- hundreds of trips, where a query of this scene takes
    tens.  So in the first round 128 C queries finish while nothing is consumed, the 2 C rings
    hold 2 C x 48 = 96 C of them, and at least 32 C finished queries (less the few handed to the
    exact DFS) find their ring full, wait in their lanes and are suspended at the round's end.
    The later rounds repeat it with the chains' next rays.  The engine counts the finished
    queries it suspends while their ring is full, and PT_TUNE roundlog=2 prints the count
    (`dq_full`, the session's total so far) with every round."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    text = open(U.golden_scene_path(DRAGON)).read()
    text, nd = re.subn(r"(?m)^DIMENSIONS\s+\d+\s+\d+", "DIMENSIONS %d 128" % cus, text)
    text, ns = re.subn(r"(?m)^SAMPLES\s+\d+", "SAMPLES 1", text)
    assert nd == 1 and ns == 1
    path = str(tmp_root / "dragon_wide.txt")
    with open(path, "w") as f:
        f.write(text)
    tune = "coop=0,wg_per_cu=1,cap=384,batch=32,shade_hold=1,runend=0,budget_us=3000,roundlog=2"
    st = render_and_check(pt, path, tune, monkeypatch)
    log = capfd.readouterr().err
    full = [int(m) for m in re.findall(r"(?m)^round \d+ chains .* dq_full (\d+)$", log)]
    print("chains %d, rings hold %d; dq_full per round (running total): %r" % (128 * cus, 2 * cus * DQN, full))
    assert full and full == sorted(full)
    assert full[0] >= 128 * cus - 2 * cus * DQN - st["fallbacks"]   # the first round's, by the arithmetic above
    assert st["handoff"]["suspend"] > 0 and st["handoff"]["flush"] > 0, st["handoff"]
