"""GPU tests of the pixel-sample engine (k_pixels through pt_sample_pixels and pt_pixq_*):
Scene::Sample's loop for the caller's pixel states, bit for bit, resumable.

The cases and their expected values are those of tests/_pixels.py (the CPU oracle's renders, the
reference's recorded radiance), the same tests/test_pixels_host.py runs on the host twin.  Every
GPU run here is also held to the host twin of the same records: the states byte for byte, and
the work counters -- a record's steps depend on its state, its count and the scene only, never
on which lane ran it.
"""
import numpy as np
import pytest

import _pixels as X
import _util as U

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "node_visits", "prim_tests", "plane_tests", "aux_visits", "fallbacks", "fallbacks_ray", "samples")
GUARD = 64   # records of 0xA5 behind a device buffer's n records


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


def counters(st):
    return tuple(st[k] for k in COUNTERS)


def against_the_twin(s, state, counts, spp, out, st):
    want, host = s.selftest_pixels_host(state, counts=counts, spp=spp)
    assert out.tobytes() == want.tobytes(), "the GPU's states differ from the host twin's"
    assert st["errors"] == 0 and host["errors"] == 0 and counters(st) == counters(host)


def run_api(s, state, counts=None, spp=0):
    """pt_sample_pixels"""
    out, st = s.sample_pixels(state, counts=counts, spp=spp)
    against_the_twin(s, state, counts, spp, out, st)
    return out, st


def device_state(pt, torch, state):
    d = torch.full(((len(state) + GUARD) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
    d[:len(state) * 32] = torch.from_numpy(np.array(state).view(np.uint8)).cuda()
    return d


def read_state(pt, d, n):
    raw = d.cpu().numpy()
    assert (raw[n * 32:] == 0xA5).all(), "the run wrote past its n records"
    return raw[:n * 32].view(pt.PIXEL_DTYPE).copy()


def run_query(s, state, counts=None, spp=0, stream=None):
    """pt_pixq_* on torch tensors, the state buffer followed by guard records"""
    import torch
    pt = U.ptrace()
    n = len(state)
    with pt.PixelQuery(s, max_pixels=max(n, 1)) as q:
        d = device_state(pt, torch, state)
        dc = None if counts is None else torch.from_numpy(np.ascontiguousarray(counts, np.uint32).view(np.int32)).cuda()
        torch.cuda.synchronize()
        q.run(d, counts=dc, spp=spp, n=n, stream=stream)
        st = q.stats()
        out = read_state(pt, d, n)
    against_the_twin(s, state, counts, spp, out, st)
    return out, st


# ---- 1. whole frames ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.WHOLE_FRAMES)
def test_whole_frames_at_the_reference_sample_count(pt, name):
    X.case_whole_frame(pt, run_api, name)


# ---- 2. resume ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,splits", [("dragon_glass_40x24x7", ((3, 4), (1,) * 7, (7,))),
                                         ("hw3s4_24x40x5", ((2, 3), (5,)))])
def test_a_run_of_a_then_b_is_a_run_of_a_plus_b(pt, name, splits):
    # (that the records at the split carry saved values and none in fair parts: tests/test_pixels_host.py)
    X.case_resume(pt, run_query, name, splits)


# ---- 3. per-pixel counts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,window", [("mat_matrix_24x24x8", (0, 0, 24, 24)), ("many_lights_48x48x8", (0, 0, 24, 24))])
def test_per_pixel_counts_and_a_second_run_with_zeros(pt, name, window):
    X.case_counts(pt, run_query, name, window)


# ---- 4. shapes ----------------------------------------------------------------------------------------------
# (1,000 records are four workgroups, whose waves pull 64 records at a time: no multiple of the batch)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_first_pixels(pt, n):
    X.case_first_pixels(pt, run_query, n)


def test_scattered_pixels_with_one_twice(pt):
    X.case_scattered(pt, run_query)


def test_one_long_record_among_short_ones(pt):
    # (the run returns: the lane of the long record goes on alone while the others have left)
    X.case_one_long_record(pt, run_query)


@pytest.mark.parametrize("service", [1, 64])
def test_pixels_service_does_not_change_the_states(pt, service, monkeypatch):
    want, st0 = X.case_first_pixels(pt, run_query, 1000)
    monkeypatch.setenv("PT_TUNE", "pixels_service=%d" % service)   # read when the context is made
    got, st = X.case_first_pixels(pt, run_query, 1000)
    assert got.tobytes() == want.tobytes() and counters(st) == counters(st0)


# ---- 5. depth -----------------------------------------------------------------------------------------------
def test_ray_depth_1_by_override(pt):
    X.case_depth_1(pt, run_api)


def test_ray_depth_10(pt):
    X.case_depth_10(pt, run_query)


def test_ray_depth_0_draws_the_jitter_and_adds_zero(pt):
    X.case_depth_0(pt, run_query)


# ---- 6. seeds -----------------------------------------------------------------------------------------------
def test_seeds_are_reduced_as_minstd_rand_reduces_them(pt):
    X.case_seed_reduction(pt, run_api)


def test_arbitrary_seeds_against_the_batch_radiance_engine(pt):
    # a cross-engine check, not an oracle one (tests/_pixels.py)
    X.case_arbitrary_seeds_cross_engine(pt, run_query, lambda s, rec: s.radiance(rec))


# ---- 8. arguments and run rules -------------------------------------------------------------------------
def test_run_refuses_a_misaligned_pointer_and_more_than_max_pixels(pt):
    import torch
    path, _ = X.dragon_expected()
    with pt.Scene.load(path) as s:
        state = s.pixel_init(X.window_xy((0, 0, 64, 64))[:65])
        with pt.PixelQuery(s, max_pixels=64) as q:
            d = device_state(pt, torch, state)
            before = d.cpu().numpy().copy()
            for kw in ({"n": 65}, {"n": 8, "off": 8}, {"n": 8, "off": 4}):
                with pytest.raises(pt.PTError) as err:
                    q.run(d.data_ptr() + kw.get("off", 0), spp=1, n=kw["n"])
                assert err.value.code == pt.PT_E_INVALID, kw
            dc = torch.zeros(64, dtype=torch.int32, device="cuda")
            with pytest.raises(pt.PTError) as err:
                q.run(d, counts=dc.data_ptr() + 2, n=8)
            assert err.value.code == pt.PT_E_INVALID
            q.run(d, spp=3, n=0)   # enqueues nothing
            q.run(0, spp=3, n=0)
            st = q.stats()
            assert st["samples"] == 0 and st["rays"] == 0 and st["kernel_ms"] == 0.0
            assert np.array_equal(d.cpu().numpy(), before)


def test_a_context_serves_runs_of_different_sizes(pt):
    import torch
    path, orad = X.dragon_expected()
    with pt.Scene.load(path) as s:
        state = s.pixel_init(X.window_xy((0, 0, 64, 64)))
        with pt.PixelQuery(s, max_pixels=4096) as q:
            total = 0
            for n in (4096, 1, 700, 64):
                d = device_state(pt, torch, state[:n])
                q.run(d, spp=1, n=n)
                q.run(d, spp=1, n=n)   # the same records again: two samples in two runs
                out = read_state(pt, d, n)
                mean, _ = s.pixel_resolve(out)
                X.assert_bits(mean, orad[:n], "a run of %d" % n)
                total += 2 * n
            st = q.stats()
    assert st["samples"] == total and st["errors"] == 0 and st["kernel_ms"] > 0.0


def test_a_run_on_a_callers_stream_is_ordered_with_the_callers_work(pt):
    import torch
    path, orad = X.dragon_expected()
    n = 2048
    with pt.Scene.load(path) as s:
        state = s.pixel_init(X.window_xy((0, 0, 64, 64))[:n])
        with pt.PixelQuery(s, max_pixels=n) as q:
            stream = torch.cuda.Stream()
            d = device_state(pt, torch, state)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                q.run(d, spp=2, n=n, stream=stream.cuda_stream)
                # the caller's own work behind the run, on the same stream: the sums of the finished states
                sums = d[:n * 32].view(torch.float32).view(n, 8)[:, 4:7].clone()
                samples = d[:n * 32].view(torch.int32).view(n, 8)[:, 7].clone()
            stream.synchronize()
            st = q.stats()
            out = read_state(pt, d, n)
        mean, _ = s.pixel_resolve(out)
    assert (samples.cpu().numpy() == 2).all()
    assert np.array_equal(sums.cpu().numpy().view(np.uint32), out["sum"].view(np.uint32))
    X.assert_bits(mean, orad[:n], "a run on a caller's stream")
    assert st["samples"] == 2 * n and st["errors"] == 0


def test_sample_pixels_leaves_its_argument_alone(pt):
    path, _ = X.dragon_expected()
    with pt.Scene.load(path) as s:
        state = s.pixel_init(X.window_xy((0, 0, 64, 64))[:100])
        before = state.tobytes()
        out, st = s.sample_pixels(state, counts=np.arange(100) % 3)
    assert state.tobytes() == before and np.array_equal(out["samples"], np.arange(100) % 3)
    assert out[::3].tobytes() == state[::3].tobytes()


# ---- a context's statistics are those of the runs since the last call -----------------------------
def test_stats_report_each_run_once(pt):
    """Two equal runs of 65 records (a wave and a lane) on one context, a stats() after each: the second
    reports what the first did -- the context's counters run on, a stats() is the difference since
    the last one --, and a third stats(), with no run since, no work and no time."""
    import torch
    with pt.Scene.load(U.golden_scene_path("mat_matrix_24x24x8")) as s:
        state = s.pixel_init(X.window_xy((5, 9, 13, 5)))
        with pt.PixelQuery(s, max_pixels=65) as q:
            d1, d2 = device_state(pt, torch, state), device_state(pt, torch, state)   # (a run updates its states)
            torch.cuda.synchronize()
            q.run(d1, spp=2, n=65)
            a = q.stats()
            q.run(d2, spp=2, n=65)
            b = q.stats()
            c = q.stats()
    assert a["samples"] == 130 and a["rays"] >= 130 and a["node_visits"] > 0 and a["prim_tests"] > 0 and a["kernel_ms"] > 0.0
    assert (b["rays"], b["node_visits"], b["prim_tests"], b["samples"]) == \
        (a["rays"], a["node_visits"], a["prim_tests"], a["samples"])
    assert c["rays"] == 0 and c["samples"] == 0 and c["kernel_ms"] == 0
