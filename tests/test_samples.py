"""Sample counts that are no power of two, on the GPU against the CPU oracle.

The reference's mean is (1.f / SAMPLES) * sum (src/scene.cpp:201).  For a power of two 1 / S is
exact, and then (1 / S) * sum, sum / S and a product with an approximate reciprocal are the same
float: none of those mistakes can show at S = 1, 2, 4, 8 ...  At S = 3 a third of all sums tell
them apart, at S = 7 more than half.  Here pt_render, the progressive session (resolve in the
middle of a pass: "sum / samples so far" is the same rule with a moving S), pt_session_reset and
the launch chunking are compared with the oracle at such S -- radiance as bit patterns, and the
8-bit image.
"""
import functools

import numpy as np
import pytest

import _util as U

pytestmark = pytest.mark.gpu

W, H = 40, 24   # off the 16-pixel tile grid in both directions: 3 x 2 tiles, partial right and bottom


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


def scene_file():
    return U.scene_path("practice5_dragon_10k.txt", (W, H, 7, False, "diffuse"))


@functools.lru_cache(None)
def oracle_at(spp):
    """(image, radiance) of the oracle at spp samples; computed once per spp, never written to"""
    rgb, rad, _ = U.OracleScene(scene_file()).render(spp=spp)
    rgb.setflags(write=False)
    rad.setflags(write=False)
    return rgb, rad


def same(rgb, rad, spp):
    orgb, orad = oracle_at(spp)
    assert np.array_equal(rad.view(np.uint32), orad.view(np.uint32)), "radiance differs from the oracle at spp=%d" % spp
    assert np.array_equal(rgb, orgb), "image differs from the oracle at spp=%d" % spp


@pytest.mark.parametrize("S", [1, 3, 5, 6, 7, 10, 100])
def test_render_sample_counts_vs_oracle(pt, S):
    with pt.Scene.load(scene_file()) as s:
        rgb, rad, st = s.render(samples=S, radiance=True)
    assert st["errors"] == 0 and st["short_pixels"] == 0
    same(rgb, rad, S)


@pytest.mark.parametrize("chunk", [1, 2, 7])
def test_launch_chunks_vs_oracle(pt, chunk):
    with pt.Scene.load(scene_file()) as s:
        rgb, rad, st = s.render(samples=7, spp_per_launch=chunk, radiance=True)
    assert st["errors"] == 0 and st["short_pixels"] == 0
    same(rgb, rad, 7)


def _read(pt, sessions, drads):
    """resolve + sync every rank's session; the stitched (image, radiance)"""
    world = len(sessions)
    rgb = np.zeros((H, W, 3), np.uint8)
    rad = np.zeros((H, W, 3), np.float32)
    for r, (ss, drad) in enumerate(zip(sessions, drads)):
        ss.resolve(dev_rad=drad.data_ptr())
        ss.sync()
        pt.unpack_tiles(ss.read_packed(), W, H, r, world, out=rgb)
        pt.unpack_tiles_f32(drad.cpu().numpy(), W, H, r, world, out=rad)
    return rgb, rad


def _sessions(pt, s, world):
    import torch
    sessions = [pt.Session(s, rank=r, world=world) for r in range(world)]
    drads = [torch.zeros(ss.n_tiles * 256 * 3, dtype=torch.float32, device="cuda") for ss in sessions]
    return sessions, drads


@pytest.mark.parametrize("world", [1, 3])
def test_progressive_session_vs_oracle(pt, world):
    """trace(3), resolve: the oracle at 3 spp; trace(4) more, resolve: the oracle at 7 spp"""
    with pt.Scene.load(scene_file()) as s:
        s.prepare()
        sessions, drads = _sessions(pt, s, world)
        for ss in sessions:
            ss.trace(3)
        rgb, rad = _read(pt, sessions, drads)
        assert all(ss.stats()["short_pixels"] == 0 and ss.stats()["errors"] == 0 for ss in sessions)
        same(rgb, rad, 3)
        for ss in sessions:
            ss.trace(4)
        rgb, rad = _read(pt, sessions, drads)
        assert all(ss.stats()["short_pixels"] == 0 and ss.stats()["errors"] == 0 for ss in sessions)
        same(rgb, rad, 7)
        for ss in sessions:
            ss.close()


def test_session_reset_vs_oracle(pt):
    """trace(5), resolve, reset, trace(3), resolve: the oracle at 3 spp"""
    with pt.Scene.load(scene_file()) as s:
        s.prepare()
        sessions, drads = _sessions(pt, s, 1)
        sessions[0].trace(5)
        rgb, rad = _read(pt, sessions, drads)
        same(rgb, rad, 5)
        sessions[0].reset()
        sessions[0].trace(3)
        rgb, rad = _read(pt, sessions, drads)
        assert sessions[0].stats()["short_pixels"] == 0
        same(rgb, rad, 3)
        sessions[0].close()
