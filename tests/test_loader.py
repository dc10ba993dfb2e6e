"""The loader's rules through to pixels (MI355X): scenes of tests/_loader_cases.py whose wrong
parse changes the image, against the reference's own image and fp32 radiance of the same file
(tests/golden/make_golden_loader.py).  Bar: bit-exact, as tests/test_gpu.py's standing fixtures.
"""
import os

import numpy as np
import pytest

import _loader_cases as LC
import _util as U

pytestmark = pytest.mark.gpu
W, H, SPP = 12, 8, 2


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


def golden(name):
    base = "loader_" + name[len("render_"):]
    img = U.read_ppm(os.path.join(U.GOLDEN, "img_%s.ppm" % base))
    rad = np.fromfile(os.path.join(U.GOLDEN, "rad_%s.f32" % base), np.float32).reshape(img.shape)
    assert img.shape == (H, W, 3) and np.isfinite(rad).all()
    return img, rad


@pytest.mark.parametrize("name", sorted(LC.RENDERED))
def test_render_matches_reference(pt, name):
    img, rad = golden(name)
    with pt.Scene.loads(LC.CASES[name]) as s:
        s.prepare()
        inf = s.info
        assert (inf["width"], inf["height"], inf["samples"], inf["ray_depth"]) == (W, H, SPP, 3)
        rgb, r, st = s.render(radiance=True)
    assert st["errors"] == 0
    assert r.view(np.uint32).tolist() == rad.view(np.uint32).tolist()
    assert np.array_equal(rgb, img)


@pytest.mark.parametrize("name", sorted(LC.RENDERED))
def test_session_pass_matches_reference(pt, name):
    import torch
    img, rad = golden(name)
    with pt.Scene.loads(LC.CASES[name]) as s:
        s.prepare()
        ss = pt.Session(s, device=0)
        try:
            ss.trace(SPP)
            drad = torch.empty(ss.n_tiles * 256 * 3, dtype=torch.float32, device="cuda")
            ss.resolve(dev_rad=drad.data_ptr())
            ss.sync()
            assert ss.stats()["errors"] == 0
            rgb = np.zeros((H, W, 3), np.uint8)
            r = np.zeros((H, W, 3), np.float32)
            pt.unpack_tiles(ss.read_packed(), W, H, 0, 1, out=rgb)
            pt.unpack_tiles_f32(drad.cpu().numpy(), W, H, 0, 1, out=r)
        finally:
            ss.close()
    assert r.view(np.uint32).tolist() == rad.view(np.uint32).tolist()
    assert np.array_equal(rgb, img)
