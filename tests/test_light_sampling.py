"""The vertex step's light sampling -- sample_mix_e's one emitter test per direction, handed
on to pdf_mix_e as that emitter's first pdf point, and normal01_vec's two polar loops -- in
every engine that runs it: the path engine (`coop=0`), k_wexact / k_wshade
(`coop=0,lstack=1`), the cooperative engine (`coop=100000000`) and the default choice.
Scenes: _shade_scenes.py, one surface of every primitive kind with and without a rotation,
all diffuse, with no emitter, one box, and a rotated box plus an ellipsoid.  Against the CPU
oracle: image bytes, f32 radiance bits, ray count, errors == 0.

A rejected light sample cannot be forced by a scene: the candidate direction points at a
point on the emitter's surface, so the ray along it hits the emitter.  The rejection loop
in sample_mix_e is therefore kept the plain one (draw, test, repeat), with nothing in it
that only a rejection would run.
"""
import numpy as np
import pytest

import _shade_scenes as SC
import _util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


ENGINES = {"default": None, "path": "coop=0", "exact": "coop=0,lstack=1", "coop": "coop=100000000"}

_oracle = {}   # variant -> the oracle's (image, radiance, counters): rendered once, read only


@pytest.mark.parametrize("engine", sorted(ENGINES))
@pytest.mark.parametrize("variant", sorted(SC.EMITTERS))
def test_mixed_scene_bit_exact(pt, tmp_path, variant, engine, monkeypatch):
    if ENGINES[engine]:
        monkeypatch.setenv("PT_TUNE", ENGINES[engine])
    path = SC.write_scene(tmp_path, variant)
    if variant not in _oracle:
        _oracle[variant] = U.OracleScene(path).render()
    orgb, orad, octr = _oracle[variant]
    SC.assert_light_reached(orad, octr)
    with pt.Scene.load(path) as s:
        rgb, rad, st = s.render(radiance=True)
    assert st["errors"] == 0
    assert rad.view(np.uint32).tolist() == orad.view(np.uint32).tolist()
    assert np.array_equal(rgb, orgb)
    assert st["rays"] == octr["rays"]
