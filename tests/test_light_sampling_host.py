"""The vertex step's light sampling on the host (no GPU): the selftest integrator is the
device's code compiled for the host (pt_trace.h shade_vertex_e: sample_mix_e's one emitter
test per direction handed on to pdf_mix_e, normal01_vec's two polar loops), so its radiance,
bit-equal to the CPU oracle's, pins them.  Scenes: _shade_scenes.py, with no emitter, one
box, and a rotated box plus an ellipsoid; through the path engine's query and the
cooperative engine's, and through the exact traversal.
"""
import numpy as np
import pytest

import _shade_scenes as SC
import _util as U

pt = U.ptrace()

_oracle = {}   # variant -> the oracle's (image, radiance, counters): rendered once, read only

# how the host integrator finds its closest hits: (traversal, PT_TUNE)
QUERIES = {"path": (0, None), "coop": (0, "qengine=coop"), "exact": (1, None)}


@pytest.mark.parametrize("query", sorted(QUERIES))
@pytest.mark.parametrize("variant", sorted(SC.EMITTERS))
def test_mixed_scene_on_host_bit_exact(tmp_path, variant, query, monkeypatch):
    trav, tune = QUERIES[query]
    if tune:
        monkeypatch.setenv("PT_TUNE", tune)
    path = SC.write_scene(tmp_path, variant)
    if variant not in _oracle:
        _oracle[variant] = U.OracleScene(path).render()
    orgb, orad, octr = _oracle[variant]
    SC.assert_light_reached(orad, octr)
    with pt.Scene.load(path) as s:
        s.prepare()
        got = s.selftest_render_host(0, 0, SC.W, SC.H, traversal=trav)
    assert got.reshape(-1).view(np.uint32).tolist() == orad.reshape(-1).view(np.uint32).tolist()
    assert np.array_equal(U.oracle_tonemap(got).reshape(orgb.shape), orgb)
