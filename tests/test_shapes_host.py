"""CPU tests of the launch shapes that deep aux trees and deep paths force (qctx.cpp lane_words,
fit_block, rays_shape; wave_plan.cpp plan_wave), and the guard of the scenes that
tests/test_shapes.py takes to a GPU: every such scene is rendered here first, by the oracle, in a
child process under a time limit (tests/_ladder.py).

Expected figures are by-hand arithmetic on the rules, the scene's own tree facts, or the CPU oracle;
none comes from the device code.  All comparisons are exact.
"""
import numpy as np
import pytest

import _features as F
import _ladder as L
import _paths as P
import _pixels as X
import _util as U

pt = U.ptrace()
CUS = 256
LADDERS = ("few", "many")


# ---- 1. fit_block by hand ----------------------------------------------------------------------------
@pytest.mark.parametrize("words,block", [(63, 256), (64, 128), (127, 128), (128, 64), (255, 64), (256, None)])
def test_fit_block_by_hand(words, block):
    """lane_lds_bytes(block, aux, dfs) = (block / 64) x 64 lanes x 4 B x (max(aux, dfs) + 1) words, at most
    65,536 B:
      max 63:  256 x 4 x 64  = 65,536           fits 256
      max 64:  256 x 4 x 65  = 66,560 > 65,536;  128 x 4 x 65  = 33,280   fits 128
      max 127: 128 x 4 x 128 = 65,536           fits 128
      max 128: 128 x 4 x 129 = 66,048 > 65,536;  64 x 4 x 129  = 33,024   fits 64
      max 255: 64 x 4 x 256  = 65,536           fits 64
      max 256: 64 x 4 x 257  = 65,792 > 65,536  does not fit
    PathQuery / PixelQuery (block_both) take the larger of the two stacks, whichever it is.  RayQuery /
    FeatureQuery (block_aux_only) size k_rays' workgroup by the aux stack alone, and hold the exact
    kernel's one wave, 64 x 4 x (dfs + 1) B, to the same 64 KiB: 255 DFS words fit, 256 are refused."""
    for aux, dfs in ((words, 1), (1, words), (words, words)):
        r = pt.selftest_fit_block(aux, dfs)
        assert r["fits_both"] == (block is not None)
        assert r["block_both"] == (block or 64)
    # the aux stack alone
    r = pt.selftest_fit_block(words, 0)
    assert r["fits_aux_only"] == (block is not None) and r["block_aux_only"] == (block or 64)
    # the exact kernel's wave: the DFS stack never narrows k_rays' workgroup, and is refused beyond 255 words
    r = pt.selftest_fit_block(1, words)
    assert r["block_aux_only"] == 256 and r["fits_aux_only"] == (words <= 255)


def test_rays_refusal_is_the_other_engines_message():
    pt.selftest_fit_block(1, 256)
    assert "a lane's traversal stacks do not fit the LDS" in pt.last_error()


# ---- 2. the ladder scenes: guard, tree facts, lane shape -------------------------------------------------
@pytest.fixture(scope="module", params=LADDERS)
def ladder(request):
    """(emitters, path, prepared scene): the guard has rendered the scene by then"""
    path = L.ladder(request.param)
    with pt.Scene.load(path) as s:
        s.prepare()
        yield request.param, path, s


def test_ladder_emitters():
    assert L.n_emitters("few") == 8 == L.QC_NEM and L.n_emitters("many") > L.QC_NEM
    for em in LADDERS:
        assert all(L.in_band(k) for k in range(L.N_PRIMS) if L.emissive(em, k))


def test_ladder_tree_and_lane_shape(ladder):
    em, path, s = ladder
    info = L.check_tree(s.info)
    assert info["n_emitters"] == L.n_emitters(em) and info["n_prims"] == L.N_PRIMS and info["n_planes"] == 0
    r = pt.selftest_lane_shape(s)
    stack = s.wave_plan(CUS)["aux_stack_words"]
    print("ladder %s: aux_depth %d, auxw_stack %d, max_stack %d, %d aux nodes" %
          (em, info["aux_depth"], stack, info["max_stack"], info["n_aux_nodes"]))
    # a depth-first descent of the 4-wide aux tree keeps 3 siblings per level, and the node in hand
    assert stack == 3 * info["aux_depth"] + 1
    assert r["aux_words"] == min(3 * info["aux_depth"] + 1, L.PT_QUERY_SP_MAX) >= 64
    assert r["dfs_words"] == info["max_stack"] < 64
    assert r["block_both"] == r["block_aux_only"] == 128 and r["fits_both"] and r["fits_aux_only"]


# ---- 3. plan_wave on 256 CUs, by hand ----------------------------------------------------------------------
def _invariant(p):
    assert p["carry_cap"] <= p["n_slots"]
    assert p["carry_cap"] >= min(p["n_slots"], p["lane_cap"])
    return p


def carry_query_words():
    """sizeof(Query) / 4, from the committed fixtures' plans: carry_words = (Q + 1 + stack + 3) & ~3 holds
    for each of them (pt_kernels.h carry_record_words); the values of Q that fit them all"""
    ok = set(range(1, 256))
    for name in ("standin_48x32x4", "dragon_64x64x16", "hw3s6_48x48x8", "mat_matrix_24x24x8", "rabbid_48x48x4"):
        with pt.Scene.load(U.golden_scene_path(name)) as s:
            p = s.wave_plan(CUS)
        ok &= {q for q in ok if (q + 1 + p["aux_stack_words"] + 3) & ~3 == p["carry_words"]}
    assert ok
    return ok


def test_ladder_plan_by_hand(ladder, monkeypatch):
    """aux_depth d >= 21: coop_reserve = 3 (d + 2) >= 69, so a team's expansion needs reserve + 64 >= 133
    words.  Teams of 8 and 16 have qc_stack_words = 128: refused.  Teams of 4 expand into their wave's
    pool, 16 chains x 64 = 1,024 words: admitted (max_stack <= 64).  Teams of 32 have 192, whole-wave
    teams 448: admitted while reserve + 64 <= 192, i.e. d <= 40."""
    em, path, s = ladder
    info = s.info
    reserve = 3 * (info["aux_depth"] + 2)
    assert 128 < reserve + 64 <= 192 and info["max_stack"] <= 64
    p = _invariant(s.wave_plan(CUS))
    assert p["coop_reserve"] == reserve and p["coop_max"] == CUS * 192 and p["coop_team"] == 4
    # 24 x 16 pixels in 16 x 16 tiles: 2 tiles (the second half empty), 512 slots -- fewer than the query lanes
    assert (L.W, L.H) == (24, 16) and p["n_tiles_local"] == 2 and p["n_slots"] == 512 and p["lane_cap"] == 512
    assert {p["carry_words"]} == {(q + 1 + p["aux_stack_words"] + 3) & ~3 for q in carry_query_words()}
    if em == "few":
        # teams of 4 in the early launch: 256 CUs x 1 workgroup x 4 waves x 16 chains
        assert (p["big"], p["side_team"], p["early_k"]) == (0, 4, 16384)
    else:
        # more emitters than the LDS table: the BIG instantiation has teams of 8 only, which this tree
        # is refused -- whole-wave teams, and no early launch beside them
        assert (p["big"], p["side_team"], p["early_k"]) == (1, 64, 0)
        assert p["carry_cap"] == p["lane_cap"]
    for team in (8, 16):
        monkeypatch.setenv("PT_TUNE", "coop_team=%d" % team)
        q = _invariant(s.wave_plan(CUS))
        assert (q["coop_team"], q["early_k"], q["coop_reserve"]) == (64, 0, reserve)
    monkeypatch.setenv("PT_TUNE", "coop_team=32,coop_grow_mid=100")
    q = _invariant(s.wave_plan(CUS))
    assert (q["coop_team"], q["coop_grow_mid"], q["early_k"]) == (32, 100, 0)


# ---- 4. the oracle against the host execution of the device code -----------------------------------------------
def test_ladder_render_host_matches_the_oracle(ladder):
    em, path, s = ladder
    _, orad, _ = L.guarded(path)
    assert (orad != 0).any(axis=2).sum() * 2 >= L.W * L.H
    got = s.selftest_render_host(0, 0, L.W, L.H)
    assert got.view(np.uint32).tolist() == orad.view(np.uint32).tolist()


def test_ladder_paths_host_matches_the_oracle(ladder):
    em, path, s = ladder
    e = L.path_case(pt, path)
    assert e["nonzero"] * 2 >= len(e["records"]), "fewer than half of the oracle's pixels are non-zero"
    got, ctr = s.selftest_paths_host(e["records"])
    P.assert_radiance(got, e["rad"])
    assert int(got["rays"].sum()) == e["rays"] == ctr["rays"] and ctr["errors"] == 0


@pytest.mark.parametrize("spp", [2, 3, 4])   # (with path_case's 1: every count test_shapes.py uses)
def test_ladder_pixels_host_matches_the_oracle(ladder, spp):
    em, path, s = ladder
    window = (0, 0, L.W, L.H)
    _, orad, octr = L.guarded(path, window, spp)
    out, st = s.selftest_pixels_host(s.pixel_init(X.window_xy(window)), spp=spp)
    mean, _ = s.pixel_resolve(out)
    X.assert_bits(mean, orad.reshape(-1, 3), "ladder %s at %d samples" % (em, spp))
    assert st["rays"] == octr["rays"] and st["errors"] == 0


def test_ladder_features_host_matches_the_oracle(ladder):
    em, path, s = ladder
    xy = F.centres(path)
    want, _ = F.expected(pt, path, xy)
    hit = want["id"] >= 0
    assert hit.sum() * 2 >= len(want) and len(np.unique(want["id"][hit])) >= 8
    got, ctr = s.selftest_features(xy)
    F.assert_records(got, want)
    assert ctr["rays"] == len(xy) and ctr["errors"] == 0


# ---- 5. the stall, pinned down ---------------------------------------------------------------------------------
def test_extreme_scale_emitters_are_what_stalls_and_the_guard_catches_it():
    """INTEGRATION.md "Known stall": with EMISSION on primitives of every scale the oracle -- as the
    untouched reference -- never finishes pixel (0, 0) of the 24 x 16 frame: the rejection loop of the
    box light sampler (pt_oracle.cpp sample_box; pt_core.h sample_mix_e) draws directions towards a
    box of half-size 4e-7 from 200 units away, where one ulp of the unit direction is 30 times the
    box.  The guard turns that into a failure within its limit (2 s here); the same rows without the
    pixel still render, and the host execution agrees with the oracle on them."""
    path = L.ladder("stall")
    with pytest.raises(AssertionError, match="must not reach a GPU"):
        L.guarded(path, (0, 0, 1, 1), 2, seconds=2)
    _, orad, _ = L.guarded(path, (1, 0, 7, 1), 2)
    with pt.Scene.load(path) as s:
        got = s.selftest_render_host(1, 0, 7, 1, spp=2)
    assert got.view(np.uint32).tolist() == orad.view(np.uint32).tolist()


# ---- 6. the mirror boxes of the deep-path GPU tests -------------------------------------------------------------
@pytest.mark.parametrize("depth", [300, 2000, 5000])
def test_mirror_box_guard_and_host_paths(depth):
    path = L.mirror_box(depth)
    _, _, octr = L.guarded(path)
    assert octr["rays"] > 64 * 2 * 256   # most paths are longer than 255 vertices
    e = L.path_case(pt, path)
    print("mirror box at depth %d: %d of %d one-sample pixels non-zero, %d rays" % (depth, e["nonzero"], len(e["records"]), e["rays"]))
    assert e["nonzero"] >= 8   # (a path cut at RAY_DEPTH returns 0: only those that reach the lamp carry light)
    with pt.Scene.load(path) as s:
        got, ctr = s.selftest_paths_host(e["records"])
        info = s.info
    P.assert_radiance(got, e["rad"])
    assert int(got["rays"].sum()) == e["rays"] and ctr["errors"] == 0
    assert info["ray_depth"] == depth and info["aux_depth"] < 21   # (the default workgroup: the depth alone shapes it)
