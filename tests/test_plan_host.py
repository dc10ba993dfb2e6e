"""CPU tests of session set-up without a device (pt_selftest_wave_plan): the session's
geometry, the wavefront pass's plan (wave_plan.cpp plan_wave) and the arena's size, on a
device of 256 compute units.

Every expected figure is derived by hand from plan_wave's rules, with these constants of
pt_kernels.h: PT_NQ_BASE = PT_NQ_FULL = 2, path_wg_per_cu(nq) = 3 waves x 4 SIMDs / (nq + 1)
= 4 (nq 2) or 3 (nq 3), QC_WAVES = 4, QC_FOLD = 6, the step mixes' defaults {3, 32, 1, 64}
and end_min 48 in the low rounds.
"""
import pytest

import _util as U

pt = U.ptrace()
CUS = 256


@pytest.fixture(scope="module")
def c3():
    with pt.Scene.load(U.scene_path("c3")) as s:
        yield s.prepare()


def _invariant(p):
    """the carry queue holds what a round can append, and never more than the pixels"""
    assert p["carry_cap"] <= p["n_slots"]
    assert p["carry_cap"] >= min(p["n_slots"], p["lane_cap"])
    return p


def test_plan_config3_full_frame(c3):
    """1920x1080: 120 x 68 = 8,160 tiles, 2,088,960 slots.
    path_grid = full_grid = 256 x 4; shade_grid = min(256 x 8, 8,160); ticks = 2,500 us and
    5,000 us x 100; query lanes = 1,024 x 2 x 64 = 131,072 = lane_cap (fewer than the pixels);
    coop_max = 256 x 192; path_sparse = min(1,024 x 2 x 32 = 65,536, coop_max); with the
    cooperative engine path_runend = 0 and not automatic; coop_grow = 256 x 16; early_at = lowq
    = 256 x 768; the scene is admitted to teams of 4, so early_k = 256 x 1 x 4 waves x 16 chains
    = 16,384 and carry_cap = 131,072 + 16,384; low_grid = min(1,024, 256 x 2)."""
    p = _invariant(c3.wave_plan(CUS))
    want = dict(
        n_tiles_local=8160, n_slots=2088960, path_grid=1024, full_nq=2, full_grid=1024, shade_grid=2048,
        path_budget=1024, path_ticks=250000, low_ticks=500000, lane_cap=131072, coop_max=49152, coop_grid=2048,
        path_sparse=49152, path_runend=0, runend_auto=0, sparse_steps=8, round_batch=1, coop_team=4, side_team=4,
        coop_grow=4096, coop_grow_mid=0, early_wg=1, early_at=196608, early_k=16384, carry_cap=147456,
        lowq=196608, low_grid=512, mix=(3, 32, 1, 64), mix_low=(3, 32, 1, 48), coop_order=1, big=0)
    assert {k: p[k] for k in want} == want
    # the aux tree's facts are the build's: relations, not figures.  A descent keeps at most 3
    # entries per level; a carry record (16-B units) holds a query, its slot and the scene's
    # aux stack words.
    assert p["coop_reserve"] == 3 * (c3.info["aux_depth"] + 2)
    assert p["aux_stack_words"] >= 1
    assert p["carry_words"] % 4 == 0 and p["carry_words"] >= 2 + p["aux_stack_words"]
    # the allocation's size, as the set-up before plan_wave printed it ahead of its hipMalloc on
    # a 256-CU device for this md5-pinned scene (profiles/r12_plan): it fixes every section's
    # size, carry_words among them
    assert p["arena_bytes"] == 771140864


def test_plan_config3_rank0_of_8(c3):
    """120 tiles per row deal 15 to each of 8 ranks in every one of 68 rows: 1,020 tiles,
    261,120 slots; shade_grid = min(2,048, 1,020); the query lanes are still fewer than the
    pixels, so lane_cap and carry_cap are the full frame's."""
    p = _invariant(c3.wave_plan(CUS, rank=0, world=8))
    want = dict(n_tiles_local=1020, n_slots=261120, shade_grid=1020, lane_cap=131072, carry_cap=147456)
    assert {k: p[k] for k in want} == want
    assert p["arena_bytes"] == 209936896   # (recorded as the full frame's: profiles/r12_plan)


def test_plan_small_image_caps_at_the_pixels():
    """64x64: 16 tiles, 4,096 slots -- fewer than the query lanes, so lane_cap = carry_cap =
    4,096 (neither ever exceeds the pixels); shade_grid = min(2,048, 16)."""
    with pt.Scene.load(U.golden_scene_path("dragon_metal_64x64x8")) as s:
        p = _invariant(s.wave_plan(CUS))
    assert (p["n_slots"], p["lane_cap"], p["carry_cap"], p["shade_grid"]) == (4096, 4096, 4096, 16)


@pytest.mark.parametrize("name", ["dragon_d10_metal_48x48x16", "dragon_d10_glass_48x48x16"])
def test_plan_deep_paths_run_the_big_instantiation(name):
    """RAY_DEPTH 10 > QC_FOLD: the BIG instantiation, which has teams of 8 only, so the early
    launch holds 256 x 1 x 4 waves x 8 chains = 8,192."""
    m = U.manifest()["deep"][name]
    with pt.Scene.load(U.scene_path(m["scene"], tuple(m["gen"]))) as s:
        p = _invariant(s.wave_plan(CUS))
    assert (p["big"], p["side_team"], p["early_k"]) == (1, 8, 8192)


TUNE = {
    # 3 workgroups of 3 query waves per CU: 768 x 3 x 64 = 147,456 lanes (more than 1,024 x 2 x 64)
    "nq=3": dict(full_nq=3, full_grid=768, lane_cap=147456, carry_cap=163840),
    # no cooperative engine: no early launch, the rounds' run-to-end stays automatic, the
    # sparse threshold is not capped by the hand-over
    "coop=0": dict(early_k=0, runend_auto=1, path_sparse=65536),
    # whole-wave teams in the early launch: there is none
    "side_team=64": dict(early_k=0, carry_cap=131072),
    # not a team size: whole-wave teams, and no early launch beside them
    "coop_team=5": dict(coop_team=64, early_k=0),
    # an explicit trip budget alone: no deadlines
    "budget=5": dict(path_budget=5, path_ticks=0, low_ticks=0),
    "early_wg=2": dict(early_k=32768),
    # 8 x 256 workgroups asked for: clamped to path_grid
    "lowq_wg=8": dict(low_grid=1024),
}


@pytest.mark.parametrize("tune", sorted(TUNE))
def test_plan_follows_pt_tune(c3, tune, monkeypatch):
    monkeypatch.setenv("PT_TUNE", tune)
    p = _invariant(c3.wave_plan(CUS))
    assert {k: p[k] for k in TUNE[tune]} == TUNE[tune]


def test_plan_refuses_nq_4(c3, monkeypatch):
    monkeypatch.setenv("PT_TUNE", "nq=4")
    with pytest.raises(pt.PTError) as e:
        c3.wave_plan(CUS)
    assert e.value.code == pt.PT_E_INVALID and "nq" in str(e.value)


def test_plan_argument_errors_need_no_device(c3):
    """the geometry's errors keep their codes and messages"""
    for kw, msg in ((dict(rank=2, world=2), "bad rank/world"), (dict(window=(1900, 0, 64, 16)), "window outside")):
        with pytest.raises(pt.PTError) as e:
            c3.wave_plan(CUS, **kw)
        assert e.value.code == pt.PT_E_INVALID and msg in str(e.value)
