"""GPU tests of the batch engines (k_rays, k_feats, k_paths, k_pixels) and the render at the launch
shapes the fixtures never force: the ladder scenes' 22-deep wide aux tree (tests/_ladder.py) takes the
batch workgroups to 128 threads and the cooperative teams of 8 and 16 out of the plan; the mirror box
at RAY_DEPTH 300, 2,000 and 5,000 takes the fold area to its 1 GiB bound, through it (fewer
workgroups, then narrower ones) and past it (PT_E_OOM).

Every scene here has been rendered by the oracle first, at the size and sample count used, in a child
process under a time limit (L.guarded; tests/test_shapes_host.py runs the same guard in the CPU suite).
Expected values are the oracle's, by-hand arithmetic on the shape rules, and -- for the work counters
-- the host execution of the same device code; never the device's own.  All comparisons are exact.
"""
import numpy as np
import pytest

import _features as F
import _filter as FL
import _ladder as L
import _paths as P
import _pixels as X
import _rays as R
import _util as U
from test_paths import _check_buffers as check_path_buffers, _device_buffers as path_buffers, counters
from test_pixels import run_api as pixels_api, run_query as pixels_query
from test_rays import _check_buffer as check_ray_buffer, _device_buffers as ray_buffers, assert_hits, oracle_hits

pytestmark = pytest.mark.gpu
EDGES = [1, 63, 64, 65, 129, 257]   # 129: one lane past a 128-thread workgroup
WINDOW = (0, 0, L.W, L.H)
FOLD_MAX = 2 ** 30


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


@pytest.fixture(scope="module")
def cus(pt):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module", params=["few", "many"])
def lad(request, pt):
    """(emitters, path, prepared scene) of a ladder scene, guarded"""
    path = L.ladder(request.param)
    with pt.Scene.load(path) as s:
        s.prepare()
        L.check_tree(s.info)
        yield request.param, path, s


def assert_block_128(pt, q, cus, fold_depth=None):
    block, max_grid, per_cu = pt.selftest_ctx_shape(q)
    assert block == 128, "the ladder's aux stack should take the workgroup to 128 threads"
    if fold_depth is None:
        assert per_cu == 16 and max_grid == cus * 16   # 2,048 lanes per compute unit
    else:
        assert per_cu >= 1 and max_grid == cus * per_cu   # (RAY_DEPTH 4: far below the fold area's bound)
        assert max_grid * block * fold_depth * 16 <= FOLD_MAX


# ---- 1. RayQuery / Scene.intersect ------------------------------------------------------------------------------
_rays = {}


def ladder_rays(pt, em, path, s):
    """_rays.ray_sets of the scene, the oracle's answers and the host's counters; computed once"""
    if em not in _rays:
        sets = R.ray_sets(s)
        want = [oracle_hits(pt, path, r) for r in sets]
        host = [s.selftest_ray_intersection(r, traversal=0)[2] for r in sets]
        for a in list(sets) + want:
            a.setflags(write=False)
        _rays[em] = (sets, want, host)
    return _rays[em]


def test_intersect_matches_the_oracle_and_the_host_counters(pt, lad, cus):
    em, path, s = lad
    sets, want, host = ladder_rays(pt, em, path, s)
    with pt.RayQuery(s, max_rays=64) as q:
        assert_block_128(pt, q, cus)
    hits = int((want[0]["id"] >= 0).sum())
    print("ladder %s: %d of %d first-set rays hit, host fallbacks (second set) %d" % (em, hits, len(sets[0]), host[1]["fallbacks"]))
    assert hits >= 300 and int((want[1]["id"] == -1).sum()) >= 32 and host[1]["fallbacks"] >= 32
    for rays, w, h in zip(sets, want, host):
        got, st = s.intersect(rays)
        assert_hits(pt, got, w)
        assert st["errors"] == 0 and st["rays"] == len(rays) and st["plane_tests"] == 0
        assert (st["node_visits"], st["prim_tests"], st["aux_visits"], st["fallbacks"]) == \
            (h["nodes"], h["prim_tests"], h["aux"], h["fallbacks"])
    assert st["fallbacks_ray"] == 32   # (the second set's 4 x 8 rays with a non-finite component)


@pytest.mark.parametrize("n", EDGES)
def test_ray_query_wave_edges(pt, lad, cus, n):
    import torch
    em, path, s = lad
    sets, want, _ = ladder_rays(pt, em, path, s)
    # (from the second set's end backwards: its non-finite rays among them)
    rays, w = np.ascontiguousarray(sets[1][::-1]), np.ascontiguousarray(want[1][::-1])
    with pt.RayQuery(s, max_rays=512) as q:
        assert_block_128(pt, q, cus)
        d_rays, d_hits = ray_buffers(torch, rays, n)
        q.run(d_rays, d_hits)
        st = q.stats()
        check_ray_buffer(pt, d_hits, w, n)
    assert st["rays"] == n and st["errors"] == 0


# ---- 2. Scene.features ------------------------------------------------------------------------------------------------
def test_features_match_the_oracle_and_the_host_counters(pt, lad, cus):
    em, path, s = lad
    with pt.FeatureQuery(s, max_points=64) as q:
        assert_block_128(pt, q, cus)
    for xy in (F.centres(path), F.subpixel_set(path)):
        want, _ = F.expected(pt, path, xy)
        host_rec, host = s.selftest_features(xy)
        got, st = s.features(xy)
        F.assert_records(got, want)
        F.assert_records(host_rec, want)
        assert st["errors"] == 0 and st["rays"] == len(xy) and st["plane_tests"] == 0
        assert (st["node_visits"], st["prim_tests"], st["aux_visits"], st["fallbacks"], st["fallbacks_ray"]) == \
            (host["node_visits"], host["prim_tests"], host["aux_visits"], host["fallbacks"], host["fallbacks_ray"])
    assert st["fallbacks_ray"] == F.NONFINITE


# ---- 3. PathQuery / Scene.radiance --------------------------------------------------------------------------------------
def test_radiance_matches_the_oracle_and_the_host_counters(pt, lad, cus):
    em, path, s = lad
    e = L.path_case(pt, path)
    _, host = s.selftest_paths_host(e["records"])
    with pt.PathQuery(s, max_paths=64) as q:
        assert_block_128(pt, q, cus, fold_depth=4)
    got, st = s.radiance(e["records"])
    P.assert_radiance(got, e["rad"])
    assert int(got["rays"].sum()) == e["rays"] and (got["rays"] >= 1).all()
    assert st["errors"] == 0 and st["rays"] == e["rays"] and counters(st) == counters(host)


@pytest.mark.parametrize("n", EDGES)
def test_path_query_wave_edges(pt, lad, cus, n):
    import torch
    em, path, s = lad
    e = L.path_case(pt, path)
    # (from row 4 on, 288 records: towards the image's centre, where the ladder's small rungs are)
    rec, rad = e["records"][L.W * 4:], e["rad"][L.W * 4:]
    assert len(rec) >= n
    host, _ = s.selftest_paths_host(rec[:n])
    with pt.PathQuery(s, max_paths=512) as q:
        assert_block_128(pt, q, cus, fold_depth=4)
        d_in, d_out = path_buffers(torch, rec, n)
        q.run(d_in, d_out, n=n)
        st = q.stats()
        got = check_path_buffers(pt, d_in, d_out, rec, rad, n)
    assert st["rays"] == int(host["rays"].sum()) == int(got["rays"].sum()) and st["errors"] == 0


# ---- 4. PixelQuery / sample_pixels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [pixels_api, pixels_query], ids=["sample_pixels", "PixelQuery"])
def test_pixels_match_the_oracle_and_the_host_twin(pt, lad, cus, run):
    em, path, s = lad
    _, orad, octr = L.guarded(path, WINDOW, 3)
    with pt.PixelQuery(s, max_pixels=64) as q:
        assert_block_128(pt, q, cus, fold_depth=4)
    out, st = run(s, s.pixel_init(X.window_xy(WINDOW)), spp=3)   # (and against selftest_pixels_host: test_pixels.py)
    mean, _ = s.pixel_resolve(out)
    X.assert_bits(mean, orad.reshape(-1, 3), "ladder %s at 3 samples" % em)
    assert st["rays"] == octr["rays"] and st["errors"] == 0 and st["samples"] == 3 * L.W * L.H


@pytest.mark.parametrize("n", [65, 129, 257])
def test_pixels_ragged_counts(pt, lad, n):
    """the first n pixels, pixel k at 1 + k % 4 samples; then each brought to 4"""
    em, path, s = lad
    counts = (1 + np.arange(n) % 4).astype(np.uint32)
    orads = {c: L.guarded(path, WINDOW, c)[1].reshape(-1, 3)[:n] for c in (1, 2, 3, 4)}
    want = np.zeros((n, 3), np.float32)
    for c in orads:
        want[counts == c] = orads[c][counts == c]
    state = s.pixel_init(X.window_xy(WINDOW)[:n])
    mid, st = pixels_query(s, state, counts=counts)
    mean, _ = s.pixel_resolve(mid)
    X.assert_bits(mean, want, "ladder %s at 1 + k %% 4 samples" % em)
    assert np.array_equal(mid["samples"], counts) and st["samples"] == int(counts.sum()) and st["errors"] == 0
    end, st2 = pixels_query(s, mid, counts=(4 - counts).astype(np.uint32))
    mean, _ = s.pixel_resolve(end)
    X.assert_bits(mean, orads[4], "ladder %s brought to 4 samples" % em)
    assert end[counts == 4].tobytes() == mid[counts == 4].tobytes(), "a count of 0 changed its record"


# ---- 5. the render ----------------------------------------------------------------------------------------------------------
RENDERS = {"default": None, "path": "coop=0", "coop_team8": "coop_team=8", "lstack4": "lstack=4", "path_lstack4": "coop=0,lstack=4"}


@pytest.mark.parametrize("engine", sorted(RENDERS))
def test_render_matches_the_oracle(pt, lad, engine, monkeypatch):
    """A window of at most 4,096 pixels runs the cooperative engine from the start: `default`, `coop_team8`
    (teams of 8 asked for, which the plan turns into whole-wave teams: test_shapes_host.py) and `lstack4`
    are cooperative renders, `path` and `path_lstack4` the path engine's -- the last with a 4-word aux
    stack that this tree's queries outgrow, so rays go through the exact hand-over."""
    em, path, s = lad
    orgb, orad, octr = L.guarded(path)
    if RENDERS[engine]:
        monkeypatch.setenv("PT_TUNE", RENDERS[engine])
    rgb, rad, st = s.render(radiance=True)
    assert st["errors"] == 0 and st["short_pixels"] == 0
    assert rad.view(np.uint32).tolist() == orad.view(np.uint32).tolist()
    assert np.array_equal(rgb, orgb)
    assert st["rays"] == octr["rays"]
    if engine.startswith("path"):
        assert st["coop_launches"] == 0
    else:
        assert st["coop_launches"] >= 1
    if engine == "path_lstack4":
        assert st["handoff"]["exact"] > 0, st["handoff"]


# ---- 6. one session pass with per-pixel counts, and the filter on its resolve ---------------------------------------------
def test_session_counts_and_the_filter_on_its_resolve(pt, lad):
    import torch
    em, path, s = lad
    xy = pt.rank_pixels(L.W, L.H, 0, 1)
    counts = np.where((xy[:, 0] + xy[:, 1]) % 2 == 0, 2, 3).astype(np.uint32)
    flat = xy[:, 1].astype(np.int64) * L.W + xy[:, 0]
    want = np.zeros((L.W * L.H, 3), np.float32)
    rays = {}
    for c in (2, 3):
        _, orad, octr = L.guarded(path, WINDOW, c)
        want[flat[counts == c]] = orad.reshape(-1, 3)[flat[counts == c]]
        rays[c] = octr["rays"]
    feat, _ = F.expected(pt, path, F.centres(path))
    ss = pt.Session(s)
    try:
        d_rad = torch.zeros(ss.n_tiles * 256 * 3, dtype=torch.float32, device="cuda")
        ss.trace_counts(counts)
        ss.resolve(None, d_rad.data_ptr())
        ss.sync()
        st = ss.stats()
        rows = pt.unpack_tiles_f32(d_rad.cpu().numpy(), L.W, L.H, 0, 1)
        got_feat = ss.features()
        with pt.FilterQuery(s) as q:
            d_out = torch.full((L.W * L.H * 12 + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
            q.run(d_rad, d_out, layout=pt.FILTER_TILES)
            made = q.stats()
            raw = d_out.cpu().numpy()
    finally:
        ss.close()
    X.assert_bits(rows.reshape(-1, 3), want, "ladder %s, a checkerboard of 2 and 3 samples" % em)
    # (a pixel's rays are its own stream's: between all pixels at 2 samples and all at 3)
    assert st["errors"] == 0 and rays[2] < st["rays"] < rays[3]
    F.assert_records(got_feat, feat[flat])
    assert (raw[L.W * L.H * 12:] == 0xA5).all(), "the filter wrote past its frame"
    filtered, _ = FL.filtered(feat.reshape(L.H, L.W), rows)
    FL.assert_frames(raw[:L.W * L.H * 12].view(np.float32).reshape(L.H, L.W, 3), filtered, "the filter on the session's resolve")
    assert made["errors"] == 0


# ---- 7. deep paths in the batch engines ---------------------------------------------------------------------------------------
def shapes_of(pt, s):
    """((block, max_grid, per_cu) of a PathQuery, of a PixelQuery) on the scene"""
    with pt.PathQuery(s, max_paths=64) as a, pt.PixelQuery(s, max_pixels=64) as b:
        return pt.selftest_ctx_shape(a), pt.selftest_ctx_shape(b)


def test_depth_300_at_the_fold_bound(pt, cus):
    """4,800 B of fold records per resident lane: a full grid of 2^19 lanes would take 2.3 GiB"""
    path = L.mirror_box(300)
    e = L.path_case(pt, path)
    _, orad, octr = L.guarded(path)
    with pt.Scene.load(path) as s:
        for block, max_grid, per_cu in shapes_of(pt, s):
            assert block * max_grid * 300 * 16 <= FOLD_MAX and max_grid >= cus
            if cus * per_cu * block * 4800 > FOLD_MAX:
                assert max_grid == max(cus, FOLD_MAX // (block * 4800))
            else:
                assert max_grid == cus * per_cu
        _, host = s.selftest_paths_host(e["records"])
        got, st = s.radiance(e["records"])
        P.assert_radiance(got, e["rad"])
        assert st["errors"] == 0 and st["rays"] == e["rays"] == int(got["rays"].sum()) and counters(st) == counters(host)
        out, pst = pixels_api(s, s.pixel_init(X.window_xy((0, 0, 8, 8))), spp=2)
        mean, _ = s.pixel_resolve(out)
    X.assert_bits(mean, orad.reshape(-1, 3), "mirror box at depth 300")
    assert pst["rays"] == octr["rays"] > 64 * 2 * 256 and pst["errors"] == 0


@pytest.mark.parametrize("n", [65, 4096])
def test_depth_2000_on_a_folded_shape(pt, cus, n):
    """32,000 B per resident lane.  On 256 CUs: 2^30 / (256 x 32,000) = 131 workgroups < 256, so one per
    compute unit, and 256 x 256 x 32,000 > 2^30 >= 256 x 128 x 32,000: block 128, grid 256."""
    import torch
    path = L.mirror_box(2000)
    e = L.path_case(pt, path)
    assert e["rays"] > 64 * 256   # most paths are longer than 255 vertices
    idx = np.random.default_rng(n).permutation(n) % len(e["records"])
    rec, rad = np.ascontiguousarray(e["records"][idx]), np.ascontiguousarray(e["rad"][idx])
    assert pt.selftest_fold_shape(256, 8, 256, 2000) == (128, 256)
    with pt.Scene.load(path) as s:
        host, _ = s.selftest_paths_host(e["records"])
        for block, max_grid, per_cu in shapes_of(pt, s):
            assert (block, max_grid) == pt.selftest_fold_shape(cus, per_cu, 256, 2000)
            if cus == 256:
                assert (block, max_grid) == (128, 256)
        with pt.PathQuery(s, max_paths=n) as q:
            d_in, d_out = path_buffers(torch, rec, n)
            q.run(d_in, d_out, n=n)
            st = q.stats()
            got = check_path_buffers(pt, d_in, d_out, rec, rad, n)
        if n == 65:
            _, orad, octr = L.guarded(path)
            out, pst = pixels_query(s, s.pixel_init(X.window_xy((0, 0, 8, 8))), spp=2)
            mean, _ = s.pixel_resolve(out)
            X.assert_bits(mean, orad.reshape(-1, 3), "mirror box at depth 2,000")
            assert pst["rays"] == octr["rays"] and pst["errors"] == 0
    assert st["errors"] == 0 and st["rays"] == int(host["rays"][idx].sum()) == int(got["rays"].sum())


def test_depth_5000_is_refused_and_runs_nothing(pt, cus):
    """one wave per compute unit still takes cus x 64 x 5,000 x 16 B: above 2^30 from 210 compute units on"""
    import torch
    assert cus * 64 * 5000 * 16 > FOLD_MAX, "a device of fewer than 210 compute units holds this depth"
    path = L.mirror_box(5000)
    e = L.path_case(pt, path)
    with pt.Scene.load(path) as s:
        s.prepare()
        with pt.RayQuery(s, max_rays=4096) as sibling:
            state = s.pixel_init(X.window_xy((0, 0, 8, 8)))
            for make in (lambda: pt.PathQuery(s, max_paths=64), lambda: pt.PixelQuery(s, max_pixels=64),
                         lambda: s.radiance(e["records"]), lambda: s.sample_pixels(state, spp=1)):
                with pytest.raises(pt.PTError) as err:
                    make()
                assert err.value.code == pt.PT_E_OOM and "RAY_DEPTH too large" in pt.last_error()
            torch.cuda.synchronize()
            quiet = sibling.stats()
            assert quiet["rays"] == 0 and quiet["kernel_ms"] == 0
        # the engines without a fold area still work on it
        first, _ = R.ray_sets(s)
        got, st = s.intersect(first)
        assert_hits(pt, got, oracle_hits(pt, path, first))
        assert st["errors"] == 0 and st["rays"] == len(first)
        xy = F.centres(path)
        feat, fst = s.features(xy)
        F.assert_records(feat, F.expected(pt, path, xy)[0])
        assert fst["errors"] == 0 and fst["rays"] == len(xy)
