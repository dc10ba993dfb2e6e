"""GPU tests of the session-state hand-over (include/pt.h "session states": pt_session_pixels,
pt_session_export / import and their host forms; ptrace.Session.n_pixels / export_states /
import_states): a session's pixels leave as pt_pixel_state records and come back, bit for bit.

Expected values never come from the code under test: the reference's recorded radiance and image
of the fixtures, the CPU oracle at intermediate sample counts (tests/_pixels.py oracle_render), and
the pixel-sample engine's host twin (Scene.selftest_pixels_host) for whole 32-byte records.
Comparisons are on bytes and f32 bits.  tests/test_states_host.py has the record order and the
import's classification without a GPU.
"""
import numpy as np
import pytest

import _pixels as X
import _util as U

pytestmark = pytest.mark.gpu
NAME = "dragon_glass_40x24x7"       # 3 x 2 tiles, the right and bottom ones partial
W, H, S = 40, 24, 7
WINDOW = (5, 3, 30, 18)
GUARD = 64                          # records of 0xA5 behind a device buffer's n records
ENGINES = ["", "coop=0", "coop=100000000", "engine=mega"]

_cache = {}


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


@pytest.fixture()
def scene(pt):
    with pt.Scene.load(X.golden(NAME)[1]) as s:
        s.prepare()
        assert (s.info["width"], s.info["height"], s.info["samples"]) == (W, H, S)
        yield s


def twin(pt, spp, name=NAME, size=(W, H)):
    """the host twin's states of the whole frame after spp samples, in a one-rank export's order"""
    if (name, spp) not in _cache:
        with pt.Scene.load(X.golden(name)[1]) as s:
            init = s.pixel_init(pt.rank_pixels(size[0], size[1], 0, 1))
            out, ctr = (init, {"errors": 0}) if spp == 0 else s.selftest_pixels_host(init, spp=spp)
        assert ctr["errors"] == 0
        out.setflags(write=False)
        _cache[name, spp] = out
    return _cache[name, spp]


def of_pixels(states, xy, width=W):
    """the records of `states` (a whole frame in a one-rank export's order) for the pixels xy"""
    at = np.full(int(states["y"].max() + 1) * width, -1)
    at[states["y"] * width + states["x"]] = np.arange(len(states))
    return states[at[xy[:, 1] * width + xy[:, 0]]]


def finish(pt, ss, size=(W, H), rank=0, world=1):
    """resolve: (image, radiance) of the session's window with its own tiles filled in"""
    import torch
    drad = torch.empty(max(ss.n_tiles, 1) * 256 * 3, dtype=torch.float32, device="cuda")
    ss.resolve(dev_rad=drad.data_ptr())
    ss.sync()
    st = ss.stats()
    assert st["errors"] == 0 and st["short_pixels"] == 0
    rgb = pt.unpack_tiles(ss.read_packed(), size[0], size[1], rank, world)
    rad = pt.unpack_tiles_f32(drad.cpu().numpy(), size[0], size[1], rank, world)
    return rgb, rad, st


def assert_fixture(rgb, rad, name=NAME, window=None):
    _, _, img, want = X.golden(name)
    if window:
        x0, y0, w, h = window
        img, want = img[y0:y0 + h, x0:x0 + w], want[y0:y0 + h, x0:x0 + w]
    X.assert_bits(rad.reshape(-1, 3), want.reshape(-1, 3), name + ": radiance")
    assert np.array_equal(rgb, img)


def assert_mean_is_oracle(pt, s, states, spp):
    mean, _ = s.pixel_resolve(states)
    orad = X.oracle_render(X.golden(NAME)[1], (0, 0, W, H), spp)[1]
    X.assert_bits(mean, orad[states["y"] * W + states["x"]], "the exported states' mean at %d samples" % spp)


def device_records(states, extra=GUARD):
    import torch
    d = torch.full(((len(states) + extra) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
    if len(states):
        d[:len(states) * 32] = torch.from_numpy(np.array(states).view(np.uint8)).cuda()
    torch.cuda.synchronize()
    return d


def read_records(pt, d, n):
    raw = d.cpu().numpy()
    assert (raw[n * 32:] == 0xA5).all(), "the call wrote past its n records"
    return raw[:n * 32].view(pt.PIXEL_DTYPE).copy()


# ---- 1. fresh ---------------------------------------------------------------------------------------
def test_a_new_sessions_export_is_pixel_init(pt, scene):
    ss = pt.Session(scene)
    assert ss.n_pixels == 960 == W * H
    got = ss.export_states()
    want = scene.pixel_init(pt.rank_pixels(W, H, 0, 1))
    assert got.dtype == pt.PIXEL_DTYPE and got.tobytes() == want.tobytes() == twin(pt, 0).tobytes()
    assert ss.stats()["samples"] == 0
    ss.close()


def test_a_session_without_pixels_exports_none_and_takes_none(pt, scene):
    ss = pt.Session(scene, rank=1, world=2, window=(0, 0, 16, 16))
    assert ss.n_pixels == 0 and len(ss.export_states()) == 0
    assert ss.import_states(np.array(twin(pt, 3))) == 0
    assert ss.import_states(device_records(twin(pt, 3)), n=960) == 0
    ss.close()


# ---- 2. export --------------------------------------------------------------------------------------
def test_export_after_3_and_after_7_samples(pt, scene):
    ss = pt.Session(scene)
    ss.trace(3)
    at3 = ss.export_states()
    assert at3.tobytes() == twin(pt, 3).tobytes(), "the session's states at 3 samples differ from the host twin's"
    assert_mean_is_oracle(pt, scene, at3, 3)
    # the condition without which the case does not show that the saved value travels (as
    # tests/test_pixels_host.py has it for this frame's 3 | 4 split)
    saved = (at3["rng"] & X.SAVED_BIT) != 0
    assert saved.sum() * 10 >= len(saved) and (~saved).sum() * 10 >= len(saved)
    assert (at3["saved"][saved] != 0).all() and not at3["saved"][~saved].view(np.uint32).any()
    assert ss.stats()["samples"] == 960 * 3
    ss.trace(4)
    d = device_records(np.zeros(0, pt.PIXEL_DTYPE), extra=960 + GUARD)
    assert ss.export_states(dev=d) is d
    at7 = read_records(pt, d, 960)
    assert at7.tobytes() == twin(pt, 7).tobytes()
    mean, rgb = scene.pixel_resolve(at7)
    _, _, img, rad = X.golden(NAME)
    X.assert_bits(mean, rad[at7["y"], at7["x"]], "the exported states' mean at 7 samples")
    assert np.array_equal(rgb, img[at7["y"], at7["x"]])
    assert_fixture(*finish(pt, ss)[:2])
    ss.close()


# ---- 3. round trip ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tune,reverse", [(t, False) for t in ENGINES] + [("", True)])
def test_round_trip_through_a_second_session(pt, scene, tune, reverse, monkeypatch):
    if tune:
        monkeypatch.setenv("PT_TUNE", tune)   # read at session creation
    else:
        monkeypatch.delenv("PT_TUNE", raising=False)
    a = pt.Session(scene)
    a.trace(3)
    states = a.export_states()
    a.close()
    assert states.tobytes() == twin(pt, 3).tobytes()
    b = pt.Session(scene)
    assert b.import_states(states[::-1] if reverse else states) == 960
    assert b.stats()["samples"] == 960 * 3
    b.trace(4)
    rgb, rad, st = finish(pt, b)
    assert_fixture(rgb, rad)
    assert st["samples"] == 960 * 7 and st["short_pixels"] == 0 and st["errors"] == 0
    if tune == "engine=mega":
        assert st["rounds"] == 0   # (the megakernel ran, as tests/test_gpu.py knows it)
    assert b.export_states().tobytes() == twin(pt, 7).tobytes()
    b.close()


# ---- 4. across engines ------------------------------------------------------------------------------
def test_pixel_query_states_go_on_in_a_session(pt, scene):
    d = device_records(twin(pt, 0))
    with pt.PixelQuery(scene, max_pixels=960) as q:
        q.run(d, spp=3, n=960)
        assert q.stats()["errors"] == 0
    ss = pt.Session(scene)
    assert ss.import_states(d, n=960) == 960
    assert read_records(pt, d, 960).tobytes() == twin(pt, 3).tobytes()   # (an import leaves the records alone)
    ss.trace(4)
    assert_fixture(*finish(pt, ss)[:2])
    ss.close()


def test_session_states_go_on_in_a_pixel_query(pt, scene):
    ss = pt.Session(scene)
    ss.trace(3)
    d = device_records(np.zeros(0, pt.PIXEL_DTYPE), extra=960 + GUARD)
    ss.export_states(dev=d)
    ss.close()
    with pt.PixelQuery(scene, max_pixels=960) as q:
        q.run(d, spp=4, n=960)
        st = q.stats()
    out = read_records(pt, d, 960)
    assert st["errors"] == 0 and st["samples"] == 960 * 4
    assert out.tobytes() == twin(pt, 7).tobytes()
    mean, rgb = scene.pixel_resolve(out)
    _, _, img, rad = X.golden(NAME)
    X.assert_bits(mean, rad[out["y"], out["x"]], "a session's 3 samples and a pixel query's 4")
    assert np.array_equal(rgb, img[out["y"], out["x"]])


# ---- 5. re-shard ------------------------------------------------------------------------------------
def test_three_ranks_go_on_as_two(pt):
    name = X.DRAGON
    with pt.Scene.load(X.golden(name)[1]) as s:
        s.prepare()
        assert (s.info["width"], s.info["height"], s.info["samples"]) == (64, 64, 8)
        parts = []
        for r in range(3):
            ss = pt.Session(s, rank=r, world=3)
            ss.trace(3)
            parts.append(ss.export_states())
            assert np.array_equal(np.stack([parts[-1]["x"], parts[-1]["y"]], axis=1), pt.rank_pixels(64, 64, r, 3))
            ss.close()
        states = np.concatenate(parts)
        assert len(states) == 4096
        rgb, rad, taken = np.zeros((64, 64, 3), np.uint8), np.zeros((64, 64, 3), np.float32), []
        for r in range(2):
            ss = pt.Session(s, rank=r, world=2)
            taken.append(ss.import_states(states))
            assert taken[-1] == ss.n_pixels
            ss.trace(5)
            part_rgb, part_rad, _ = finish(pt, ss, (64, 64), r, 2)
            mine = np.zeros((4, 4), bool)
            mine.reshape(-1)[pt.rank_tiles(64, 64, r, 2)] = True
            mine = np.repeat(np.repeat(mine, 16, 0), 16, 1)
            rgb[mine], rad[mine] = part_rgb[mine], part_rad[mine]
            ss.close()
    assert sum(taken) == 4096 and taken == [2048, 2048]
    assert_fixture(rgb, rad, name)


# ---- 6. window --------------------------------------------------------------------------------------
def test_a_windows_states(pt, scene):
    x0, y0, w, h = WINDOW
    a = pt.Session(scene, window=WINDOW)
    assert a.n_pixels == 540
    a.trace(3)
    states = a.export_states()
    a.close()
    xy = pt.rank_pixels(w, h, 0, 1, x0, y0)
    assert len(states) == 540 and np.array_equal(np.stack([states["x"], states["y"]], axis=1), xy)
    assert states.tobytes() == of_pixels(twin(pt, 3), xy).tobytes()
    b = pt.Session(scene, window=WINDOW)
    assert b.import_states(states) == 540
    b.trace(4)
    rgb, rad, _ = finish(pt, b, (w, h))
    assert_fixture(rgb, rad, window=WINDOW)
    b.close()
    full = pt.Session(scene)
    with pytest.raises(pt.PTError) as e:
        full.import_states(states)
    assert e.value.code == pt.PT_E_INVALID
    assert full.export_states().tobytes() == twin(pt, 0).tobytes()
    # ... and the window takes its 540 of the whole frame's 960
    c = pt.Session(scene, window=WINDOW)
    assert c.import_states(np.array(twin(pt, 3))) == 540
    assert c.export_states().tobytes() == states.tobytes()
    c.close()
    full.close()


# ---- 7. seeds ---------------------------------------------------------------------------------------
def test_a_session_from_the_callers_seeds(pt, scene):
    xy = pt.rank_pixels(W, H, 0, 1)
    seeds = np.random.default_rng(41).integers(0, 2 ** 32, len(xy), dtype=np.uint64).astype(np.uint32)
    seeds[:3] = (0, X.M31, 2 ** 32 - 1)
    init = scene.pixel_init(xy, seeds=seeds)
    assert (init["rng"] != twin(pt, 0)["rng"]).sum() > 900
    want, ctr = scene.selftest_pixels_host(init, spp=5)
    assert ctr["errors"] == 0
    ss = pt.Session(scene)
    assert ss.import_states(init) == 960
    assert ss.export_states().tobytes() == init.tobytes()
    ss.trace(5)
    assert ss.export_states().tobytes() == want.tobytes()
    finish(pt, ss)   # (the resolve's own check: every pixel at 5 samples)
    ss.close()


# ---- 8. refusals ------------------------------------------------------------------------------------
def test_refused_imports_and_exports_leave_the_session_alone(pt, scene):
    good = np.array(twin(pt, 3))
    k = 333   # a record in the middle of a tile
    ss = pt.Session(scene)
    ss.trace(2)   # (so that a slot written by a refused import would show)
    before = ss.export_states()
    assert before.tobytes() == twin(pt, 2).tobytes()

    def variant(**fields):
        v = good.copy()
        for name, value in fields.items():
            v[name][k] = value
        return v

    cases = {
        "one owned pixel missing": np.delete(good, k),
        "one given twice": np.concatenate([good, good[k:k + 1]]),
        "one record's samples off by one": variant(samples=4),
        "x = W": variant(x=W),
        "y = H": variant(y=H),
        "rng low bits 0": variant(rng=good["rng"][k] & X.SAVED_BIT),
        "rng low bits 2^31 - 1": variant(rng=X.M31),
        "no record": good[:0],
    }
    for what, states in cases.items():
        for form in ("host", "device"):
            with pytest.raises(pt.PTError) as e:
                ss.import_states(states if form == "host" else device_records(states), n=len(states))
            assert e.value.code == pt.PT_E_INVALID, what
            assert ss.export_states().tobytes() == before.tobytes(), "%s (%s): the session changed" % (what, form)
    d = device_records(good)
    for off in (8, 4):
        with pytest.raises(pt.PTError) as e:
            ss.import_states(d.data_ptr() + off, n=960)
        assert e.value.code == pt.PT_E_INVALID and "aligned" in str(e.value)
    # export: too little room, a misaligned pointer -- nothing written
    out = device_records(good[:0], extra=960 + GUARD)
    assert pt._lib.pt_session_export(ss._h, out.data_ptr(), 959) == pt.PT_E_INVALID
    assert pt._lib.pt_session_export(ss._h, out.data_ptr() + 8, 960) == pt.PT_E_INVALID
    host = np.full(960 * 32, 0xA5, np.uint8)
    assert pt._lib.pt_session_export_host(ss._h, U._p(host), 959) == pt.PT_E_INVALID
    assert (out.cpu().numpy() == 0xA5).all() and (host == 0xA5).all()
    assert ss.export_states().tobytes() == before.tobytes()
    assert ss.stats()["samples"] == 960 * 2
    # a valid import into the same session still works
    assert ss.import_states(good) == 960
    ss.trace(4)
    rgb, rad, st = finish(pt, ss)
    assert_fixture(rgb, rad)
    assert st["samples"] == 960 * 7
    ss.close()


# ---- 9. pending work --------------------------------------------------------------------------------
def test_a_trace_not_yet_run_runs_before_the_hand_over(pt, scene):
    a = pt.Session(scene)
    a.trace(3)   # (the wavefront engine runs it at the next sync point: the export is one)
    assert a.export_states().tobytes() == twin(pt, 3).tobytes()
    a.close()
    b = pt.Session(scene)
    b.trace(2)
    assert b.import_states(np.array(twin(pt, 3))) == 960
    b.trace(4)
    rgb, rad, st = finish(pt, b)
    assert_fixture(rgb, rad)
    assert st["samples"] == 960 * 7
    b.close()
