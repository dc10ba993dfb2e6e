"""Shared pieces of tests/test_refine_host.py and tests/test_refine.py: a numpy float32 restatement of
a session's noise estimate and of the step planned from it (include/pt.h "session noise"), written from
the definition and independent of the library's code -- every operation on float32 arrays, so every
result rounded to f32, in the stated order --, and the tests' two inputs.
"""
import numpy as np

import _pixels as X

FLOOR = np.float32(2.0 ** -10)
INF = np.float32(np.inf)
U32_MAX = 0xffffffff
FIELDS = ("refined", "samples", "unmarked", "nonfinite", "capped", "worst", "least", "most")
# (golden frame, window): 40 x 24 pixels each, 3 x 2 tiles with the right and bottom ones partial
INPUTS = {"frame": ("dragon_glass_40x24x7", None), "window": ("dragon_glass_64x64x8", (8, 8, 40, 24))}
W, H = 40, 24


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def noise_of(now, mark):
    """(noise, has an estimate) of every record: now / mark are arrays of PIXEL_DTYPE, a mark with
    samples == 0 is no mark"""
    k, a = now["samples"], mark["samples"]
    est = (a != 0) & (k > a)
    with np.errstate(all="ignore"):
        inv_k = np.float32(1) / np.where(est, k, 1).astype(np.float32)
        inv_a = np.float32(1) / np.where(est, a, 1).astype(np.float32)
        m = [inv_k * now["sum"][:, c] for c in range(3)]
        p = [inv_a * mark["sum"][:, c] for c in range(3)]
        d = (np.abs(m[0] - p[0]) + np.abs(m[1] - p[1])) + np.abs(m[2] - p[2])
        l = (m[0] + m[1]) + m[2]
        lf = np.where(l > FLOOR, l, FLOOR)
        noise = d / np.sqrt(lf)
    for v in (d, l, lf, noise):
        assert v.dtype == np.float32
    return np.where(est, noise, INF).astype(np.float32), est


def spread_in_tiles(hot, x, y, origin=(0, 0), tile_rule=True):
    """hot or a hot neighbour (of 8) among the given pixels that lies in the same 16 x 16 tile of the
    window at `origin`; tile_rule=False: any hot neighbour (what a border mistake would compute)"""
    wx, wy = x.astype(np.int64) - origin[0], y.astype(np.int64) - origin[1]
    w, h = int(wx.max()) + 1, int(wy.max()) + 1
    grid = np.zeros((h + 2, w + 2), bool)
    grid[wy + 1, wx + 1] = hot
    out = np.zeros(len(hot), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            nx, ny = wx + dx, wy + dy
            same = ((nx >> 4) == (wx >> 4)) & ((ny >> 4) == (wy >> 4)) if tile_rule else True
            out |= grid[ny + 1, nx + 1] & same
    return out


def plan_of(now, mark, threshold, step, max_samples=0, spread=0, origin=(0, 0), tile_rule=True):
    """(noise, counts, result dict, hot after the spread) of a plan over the records"""
    noise, est = noise_of(now, mark)
    k = now["samples"].astype(np.int64)
    cap = max_samples if max_samples else U32_MAX
    hot = noise > np.float32(threshold)
    nan = np.isnan(noise)
    hot2 = spread_in_tiles(hot, now["x"], now["y"], origin, tile_rule) if spread else hot
    go = ~nan & hot2 & (k < cap)
    counts = np.where(go, np.minimum(step, cap - k), 0).astype(np.uint32)
    known = noise[est & np.isfinite(noise)]
    res = {"refined": int((counts > 0).sum()), "samples": int(counts.sum(dtype=np.uint64)),
           "unmarked": int((~est).sum()), "nonfinite": int(nan.sum()), "capped": int((hot2 & ~nan & (k >= cap)).sum()),
           "worst": float(known.max()) if len(known) else 0.0,
           "least": int(k.min()) if len(k) else 0, "most": int(k.max()) if len(k) else 0}
    return noise, counts, res, hot2


def assert_result(got, want, what=""):
    for f in FIELDS:
        if f == "worst":
            assert bits(got[f]) == bits(want[f]), "%s: worst %r, expected %r" % (what, got[f], want[f])
        else:
            assert got[f] == want[f], "%s: %s %r, expected %r" % (what, f, got[f], want[f])


def rank_element(noise, percent):
    """the threshold the tests take from the data: the element of rank n * percent / 100 of the sorted noise"""
    return float(np.sort(noise)[len(noise) * percent // 100])


def open_input(pt, which):
    """(scene, window or None, origin) of one of INPUTS, prepared"""
    name, window = INPUTS[which]
    s = pt.Scene.load(X.golden(name)[1])
    s.prepare()
    return s, window, (window[0], window[1]) if window else (0, 0)


def twin(s, xy, counts):
    """the pixel-sample engine's host twin: fresh states of the pixels xy after counts[i] samples"""
    counts = np.broadcast_to(np.asarray(counts, np.uint32), (len(xy),))
    out, ctr = s.selftest_pixels_host(s.pixel_init(xy), counts=np.ascontiguousarray(counts))
    assert ctr["errors"] == 0
    return out
