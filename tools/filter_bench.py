#!/usr/bin/env python3
"""The guided filter's time (k_filter through pt_filtq_run) beside the same filter composed from torch
operations, and what it does to a frame's error, on a scene's whole frame, by default the config-3
stand-in at 1920 x 1080:

  a   pt_filtq_run with the default options on a session's packed radiance (PT_FILTER_TILES), 16 spp
  b   the definition written with torch element-wise operations on device tensors (rolls, selects,
      sums: what a caller writes without the library), on the same frame unpacked to rows outside the
      timed span and on the same guides; not bit-equal to (a) -- its largest absolute difference from
      (a) over the finite pixels is reported

The two forms alternate run by run in this one process: `--warmup` rounds, then `--runs` timed ones,
events around the call(s) on one stream.  spread = (max - min) / median of one form's runs.  Then (a)
alone at 1 .. 5 levels (a level's cost is the difference of neighbours), pt_filtq_create's one-time
cost on the host's clock, and the quality: the relative RMSE -- sqrt(mean((x - ref)^2 / (ref^2 +
0.01))) over pixels and channels -- against a `--ref-spp` render by the library, before and after the
filter, at 4 and at 16 spp.  `--only-a`: form (a) alone and nothing else (for a profiler run).
Prints one JSON line.

    python tools/filter_bench.py [--scene c3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import _util as U  # noqa: E402

K = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def summary(ms):
    t = np.array(ms)
    med = float(np.median(t))
    return {"ms_min": float(t.min()), "ms_median": med, "ms_max": float(t.max()), "spread": float((t.max() - t.min()) / med)}


def torch_filter(torch, c, n, t, a, cls, o):
    """the definition (include/pt.h "guided filter") in torch float32 operations"""
    H, W = t.shape
    ys = torch.arange(H, device=c.device).view(H, 1)
    xs = torch.arange(W, device=c.device).view(1, W)
    zero, one = torch.zeros((), device=c.device), torch.ones((), device=c.device)

    def inv(g):
        return torch.where(g > 0, 1 / g, zero)

    ia = inv(torch.tensor(np.float32(o.sigma_a) * np.float32(o.sigma_a), device=c.device))
    iz = inv((o.sigma_z * t) ** 2)
    for L in range(o.levels):
        s = 1 << L
        sc = np.float32(o.sigma_c) * np.float32(2.0 ** -L)
        ic = inv(torch.tensor(sc * sc, device=c.device))
        fin = torch.isfinite(c).all(dim=2)
        acc = torch.zeros_like(c)
        ws = torch.zeros_like(t)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dx == 0 and dy == 0:
                    acc = acc + (9 / 64) * c
                    ws = ws + (9 / 64)
                    continue
                sh = (-dy * s, -dx * s)
                inside = ((ys + dy * s >= 0) & (ys + dy * s < H)) & ((xs + dx * s >= 0) & (xs + dx * s < W))
                nq, tq, aq, clsq, cq, finq = (torch.roll(v, sh, (0, 1)) for v in (n, t, a, cls, c, fin))
                d = (n * nq).sum(dim=2)
                d = torch.where(d > 0, d, zero)
                for _ in range(o.normal_pow2):
                    d = d * d
                wn = torch.where(cls == 0, one, d)
                ez = (t - tq) ** 2
                ea = ((a - aq) ** 2).sum(dim=2)
                ec = ((c - cq) ** 2).sum(dim=2)
                D = (1 + ez * iz) * (1 + ea * ia) * (1 + ec * ic)
                wt = (K[dy + 2] * K[dx + 2]) * wn / D
                keep = inside & (clsq == cls) & finq & (wt > 0)
                wt = torch.where(keep, wt, zero)
                acc = acc + wt[..., None] * torch.where(keep[..., None], cq, zero)
                ws = ws + wt
        c = torch.where(fin[..., None], acc / ws[..., None], c)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c3")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--only-a", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("filter_bench.py needs the GPU")
    pt = U.ptrace()
    scene = pt.Scene.load(U.scene_path(a.scene)).prepare()
    W, H = scene.info["width"], scene.info["height"]
    n = W * H
    ss = pt.Session(scene)
    d_rad = torch.zeros(ss.n_tiles * 256 * 3, dtype=torch.float32, device="cuda")

    def render(spp):
        """the session's frame at spp samples, packed, in d_rad (and unpacked on the host)"""
        ss.reset()
        ss.trace(spp)
        ss.resolve(None, d_rad.data_ptr())
        ss.sync()
        return pt.unpack_tiles_f32(d_rad.cpu().numpy(), W, H, 0, 1).reshape(H, W, 3)

    t0 = time.perf_counter()
    q = pt.FilterQuery(scene)
    create_ms = (time.perf_counter() - t0) * 1e3
    made = q.stats()
    assert made["rays"] == n
    opts = pt.FilterOpts.default(layout=pt.FILTER_TILES)
    rows16 = render(a.spp)
    d_out = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def run_a():
        q.run(d_rad, d_out, stream=stream.cuda_stream, opts=opts)

    out = {"scene": a.scene, "width": W, "height": H, "pixels": n, "spp": a.spp, "warmup": a.warmup, "runs": a.runs,
           "options": opts.as_dict(), "create_ms": create_ms}
    if a.only_a:
        ms = [timed(run_a) for _ in range(a.warmup + a.runs)][a.warmup:]
        q.stats()
        out["a"] = summary(ms)
        print(json.dumps(out))
        return

    # (b)'s inputs: the frame in rows and the guides as tensors, from the same feature records
    ys, xs = np.mgrid[0:H, 0:W]
    centres = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float32)
    feat = scene.features(centres)[0].reshape(H, W)
    hit = feat["id"] >= 0
    cls = np.where(hit, 1 + feat["material"] + 4 * (feat["emission"] != 0).any(axis=2), 0).astype(np.int32)
    g_n, g_t, g_a, g_cls = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (feat["n"], feat["t"], feat["albedo"], cls))
    d_rows = torch.from_numpy(np.ascontiguousarray(rows16)).cuda()
    ro = pt.FilterOpts.default()
    res_b = [None]

    def run_b():
        with torch.cuda.stream(stream):
            res_b[0] = torch_filter(torch, d_rows, g_n, g_t, g_a, g_cls, ro)

    ms = {"a": [], "b": []}
    for it in range(a.warmup + a.runs):
        for name, fn in (("a", run_a), ("b", run_b)):
            t = timed(fn)
            if it >= a.warmup:
                ms[name].append(t)
    st = q.stats()
    got_a = d_out.cpu().numpy().reshape(H, W, 3)
    got_b = res_b[0].cpu().numpy()
    both = np.isfinite(got_a) & np.isfinite(got_b)
    out["a"] = dict(summary(ms["a"]), kernel_ms_per_run=st["kernel_ms"] / (a.warmup + a.runs))
    out["b"] = dict(summary(ms["b"]), max_abs_diff_from_a=float(np.abs(got_a - got_b)[both].max()),
                    pixels_finite_in_one_only=int((np.isfinite(got_a) != np.isfinite(got_b)).any(axis=2).sum()))
    out["a_median_below_b_min"] = bool(out["a"]["ms_median"] < out["b"]["ms_min"])

    # (a) at 1 .. 5 levels
    out["levels"] = {}
    for lv in range(1, 6):
        o = pt.FilterOpts.default(layout=pt.FILTER_TILES, levels=lv)
        t = [timed(lambda: q.run(d_rad, d_out, stream=stream.cuda_stream, opts=o)) for _ in range(a.warmup + a.runs)]
        out["levels"][str(lv)] = summary(t[a.warmup:])
    q.stats()

    # quality against the library's own long render
    # (over the pixels that are finite in the reference and in the frame: the filter keeps the others)
    def rel_rmse(x, ref, ok):
        x, ref = x[ok].astype(np.float64), ref[ok].astype(np.float64)
        return float(np.sqrt(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01))))

    ref = render(a.ref_spp).copy()
    out["quality"] = {"ref_spp": a.ref_spp}
    for spp in (4, 16):
        rows = render(spp)
        q.run(d_rad, d_out, opts=opts)
        q.stats()
        filt = d_out.cpu().numpy().reshape(H, W, 3)
        ok = np.isfinite(ref).all(axis=2) & np.isfinite(rows).all(axis=2)
        assert np.isfinite(filt[ok]).all()
        out["quality"][str(spp)] = {"rel_rmse_before": rel_rmse(rows, ref, ok), "rel_rmse_after": rel_rmse(filt, ref, ok),
                                    "pixels_left_out": int((~ok).sum())}
    q.close()
    ss.close()
    scene.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
