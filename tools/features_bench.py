#!/usr/bin/env python3
"""The first-hit feature engine's rate (k_feats + k_feats_exact through pt_featq_run) beside the
ray-query engine's on the same rays, on a scene's whole frame, by default the config-3 stand-in at
1920 x 1080:

  a     pt_featq_run on the frame's pixel centres (one position per pixel)
  a16   pt_featq_run on 16 positions per pixel (a 4 x 4 grid inside the pixel), in runs of 2^24
  b     pt_rayq_run on the rays of the centres, made by pt_camera_rays on the host and uploaded
        outside the timed span -- the yardstick: per point, (a) reads 16 B less (an 8-B position
        for a 24-B ray), writes 40 B more (a 64-B record for a 24-B hit) and adds one 32-B gather

The three forms alternate run by run in this one process: `--warmup` rounds, then `--runs` timed
ones, events around the run call(s) on one stream.  The features' first 24 bytes must equal (b)'s
hits byte for byte.  Then the session form: `--runs` calls of Session.features(dev) on that frame,
the host's clock around the complete-on-return call, beside Session.export_states(dev) and
Session.noise(dev) timed the same way.  spread = (max - min) / median of one form's runs.
Prints one JSON line.

    python tools/features_bench.py [--scene c3]
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

SUB_RUN = 1 << 24


def summary(ms, n):
    t = np.array(ms)
    med = float(np.median(t))
    return {"ms_min": float(t.min()), "ms_median": med, "ms_max": float(t.max()), "spread": float((t.max() - t.min()) / med),
            "mpoint_s_median": n / med / 1e3, "mpoint_s_best": n / float(t.min()) / 1e3}


def per_point(st, n):
    return {"aux_per_point": st["aux_visits"] / n, "nodes_per_point": st["node_visits"] / n,
            "prim_tests_per_point": st["prim_tests"] / n, "fallbacks": st["fallbacks"], "kernel_ms_last": st["kernel_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c3")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("features_bench.py needs the GPU")
    pt = U.ptrace()
    path = U.scene_path(a.scene)
    scene = pt.Scene.load(path).prepare()
    W, H = scene.info["width"], scene.info["height"]
    n = W * H
    ys, xs = np.mgrid[0:H, 0:W]
    centres = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float32)
    off = (np.arange(4, dtype=np.float32) + 0.5) / 4
    sub = (np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float32)[:, None, :] +
           np.stack(np.meshgrid(off, off), axis=-1).reshape(1, 16, 2)).reshape(-1, 2).astype(np.float32)
    n16 = len(sub)
    rays = scene.camera_rays(centres)
    d_xy, d_sub, d_rays = (torch.from_numpy(x).cuda() for x in (centres, sub, rays))
    d_feat = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    d_feat16 = torch.zeros(min(n16, SUB_RUN) * 64, dtype=torch.uint8, device="cuda")
    d_hits = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
    fq = pt.FeatureQuery(scene, max_points=max(n, min(n16, SUB_RUN)))
    rq = pt.RayQuery(scene, max_rays=n)
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
        fq.run(d_xy, d_feat, n=n, stream=stream.cuda_stream)

    def run_a16():
        for at in range(0, n16, SUB_RUN):
            m = min(SUB_RUN, n16 - at)
            fq.run(d_sub[at:at + m], d_feat16, n=m, stream=stream.cuda_stream)

    def run_b():
        rq.run(d_rays, d_hits, n=n, stream=stream.cuda_stream)

    ms = {"a": [], "a16": [], "b": []}
    stats = {}
    for it in range(a.warmup + a.runs):
        for name, fn, q in (("a", run_a, fq), ("a16", run_a16, fq), ("b", run_b, rq)):
            t = timed(fn)
            st = q.stats()
            assert st["errors"] == 0, st
            if it >= a.warmup:
                ms[name].append(t)
                stats[name] = st
    assert stats["a"]["rays"] == n and stats["a16"]["rays"] == n16 and stats["b"]["rays"] == n
    feat = d_feat.cpu().numpy().view(pt.FEATURE_DTYPE)
    hits = d_hits.cpu().numpy().view(pt.HIT_DTYPE)
    head = np.ascontiguousarray(feat).view(np.uint8).reshape(n, 64)[:, :24]
    assert head.tobytes() == hits.tobytes(), "the features' hits differ from the ray query's"
    out = {"scene": a.scene, "width": W, "height": H, "points": n, "points16": n16, "warmup": a.warmup, "runs": a.runs,
           "hit_fraction": float((feat["id"] >= 0).mean()),
           "a": dict(summary(ms["a"], n), **per_point(stats["a"], n)),
           "a16": dict(summary(ms["a16"], n16), **per_point(stats["a16"], n16)),
           "b": dict(summary(ms["b"], n), **per_point(stats["b"], n))}
    fq.close()
    rq.close()

    # the session form, beside two calls of the same shape (complete on return, host clock)
    ss = pt.Session(scene)
    npx = ss.n_pixels
    d_out = torch.zeros(npx * 64, dtype=torch.uint8, device="cuda")
    d_state = torch.zeros(npx * 32, dtype=torch.uint8, device="cuda")
    d_noise = torch.zeros(npx, dtype=torch.float32, device="cuda")
    ss.trace(1)
    ss.sync()
    ss.mark()
    calls = {"session_features": lambda: ss.features(dev=d_out), "session_export": lambda: ss.export_states(dev=d_state),
             "session_noise": lambda: ss.noise(dev=d_noise)}
    t0 = time.perf_counter()
    ss.features(dev=d_out)   # (the first call makes the context and the positions)
    out["session_features_first_ms"] = (time.perf_counter() - t0) * 1e3
    for name, fn in calls.items():
        t = []
        for it in range(a.warmup + a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if it >= a.warmup:
                t.append(dt)
        t = np.array(t)
        out[name] = {"ms_min": float(t.min()), "ms_median": float(np.median(t)), "ms_max": float(t.max())}
    sfeat = d_out.cpu().numpy().view(pt.FEATURE_DTYPE)
    px = pt.rank_pixels(W, H, 0, 1).astype(np.int64)
    assert sfeat.tobytes() == feat[px[:, 1] * W + px[:, 0]].tobytes(), "the session's records differ from the context's"
    ss.close()
    scene.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
