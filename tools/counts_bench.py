#!/usr/bin/env python3
"""A session's per-pixel-count pass (pt_session_trace_counts) against the pixel-sample engine
(k_pixels through pt_pixq_run) on the same states, on two workloads of a scene, by default the
config-3 stand-in:

  adaptive  every pixel at 1 sample first (not timed), then the timed run: `--more` (16) further
            samples for one pixel in `--every` (16) -- the seeded choice of tools/pixels_bench.py --,
            a count of 0 for the others
  uniform   fresh default-seed states, `--spp` (4) samples for every pixel: as per-pixel counts,
            as pt_session_trace(spp) (what the two extra kernels and the read-back cost), and in k_pixels

The forms alternate run by run in this one process; `--warmup` runs, then `--runs` timed ones.
Before every run, outside the timed span, the session takes the workload's start states by
pt_session_import and the pixel query's buffer is copied from them.  A timed span is the host's
clock around the call and the wait for its work (pt_session_sync / the stream's synchronize): the
session's pass counts its rounds on the host, so an event pair would not cover it.  The final states
of the forms must be equal byte for byte, and their ray counts equal.  Mray/s = the run's
RayIntersection calls / the span; spread = (max - min) / median of one form's runs.  `--roundlog`
adds one adaptive session run under PT_TUNE roundlog=2 (its rounds on stderr).  Prints one JSON line.

    python tools/counts_bench.py [--scene c3] [--roundlog]
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


def summary(ms, rays):
    t = np.array(ms)
    med = float(np.median(t))
    return {"ms_median": med, "ms_min": float(t.min()), "ms_max": float(t.max()), "spread": float((t.max() - t.min()) / med),
            "mray_s_median": rays / med / 1e3, "mray_s_best": rays / float(t.min()) / 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c3")
    ap.add_argument("--spp", type=int, default=4, help="samples per pixel of the uniform workload")
    ap.add_argument("--more", type=int, default=16, help="adaptive: further samples of a chosen pixel")
    ap.add_argument("--every", type=int, default=16, help="adaptive: one pixel in this many is chosen")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--roundlog", action="store_true", help="one more adaptive session run with its rounds on stderr")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("counts_bench.py needs the GPU")
    pt = U.ptrace()
    with pt.Scene.load(U.scene_path(a.scene)) as s:
        s.prepare()
        inf = s.info
        w, h = inf["width"], inf["height"]
        ss = pt.Session(s, device=0)
        n = ss.n_pixels
        assert n == w * h
        q = pt.PixelQuery(s, max_pixels=n)
        stream = torch.cuda.Stream()
        # the start states, in the session's export order: fresh, and every pixel at 1 sample
        d_fresh = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        d_one = torch.empty_like(d_fresh)
        ss.export_states(dev=d_fresh)
        ss.trace(1)
        ss.export_states(dev=d_one)
        # (the choice of tools/pixels_bench.py, which draws it per pixel in row-major order)
        xy = pt.rank_pixels(w, h, 0, 1).astype(np.int64)
        chosen = np.random.default_rng(7).integers(0, a.every, n) == 0
        adaptive = np.where(chosen[xy[:, 1] * w + xy[:, 0]], a.more, 0).astype(np.int32)
        d_adaptive = torch.from_numpy(adaptive).cuda()
        d_uniform = torch.full((n,), a.spp, dtype=torch.int32, device="cuda")
        d_state = torch.empty_like(d_fresh)
        d_out = torch.empty_like(d_fresh)
        torch.cuda.synchronize()

        def session_run(d_start, counts, spp):
            ss.import_states(d_start, n=n)
            r0 = ss.stats()["rays"]
            t0 = time.perf_counter()
            if counts is None:
                ss.trace(spp)
            else:
                ss.trace_counts(counts, n=n)
            ss.sync()
            ms = (time.perf_counter() - t0) * 1e3
            st = ss.stats()
            assert st["errors"] == 0
            ss.export_states(dev=d_out)
            return ms, st["rays"] - r0

        def pixels_run(d_start, counts, spp):
            with torch.cuda.stream(stream):
                d_state.copy_(d_start)
            stream.synchronize()
            t0 = time.perf_counter()
            q.run(d_state, counts=counts, spp=spp, n=n, stream=stream.cuda_stream)
            stream.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            st = q.stats()
            assert st["errors"] == 0
            return ms, st["rays"]

        work = {
            "adaptive": (d_one, int(adaptive.sum()), [("session_counts", session_run, d_adaptive, 0),
                                                      ("k_pixels", pixels_run, d_adaptive, 0)]),
            "uniform": (d_fresh, n * a.spp, [("session_counts", session_run, d_uniform, 0),
                                             ("session_trace", session_run, None, a.spp),
                                             ("k_pixels", pixels_run, d_uniform, 0)]),
        }
        out = {"scene": a.scene, "pixels": n, "warmup": a.warmup, "runs": a.runs, "workloads": {}}
        for wl, (d_start, samples, forms) in work.items():
            ms = {name: [] for name, _, _, _ in forms}
            rays = None
            for it in range(a.warmup + a.runs):
                finals = []
                for name, run, counts, spp in forms:
                    t, r = run(d_start, counts, spp)
                    rays = r if rays is None else rays
                    assert r == rays, "%s: %d rays, the other forms %d" % (name, r, rays)
                    finals.append((d_out if run is session_run else d_state).clone())
                    if it >= a.warmup:
                        ms[name].append(t)
                assert all(torch.equal(finals[0], f) for f in finals[1:]), "%s: the forms' final states differ" % wl
            res = {"records": n, "records_run": int((adaptive != 0).sum()) if wl == "adaptive" else n, "samples": samples,
                   "rays": rays, "states_equal": True}
            for name, _, _, _ in forms:
                res[name] = summary(ms[name], rays)
            out["workloads"][wl] = res
        if a.roundlog:
            os.environ["PT_TUNE"] = "roundlog=2"   # (read by every pass)
            session_run(d_one, d_adaptive, 0)
            os.environ.pop("PT_TUNE", None)
        q.close()
        ss.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
