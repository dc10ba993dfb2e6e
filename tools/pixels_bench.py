#!/usr/bin/env python3
"""The pixel-sample engine's rate (k_pixels through pt_pixq_run) on two workloads of a scene, by
default the config-3 stand-in:

  uniform   every pixel of the frame, fresh default-seed states, `--spp` (4) samples each
  adaptive  every pixel at 1 sample first (not timed), then the timed run: `--more` (16) further
            samples for one pixel in `--every` (16), a count of 0 for the others

Each timed run is one workload's states and counts already on the device -- copied from a kept
start state before every run, outside the timed span --, timed by events around pt_pixq_run on
one stream; `--warmup` runs, then `--runs` timed ones.  Several forms alternate run by run in this
one process, and their states after a run must be equal byte for byte: each
`--form NAME[,LIB[,TUNE]]` is a libpt.so (empty: the tree's build; the kernel's plain form is built
with `make OUT=build_plain DEFS=-DPT_PIXELS_PLAIN`, another occupancy with
`DEFS=-DPT_PIXELS_WAVES_PER_EU=N`, 0 = the compiler's choice) and the PT_TUNE string its context is
made under (`pixels_service=N`).  The rate is Mray/s = the run's RayIntersection calls (pt_stats.rays)
/ the event time; the spread is that of one form's repeated runs: (max - min) / median.  Prints
one JSON line.

    python tools/pixels_bench.py [--scene c3] \\
        [--form plain,raytracing-course_amd/build_plain/libpt.so] [--form s8,,pixels_service=8]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import _util as U  # noqa: E402
from rays_bench import load_ptrace  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c3")
    ap.add_argument("--spp", type=int, default=4, help="samples per pixel of the uniform workload")
    ap.add_argument("--more", type=int, default=16, help="adaptive: further samples of a chosen pixel")
    ap.add_argument("--every", type=int, default=16, help="adaptive: one pixel in this many is chosen")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--form", action="append", default=[], metavar="NAME[,LIB[,TUNE]]",
                    help="a form to run beside the tree's build as it ships (repeatable)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pixels_bench.py needs the GPU")
    specs = [("shipped", "", "")] + [tuple((f.split(",", 2) + ["", ""])[:3]) for f in a.form]
    mods = {}
    for _, lib, _ in specs:
        if lib not in mods:
            mods[lib] = load_ptrace(lib or None, "x%d" % len(mods))
    path = U.scene_path(a.scene)
    scenes = {lib: pt.Scene.load(path).prepare() for lib, pt in mods.items()}
    pt0, s0 = mods[specs[0][1]], scenes[specs[0][1]]
    inf = s0.info
    w, h = inf["width"], inf["height"]
    n = w * h
    k = np.arange(n)
    fresh = s0.pixel_init(np.stack([k % w, k // w], axis=1))
    ctxs = []
    for name, lib, tune in specs:
        # (PT_TUNE is read when a context is made)
        if tune:
            os.environ["PT_TUNE"] = tune
        ctxs.append((name, mods[lib], mods[lib].PixelQuery(scenes[lib], max_pixels=n)))
        os.environ.pop("PT_TUNE", None)
    stream = torch.cuda.Stream()
    d_fresh = torch.from_numpy(fresh.view(np.uint8)).cuda()
    # the adaptive workload's start: every pixel at 1 sample (the shipped form's run), and its counts:
    # a seeded choice of one pixel in `every`
    d_one = d_fresh.clone()
    torch.cuda.synchronize()
    ctxs[0][2].run(d_one, spp=1, n=n, stream=stream.cuda_stream)
    ctxs[0][2].stats()
    counts = np.where(np.random.default_rng(7).integers(0, a.every, n) == 0, a.more, 0).astype(np.int32)
    d_counts = torch.from_numpy(counts).cuda()
    work = {"uniform": (d_fresh, None, a.spp, n * a.spp), "adaptive": (d_one, d_counts, 0, int(counts.sum()))}
    out = {"scene": a.scene, "pixels": n, "warmup": a.warmup, "runs": a.runs, "forms": [list(s) for s in specs],
           "workloads": {}}
    for wl, (d_start, d_cnt, spp, samples) in work.items():
        d_state = [torch.empty_like(d_start) for _ in ctxs]
        ms = {name: [] for name, _, _ in ctxs}
        stats = {}
        for it in range(a.warmup + a.runs):
            for j, (name, pt, q) in enumerate(ctxs):
                with torch.cuda.stream(stream):
                    d_state[j].copy_(d_start)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                q.run(d_state[j], counts=d_cnt, spp=spp, n=n, stream=stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                st = q.stats()
                if it >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
                    stats[name] = st
        rays = stats[ctxs[0][0]]["rays"]
        res = {"records": n, "records_run": n if d_cnt is None else int((counts != 0).sum()), "samples": samples,
               "rays": rays, "rays_per_sample": rays / samples}
        for name, pt, q in ctxs:
            st, t = stats[name], np.array(ms[name])
            assert st["errors"] == 0 and st["rays"] == rays and st["samples"] == samples, st
            res[name] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max()),
                         "spread": float((t.max() - t.min()) / np.median(t)),
                         "mray_s_median": rays / float(np.median(t)) / 1e3, "mray_s_best": rays / float(t.min()) / 1e3,
                         "msample_s_median": samples / float(np.median(t)) / 1e3, "kernel_ms_last": st["kernel_ms"],
                         "fallbacks": st["fallbacks"]}
        if len(ctxs) > 1:
            res["states_equal"] = all(bool(torch.equal(d_state[0], o)) for o in d_state[1:])
            assert res["states_equal"], "the forms' states differ"
        out["workloads"][wl] = res
        del d_state
    for _, _, q in ctxs:
        q.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
