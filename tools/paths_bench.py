#!/usr/bin/env python3
"""The batch radiance engine's rate (k_paths through pt_pathq_run) on two workloads of a scene,
by default the config-3 stand-in:

  camera  the scene's own camera, one jittered sample per pixel (pt_camera_rays), seed = the
          pixel's index
  bvh     the BVH-heavy rays of tests/_rays.py (short rays in random directions near random
          primitives) as path starts, `--paths` of them, seed = the path's index

Each run is one workload's records already on the device, timed by events around pt_pathq_run on
one stream; `--warmup` runs, then `--runs` timed ones.  Several forms alternate run by run in this
one process, and their output buffers must be equal byte for byte: each `--form NAME[,LIB[,TUNE]]`
is a libpt.so (empty: the tree's build; the kernel's plain form is built with
`make OUT=build_plain DEFS=-DPT_PATHS_PLAIN`) and the PT_TUNE string its context is made under
(`paths_service=N`).  The rate is Mray/s = the paths' RayIntersection calls (the sum of the
records' `rays`) / the event time; the spread is that of one form's repeated runs:
(max - min) / median.  `--bench-json FILE` adds, for context only, the Mray/s of a bench.py
result line kept in FILE (the render of the same scene).  Prints one JSON line.

    python tools/paths_bench.py [--scene c3] [--paths 2097152] \\
        [--form plain,raytracing-course_amd/build_plain/libpt.so] [--form s8,,paths_service=8]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import _rays as R  # noqa: E402
import _util as U  # noqa: E402
from rays_bench import load_ptrace  # noqa: E402


def camera_records(pt, scene, rng):
    inf = scene.info
    w, h = inf["width"], inf["height"]
    xy = np.stack(np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32)), axis=-1).reshape(-1, 2)
    xy = xy + rng.random(xy.shape, np.float32)
    rays = scene.camera_rays(xy)
    rec = np.zeros(len(rays), pt.PATH_DTYPE)
    rec["o"], rec["d"], rec["seed"] = rays[:, :3], rays[:, 3:], np.arange(len(rays))
    return rec


def bvh_records(pt, scene, n, rng):
    rays = R.bvh_rays(scene, n, rng)
    rec = np.zeros(n, pt.PATH_DTYPE)
    rec["o"], rec["d"], rec["seed"] = rays[:, :3], rays[:, 3:], np.arange(n)
    return rec


def bench_value(path):
    """the last bench.py result line of a file: its Mray/s"""
    value = None
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith("{"):
                try:
                    d = json.loads(line)
                except ValueError:
                    continue
                if d.get("unit") == "Mray/s" and "value" in d:
                    value = d["value"]
    return value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c3")
    ap.add_argument("--paths", type=int, default=1 << 21, help="paths of the bvh workload")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--form", action="append", default=[], metavar="NAME[,LIB[,TUNE]]",
                    help="a form to run beside the tree's build as it ships (repeatable)")
    ap.add_argument("--bench-json", default=None, help="a file holding a bench.py result line (context only)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("paths_bench.py needs the GPU")
    specs = [("shipped", "", "")] + [tuple((f.split(",", 2) + ["", ""])[:3]) for f in a.form]
    mods = {}
    for _, lib, _ in specs:
        if lib not in mods:
            mods[lib] = load_ptrace(lib or None, "p%d" % len(mods))
    path = U.scene_path(a.scene)
    rng = np.random.default_rng(R.SEED)
    scenes = {lib: pt.Scene.load(path).prepare() for lib, pt in mods.items()}
    pt0, s0 = mods[specs[0][1]], scenes[specs[0][1]]
    work = {"camera": camera_records(pt0, s0, rng), "bvh": bvh_records(pt0, s0, a.paths, rng)}
    cap = max(len(r) for r in work.values())
    ctxs = []
    for name, lib, tune in specs:
        # (PT_TUNE is read when a context is made)
        if tune:
            os.environ["PT_TUNE"] = tune
        ctxs.append((name, mods[lib], mods[lib].PathQuery(scenes[lib], max_paths=cap)))
        os.environ.pop("PT_TUNE", None)
    out = {"scene": a.scene, "warmup": a.warmup, "runs": a.runs, "forms": [list(s) for s in specs], "workloads": {}}
    if a.bench_json:
        out["bench_mray_s"] = bench_value(a.bench_json)
    stream = torch.cuda.Stream()
    for wl, rec in work.items():
        n = len(rec)
        d_in = torch.from_numpy(rec.view(np.uint8)).cuda()
        d_out = [torch.zeros(n * 16, dtype=torch.uint8, device="cuda") for _ in ctxs]
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in ctxs}
        stats = {}
        for it in range(a.warmup + a.runs):
            for k, (name, pt, q) in enumerate(ctxs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                q.run(d_in, d_out[k], n=n, stream=stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                st = q.stats()
                if it >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
                    stats[name] = st
        got = d_out[0].cpu().numpy().view(pt0.RADIANCE_DTYPE)
        rays = int(got["rays"].sum())
        res = {"paths": n, "rays": rays, "rays_per_path": rays / n,
               "nonzero_fraction": float((got["rgb"] != 0).any(axis=1).mean())}
        for name, pt, q in ctxs:
            st, t = stats[name], np.array(ms[name])
            assert st["errors"] == 0 and st["rays"] == rays, st
            res[name] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max()),
                         "spread": float((t.max() - t.min()) / np.median(t)),
                         "mray_s_median": rays / float(np.median(t)) / 1e3, "mray_s_best": rays / float(t.min()) / 1e3,
                         "mpath_s_median": n / float(np.median(t)) / 1e3, "kernel_ms_last": st["kernel_ms"],
                         "aux_per_ray": st["aux_visits"] / rays, "nodes_per_ray": st["node_visits"] / rays,
                         "prim_tests_per_ray": st["prim_tests"] / rays, "fallbacks": st["fallbacks"]}
        if len(ctxs) > 1:
            res["outputs_equal"] = all(bool(torch.equal(d_out[0], o)) for o in d_out[1:])
            assert res["outputs_equal"], "the forms' output buffers differ"
        out["workloads"][wl] = res
        del d_in, d_out
    for _, _, q in ctxs:
        q.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
