#!/usr/bin/env python3
"""The ray-query engine's rate (k_rays + k_rays_exact through pt_rayq_run) on two workloads of
a scene, by default the config-3 stand-in:

  primary     one origin at the scene's camera position, targets uniform in the BVH's root box
  incoherent  the BVH-heavy recipe of tests/_rays.py (short rays in random directions near
              random primitives)

Each run is `--rays` rays already on the device, timed by events around pt_rayq_run on one
stream; `--warmup` runs, then `--runs` timed ones.  Several forms alternate run by run in this
one process, and their hit buffers must be equal byte for byte: each `--form NAME[,LIB[,TUNE]]`
is a libpt.so (empty: the tree's build; the kernel's plain form is built with
`make OUT=build_plain DEFS=-DPT_RAYS_PLAIN`) and the PT_TUNE string its context is made under
(`rays_service=N`); a ptrace.py beside LIB is loaded for it (another commit's build).  The spread is that of one form's repeated runs: (max - min) / median.

Algorithmic bytes per ray come from the counters times the record sizes (aux node 128 B,
reference node 32 B, primitive 48 B, plane record 80 B) plus the 24-B ray and the 24-B hit.
Prints one JSON line.

    python tools/rays_bench.py [--scene c3] [--rays 16777216] [--form plain,raytracing-course_amd/build_plain/libpt.so]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import _rays as R  # noqa: E402
import _util as U  # noqa: E402


def load_ptrace(lib, tag):
    """ptrace over `lib` (None: the tree's build) as its own module; a ptrace.py beside `lib` -- the
    build of another commit, whose library may lack this tree's newer entry points -- is the one loaded"""
    old = os.environ.get("PT_LIB")
    src = os.path.join(U.PKG, "ptrace.py")
    if lib:
        os.environ["PT_LIB"] = os.path.abspath(lib)
        beside = os.path.join(os.path.dirname(os.path.abspath(lib)), "ptrace.py")
        if os.path.exists(beside):
            src = beside
    try:
        spec = importlib.util.spec_from_file_location("ptrace_" + tag, src)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if lib:
            if old is None:
                del os.environ["PT_LIB"]
            else:
                os.environ["PT_LIB"] = old
    return mod


def camera_position(path):
    with open(path) as f:
        for line in f:
            w = line.split()
            if w and w[0] == "CAMERA_POSITION":
                return np.array([float(v) for v in w[1:4]], np.float32)
    raise SystemExit("no CAMERA_POSITION in %s" % path)


def primary_rays(scene, path, n, rng):
    nodes, _ = scene.dump_bvh()
    root = np.frombuffer(nodes, np.float32, 6)
    o = camera_position(path)
    target = rng.uniform(root[0:3], root[3:6], (n, 3)).astype(np.float32)
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([np.broadcast_to(o, (n, 3)), d], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c3")
    ap.add_argument("--rays", type=int, default=1 << 24)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--form", action="append", default=[], metavar="NAME[,LIB[,TUNE]]",
                    help="a form to run beside the tree's build as it ships (repeatable)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rays_bench.py needs the GPU")
    specs = [("shipped", "", "")] + [tuple((f.split(",", 2) + ["", ""])[:3]) for f in a.form]
    mods = {}
    for _, lib, _ in specs:
        if lib not in mods:
            mods[lib] = load_ptrace(lib or None, str(len(mods)))
    path = U.scene_path(a.scene)
    n = a.rays
    rng = np.random.default_rng(R.SEED)
    out = {"scene": a.scene, "rays_per_run": n, "warmup": a.warmup, "runs": a.runs, "workloads": {}}
    scenes = {lib: pt.Scene.load(path).prepare() for lib, pt in mods.items()}
    ctxs = []
    for name, lib, tune in specs:
        # (PT_TUNE is read when a context is made)
        if tune:
            os.environ["PT_TUNE"] = tune
        ctxs.append((name, mods[lib], mods[lib].RayQuery(scenes[lib], max_rays=n)))
        os.environ.pop("PT_TUNE", None)
    stream = torch.cuda.Stream()
    for wl in ("primary", "incoherent"):
        s0 = scenes[specs[0][1]]
        rays = primary_rays(s0, path, n, rng) if wl == "primary" else R.bvh_rays(s0, n, rng)
        d_rays = torch.from_numpy(rays).cuda()
        d_hits = [torch.zeros(n * 24, dtype=torch.uint8, device="cuda") for _ in ctxs]
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in ctxs}
        stats = {}
        for it in range(a.warmup + a.runs):
            for k, (name, pt, q) in enumerate(ctxs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                q.run(d_rays, d_hits[k], n=n, stream=stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                st = q.stats()
                if it >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
                    stats[name] = st
        res = {}
        for k, (name, pt, q) in enumerate(ctxs):
            st, t = stats[name], np.array(ms[name])
            assert st["errors"] == 0 and st["rays"] == n, st
            bytes_per_ray = (st["aux_visits"] * st["aux_bytes"] + st["node_visits"] * st["node_bytes"] +
                             st["prim_tests"] * st["prim_bytes"] + st["plane_tests"] * 80) / n + 48
            res[name] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max()),
                         "spread": float((t.max() - t.min()) / np.median(t)),
                         "mray_s_median": n / float(np.median(t)) / 1e3, "mray_s_best": n / float(t.min()) / 1e3,
                         "kernel_ms_last": st["kernel_ms"], "bytes_per_ray": bytes_per_ray,
                         "aux_per_ray": st["aux_visits"] / n, "nodes_per_ray": st["node_visits"] / n,
                         "prim_tests_per_ray": st["prim_tests"] / n, "fallbacks": st["fallbacks"]}
        if len(ctxs) > 1:
            res["outputs_equal"] = all(bool(torch.equal(d_hits[0], h)) for h in d_hits[1:])
            assert res["outputs_equal"], "the forms' hit buffers differ"
        hits = d_hits[0].cpu().numpy().view(ctxs[0][1].HIT_DTYPE)
        res["hit_fraction"] = float((hits["id"] >= 0).mean())
        out["workloads"][wl] = res
        del d_rays, d_hits
    for _, _, q in ctxs:
        q.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
