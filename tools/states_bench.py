#!/usr/bin/env python3
"""The cost of a session's state hand-over (pt_session_export / pt_session_import, device pointers)
on a scene, by default the config-3 stand-in at 1920 x 1080, world 1: every owned pixel's 32-byte
record out of the session and in again.

A session traces `--spp` (1) samples twice -- the second pass is timed: the context figure, what the
session does between two hand-overs --, then exports into a device buffer and imports from it,
`--warmup` (3) calls and `--runs` (10) timed ones each.  Both calls are complete on return, so a
call's time is the host clock around it (it ends in the call's own stream synchronise): the export's
one kernel, the import's memset, two counting kernels, the result's read-back and the write kernel.
After the last import the exported records are compared with a fresh export byte for byte.  Prints
one JSON line.

    python tools/states_bench.py [--scene c3] [--spp 1]
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


def spread(ms):
    t = np.array(ms)
    return {"ms_min": float(t.min()), "ms_median": float(np.median(t)), "ms_max": float(t.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c3")
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("states_bench.py needs the GPU")
    pt = U.ptrace()
    with pt.Scene.load(U.scene_path(a.scene)) as s:
        s.prepare()
        ss = pt.Session(s, device=0)
        n = ss.n_pixels
        passes = []
        for _ in range(2):
            t0 = time.perf_counter()
            ss.trace(a.spp)
            ss.sync()
            passes.append((time.perf_counter() - t0) * 1e3)
        d = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        times = {"export": [], "import": []}
        for it in range(a.warmup + a.runs):
            t0 = time.perf_counter()
            ss.export_states(dev=d)
            t1 = time.perf_counter()
            taken = ss.import_states(d, n=n)
            t2 = time.perf_counter()
            assert taken == n
            if it >= a.warmup:
                times["export"].append((t1 - t0) * 1e3)
                times["import"].append((t2 - t1) * 1e3)
        first = d.clone()
        ss.export_states(dev=d)
        same = bool(torch.equal(first, d))
        st = ss.stats()
        ss.close()
    assert same and st["errors"] == 0 and st["samples"] == n * 2 * a.spp
    out = {"scene": a.scene, "pixels": n, "bytes_per_call": n * 32, "warmup": a.warmup, "runs": a.runs,
           "pass_spp": a.spp, "pass_ms_first": passes[0], "pass_ms": passes[1], "states_kept": same}
    for k, ms in times.items():
        out[k] = spread(ms)
        out[k]["gb_s_median"] = n * 32 / out[k]["ms_median"] / 1e6
    print(json.dumps(out))


if __name__ == "__main__":
    main()
