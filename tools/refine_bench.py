#!/usr/bin/env python3
"""One adaptive step inside the session (pt_session_refine) against the caller's loop it replaces
(device export, the noise formula in torch, pt_session_trace_counts), on a scene's whole frame, by
default the config-3 stand-in at 1920 x 1080, one rank:

  every pixel goes to `--first` (8) samples, is marked there, and goes on to `--second` (16); the timed
  step gives every pixel whose noise is above the threshold `--step` (16) more samples.  The threshold is
  taken from the data: the element of rank 90 % of the sorted noise (Session.noise()).

  refine    Session.refine(threshold, step) and the wait for its pass
  caller    Session.export_states(dev), the formula of include/pt.h "session noise" on the export and on
            the export kept from the mark, in torch float32 ops on the device, Session.trace_counts of
            the counts it makes, and the wait for the pass

Two sessions, one per form, alternate run by run in this one process; `--warmup` pairs, then `--runs`
timed ones.  Before every run, outside the timed span, the form's session is put back: the states at
`--first` samples imported, (refine:) marked, and traced to `--second`.  A timed span is the host's clock
around the calls and the wait for their work.  After each pair the two sessions' exports must be equal
byte for byte, and so must their ray counts.  spread = (max - min) / median of one form's runs.
Prints one JSON line.

    python tools/refine_bench.py [--scene c3]
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


def summary(ms):
    t = np.array(ms)
    med = float(np.median(t))
    return {"ms_min": float(t.min()), "ms_median": med, "ms_max": float(t.max()), "spread": float((t.max() - t.min()) / med)}


def torch_counts(torch, d_now, d_mark, threshold, step):
    """the counts of include/pt.h "session noise" (spread 0, no cap) for two exports on the device:
    float32 ops, one rounding each, in the stated order"""
    now, mark = d_now.view(torch.int32).view(-1, 8), d_mark.view(torch.int32).view(-1, 8)
    k, a = now[:, 7], mark[:, 7]
    est = (a != 0) & (k > a)
    kf, af = k.to(torch.float32), a.to(torch.float32)
    m = (torch.ones_like(kf) / kf)[:, None] * now[:, 4:7].view(torch.float32)
    p = (torch.ones_like(af) / af)[:, None] * mark[:, 4:7].view(torch.float32)
    d = (m - p).abs()
    d = (d[:, 0] + d[:, 1]) + d[:, 2]
    l = (m[:, 0] + m[:, 1]) + m[:, 2]
    floor = torch.full_like(l, 2.0 ** -10)
    noise = d / torch.sqrt(torch.where(l > floor, l, floor))
    noise = torch.where(est, noise, torch.full_like(noise, float("inf")))
    return torch.where(noise > threshold, step, 0).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c3")
    ap.add_argument("--first", type=int, default=8, help="samples of every pixel at the mark")
    ap.add_argument("--second", type=int, default=16, help="samples of every pixel before the timed step")
    ap.add_argument("--step", type=int, default=16, help="further samples of a pixel above the threshold")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("refine_bench.py needs the GPU")
    pt = U.ptrace()
    with pt.Scene.load(U.scene_path(a.scene)) as s:
        s.prepare()
        w, h = s.info["width"], s.info["height"]
        sa, sb = pt.Session(s, device=0), pt.Session(s, device=0)
        n = sa.n_pixels
        assert n == w * h
        d_mark = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        d_a, d_b = torch.empty_like(d_mark), torch.empty_like(d_mark)
        d_plan = torch.empty(n, dtype=torch.int32, device="cuda")
        sa.trace(a.first)
        sa.export_states(dev=d_mark)
        torch.cuda.synchronize()

        def put_back(ss, mark):
            ss.import_states(d_mark, n=n)
            if mark:
                ss.mark()
            ss.trace(a.second - a.first)
            ss.sync()
            return ss.stats()["rays"]

        put_back(sa, True)
        threshold = float(np.sort(sa.noise())[n * 90 // 100])
        out = {"scene": a.scene, "pixels": n, "first": a.first, "second": a.second, "step": a.step, "threshold": threshold,
               "warmup": a.warmup, "runs": a.runs}
        ms = {"refine": [], "caller": []}
        for it in range(a.warmup + a.runs):
            # (a) the step inside the session
            r0 = put_back(sa, True)
            if it == 0:
                sa.plan(threshold, a.step, dev=d_plan)
            t0 = time.perf_counter()
            res = sa.refine(threshold, a.step)
            sa.sync()
            t_a = (time.perf_counter() - t0) * 1e3
            st = sa.stats()
            assert st["errors"] == 0 and st["short_pixels"] == 0
            rays_a = st["rays"] - r0
            sa.export_states(dev=d_a)
            # (b) the caller's loop of today
            r0 = put_back(sb, False)
            t0 = time.perf_counter()
            sb.export_states(dev=d_b)
            counts = torch_counts(torch, d_b, d_mark, threshold, a.step)
            torch.cuda.synchronize()   # (the session's stream is not torch's)
            sb.trace_counts(counts, n=n)
            sb.sync()
            t_b = (time.perf_counter() - t0) * 1e3
            st = sb.stats()
            assert st["errors"] == 0 and st["short_pixels"] == 0
            rays_b = st["rays"] - r0
            sb.export_states(dev=d_b)
            torch.cuda.synchronize()
            if it == 0:
                differ = int((counts != d_plan).sum())
                assert differ == 0, "torch's counts differ from the session's plan for %d pixels" % differ
            assert torch.equal(d_a, d_b), "run %d: the two sessions' exports differ" % it
            assert rays_a == rays_b, "run %d: %d rays against %d" % (it, rays_a, rays_b)
            if it >= a.warmup:
                ms["refine"].append(t_a)
                ms["caller"].append(t_b)
        out.update({"refined": res["refined"], "samples": res["samples"], "worst": res["worst"], "rays": rays_a,
                    "exports_equal": True, "refine": summary(ms["refine"]), "caller": summary(ms["caller"])})
        sa.close()
        sb.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
