#!/usr/bin/env python3
"""Static instruction counts per kernel from a device assembly listing: the output of the
Makefile's DEVFLAGS plus `-S --cuda-device-only` on one unit (csrc/device/*.hip).

    python tools/kernel_insts.py pt_path.s [--kernel k_wpath]

Per function: the instruction total, the VALU (v_*), scalar (s_*, scalar loads and branches
included), LDS (ds_*) and vector-memory (global_/flat_/buffer_/scratch_) totals, the v_mov*
count, the longest run of consecutive v_mov* and the *_saveexec_* count.  Classified by
mnemonic prefix only; these are instructions in the code, not instructions executed.
"""
import argparse
import json
import re

CLASSES = (("valu", ("v_",)), ("scalar", ("s_",)), ("lds", ("ds_",)),
           ("vmem", ("global_", "flat_", "buffer_", "scratch_")))


def count(path):
    out, cur, run = {}, None, 0
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur = out[m.group(1)] = dict.fromkeys(["insts", "valu", "scalar", "lds", "vmem", "other", "v_mov",
                                                   "max_mov_run", "saveexec"], 0)
            run = 0
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        m = re.match(r"\s+([a-z][a-z0-9_]*)(\s|$)", line)
        if cur is None or not m:
            continue   # labels, directives (.xxx), comments
        op = m.group(1)
        cur["insts"] += 1
        cur[next((c for c, pre in CLASSES if op.startswith(pre)), "other")] += 1
        run = run + 1 if op.startswith("v_mov") else 0
        cur["v_mov"] += run > 0
        cur["max_mov_run"] = max(cur["max_mov_run"], run)
        cur["saveexec"] += "_saveexec_" in op
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("--kernel", default="", help="only functions whose mangled name contains this")
    a = ap.parse_args()
    for name, c in count(a.listing).items():
        if a.kernel in name:
            print(json.dumps({"kernel": name, **c}))
