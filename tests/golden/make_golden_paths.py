#!/usr/bin/env python3
"""Regenerate the batch radiance fixtures from the UNMODIFIED reference renderer.

Runs only where the reference's sources are present: it builds oracle/_ref/ref_harness
(oracle/build_ref.sh, as tests/golden/make_golden.py does) and records the reference's own
pre-tonemap radiance of SAMPLES-1 variants of three scenes (tests/_paths.py S1).  At one sample
a pixel's radiance is (1.f / 1) * (0 + RayTrace(first sample)): what one batch radiance record
built from that pixel must return.  Data only; no reference source is copied.

Outputs (little-endian):
  rad_s1_<name>.f32        reference mean radiance at SAMPLES 1, W*H*3 f32
  paths_manifest.json      per fixture: scene source, generator args, size, md5s

The CPU oracle (oracle/pt_oracle.cpp) must equal every recorded file byte for byte.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402

import _paths as P  # noqa: E402
import _util as U  # noqa: E402

REF = os.path.join(REPO, "oracle", "_ref")


def md5f(path):
    with open(path, "rb") as f:
        return hashlib.md5(f.read()).hexdigest()


def main():
    subprocess.check_call(["sh", os.path.join(REPO, "oracle", "build_ref.sh")])
    harness = os.path.join(REF, "ref_harness")
    if not os.path.exists(harness):
        print("reference not present; cannot regenerate fixtures", file=sys.stderr)
        return 1
    manifest = {"generator": "tests/golden/make_golden_paths.py", "reference": "FeggieBoss/raytracing-course hw5",
                "radiance": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (src, gen) in P.S1.items():
            sc = P.s1_scene(name)
            rad = os.path.join(HERE, "rad_s1_%s.f32" % name)
            subprocess.check_call([harness, "render", sc, os.path.join(tmp, name + ".ppm"), rad])
            o = U.OracleScene(sc)
            assert o.samples == 1, name
            _, orad, _ = o.render()
            ref = np.fromfile(rad, np.float32).reshape(orad.shape)
            assert np.array_equal(orad.view(np.uint32), ref.view(np.uint32)), name + ": the oracle's radiance differs"
            manifest["radiance"][name] = {"scene": src, "gen": list(gen) if gen else None, "width": o.W, "height": o.H,
                                          "rad_md5": md5f(rad), "scene_md5": md5f(sc)}
            print("radiance", name, manifest["radiance"][name]["rad_md5"])
    with open(os.path.join(HERE, "paths_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
