#!/usr/bin/env python3
"""Regenerate the loader fixtures from the UNMODIFIED reference's own Scene::Load.

Runs only where the reference sources exist (oracle/build_ref.sh builds oracle/_ref/ref_harness
from them).  For every case of tests/_loader_cases.py it records what `ref_harness parse` wrote
(the parse, every field as its raw bits) and the reference's stderr lines; for the cases in
_loader_cases.RENDERED also the reference's image and fp32 radiance (`ref_harness render`).
Only what the reference wrote is kept: no reference source is copied.

Outputs:
  loader_cases.json              per case: the md5 of its text, the dump (hex: an 80-byte header,
                                 then 100 bytes per primitive in file order; oracle/ref_harness.cpp
                                 mode parse; the fields that no line of the file wrote, which the
                                 reference leaves to the stack, zeroed: _loader_cases.unset_words)
                                 and the stderr lines in order
  img_loader_<case>.ppm          reference P6 output of a rendered case
  rad_loader_<case>.f32          its pre-tonemap mean radiance, w*h*3 f32

A case whose harness run fails or takes more than a minute (the reference can loop for ever on a
scene it parsed), or a rendered case whose radiance is not finite, stops the
generator: no case is dropped silently.
"""
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
import _loader_cases  # noqa: E402

REF = os.path.join(REPO, "oracle", "_ref")
OUT = os.path.join(HERE, "loader_cases.json")


def render_name(case):
    return "loader_" + case[len("render_"):]


def main():
    subprocess.check_call(["sh", os.path.join(REPO, "oracle", "build_ref.sh")])
    harness = os.path.join(REF, "ref_harness")
    if not os.path.exists(harness):
        sys.exit("no reference harness: the reference sources are not on this machine")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        sc, dump = os.path.join(tmp, "case.txt"), os.path.join(tmp, "case.bin")
        for name, text in _loader_cases.CASES.items():
            with open(sc, "wb") as f:
                f.write(text)
            if os.path.exists(dump):
                os.remove(dump)
            r = subprocess.run([harness, "parse", sc, dump], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
            if r.returncode != 0:
                sys.exit("case %s: ref_harness parse exited with %d: %s" % (name, r.returncode, r.stderr[-500:]))
            with open(dump, "rb") as f:
                b = f.read()
            if len(b) < 80 or (len(b) - 80) % 100:
                sys.exit("case %s: a dump of %d bytes" % (name, len(b)))
            b = _loader_cases.mask_unset(text, b)   # the fields no line wrote: the stack's, not the parse's
            err = r.stderr.decode("latin-1")
            assert err == "" or err.endswith("\n"), (name, err)
            out[name] = {"text_md5": _loader_cases.text_md5(name), "dump": b.hex(), "stderr": err.split("\n")[:-1]}
        rendered = []   # written here first: a check that fails leaves tests/golden as it was
        for name, text in _loader_cases.RENDERED.items():
            with open(sc, "wb") as f:
                f.write(text)
            ppm, radf = os.path.join(tmp, "img_%s.ppm" % render_name(name)), os.path.join(tmp, "rad_%s.f32" % render_name(name))
            rendered += [ppm, radf]
            r = subprocess.run([harness, "render", sc, ppm, radf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
            if r.returncode != 0:
                sys.exit("case %s: ref_harness render exited with %d: %s" % (name, r.returncode, r.stderr[-500:]))
            with open(radf, "rb") as f:
                raw = f.read()
            rad = struct.unpack("<%df" % (len(raw) // 4), raw)
            if len(rad) != 12 * 8 * 3:
                sys.exit("case %s: %d radiance values, not a 12 x 8 frame's" % (name, len(rad)))
            if not all(abs(v) < float("inf") for v in rad):   # (false for a NaN too)
                sys.exit("case %s: the reference's radiance is not finite; replace the case" % name)
            if len(set(rad)) < 8:
                sys.exit("case %s: an all but uniform frame shows no parse" % name)
        missing = set(_loader_cases.CASES) - set(out)
        assert not missing, missing
        for f in rendered:
            shutil.copyfile(f, os.path.join(HERE, os.path.basename(f)))
    with open(OUT, "w") as f:
        json.dump({"format": "header 80 B + 100 B per primitive; see oracle/ref_harness.cpp (parse)", "cases": out}, f,
                  indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, %d rendered" % (OUT, len(out), len(_loader_cases.RENDERED)))


if __name__ == "__main__":
    main()
