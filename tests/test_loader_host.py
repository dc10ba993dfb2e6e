"""The scene loader against the reference's own Scene::Load (no GPU).

tests/golden/loader_cases.json holds, for every text of tests/_loader_cases.py, what the unmodified
reference parsed (every field's raw bits, primitives in file order) and what it wrote to stderr.
The library's parse and the CPU restatement's must both equal it byte for byte (apart from the
fields that no line of the file wrote, which the reference leaves to the stack: zeroed on both
sides, _loader_cases.unset_words); the restatement
then judges the threaded parse of a large file on the same full records.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _loader_cases as LC
import _util as U

pt = U.ptrace()

with open(os.path.join(U.GOLDEN, "loader_cases.json")) as _f:
    FIXTURES = json.load(_f)["cases"]

HEADER_FIELDS = ["width", "height", "samples", "ray_depth", "fov_x"] + [
    "%s.%s" % (v, a) for v in ("bg", "cam.pos", "cam.right", "cam.up", "cam.forward") for a in "xyz"]
PRIM_FIELDS = ["type"] + ["%s.%s" % (v, a) for v in ("shape0", "shape1", "shape2", "pos") for a in "xyz"] + [
    "rot.x", "rot.y", "rot.z", "rot.w"] + ["%s.%s" % (v, a) for v in ("col", "emission") for a in "rgb"] + ["material", "ior"]
assert len(HEADER_FIELDS) == 20 and len(PRIM_FIELDS) == 25


def describe(got, want):
    """the fields in which two dumps differ, by name (for the assertion's message)"""
    if len(got) != len(want):
        return "%d primitives, the reference has %d" % ((len(got) - 80) // 100, (len(want) - 80) // 100)
    g, w = np.frombuffer(got, np.uint32), np.frombuffer(want, np.uint32)
    out = []
    for i in np.nonzero(g != w)[0]:
        name = HEADER_FIELDS[i] if i < 20 else "prim %d %s" % ((i - 20) // 25, PRIM_FIELDS[(i - 20) % 25])
        out.append("%s: %08x, the reference has %08x" % (name, g[i], w[i]))
    return "; ".join(out)


def test_fixtures_cover_the_table():
    assert set(FIXTURES) == set(LC.CASES)
    for name in LC.CASES:
        assert FIXTURES[name]["text_md5"] == LC.text_md5(name), "%s changed after its fixture was recorded" % name


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_library_parse_is_the_references(name):
    want = bytes.fromhex(FIXTURES[name]["dump"])
    with pt.Scene.loads(LC.CASES[name]) as s:
        got, warnings = s.selftest_scene_dump()
        n_warnings = s.info["n_warnings"]
    got = LC.mask_unset(LC.CASES[name], got)
    assert got == want, describe(got, want)
    assert warnings == FIXTURES[name]["stderr"]
    assert n_warnings == len(FIXTURES[name]["stderr"])


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_oracle_parse_is_the_references(name):
    want = bytes.fromhex(FIXTURES[name]["dump"])
    got, warnings = U.OracleScene.parse_dump(LC.CASES[name])
    got = LC.mask_unset(LC.CASES[name], got)
    assert got == want, describe(got, want)
    assert warnings == FIXTURES[name]["stderr"]


def _big_text():
    """More than 1 MiB of the cases' own blocks and top-level lines (overflowing and long tokens
    among them), so that the parse runs in several stretches; long filler lines of varying
    length move the stretch cuts through the interesting lines."""
    picks = ["float_overflow_1e50", "float_long_128", "float_long_300_exp", "float_overflow_neg_1e39", "every_command",
             "stale_stream_BG_COLOR", "float_form_1e_plus", "two_type_lines", "float_fast_2p24_plus1", "stale_stream_FOO",
             "float_long_129_exp", "metallic_then_dielectric", "stale_stream_overflow", "float_flt_max_above_half"]
    parts, size, k = [], 0, 0
    while size < (1 << 20) + (1 << 18):
        t = LC.CASES[picks[k % len(picks)]]
        if not t.endswith(b"\n"):
            t += b"\n"
        # (a blank line: every pick then starts at the top level, as in its own file)
        filler = b"\nUNKNOWN_%d %s\n" % (k, b"x" * (37 * k % 211))
        parts += [t, filler]
        size += len(t) + len(filler)
        k += 1
    return b"".join(parts)


OVERFLOW_TOKEN = re.compile(rb"(?<!\S)[+-]?(1e50|1e39)(?!\S)")
LONG_TOKEN = re.compile(rb"(?<!\S)[0-9.e]{128,}(?!\S)")


def test_parallel_parse_full_records():
    """The stretch parse on full records against the restatement (which the fixtures pin): at the
    library's own choice of stretches and at given stretch counts, so that several stretches run
    whatever the machine; and among the cuts taken there are ones whose neighbouring line -- the last
    of one stretch or the first lines of the next -- holds an overflowing token, and a token of 128
    characters or more."""
    text = _big_text()
    assert len(text) > (1 << 20)
    want, want_warnings = U.OracleScene.parse_dump(text)
    assert len(want) > 80 + 100 * 1000
    with pt.Scene.loads(text) as s:
        got, warnings = s.selftest_scene_dump()
    assert got == want, describe(got, want)[:2000]
    assert warnings == want_warnings
    near = {"overflow": 0, "long": 0}
    for stretches, pad in ((1, 0), (2, 0), (3, 1), (7, 0), (16, 0), (16, 4097), (13, 70001)):
        # (the pad shifts every cut: the same scene behind a line of spaces)
        t = (b" " * pad + b"\n" if pad else b"") + text
        s, cuts = pt.Scene.selftest_loads_stretches(t, stretches)
        with s:
            got, warnings = s.selftest_scene_dump()
        assert got == want, "%d stretches: %s" % (stretches, describe(got, want)[:2000])
        assert warnings == want_warnings
        # thousands of blocks: every cut asked for is found, each at the start of a NEW_PRIMITIVE line
        assert len(cuts) == stretches + 1 and cuts[0] == 0 and cuts[-1] == len(t) and cuts == sorted(set(cuts))
        for c in cuts[1:-1]:
            assert t[c - 1:c] == b"\n" and t[c:c + 13] == b"NEW_PRIMITIVE" and t[c + 13:c + 14] in b" \n"
            before = t[:c].rsplit(b"\n", 2)[-2]               # the last line of the stretch that ends here
            after = b"\n".join(t[c:c + 2000].split(b"\n")[1:4])   # the three lines after NEW_PRIMITIVE
            near["overflow"] += bool(OVERFLOW_TOKEN.search(before) or OVERFLOW_TOKEN.search(after))
            near["long"] += bool(LONG_TOKEN.search(before) or LONG_TOKEN.search(after))
    assert near["overflow"] >= 3 and near["long"] >= 3, near


def test_dump_refused_after_prepare():
    with pt.Scene.loads(LC.CASES["every_command"]) as s:
        s.prepare()
        with pytest.raises(pt.PTError) as e:
            s.selftest_scene_dump()
        assert e.value.code == pt.PT_E_INVALID


def test_parser_memory_safety_on_every_prefix(tmp_path):
    """scene_load.cpp alone under AddressSanitizer and UBSan, in a stand-alone program run as a
    child process: every case text and every prefix of it, each in an exactly-sized heap buffer,
    and the stretch cuts on small and on large texts (tests/loader_prefixes_main.cpp).  Sanitizer
    runs belong to the machine without a GPU: where there is a GPU device node the test does not
    build or start the program.  Measured on 16 CPUs: 2.4 s to build, 2.6 s to run."""
    import struct
    if os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer runs are for the CPU-only run")
    exe = str(tmp_path / "loader_prefixes")
    src = os.path.join(U.PKG, "csrc")
    # (the library's host compiler and flags: the scene header takes in device headers that g++ does not accept)
    rocm = os.environ.get("ROCM", "/opt/rocm")
    subprocess.check_call([os.path.join(rocm, "lib", "llvm", "bin", "clang++"), "-std=c++17", "-O1", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-mf16c",
                           "-D__HIP_PLATFORM_AMD__", "-pthread", "-I" + src, "-I" + os.path.join(U.REPO, "include"),
                           "-I" + os.path.join(rocm, "include"),
                           os.path.join(U.REPO, "tests", "loader_prefixes_main.cpp"),
                           os.path.join(src, "host", "scene_load.cpp"), "-o", exe])
    blob = struct.pack("<I", len(LC.CASES)) + b"".join(struct.pack("<I", len(t)) + t for t in LC.CASES.values())
    (tmp_path / "cases.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "cases.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode("latin-1")[-3000:]
    want = sum(len(t) + 1 for t in LC.CASES.values()) + 4 + 9
    assert r.stdout.decode().startswith("inputs=%d " % want), r.stdout
