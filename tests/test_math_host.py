"""The device code's scalar building blocks (pt_core.h, pt_trace.h), compiled for the host and
run through pt_selftest_math(device = -1), against the oracle's own functions, numpy's IEEE
operations and the reference's recorded RNG streams -- bit for bit, no GPU needed.
tests/test_math.py runs the same checks on the GPU; tests/_math_cases.py holds the inputs.
"""
import numpy as np
import pytest

import _math_cases as K
import _util as U

pt = U.ptrace()


def test_ops_mirror_the_abi():
    import re
    hdr = open(U.os.path.join(U.REPO, "include", "pt.h")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"PT_MATH_([A-Z0-9]+) = (\d+)", hdr)}
    assert ids == {k: v[0] for k, v in pt.MATH_OPS.items()} and len(ids) == 7
    dev = open(U.os.path.join(U.PKG, "csrc", "device", "pt_selftest.h")).read()
    assert {m.group(1): int(m.group(2)) for m in re.finditer(r"MATH_([A-Z0-9]+) = (\d+)u", dev) if m.group(1) != "N"} == ids


def test_bad_calls_are_errors():
    x = np.ones(4, np.float32)
    assert pt._lib.pt_selftest_math(-1, 99, 4, U._p(x), U._p(x)) == pt.PT_E_INVALID
    assert pt._lib.pt_selftest_math(-1, 0, 4, None, U._p(x)) == pt.PT_E_INVALID
    rec = K.rng_records([1, 2], 8)
    rec["n"][1] = 9    # one output length per call
    with pytest.raises(pt.PTError):
        pt.selftest_math("RNG", rec)


def test_logf_host():
    K.check_logf(-1)


def test_rng_host():
    K.check_rng(-1)


def test_chosen_first_draws_are_the_edge_cases():
    """the RNG test's chosen seeds do produce what they were chosen for (on the oracle): uniforms
    that the `u >= 1` clamp holds at nextafter(1, 0), and an exact 0"""
    first = K.rng_ref(K.chosen_seeds(), 4)[:, 0]
    t = np.array(K.chosen_first_draws(), np.int64)
    assert first[0] == 0 and t[0] == 1
    top = np.float32(np.nextafter(np.float32(1), np.float32(0)))
    assert (first[t - 1 >= 2**31 - 64] == top).all() and (t - 1 >= 2**31 - 64).sum() == 62
    assert (first[1:][t[1:] - 1 < 2**31 - 64] <= top).all()


def test_normal3_host():
    K.check_normal3(-1)


def test_cosine_host():
    K.check_cosine(-1)


def test_fresnel_host():
    K.check_fresnel(-1)


def test_resolve_host():
    K.check_resolve(-1)


def test_resolve_inputs_bite():
    """the RESOLVE sums tell (1.f / S) * sum from sum / S at every S used (not at a power of two),
    and the S = 1 points sit on every step of the byte"""
    s = K.resolve_sums()
    for S in K.RESOLVE_S:
        differ = ((np.float32(1) / np.float32(S)) * s != s / np.float32(S)).mean()
        assert (differ == 0) if S == 4096 else (differ > 0.1), (S, differ)
    by = K.oracle_bytes(K.f32(K.resolve_step_points())).reshape(255, 5)
    k = np.arange(255)
    assert (by[:, 1] == k).all() and (by[:, 2] == k + 1).all()


def test_arith_host():
    K.check_arith(-1)


@pytest.mark.slow
def test_logf_exhaustive():
    """pt_core.h's claim: logf_glibc equals the host libm's logf (std::log(float), what the
    reference's normal_distribution calls) on EVERY float in (0, 1].  The product evaluates its
    function in chunks of 2^24 (threaded); the oracle compares each chunk with its own std::log
    on up to 16 threads.  The oracle does not link the product."""
    lib = U.oracle()
    bad = 0
    total = 0
    step = 1 << 24
    for lo in range(1, K.ONE + 1, step):
        x = K.f32(np.arange(lo, min(lo + step, K.ONE + 1), dtype=np.uint32))
        got = pt.selftest_math("LOGF", x)
        bad += lib.oracle_logf_mismatches(len(x), U._p(x), U._p(got))
        total += len(x)
    assert total == K.ONE == 1065353216
    assert bad == 0
