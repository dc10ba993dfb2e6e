"""The device code's scalar building blocks (pt_core.h, pt_trace.h) evaluated ON THE GPU by
k_selftest_math (pt_selftest_math, device 0), one launch per call: against the same references
as tests/test_math_host.py (the oracle's functions, numpy's IEEE operations, the reference's
recorded RNG streams) and against the host build's output of the same call, bit for bit.
A compiler or flag change that swaps an IEEE divide or square root for an approximation,
contracts an FMA inside logf_glibc or flushes denormals shows here on the inputs built to meet it
(tests/_math_cases.py), not only where a 48x48 render happens to step on it.
"""
import pytest

import _math_cases as K
import _util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    mod = U.ptrace()
    if not U.gpu_available():
        pytest.fail("GPU tests need a visible gfx950 device")
    return mod


def _vs_host(op, pairs):
    for rec, got in pairs:
        K.assert_same(op, "the host build (device = -1)", rec, got, K.run(op, rec, -1))


def test_logf_gpu(pt):
    _vs_host("LOGF", [K.check_logf(0)])


def test_rng_gpu(pt):
    _vs_host("RNG", K.check_rng(0))


def test_normal3_gpu(pt):
    _vs_host("NORMAL3", [K.check_normal3(0)])


def test_cosine_gpu(pt):
    _vs_host("COSINE", [K.check_cosine(0)])


def test_fresnel_gpu(pt):
    _vs_host("FRESNEL", [K.check_fresnel(0)])


def test_resolve_gpu(pt):
    _vs_host("RESOLVE", K.check_resolve(0))


def test_arith_gpu(pt):
    _vs_host("ARITH", [K.check_arith(0)])
