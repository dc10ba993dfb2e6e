"""Inputs and references of the pt_selftest_math tests (test_math_host.py on the host build of the
device functions, test_math.py on the GPU): the scalar building blocks of pt_core.h / pt_trace.h
against the oracle's own functions (oracle/pt_oracle.cpp: the ones its ray_trace / sample_pixel /
tonemap call, so the image fixtures pin them), numpy's IEEE operations and the committed rng_*.f32.

Every comparison is equality of bit patterns.  The one allowance: where the reference's result is a
NaN, any NaN passes -- IEEE 754 leaves a NaN's sign and payload to the implementation (x86 makes
0xffc00000 of inf - inf, other hardware 0x7fc00000), and nothing in the render reads them.
"""
import functools

import numpy as np

import _util as U

F32, U32 = np.float32, np.uint32
M31 = 2147483647            # minstd_rand's modulus
ONE = 0x3f800000            # bits of 1.0f


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def run(op, records, device):
    return U.ptrace().selftest_math(op, records, device=device)


# ------------------------------------------------------------------ compare --
def _words(a):
    """a record array as uint32 words, one row per record"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), -1)


def _nan_mask(a):
    """per uint32 word of each record: True where the word belongs to a NaN float field"""
    a = np.ascontiguousarray(a)
    n = len(a)
    if a.dtype.names is None:
        flat = a.reshape(n, -1)
        if a.dtype == np.float32:
            return np.isnan(flat)
        if a.dtype == np.float64:
            return np.repeat(np.isnan(flat), 2, axis=1)
        return np.zeros((n, flat.shape[1] * a.dtype.itemsize // 4), bool)
    cols = []
    for name in a.dtype.names:
        cols.append(_nan_mask(np.ascontiguousarray(a[name])))
    return np.concatenate(cols, axis=1)


def assert_same(op, what, records, got, ref):
    """got == ref as bit patterns (a NaN of the reference: any NaN); the message names the op, the
    first differing input as hex words, and both outputs"""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape[0] == ref.shape[0] == len(records), (op, what, got.shape, ref.shape, len(records))
    g, r = _words(got), _words(ref)
    assert g.shape == r.shape, (op, what, g.shape, r.shape)
    ok = (g == r) | (_nan_mask(got) & _nan_mask(ref))
    bad = np.flatnonzero(~ok.all(axis=1))
    if len(bad):
        i = int(bad[0])
        hexw = lambda a: " ".join("%08x" % w for w in _words(np.ascontiguousarray(a))[i][:24])  # noqa: E731
        raise AssertionError("%s vs %s: %d of %d elements differ; first at %d: in = %s | got = %s | want = %s" % (
            op, what, len(bad), len(records), i, hexw(records), hexw(got), hexw(ref)))


# --------------------------------------------------------------------- LOGF --
@functools.lru_cache(None)
def logf_inputs():
    parts = [np.arange(0x100, ONE + 1, 0x100, dtype=np.uint32)]          # every float in (0, 1], low 8 bits 0
    for j in range(16):                                                  # the table's sub-interval breakpoints
        ix = 0x3f330000 + (j << 19)
        if ix > ONE:
            ix -= 1 << 23                                                # ... of the binade below 1
        parts.append(np.arange(ix - 4096, ix + 4096, dtype=np.uint32))
    edges = np.arange(1, 128, dtype=np.uint32) << 23                     # binade edges, a float either side
    parts += [edges - 1, edges, np.minimum(edges + 1, ONE)]
    k = np.arange(0, 24, dtype=np.uint32)                                # subnormals 2^k - 1, 2^k; 2^23 = the
    parts += [np.maximum((U32(1) << k) - 1, 1).astype(np.uint32), U32(1) << k]   # smallest normal
    parts.append(np.array([1, 2, ONE - 1, ONE], np.uint32))
    # r2 of the polar method's pairs, drawn as rng_normal draws them from the oracle's uniforms
    u = U.oracle_rng(12345, 131072)[:131072]
    a = (2.0 * u[0::2].astype(np.float64) - 1.0).astype(F32)
    b = (2.0 * u[1::2].astype(np.float64) - 1.0).astype(F32)
    r2 = (a * a + b * b).astype(F32)
    parts.append(bits(r2[(r2 <= 1) & (r2 != 0)]))
    x = f32(np.concatenate(parts))
    assert ((x > 0) & (x <= 1)).all()
    return x


@functools.lru_cache(None)
def logf_ref():
    x = logf_inputs()
    out = np.zeros_like(x)
    U.oracle().oracle_logf(len(x), U._p(x), U._p(out))
    return out


# ---------------------------------------------------------------------- RNG --
RNG_N = 256


def rng_records(seeds, n):
    rec = np.zeros(len(seeds), U.ptrace().MATH_OPS["RNG"][1])
    rec["seed"] = np.asarray(seeds, np.uint64).astype(np.uint32)
    rec["n"] = n
    return rec


@functools.lru_cache(None)
def rng_seeds():
    k = np.arange(512, dtype=np.int64)
    s = np.concatenate([np.arange(1024), 2**31 - 1 - k, 2**31 - 1 + k, 2**32 - 1 - k,
                        [1920 * 1080 - 1, 3840 * 2160 - 1]])
    return np.unique(s).astype(np.uint32)


def chosen_first_draws():
    """t: the engine's first output.  t - 1 is the integer generate_canonical turns into a float:
    from 2^31 - 64 on it rounds to 2^31, the uniform to 1.0 and the `u >= 1` clamp acts (t within
    64 of 2^31 - 64, up to the largest state 2^31 - 2); t = 1 gives the uniform exactly 0, so
    a = -1 and the pair is rejected."""
    return [1] + list(range(2**31 - 128, 2**31 - 1))


@functools.lru_cache(None)
def chosen_seeds():
    inv = pow(48271, -1, M31)
    seeds = [t * inv % M31 for t in chosen_first_draws()]
    assert all(s * 48271 % M31 == t for s, t in zip(seeds, chosen_first_draws())) and len(seeds) == 128
    return np.array(seeds, np.uint32)


def rng_ref(seeds, n):
    return np.stack([U.oracle_rng(int(s), n) for s in seeds])


# ------------------------------------------------------------ NORMAL3 / COSINE
@functools.lru_cache(None)
def normal3_records():
    rec = np.zeros(2 * 4096, U.ptrace().MATH_OPS["NORMAL3"][1])
    rec["seed"] = np.tile(np.arange(4096, dtype=np.uint32), 2)
    rec["pre"] = np.repeat(np.array([0, 1], np.uint32), 4096)
    return rec


def _vecs(n):
    return np.zeros(n, U.ptrace().MATH_OPS["NORMAL3"][2])


@functools.lru_cache(None)
def normal3_ref():
    rec = normal3_records()
    out = _vecs(len(rec))
    U.oracle().oracle_normal_vecs(len(rec), U._p(rec), U._p(out))
    return out


@functools.lru_cache(None)
def cosine_records():
    """1,024 seeds x both `pre` x 15 normals: the six axes, the eight unit diagonals, and the
    opposite of the stream's own first vector (dir + n is then about 0: the two early returns)"""
    d = np.float32(1) / np.sqrt(np.float32(3))
    fixed = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    fixed += [(sx * d, sy * d, sz * d) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    fixed = np.array(fixed, np.float32)
    seeds = np.arange(1024, dtype=np.uint32)
    first = {}
    for pre in (0, 1):
        r = np.zeros(len(seeds), U.ptrace().MATH_OPS["NORMAL3"][1])
        r["seed"], r["pre"] = seeds, pre
        o = _vecs(len(r))
        U.oracle().oracle_normal_vecs(len(r), U._p(r), U._p(o))
        v = o["v"][:, 0, :]
        k = (np.float32(1) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])).astype(F32)
        first[pre] = (-(v * k[:, None])).astype(F32)
    rec = np.zeros(len(seeds) * 2 * 15, U.ptrace().MATH_OPS["COSINE"][1])
    rec = rec.reshape(2, len(seeds), 15)
    for pre in (0, 1):
        rec[pre]["seed"] = seeds[:, None]
        rec[pre]["pre"] = pre
        rec[pre]["n"][:, :14, :] = fixed[None]
        rec[pre]["n"][:, 14, :] = first[pre]
    return np.ascontiguousarray(rec.reshape(-1))


@functools.lru_cache(None)
def cosine_ref():
    rec = cosine_records()
    out = _vecs(len(rec))
    U.oracle().oracle_sample_cosine(len(rec), U._p(rec), U._p(out))
    return out


# ------------------------------------------------------------------ FRESNEL --
ETAS = [(1, 1.5), (1.5, 1), (1, 0.7), (0.7, 1), (1, 2.4), (2.4, 1), (1, 1)]


@functools.lru_cache(None)
def fresnel_records():
    pos = np.arange(0, ONE + 1, ONE // 65536, dtype=np.uint32)            # [0, 1] at a stride of bits
    neg = pos[1:] | U32(0x80000000)                                       # its mirror in [-1, 0)
    near1 = np.arange(ONE - 4, ONE + 5, dtype=np.uint32)                  # 1 -+ a few ulps
    special = np.concatenate([np.array([0, 1, 0x80000000, 0x80000001], np.uint32), near1, near1 | U32(0x80000000)])
    cosn = f32(np.concatenate([pos, neg, special]))
    rec = np.zeros((len(ETAS), len(cosn)), U.ptrace().MATH_OPS["FRESNEL"][1])
    for k, (e1, e2) in enumerate(ETAS):
        rec[k]["eta1"], rec[k]["eta2"], rec[k]["cosn"] = e1, e2, cosn
    return np.ascontiguousarray(rec.reshape(-1))


@functools.lru_cache(None)
def fresnel_ref():
    rec = fresnel_records()
    out = np.zeros(len(rec), F32)
    U.oracle().oracle_fresnel(len(rec), U._p(rec), U._p(out))
    return out


# ------------------------------------------------------------------ RESOLVE --
RESOLVE_S = [3, 5, 7, 100, 255, 1000, 4096]


def oracle_bytes(mean):
    """the oracle's 8-bit value of each mean (its tonemap works on triples)"""
    mean = np.ascontiguousarray(mean, F32)
    pad = (-len(mean)) % 3
    t = U.oracle_tonemap(np.concatenate([mean, np.zeros(pad, F32)]))
    return t.reshape(-1)[:len(mean)]


@functools.lru_cache(None)
def resolve_step_points():
    """With S = 1 the mean is the sum.  For each of the 255 steps k -> k+1 of the oracle's byte:
    the smallest x in [0, 16] whose byte is > k (bisection on float bits, all steps at once), and
    its two neighbours on each side."""
    k = np.arange(255)
    lo = np.zeros(255, np.int64)
    hi = np.full(255, 0x41800000, np.int64)   # bits of 16.0f
    assert (oracle_bytes(f32(hi.astype(np.uint32))) == 255).all() and oracle_bytes(f32(np.uint32([0])))[0] == 0
    while (lo < hi).any():
        mid = (lo + hi) // 2
        up = oracle_bytes(f32(mid.astype(np.uint32))) > k
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid + 1)
    x = (lo[:, None] + np.arange(-2, 3)[None, :]).reshape(-1)
    return np.maximum(x, 0).astype(np.uint32)


@functools.lru_cache(None)
def resolve_sums():
    return f32(np.arange(1 << 20, dtype=np.uint32) * U32(0x41800000 // (1 << 20)))   # [0, 16) at a stride of bits


def resolve_records(sums, S):
    rec = np.zeros(len(sums), U.ptrace().MATH_OPS["RESOLVE"][1])
    rec["sum"], rec["samples"] = sums, S
    return rec


@functools.lru_cache(None)
def resolve_cases():
    """[(label, records)]: S = 1 on the byte steps, a stride of [0, 16) and the special values; then
    the same stride at every S of RESOLVE_S (one call each)"""
    special = np.array([-0.0, 1e-45, -1e-3, -1.0, 1e18, np.finfo(F32).max, np.inf, -np.inf, np.nan], F32)
    first = np.concatenate([f32(resolve_step_points()), resolve_sums(), special])
    return [("S=1", resolve_records(first, 1))] + [("S=%d" % S, resolve_records(resolve_sums(), S)) for S in RESOLVE_S]


def resolve_ref(rec):
    out = np.zeros(len(rec), U.ptrace().MATH_OPS["RESOLVE"][2])
    with np.errstate(all="ignore"):
        out["mean"] = (np.float32(1) / rec["samples"].astype(F32)) * rec["sum"]
    out["byte"] = oracle_bytes(out["mean"])
    return out


# -------------------------------------------------------------------- ARITH --
@functools.lru_cache(None)
def arith_records():
    """2^16 pairs: random bit patterns; quotients and narrowed values that are subnormal; subnormal
    operands; +-0 and +-inf against everything"""
    rng = np.random.default_rng(20250)
    n = 1 << 14
    rec = np.zeros(4 * n, U.ptrace().MATH_OPS["ARITH"][1])
    a, b, ad, bd = (rec[k].reshape(4, n) for k in ("a", "b", "ad", "bd"))
    # 0: random bit patterns, f32 and f64
    a[0], b[0] = f32(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)), f32(
        rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32))
    ad[0] = rng.integers(0, 1 << 64, n, dtype=np.uint64).view(np.float64)
    bd[0] = rng.integers(0, 1 << 64, n, dtype=np.uint64).view(np.float64)
    # 1: subnormal quotients (f32: |a / b| < 2^-126; f64: < 2^-1022) and f64 values that narrow to
    #    subnormal floats or halfway between two of them
    with np.errstate(all="ignore"):
        a[1] = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-126, -100, n)).astype(F32)
        b[1] = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(1, 40, n)).astype(F32) * rng.choice([-1, 1], n).astype(F32)
        ad[1] = rng.uniform(1, 2, n) * 2.0 ** rng.integers(-1022, -1000, n).astype(np.float64)
        bd[1] = rng.uniform(1, 2, n) * 2.0 ** rng.integers(1, 60, n).astype(np.float64)
        half = n // 2
        ad[1][:half] = rng.integers(1, 1 << 24, half).astype(np.float64) * 2.0 ** -150     # odd multiples: ties
        ad[1][half:half + half // 2] = rng.uniform(1, 2, half // 2) * 2.0 ** rng.integers(-150, -126, half // 2)
        bd[1][:half] = rng.uniform(1, 2, half)
    # 2: subnormal operands
    a[2], b[2] = f32(rng.integers(1, 1 << 23, n).astype(U32)), f32(rng.integers(1, 1 << 23, n).astype(U32))
    b[2][::2] = (rng.uniform(0.25, 4, n // 2)).astype(F32)
    ad[2] = rng.integers(1, 1 << 52, n, dtype=np.uint64).view(np.float64)
    bd[2] = rng.integers(1, 1 << 52, n, dtype=np.uint64).view(np.float64)
    bd[2][::2] = rng.uniform(0.25, 4, n // 2)
    # 3: +-0 and +-inf against themselves and random values
    sp = np.array([0.0, -0.0, np.inf, -np.inf], np.float64)
    a[3], b[3] = a[0], b[0]
    ad[3], bd[3] = ad[0], bd[0]
    i = np.arange(n)
    for arr, arrd, sel in ((a[3], ad[3], i % 3 != 2), (b[3], bd[3], i % 3 != 1)):
        arr[sel] = sp[(i[sel] // 3) % 4].astype(F32)
        arrd[sel] = sp[(i[sel] // 12) % 4]
    return np.ascontiguousarray(rec)


@functools.lru_cache(None)
def arith_ref():
    rec = arith_records()
    out = np.zeros(len(rec), U.ptrace().MATH_OPS["ARITH"][2])
    with np.errstate(all="ignore"):
        out["quot"] = rec["a"] / rec["b"]
        out["root"] = np.sqrt(np.abs(rec["a"]))
        out["quotd"] = rec["ad"] / rec["bd"]
        out["rootd"] = np.sqrt(np.abs(rec["ad"]))
        out["narrow"] = rec["ad"].astype(F32)
        out["round_trip"] = rec["a"].astype(np.float64).astype(F32)
    return out


# ------------------------------------------------- the checks, per device ----
def check_logf(device):
    x = logf_inputs()
    got = run("LOGF", x, device)
    assert_same("LOGF", "oracle_logf", x, got, logf_ref())
    return x, got


def check_rng(device):
    """(records, output) of the three input sets, each one call"""
    outs = []
    M = U.manifest()
    seeds = np.array(sorted(int(s) for s in M["rng"]), np.uint64)
    n = M["rng"][str(int(seeds[0]))]["n"]
    rec = rng_records(seeds, n)
    got = run("RNG", rec, device)
    ref = np.stack([np.fromfile(U.os.path.join(U.GOLDEN, "rng_%d.f32" % s), F32) for s in seeds])
    assert len(seeds) == 8 and n == 2048
    assert_same("RNG", "the reference's rng_*.f32", rec, got, ref)
    outs.append((rec, got))
    for what, s in (("oracle_rng", rng_seeds()), ("oracle_rng (chosen first draws)", chosen_seeds())):
        rec = rng_records(s, RNG_N)
        got = run("RNG", rec, device)
        assert_same("RNG", what, rec, got, rng_ref(s, RNG_N))
        outs.append((rec, got))
    return outs


def check_normal3(device):
    rec = normal3_records()
    got = run("NORMAL3", rec, device)
    ref = normal3_ref()
    for pre in (0, 1):   # (named apart: the two-loop restatement differs between them)
        m = rec["pre"] == pre
        assert_same("NORMAL3", "oracle_normal_vecs, pre=%d" % pre, rec[m], got[m], ref[m])
    return rec, got


def check_cosine(device):
    rec = cosine_records()
    got = run("COSINE", rec, device)
    ref = cosine_ref()
    # the early returns are met: some samples are the normal itself
    same = (ref["v"].view(np.uint32) == rec["n"].view(np.uint32)[:, None, :]).all(axis=2)
    assert same.any() and not same.all()
    assert_same("COSINE", "oracle_sample_cosine", rec, got, ref)
    return rec, got


def check_fresnel(device):
    rec = fresnel_records()
    got = run("FRESNEL", rec, device)
    ref = fresnel_ref()
    assert (ref == -1).any() and ((ref > 0) & (ref < 1)).any()   # both branches
    assert_same("FRESNEL", "oracle_fresnel", rec, got, ref)
    return rec, got


def check_resolve(device):
    outs = []
    for label, rec in resolve_cases():
        got = run("RESOLVE", rec, device)
        assert_same("RESOLVE", "(1.f / S) * sum and oracle_tonemap, " + label, rec, got, resolve_ref(rec))
        outs.append((rec, got))
    return outs


def check_arith(device):
    rec = arith_records()
    got = run("ARITH", rec, device)
    assert_same("ARITH", "numpy IEEE", rec, got, arith_ref())
    return rec, got
