// pt_selftest.h -- pt_selftest_math's operations: the scalar building blocks of pt_core.h and
// pt_trace.h, one record in and one record out per element, evaluated by the very functions
// the render kernels call.  math_one() is the whole of it: k_selftest_math (pt_selftest.hip)
// runs it one element per thread on the device, selftest.cpp in a loop on the host.
// Tests only; never used by pt_render.
#pragma once
#include "pt_trace.h"

namespace pt {

// op numbers of pt_selftest_math (include/pt.h PT_MATH_*)
enum : uint32_t { MATH_LOGF = 0u, MATH_RNG = 1u, MATH_NORMAL3 = 2u, MATH_COSINE = 3u, MATH_FRESNEL = 4u,
                  MATH_RESOLVE = 5u, MATH_ARITH = 6u, MATH_N = 7u };

struct MathSeedIn { uint32_t seed, pre; };                   // NORMAL3 (RNG: pre = the draws per stream)
struct MathCosineIn { uint32_t seed, pre; float n[3]; };
struct MathVecsOut { float v[8][3]; };                       // 8 consecutive vectors
struct MathFresnelIn { float eta1, eta2, cosn; };
struct MathResolveIn { float sum; uint32_t samples; };
struct MathResolveOut { float mean; uint32_t byte; };
struct MathArithIn { float a, b; double ad, bd; };
struct MathArithOut { float quot, root; double quotd, rootd; float narrow, round_trip; };

// bytes per element (RNG's output: 12 per draw, see math_out_bytes)
PT_HD uint32_t math_in_bytes(uint32_t op) {
    return op == MATH_LOGF ? 4u : op == MATH_RNG || op == MATH_NORMAL3 ? (uint32_t)sizeof(MathSeedIn)
         : op == MATH_COSINE ? (uint32_t)sizeof(MathCosineIn) : op == MATH_FRESNEL ? (uint32_t)sizeof(MathFresnelIn)
         : op == MATH_RESOLVE ? (uint32_t)sizeof(MathResolveIn) : (uint32_t)sizeof(MathArithIn);
}
PT_HD uint32_t math_out_bytes(uint32_t op, uint32_t rng_n) {
    return op == MATH_LOGF || op == MATH_FRESNEL ? 4u : op == MATH_RNG ? 12u * rng_n
         : op == MATH_NORMAL3 || op == MATH_COSINE ? (uint32_t)sizeof(MathVecsOut)
         : op == MATH_RESOLVE ? (uint32_t)sizeof(MathResolveOut) : (uint32_t)sizeof(MathArithOut);
}

// a stream as the integrator meets it: seeded, then `pre` normal draws made (pre odd: a value is saved)
PT_HD Rng math_stream(uint32_t seed, uint32_t pre) {
    Rng R = rng_seed(seed);
    for (uint32_t k = 0; k < pre; ++k) (void)rng_normal(R);
    return R;
}

// element i of `op`: in / out are the calls' whole arrays, thr the gamma thresholds (RESOLVE),
// rng_n the draws per stream (RNG: every element's `pre`)
PT_HD void math_one(uint32_t op, uint64_t i, const void* in, void* out, const float* thr, uint32_t rng_n) {
    if (op == MATH_LOGF) {
        static_cast<float*>(out)[i] = logf_glibc(static_cast<const float*>(in)[i]);
    } else if (op == MATH_RNG) {
        // n uniform draws, n normal draws and n mixed draws, each from a fresh stream
        const uint32_t seed = static_cast<const MathSeedIn*>(in)[i].seed;
        float* o = static_cast<float*>(out) + i * 3ull * rng_n;
        Rng R = rng_seed(seed);
        for (uint32_t k = 0; k < rng_n; ++k) o[k] = rng_uniform(R);
        R = rng_seed(seed);
        for (uint32_t k = 0; k < rng_n; ++k) o[rng_n + k] = rng_normal(R);
        R = rng_seed(seed);
        for (uint32_t k = 0; k < rng_n; ++k) {
            const bool use_u = ((k * 2654435761u) >> 7) & 1u;
            o[2u * rng_n + k] = use_u ? rng_uniform(R) : rng_normal(R);
        }
    } else if (op == MATH_NORMAL3) {
        const MathSeedIn I = static_cast<const MathSeedIn*>(in)[i];
        MathVecsOut& O = static_cast<MathVecsOut*>(out)[i];
        Rng R = math_stream(I.seed, I.pre);
        for (int k = 0; k < 8; ++k) {
            const f3 v = normal01_vec(R);
            O.v[k][0] = v.x; O.v[k][1] = v.y; O.v[k][2] = v.z;
        }
    } else if (op == MATH_COSINE) {
        const MathCosineIn I = static_cast<const MathCosineIn*>(in)[i];
        MathVecsOut& O = static_cast<MathVecsOut*>(out)[i];
        Rng R = math_stream(I.seed, I.pre);
        for (int k = 0; k < 8; ++k) {
            const f3 v = sample_cosine(R, mk3(I.n[0], I.n[1], I.n[2]));
            O.v[k][0] = v.x; O.v[k][1] = v.y; O.v[k][2] = v.z;
        }
    } else if (op == MATH_FRESNEL) {
        const MathFresnelIn I = static_cast<const MathFresnelIn*>(in)[i];
        float sin2, rr;
        static_cast<float*>(out)[i] = fresnel_schlick(I.eta1, I.eta2, I.cosn, sin2, rr) ? rr : -1.f;
    } else if (op == MATH_RESOLVE) {
        const MathResolveIn I = static_cast<const MathResolveIn*>(in)[i];
        MathResolveOut O;
        O.byte = resolve_channel(I.sum, I.samples, thr, O.mean);
        static_cast<MathResolveOut*>(out)[i] = O;
    } else {
        // the operations pt_core.h takes to be IEEE, denormals kept: f32 and f64 divide and
        // square root, and the conversions between the two
        const MathArithIn I = static_cast<const MathArithIn*>(in)[i];
        MathArithOut O;
        O.quot = I.a / I.b;
        O.root = fsqrt(fabs_(I.a));
        O.quotd = I.ad / I.bd;
        O.rootd = sqrt(fabs(I.ad));
        O.narrow = (float)I.ad;
        O.round_trip = (float)(double)I.a;
        static_cast<MathArithOut*>(out)[i] = O;
    }
}

}  // namespace pt

#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
hipError_t pt_launch_selftest_math(uint32_t op, uint64_t n, const void* in, void* out, const float* thr,
                                   uint32_t rng_n, hipStream_t s);
// q_decide (pt_query.h) on n Query records in device memory, in place, a record per lane
hipError_t pt_launch_selftest_decide(uint64_t n, void* states, hipStream_t s);
#endif
