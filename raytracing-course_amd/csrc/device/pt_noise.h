// pt_noise.h -- a session's own noise estimate and the adaptive step it plans from it (pt_noise.hip,
// host/noise.cpp): a pixel's noise from its sum now and its sum at an earlier count (its mark), the
// counts a set of options makes of it, and the in-tile neighbour rule.  Host and device compile the
// same functions (pt_selftest_refine_plan runs them without a device).  DESIGN.md §4.10.
//
// f32 throughout, every operation rounded (-ffp-contract=off: no FMA), in the order written here, so
// that a float32 restatement agrees bit for bit.
#pragma once
#include "pt_counts.h"

namespace pt {

// A pixel now is (sum, k): its f32 sum and its own count (a ragged session: S - lag).  Its mark is
// (msum, a): the sum it held at the count a; a = 0 is "no mark".  Without a mark, or with no sample
// since it, there is no estimate.
PT_HD bool noise_has_estimate(uint32_t k, uint32_t a) { return a != 0u && k > a; }

// The noise of a pixel that has an estimate: the distance of its mean now from its mean at the mark,
// summed over the channels, over the root of its brightness (floored at 2^-10; a select, so that a
// NaN brightness takes the floor).  Never negative: finite, +inf or NaN.
PT_HD float noise_estimate(const float sum[3], uint32_t k, const float msum[3], uint32_t a) {
    const float mr = sample_mean(sum[0], k), mg = sample_mean(sum[1], k), mb = sample_mean(sum[2], k);
    const float pr = sample_mean(msum[0], a), pg = sample_mean(msum[1], a), pb = sample_mean(msum[2], a);
    const float d = (fabs_(mr - pr) + fabs_(mg - pg)) + fabs_(mb - pb);
    const float l = (mr + mg) + mb;
    const float lf = (l > 0x1p-10f) ? l : 0x1p-10f;
    return d / fsqrt(lf);
}
PT_HD float noise_none() { return u2f(0x7f800000u); }   // no estimate: +inf
PT_HD float noise_of(const float sum[3], uint32_t k, const float msum[3], uint32_t a) {
    return noise_has_estimate(k, a) ? noise_estimate(sum, k, msum, a) : noise_none();
}
PT_HD bool noise_is_nan(float noise) { return noise != noise; }

// a step's options as the kernels take them (pt_refine_opts, max_samples = 0 replaced by 2^32 - 1)
struct NoiseOpts {
    float threshold;
    uint32_t step, max_samples, spread;
};
PT_HD bool noise_opts_ok(float threshold, uint32_t step, uint32_t spread) {
    return threshold >= 0.f && step != 0u && spread <= 1u;   // (a NaN threshold fails the comparison)
}
PT_HD uint32_t noise_cap(uint32_t max_samples) { return max_samples ? max_samples : 0xffffffffu; }

// strict: false for NaN, true for +inf -- computed, or "no estimate"
PT_HD bool noise_hot(float noise, float threshold) { return noise > threshold; }

// The tile's 256 hot flags as four 64-bit words (bit lane & 63 of word lane >> 6: a wave's ballot);
// padding lanes are never hot.  Whether `lane` or one of its 8 neighbours inside the tile is hot: the
// rule never looks across the tile's border, where another rank's pixels may lie.
PT_HD bool noise_spread(const unsigned long long hot[4], uint32_t lane) {
    const uint32_t x = lane & 15u, y = lane >> 4;
    bool any = false;
    for (uint32_t dy = 0u; dy < 3u; ++dy)
        for (uint32_t dx = 0u; dx < 3u; ++dx) {
            const uint32_t nx = x + dx - 1u, ny = y + dy - 1u;   // (below 0 wraps past 15)
            if (nx < 16u && ny < 16u) {
                const uint32_t l = ny * 16u + nx;
                any = any || ((hot[l >> 6] >> (l & 63u)) & 1ull) != 0ull;
            }
        }
    return any;
}

// the samples a pixel at count k takes in the step (hot2: hot after the spread)
PT_HD uint32_t noise_count(bool nan, bool hot2, uint32_t k, const NoiseOpts& o) {
    if (nan || !hot2 || k >= o.max_samples) return 0u;
    const uint32_t room = o.max_samples - k;
    return o.step < room ? o.step : room;
}
PT_HD bool noise_capped(bool nan, bool hot2, uint32_t k, const NoiseOpts& o) { return hot2 && !nan && k >= o.max_samples; }

// a plan's result block (u64 words, zeroed before k_noise_plan)
enum : uint32_t {
    NR_REFINED = 0u,    // pixels with a count above 0
    NR_SAMPLES = 1u,    // the counts' sum (k_counts_scan's CR_SUM)
    NR_UNMARKED = 2u,   // owned pixels without an estimate
    NR_NONFINITE = 3u,  // owned pixels with a NaN noise
    NR_CAPPED = 4u,     // hot, not NaN, and at max_samples already
    NR_WORST = 5u,      // the bits of the largest finite noise of a pixel that has an estimate
    NR_MAX_TOTAL = 6u,  // k_counts_scan's CR_MAX_TOTAL and CR_NMIN_TOTAL for these counts
    NR_NMIN_TOTAL = 7u,
    NR_WORDS = 8u
};

// what one pixel adds to a plan's result (the kernel reduces the fields over a wave, the hook over all)
struct NoisePixel {
    float noise;
    uint32_t count;
    bool unmarked, nan, capped;
};
PT_HD NoisePixel noise_pixel(float noise, bool estimate, bool hot2, uint32_t k, const NoiseOpts& o) {
    NoisePixel r;
    r.noise = noise;
    r.nan = noise_is_nan(noise);
    r.unmarked = !estimate;
    r.count = noise_count(r.nan, hot2, k, o);
    r.capped = noise_capped(r.nan, hot2, k, o);
    return r;
}
// the pixel's word for NR_WORST (0: nothing to report -- a noise of 0 is the result's default too)
PT_HD uint32_t noise_worst_bits(float noise, bool estimate) {
    return estimate && noise < noise_none() ? f2u(noise) : 0u;   // (NaN and +inf fail the comparison)
}

struct NoiseParams {
    TileMap tm;
    PixelState st;
    uint32_t n_tiles_local;
    const uint32_t* tile_rec;     // per local tile: the export's first record of that tile
    const uint32_t* lag;          // per slot (pt_counts.h; null: a session that was never ragged)
    uint4* mark;                  // per slot: {the sum's three words, the count}; all zero: no mark
    unsigned long long* res;      // plan: NR_* words
    uint32_t S;                   // the session's virtual count
    NoiseOpts o;
    uint32_t classify;            // plan: 0 = the noise alone (pt_session_noise: no options, no result)
    float* noise;                 // plan: per record, in export order (null: not wanted)
    uint32_t* counts;             // plan: the same for the counts; commit: the accepted plan's counts
};

}  // namespace pt

hipError_t pt_launch_noise_mark(const pt::NoiseParams& p, hipStream_t s);
hipError_t pt_launch_noise_plan(const pt::NoiseParams& p, hipStream_t s);
hipError_t pt_launch_noise_commit(const pt::NoiseParams& p, hipStream_t s);
