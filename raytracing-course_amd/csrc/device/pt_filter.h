// pt_filter.h -- the guided filter of a frame (pt_filter.hip, host/filtq.cpp): an edge-stopping
// a-trous wavelet over the radiance, its weights made from the first-hit features of the pixels
// (normal, depth, albedo, a class) and from the colours themselves.  The definition is the comment of
// include/pt.h's section "guided filter"; this file is that definition as code.  Host and device
// compile the same functions (pt_selftest_filter_host runs them without a device).  DESIGN.md §4.12.
//
// f32 throughout, every operation rounded (-ffp-contract=off: no FMA), in the order written here, so
// that a float32 restatement agrees bit for bit.  No transcendental function; one IEEE divide per tap.
#pragma once
#include "pt_feats.h"

namespace pt {

// a pixel's guide, 32 B, moved as two 16-B pieces: {n.x, n.y, n.z, t} {albedo.rgb, cls}
struct FilterGuide { uint4 w[2]; };

// The guide of a feature record.  cls: 0 on a miss, else 1 + material + 4 * (the primitive emits).
// n, t and albedo are the record's words (a record the library made holds zeros there on a miss).
PT_HD void filter_guide(const Feature& f, FilterGuide& g) {
    const bool hit = (int32_t)f.w[0].x >= 0;
    const bool emits = u2f(f.w[2].z) != 0.f || u2f(f.w[2].w) != 0.f || u2f(f.w[3].x) != 0.f;
    const uint32_t cls = hit ? 1u + f.w[3].y + (emits ? 4u : 0u) : 0u;
    g.w[0] = make_uint4(f.w[0].z, f.w[0].w, f.w[1].x, f.w[0].y);
    g.w[1] = make_uint4(f.w[1].z, f.w[1].w, f.w[2].x, cls);
}

// pt_filter_opts' layouts
enum : uint32_t { FILTER_ROWMAJOR = 0u, FILTER_TILES = 1u };
constexpr uint32_t FILTER_MAX_LEVELS = 8u, FILTER_MAX_POW2 = 8u;
// a frame's pixels are indexed in 32 bits, 16 B each at the most
constexpr unsigned long long FILTER_MAX_PIXELS = 1ull << 27;

PT_HD bool filter_finite1(float v) { return (f2u(v) & 0x7f800000u) != 0x7f800000u; }
PT_HD bool filter_opts_ok(uint32_t levels, float sigma_c, float sigma_z, float sigma_a, uint32_t normal_pow2,
                          uint32_t layout) {
    // (a NaN sigma fails its comparison)
    return levels >= 1u && levels <= FILTER_MAX_LEVELS && sigma_c >= 0.f && filter_finite1(sigma_c) && sigma_z >= 0.f &&
           filter_finite1(sigma_z) && sigma_a >= 0.f && filter_finite1(sigma_a) && normal_pow2 <= FILTER_MAX_POW2 &&
           layout <= FILTER_TILES;
}

// 1 / g for a positive g, else 0: a select, so that a NaN takes 0 (a sigma of 0 switches its weight off)
PT_HD float filter_inv(float g) { return g > 0.f ? 1.f / g : 0.f; }

// one level's constants: the step, 1 / (sigma_c 2^-L)^2, 1 / sigma_a^2, sigma_z, the normal's squarings
struct FilterLevel {
    uint32_t s;
    float ic, ia, sigma_z;
    uint32_t pow2;
};
PT_HD FilterLevel filter_level(uint32_t L, float sigma_c, float sigma_z, float sigma_a, uint32_t normal_pow2) {
    FilterLevel lv;
    lv.s = 1u << L;
    const float sc = sigma_c * u2f((127u - L) << 23);   // 2^-L
    lv.ic = filter_inv(sc * sc);
    lv.ia = filter_inv(sigma_a * sigma_a);
    lv.sigma_z = sigma_z;
    lv.pow2 = normal_pow2;
    return lv;
}

// K = {1/16, 1/4, 3/8, 1/4, 1/16} at d = -2 .. 2
PT_HD float filter_k(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// a pixel's colour at a level and whether its three channels are finite
struct FilterColour {
    float r, g, b;
    uint32_t finite;
};
PT_HD FilterColour filter_colour(float r, float g, float b) {
    return FilterColour{r, g, b, (filter_finite1(r) && filter_finite1(g) && filter_finite1(b)) ? 1u : 0u};
}

// where a level reads its colours: the caller's 12-B pixels row-major ...
struct FilterSrcRows {
    const float* in;
    uint32_t w;
    PT_HD FilterColour operator()(uint32_t x, uint32_t y) const {
        const float* p = in + 3u * (y * w + x);
        return filter_colour(p[0], p[1], p[2]);
    }
};
// ... or as a world-1 session packs them (16 x 16 tiles row-major, a tile's pixels row-major, edge tiles
// padded: what pt_unpack_tiles_f32 reads) ...
struct FilterSrcTiles {
    const float* in;
    uint32_t tiles_x;
    PT_HD FilterColour operator()(uint32_t x, uint32_t y) const {
        const float* p = in + 3u * ((((y >> 4) * tiles_x + (x >> 4)) << 8) + ((y & 15u) << 4) + (x & 15u));
        return filter_colour(p[0], p[1], p[2]);
    }
};
// ... or the previous level's 16-B colours, row-major, the finite flag in the fourth word
struct FilterSrcLevel {
    const uint4* c;
    uint32_t w;
    PT_HD FilterColour operator()(uint32_t x, uint32_t y) const {
        const uint4 v = c[y * w + x];
        return FilterColour{u2f(v.x), u2f(v.y), u2f(v.z), v.w};
    }
};
PT_HD uint4 filter_pack(const FilterColour& c) { return make_uint4(f2u(c.r), f2u(c.g), f2u(c.b), c.finite); }

// One level for pixel (x, y) of a w x h window.  guides: row-major.  A pixel whose colour is not finite
// keeps its words.  Otherwise the 25 taps in the definition's order -- dy outer, dx inner, the centre in
// its place with the weight 9/64 --; a tap outside the window, of another class or with a non-finite
// colour is loaded from the centre instead and enters with the weight 0 and the colour 0, which adds
// nothing, bit for bit.
template <class Src>
PT_HD FilterColour filter_pixel(const Src& src, const FilterGuide* guides, uint32_t w, uint32_t h, uint32_t x, uint32_t y,
                                const FilterLevel& lv) {
    const FilterColour cp = src(x, y);
    if (!cp.finite) return cp;
    const uint4 gp0 = guides[y * w + x].w[0], gp1 = guides[y * w + x].w[1];
    const float npx = u2f(gp0.x), npy = u2f(gp0.y), npz = u2f(gp0.z), tp = u2f(gp0.w);
    const float ap0 = u2f(gp1.x), ap1 = u2f(gp1.y), ap2 = u2f(gp1.z);
    const uint32_t clsp = gp1.w;
    float gz = lv.sigma_z * tp;
    gz = gz * gz;
    const float iz = filter_inv(gz);
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, ws = 0.f;
    // A row of five taps at a time, in three steps: the row's loads and normal terms (fifteen 16-B loads
    // in flight per lane; all 25 taps unrolled take every register a lane can have), the squarings of
    // the five terms in one loop (a loop per tap would make each tap wait for its own loads), the weights
    // and sums in the taps' order.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int dy = -2; dy <= 2; ++dy) {
        uint4 gq0[5], gq1[5];
        FilterColour cq[5];
        bool keep[5];
        float d[5];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < 5; ++j) {
            // (below 0 wraps past w, h; the centre's own entry is loaded like a tap's and not used)
            const uint32_t qx = x + (uint32_t)(j - 2) * lv.s, qy = y + (uint32_t)dy * lv.s;
            const bool inside = qx < w && qy < h;
            const uint32_t lx = inside ? qx : x, ly = inside ? qy : y;
            gq0[j] = guides[ly * w + lx].w[0];
            gq1[j] = guides[ly * w + lx].w[1];
            cq[j] = src(lx, ly);
            // (no short circuit: the words are part of the pieces loaded anyway)
            keep[j] = inside & (gq1[j].w == clsp) & (cq[j].finite != 0u);
            const float dn = (npx * u2f(gq0[j].x) + npy * u2f(gq0[j].y)) + npz * u2f(gq0[j].z);
            d[j] = dn > 0.f ? dn : 0.f;
        }
        for (uint32_t k = 0u; k < lv.pow2; ++k) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int j = 0; j < 5; ++j) d[j] = d[j] * d[j];
        }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < 5; ++j) {
            if (j == 2 && dy == 0) {
                const float wc = 0.140625f;   // 9/64, by definition
                acc0 = acc0 + wc * cp.r;
                acc1 = acc1 + wc * cp.g;
                acc2 = acc2 + wc * cp.b;
                ws = ws + wc;
                continue;
            }
            const float wn = clsp == 0u ? 1.f : d[j];
            const float dz = tp - u2f(gq0[j].w), ez = dz * dz;
            const float da0 = ap0 - u2f(gq1[j].x), da1 = ap1 - u2f(gq1[j].y), da2 = ap2 - u2f(gq1[j].z);
            const float ea = (da0 * da0 + da1 * da1) + da2 * da2;
            const float dc0 = cp.r - cq[j].r, dc1 = cp.g - cq[j].g, dc2 = cp.b - cq[j].b;
            const float ec = (dc0 * dc0 + dc1 * dc1) + dc2 * dc2;
            const float D = ((1.f + ez * iz) * (1.f + ea * lv.ia)) * (1.f + ec * lv.ic);
            float wt = (filter_k(dy) * filter_k(j - 2) * wn) / D;
            wt = wt > 0.f ? wt : 0.f;
            wt = keep[j] ? wt : 0.f;
            acc0 = acc0 + wt * (keep[j] ? cq[j].r : 0.f);
            acc1 = acc1 + wt * (keep[j] ? cq[j].g : 0.f);
            acc2 = acc2 + wt * (keep[j] ? cq[j].b : 0.f);
            ws = ws + wt;
        }
    }
    const float inv = 1.f / ws;   // ws >= 9/64
    return filter_colour(acc0 * inv, acc1 * inv, acc2 * inv);
}

// the centre of window pixel i (row-major) of a window at (x0, y0), w wide
PT_HD FeatXY filter_centre(uint32_t x0, uint32_t y0, uint32_t w, uint32_t i) {
    return feature_centre(x0 + i % w, y0 + i / w);
}

struct FilterGuideParams {
    const Feature* feat;   // n records, 16-B aligned
    FilterGuide* guides;
    FeatXY* xy;            // k_filter_centres: the positions of window pixels first .. first + n - 1
    uint32_t n, first;
    uint32_t x0, y0, w;
};

struct FilterParams {
    const FilterGuide* guides;
    const float* in;       // the caller's input (the first level)
    const uint4* src;      // the previous level's colours (the later levels)
    uint4* dst;            // this level's colours (every level but the last)
    float* out;            // the caller's output (the last level), 12-B pixels row-major
    uint8_t* rgb;          // optional: its 8-bit form
    const float* thr;      // the scene's 256 gamma thresholds
    uint32_t w, h, tiles_x;
    FilterLevel lv;
};

}  // namespace pt

// k_filter_centres: the centres of n window pixels; k_filter_guides: n records -> n guides
hipError_t pt_launch_filter_centres(const pt::FilterGuideParams& p, hipStream_t s);
hipError_t pt_launch_filter_guides(const pt::FilterGuideParams& p, hipStream_t s);
// one level: in_kind 0 = the previous level's colours, 1 = the caller's row-major input, 2 = the caller's
// packed tiles; last: writes the caller's output (and rgb) instead of the context's colours
hipError_t pt_launch_filter_level(const pt::FilterParams& p, uint32_t in_kind, bool last, hipStream_t s);
