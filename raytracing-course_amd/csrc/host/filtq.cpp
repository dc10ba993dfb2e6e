// filtq.cpp -- the guided filter's host side (pt_filtq_*, pt_filter) and its host mirror
// (pt_selftest_filter_host): a window's guides, made once from the first-hit features of its pixel
// centres, and one kernel launch per a-trous level over the caller's radiance.
#include <string.h>

#include "api_internal.h"

static_assert(sizeof(pt_filter_opts) == 24 && offsetof(pt_filter_opts, sigma_c) == 4 &&
                  offsetof(pt_filter_opts, normal_pow2) == 16 && offsetof(pt_filter_opts, layout) == 20 &&
                  sizeof(pt::FilterGuide) == 32 && PT_FILTER_ROWMAJOR == pt::FILTER_ROWMAJOR &&
                  PT_FILTER_TILES == pt::FILTER_TILES,
              "filter options and guides: ABI and device layouts differ");

namespace pti {
namespace {

constexpr uint32_t kGuideChunk = 1u << 22;   // guide points per feature run

bool opts_ok(const pt_filter_opts* o) {
    return o && pt::filter_opts_ok(o->levels, o->sigma_c, o->sigma_z, o->sigma_a, o->normal_pow2, o->layout);
}

uint32_t tiles_x_of(uint32_t w) { return (w + 15u) / 16u; }
// the input's floats: the window's pixels, or its tiles with their padding
size_t input_floats(uint32_t w, uint32_t h, uint32_t layout) {
    if (layout == PT_FILTER_TILES) return (size_t)tiles_x_of(w) * ((h + 15u) / 16u) * 256u * 3u;
    return (size_t)w * h * 3u;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + nb && pb < pa + na;
}

int check_window(uint32_t W, uint32_t H, uint32_t& x0, uint32_t& y0, uint32_t& w, uint32_t& h) {
    if (w == 0u) {
        x0 = 0u; y0 = 0u; w = W; h = H;
    }
    if (w == 0u || h == 0u || (uint64_t)x0 + w > W || (uint64_t)y0 + h > H) return fail(PT_E_INVALID, "window outside the image");
    if ((uint64_t)w * h > pt::FILTER_MAX_PIXELS || (h + 15u) / 16u > 65535u)
        return fail(PT_E_INVALID, "window too large for the filter (at most 2^27 pixels, 2^20 rows)");
    return PT_OK;
}

pt::FilterGuide* guides_of(const pt_filtq* q) { return reinterpret_cast<pt::FilterGuide*>(q->arena); }
uint4* colours_of(const pt_filtq* q, uint32_t set) {
    const size_t n = (size_t)q->w * q->h;
    return reinterpret_cast<uint4*>(q->arena + n * sizeof(pt::FilterGuide)) + (size_t)set * n;
}

// the window's guides: a temporary feature context on the pixel centres, chunk by chunk
int make_guides(pt_filtq* q) {
    const uint64_t n = (uint64_t)q->w * q->h;
    const uint32_t cap = (uint32_t)std::min<uint64_t>(n, kGuideChunk);
    pt_featq* fq = nullptr;
    int rc = pt_featq_create(q->sc, q->dev, cap, &fq);
    if (rc) return rc;
    void* xy = nullptr;
    void* feat = nullptr;
    auto done = [&](int code) {
        (void)hipFree(xy);
        (void)hipFree(feat);
        pt_featq_free(fq);
        return code;
    };
    if (hipMalloc(&xy, (size_t)cap * sizeof(pt::FeatXY)) != hipSuccess ||
        hipMalloc(&feat, (size_t)cap * sizeof(pt::Feature)) != hipSuccess)
        return done(fail(PT_E_OOM, "filter guides: hipMalloc failed"));
    for (uint64_t at = 0; at < n; at += cap) {
        pt::FilterGuideParams p;
        memset(&p, 0, sizeof(p));
        p.feat = static_cast<const pt::Feature*>(feat);
        p.guides = guides_of(q);
        p.xy = static_cast<pt::FeatXY*>(xy);
        p.n = (uint32_t)std::min<uint64_t>(cap, n - at);
        p.first = (uint32_t)at;
        p.x0 = q->x0; p.y0 = q->y0; p.w = q->w;
        if (pt_launch_filter_centres(p, nullptr) != hipSuccess) return done(fail(PT_E_HIP, "filter centres: launch failed"));
        if ((rc = pt_featq_run(fq, nullptr, p.n, static_cast<const float*>(xy), static_cast<pt_feature*>(feat)))) return done(rc);
        if (pt_launch_filter_guides(p, nullptr) != hipSuccess) return done(fail(PT_E_HIP, "filter guides: launch failed"));
    }
    if (hipStreamSynchronize(nullptr) != hipSuccess) return done(fail(PT_E_HIP, "filter guides failed"));
    q->guide_points += n;
    return done(PT_OK);
}

// the levels' launch parameters for one run (host mirror: the same sequence)
template <class Launch>
int run_levels(const pt_filter_opts& o, Launch launch) {
    for (uint32_t L = 0; L < o.levels; ++L) {
        const pt::FilterLevel lv = pt::filter_level(L, o.sigma_c, o.sigma_z, o.sigma_a, o.normal_pow2);
        // level 0 reads the caller's input; level L writes set L & 1, which level L + 1 reads
        if (const int rc = launch(lv, L == 0u ? 1u + o.layout : 0u, L + 1u == o.levels, (L + 1u) & 1u, L & 1u)) return rc;
    }
    return PT_OK;
}

}  // namespace
}  // namespace pti

using namespace pti;

extern "C" {

void pt_filter_opts_default(pt_filter_opts* o) {
    if (!o) return;
    o->levels = 3u;
    o->sigma_c = 1.f;
    o->sigma_z = 0.05f;
    o->sigma_a = 0.1f;
    o->normal_pow2 = 5u;
    o->layout = PT_FILTER_ROWMAJOR;
}

int pt_filtq_create(pt_scene* s, int device, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, pt_filtq** out) {
    if (!s || !out) return fail(PT_E_INVALID, "null argument");
    int rc = check_device(device);
    if (rc) return rc;
    if ((rc = pt_scene_prepare(s))) return rc;
    if ((rc = check_window(s->hs.W, s->hs.H, x0, y0, w, h))) return rc;
    DevScene* ds = nullptr;
    double up_ms = 0.0;
    if ((rc = ensure_device_scene(s, device, false, &ds, &up_ms))) return rc;
    auto* q = new pt_filtq();
    q->sc = s;
    q->dev = device;
    q->x0 = x0; q->y0 = y0; q->w = w; q->h = h;
    q->thr = ds->thr;
    auto cleanup = [&](int code) {
        pt_filtq_free(q);
        return code;
    };
    const size_t n = (size_t)w * h;
    if (hipSetDevice(device) != hipSuccess) return cleanup(fail(PT_E_HIP, "hipSetDevice failed"));
    if (hipMalloc(reinterpret_cast<void**>(&q->arena), n * (sizeof(pt::FilterGuide) + 2u * sizeof(uint4))) != hipSuccess)
        return cleanup(fail(PT_E_OOM, "filter buffers: hipMalloc failed"));
    if (!q->t.create()) return cleanup(fail(PT_E_HIP, "filter set-up failed"));
    if ((rc = make_guides(q))) return cleanup(rc);
    *out = q;
    return PT_OK;
}

int pt_filtq_set_features(pt_filtq* q, void* stream, const pt_feature* dev_features) {
    if (!q) return fail(PT_E_INVALID, "null filter context");
    if (!dev_features) return fail(PT_E_INVALID, "null feature buffer");
    if (reinterpret_cast<uintptr_t>(dev_features) & 15u) return fail(PT_E_INVALID, "the feature buffer must be 16-byte aligned");
    HIP_TRY(hipSetDevice(q->dev));
    if (const int rc = q->t.settle()) return rc;   // (the last run still reads the guides)
    pt::FilterGuideParams p;
    memset(&p, 0, sizeof(p));
    p.feat = reinterpret_cast<const pt::Feature*>(dev_features);
    p.guides = guides_of(q);
    p.n = q->w * q->h;
    HIP_TRY(pt_launch_filter_guides(p, static_cast<hipStream_t>(stream)));
    return PT_OK;
}

int pt_filtq_run(pt_filtq* q, void* stream, const pt_filter_opts* opts, const float* dev_in, float* dev_out,
                 uint8_t* dev_rgb) {
    if (!q) return fail(PT_E_INVALID, "null filter context");
    if (!opts_ok(opts))
        return fail(PT_E_INVALID, "filter options: levels 1..8, sigmas >= 0 and finite, normal_pow2 0..8, a known layout");
    if (!dev_in || !dev_out) return fail(PT_E_INVALID, "null input or output buffer");
    if ((reinterpret_cast<uintptr_t>(dev_in) | reinterpret_cast<uintptr_t>(dev_out)) & 3u)
        return fail(PT_E_INVALID, "the input and output buffers must be 4-byte aligned");
    const size_t n = (size_t)q->w * q->h;
    const size_t in_bytes = input_floats(q->w, q->h, opts->layout) * sizeof(float), out_bytes = n * 3u * sizeof(float);
    if (overlap(dev_in, in_bytes, dev_out, out_bytes) ||
        (dev_rgb && (overlap(dev_in, in_bytes, dev_rgb, n * 3u) || overlap(dev_out, out_bytes, dev_rgb, n * 3u))))
        return fail(PT_E_INVALID, "the input and output ranges overlap");
    HIP_TRY(hipSetDevice(q->dev));
    // one run at a time: the levels' colours are the context's
    if (const int rc = q->t.settle()) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    pt::FilterParams p;
    memset(&p, 0, sizeof(p));
    p.guides = guides_of(q);
    p.in = dev_in;
    p.out = dev_out;
    p.rgb = dev_rgb;
    p.thr = q->thr;
    p.w = q->w; p.h = q->h;
    p.tiles_x = tiles_x_of(q->w);
    HIP_TRY(hipEventRecord(q->t.e0, st));
    const int rc = run_levels(*opts, [&](const pt::FilterLevel& lv, uint32_t in_kind, bool last, uint32_t from, uint32_t to) {
        p.lv = lv;
        p.src = colours_of(q, from);
        p.dst = colours_of(q, to);
        HIP_TRY(pt_launch_filter_level(p, in_kind, last, st));
        return (int)PT_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipEventRecord(q->t.e1, st));
    q->t.pending = true;
    return PT_OK;
}

int pt_filtq_stats(pt_filtq* q, pt_stats* st) {
    if (!q || !st) return fail(PT_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(q->dev));
    if (const int rc = q->t.settle()) return rc;
    memset(st, 0, sizeof(*st));
    st->kernel_ms = q->t.kernel_ms;
    st->rays = q->guide_points;
    q->t.kernel_ms = 0.0;
    q->guide_points = 0;
    return PT_OK;
}

void pt_filtq_free(pt_filtq* q) {
    if (!q) return;
    (void)hipSetDevice(q->dev);
    q->t.destroy();   // (waits: the last run still uses the arena)
    (void)hipFree(q->arena);
    delete q;
}

int pt_filter(pt_scene* s, int device, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const pt_filter_opts* opts,
              const float* in, float* out, uint8_t* rgb) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (!opts_ok(opts))
        return fail(PT_E_INVALID, "filter options: levels 1..8, sigmas >= 0 and finite, normal_pow2 0..8, a known layout");
    if (!in || !out) return fail(PT_E_INVALID, "null input or output buffer");
    pt_filtq* q = nullptr;
    int rc = pt_filtq_create(s, device, x0, y0, w, h, &q);
    if (rc) return rc;
    const size_t n = (size_t)q->w * q->h, in_bytes = input_floats(q->w, q->h, opts->layout) * sizeof(float);
    void* din = nullptr;
    void* dout = nullptr;
    void* drgb = nullptr;
    auto done = [&](int code) {
        (void)hipFree(din);
        (void)hipFree(dout);
        (void)hipFree(drgb);
        pt_filtq_free(q);
        return code;
    };
    if (hipMalloc(&din, in_bytes) != hipSuccess || hipMalloc(&dout, n * 12u) != hipSuccess ||
        (rgb && hipMalloc(&drgb, n * 3u) != hipSuccess))
        return done(fail(PT_E_OOM, "filter frame buffers: hipMalloc failed"));
    if (hipMemcpy(din, in, in_bytes, hipMemcpyHostToDevice) != hipSuccess) return done(fail(PT_E_HIP, "radiance upload failed"));
    if ((rc = pt_filtq_run(q, nullptr, opts, static_cast<const float*>(din), static_cast<float*>(dout),
                           static_cast<uint8_t*>(drgb))))
        return done(rc);
    // (the null stream orders these copies after the run)
    if (hipMemcpy(out, dout, n * 12u, hipMemcpyDeviceToHost) != hipSuccess ||
        (rgb && hipMemcpy(rgb, drgb, n * 3u, hipMemcpyDeviceToHost) != hipSuccess))
        return done(fail(PT_E_HIP, "filtered frame download failed"));
    return done(PT_OK);
}

int pt_selftest_filter_host(uint32_t w, uint32_t h, const pt_feature* features, const pt_filter_opts* opts,
                            const float* in, float* out) {
    if (!features || !in || !out) return fail(PT_E_INVALID, "null argument");
    if (!opts_ok(opts))
        return fail(PT_E_INVALID, "filter options: levels 1..8, sigmas >= 0 and finite, normal_pow2 0..8, a known layout");
    if (w == 0u || h == 0u || (uint64_t)w * h > pt::FILTER_MAX_PIXELS) return fail(PT_E_INVALID, "bad frame size");
    const size_t n = (size_t)w * h;
    std::vector<pt::FilterGuide> guides(n);
    for (size_t i = 0; i < n; ++i) {
        pt::Feature f;
        memcpy(&f, features + i, sizeof(f));
        pt::filter_guide(f, guides[i]);
    }
    std::vector<uint4> col[2] = {std::vector<uint4>(opts->levels > 1u ? n : 0u), std::vector<uint4>(opts->levels > 2u ? n : 0u)};
    // k_filter's job, a pixel at a time
    auto level = [&](const auto& src, const pt::FilterLevel& lv, bool last, uint4* dst) {
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const pt::FilterColour c = pt::filter_pixel(src, guides.data(), w, h, x, y, lv);
                const size_t i = (size_t)y * w + x;
                if (last) {
                    out[3 * i] = c.r; out[3 * i + 1] = c.g; out[3 * i + 2] = c.b;
                } else {
                    dst[i] = pt::filter_pack(c);
                }
            }
    };
    return run_levels(*opts, [&](const pt::FilterLevel& lv, uint32_t in_kind, bool last, uint32_t from, uint32_t to) {
        // (level L writes set L & 1: set 1 only exists with three levels or more)
        uint4* dst = last ? nullptr : col[to].data();
        if (in_kind == 1u) level(pt::FilterSrcRows{in, w}, lv, last, dst);
        else if (in_kind == 2u) level(pt::FilterSrcTiles{in, (w + 15u) / 16u}, lv, last, dst);
        else level(pt::FilterSrcLevel{col[from].data(), w}, lv, last, dst);
        return (int)PT_OK;
    });
}

}  // extern "C"
