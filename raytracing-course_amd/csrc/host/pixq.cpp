// pixq.cpp -- the pixel-sample engine's host side (pt_pixq_*, pt_sample_pixels) and the host-only
// pt_pixel_init / pt_pixel_resolve: Scene::Sample's loop for pixel states the caller owns, on the
// scene's device copy, without a session.
#include <string.h>

#include "api_internal.h"

static_assert(sizeof(pt_pixel_state) == sizeof(pt::PixelRec) && sizeof(pt_pixel_state) == 32 &&
                  offsetof(pt_pixel_state, x) == 8 && offsetof(pt_pixel_state, sum) == 16 &&
                  offsetof(pt_pixel_state, samples) == 28,
              "pixel state: ABI and device layouts differ");

using namespace pti;

extern "C" {

int pt_pixel_init(pt_scene* s, uint64_t n, const uint32_t* xy, const uint32_t* seeds, pt_pixel_state* out) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (n > 0 && (!xy || !out)) return fail(PT_E_INVALID, "null pixel or state buffer");
    const uint32_t W = s->hs.W, H = s->hs.H;
    for (uint64_t i = 0; i < n; ++i)
        if (xy[2 * i] >= W || xy[2 * i + 1] >= H) return fail(PT_E_INVALID, "pixel outside the image");
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t x = xy[2 * i], y = xy[2 * i + 1];
        const pt::Rng R = pt::rng_seed(seeds ? seeds[i] : y * W + x);   // src/scene.cpp:216
        out[i] = pt_pixel_state{pt::pixel_rng_word(R), pt::pixel_rng_saved(R), x, y, {0.f, 0.f, 0.f}, 0u};
    }
    return PT_OK;
}

int pt_pixel_resolve(pt_scene* s, uint64_t n, const pt_pixel_state* state, float* mean, uint8_t* rgb) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (n > 0 && !state) return fail(PT_E_INVALID, "null state buffer");
    const int rc = pt_scene_prepare(s);   // (the gamma thresholds)
    if (rc) return rc;
    for (uint64_t i = 0; i < n; ++i)
        if (state[i].samples == 0u) return fail(PT_E_INVALID, "a pixel state without samples has no mean");
    for (uint64_t i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) {
            float m;
            const uint32_t b = pt::resolve_channel(state[i].sum[c], state[i].samples, s->thr, m);
            if (mean) mean[3 * i + c] = m;
            if (rgb) rgb[3 * i + c] = (uint8_t)b;
        }
    return PT_OK;
}

int pt_pixq_create(pt_scene* s, int device, uint64_t max_pixels, pt_pixq** out) {
    return qctx_create(s, device, max_pixels, "max_pixels", out, [&](pt_pixq* q, const DevScene& ds, uint32_t cus) {
        // a lane's LDS column, the resident grid and the fold area: k_paths' rules (pathq.cpp)
        const LaneWords w = lane_words(s);
        const uint32_t depth = s->hs.depth;   // RAY_DEPTH as prepared (pt_scene_override applies)
        size_t fold_bytes = 0;
        if (const int rc = qctx_fold_shape(q, w, cus, depth, pt_pixels_occupancy, "k_pixels", &fold_bytes)) return rc;
        if (const int rc = qctx_alloc(q, PT_PIXELS_CTL_BYTES, fold_bytes, "pixel-sample", PT_E_OOM)) return rc;
        q->p.S = device_view(s, ds);
        q->p.cam = make_cam(s);
        q->p.head = reinterpret_cast<unsigned long long*>(q->arena);
        q->p.counters = q->counters;
        q->p.fold = reinterpret_cast<uint4*>(q->arena + PT_PIXELS_CTL_BYTES + kQCtrBytes);
        q->p.depth = depth;
        q->p.aux_words = w.aux_words;
        q->p.dfs_words = w.dfs_words;
        q->p.service = (uint32_t)std::min(64, std::max(1, tune_int("pixels_service", PT_PIXELS_SERVICE)));
        return (int)PT_OK;
    });
}

int pt_pixq_run(pt_pixq* q, void* stream, uint64_t n, pt_pixel_state* dev_state, const uint32_t* dev_counts,
                uint32_t spp) {
    if (!q) return fail(PT_E_INVALID, "null pixel-sample context");
    if (n > q->max_items) return fail(PT_E_INVALID, "more records than the context's max_pixels");
    if (n == 0) return PT_OK;
    if (!dev_state) return fail(PT_E_INVALID, "null state buffer");
    // (the kernel moves a record as 16-B pieces, a count as a word)
    if (reinterpret_cast<uintptr_t>(dev_state) & 15u) return fail(PT_E_INVALID, "the state buffer must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(dev_counts) & 3u) return fail(PT_E_INVALID, "the count buffer must be 4-byte aligned");
    HIP_TRY(hipSetDevice(q->dev));
    // one run at a time: the control block and the fold records are the context's
    if (const int rc = q->t.settle()) return rc;
    pt::PixelsParams p = q->p;
    p.state = reinterpret_cast<pt::PixelRec*>(dev_state);
    p.counts = dev_counts;
    p.spp = spp;
    p.n = (uint32_t)n;
    const RunShape sh = qctx_shape(q, n);
    p.batch = sh.batch;
    HIP_TRY(pt_launch_pixels(p, sh.grid, q->block, static_cast<hipStream_t>(stream), q->t.e0, q->t.e1));
    q->t.pending = true;
    return PT_OK;
}

int pt_pixq_stats(pt_pixq* q, pt_stats* st) {
    unsigned long long c[PT_PIXELS_CTR_SAMPLES + 1u];   // CTR_RAYS .. CTR_FALLBACKS_RAY, samples
    if (const int rc = qctx_stats(q, PT_PIXELS_CTR_SAMPLES + 1u, st, c)) return rc;
    st->samples = c[PT_PIXELS_CTR_SAMPLES];
    return PT_OK;
}

void pt_pixq_free(pt_pixq* q) { qctx_free(q); }

int pt_sample_pixels(pt_scene* s, int device, uint64_t n, pt_pixel_state* state, const uint32_t* counts, uint32_t spp,
                     pt_stats* stats) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (n > 0 && !state) return fail(PT_E_INVALID, "null state buffer");
    // (without counts there is no count buffer: the run gets a null pointer, as the caller gave one)
    return run_chunks<pt_pixq>(
        s, device, n, stats, {pt_pixq_create, pt_pixq_stats, pt_pixq_free}, sizeof(pt_pixel_state),
        counts ? sizeof(uint32_t) : 0u, PT_E_HIP, "state / count buffers: hipMalloc failed",
        [&](void* const* d, uint64_t at, uint64_t m) {
            if (const int rc = copy_up(d[0], state + at, m * sizeof(pt_pixel_state), "state upload")) return rc;
            return counts ? copy_up(d[1], counts + at, m * sizeof(uint32_t), "state upload") : (int)PT_OK;
        },
        [&](pt_pixq* q, void* const* d, uint64_t m) {
            return pt_pixq_run(q, nullptr, m, static_cast<pt_pixel_state*>(d[0]), static_cast<const uint32_t*>(d[1]), spp);
        },
        [&](void* const* d, uint64_t at, uint64_t m) { return copy_down(state + at, d[0], m * sizeof(pt_pixel_state), "state download"); });
}

}  // extern "C"
