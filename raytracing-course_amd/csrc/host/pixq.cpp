// pixq.cpp -- the pixel-sample engine's host side (pt_pixq_*, pt_sample_pixels) and the host-only
// pt_pixel_init / pt_pixel_resolve: Scene::Sample's loop for pixel states the caller owns, on the
// scene's device copy, without a session.
#include <string.h>

#include "api_internal.h"

static_assert(sizeof(pt_pixel_state) == sizeof(pt::PixelRec) && sizeof(pt_pixel_state) == 32 &&
                  offsetof(pt_pixel_state, x) == 8 && offsetof(pt_pixel_state, sum) == 16 &&
                  offsetof(pt_pixel_state, samples) == 28,
              "pixel state: ABI and device layouts differ");

namespace pti {
namespace {

constexpr uint32_t kCtrs = PT_PIXELS_CTR_SAMPLES + 1u;   // CTR_RAYS .. CTR_FALLBACKS_RAY, samples
constexpr size_t kCtrBytes = PT_CTR_COPIES * PT_CTR_STRIDE * sizeof(unsigned long long);
constexpr uint64_t kChunk = 1ull << 22;   // pt_sample_pixels: records per upload / run / download
constexpr uint32_t kMaxLds = 65536u;      // LDS a workgroup may ask for
// the fold area's bound: RAY_DEPTH x 16 B per resident lane, as pathq.cpp has it
constexpr uint64_t kFoldMax = 1ull << 30;

// the time of the last run's kernel, once it has finished (also: the control block is free)
int settle(pt_pixq* q) {
    if (!q->pending) return PT_OK;
    HIP_TRY(hipEventSynchronize(q->e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, q->e0, q->e1));
    q->kernel_ms += ms;
    q->pending = false;
    return PT_OK;
}

}  // namespace
}  // namespace pti

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
    if (!s || !out) return fail(PT_E_INVALID, "null argument");
    if (max_pixels == 0 || max_pixels >= (1ull << 32)) return fail(PT_E_INVALID, "max_pixels must be in [1, 2^32)");
    int rc = check_device(device);
    if (rc) return rc;
    if ((rc = pt_scene_prepare(s))) return rc;
    DevScene* ds = nullptr;
    double up_ms = 0.0;
    if ((rc = ensure_device_scene(s, device, false, &ds, &up_ms))) return rc;
    DevProps props;
    if ((rc = device_props(device, &props))) return rc;
    auto* q = new pt_pixq();
    q->sc = s;
    q->dev = device;
    q->max_pixels = max_pixels;
    auto cleanup = [&](int code) {
        pt_pixq_free(q);
        return code;
    };
    // a lane's LDS column, the resident grid and the fold area: k_paths' rules (pathq.cpp)
    const uint32_t aux_words = std::min<uint32_t>(
        PT_QUERY_SP_MAX, std::max({lane_words(s, PT_TRAVERSAL_REPLAY), s->auxw_stack, 1u}));
    const uint32_t dfs_words = std::max<uint32_t>(s->max_stack, 1u);
    const uint32_t words = std::max(aux_words, dfs_words) + 1u;
    while (q->block > 64u && q->block * 4u * words > kMaxLds) q->block /= 2u;
    if (q->block * 4u * words > kMaxLds) return cleanup(fail(PT_E_SCENE, "a lane's traversal stacks do not fit the LDS"));
    if (hipSetDevice(device) != hipSuccess) return cleanup(fail(PT_E_HIP, "hipSetDevice failed"));
    int per_cu = 0;
    if (pt_pixels_occupancy(q->block, (size_t)q->block * 4u * words, &per_cu) != hipSuccess || per_cu < 1)
        return cleanup(fail(PT_E_HIP, "k_pixels does not fit a compute unit"));
    const uint32_t depth = s->hs.depth;   // RAY_DEPTH as prepared (pt_scene_override applies)
    const uint64_t lane_bytes = (uint64_t)std::max(depth, 1u) * sizeof(uint4);
    q->max_grid = (uint32_t)props.cus * (uint32_t)per_cu;
    if ((uint64_t)q->max_grid * q->block * lane_bytes > kFoldMax) {
        // fewer workgroups, then narrower ones, down to one wave per CU
        q->max_grid = (uint32_t)std::max<uint64_t>((uint64_t)props.cus, kFoldMax / (q->block * lane_bytes));
        while (q->block > 64u && (uint64_t)q->max_grid * q->block * lane_bytes > kFoldMax) q->block /= 2u;
        if ((uint64_t)q->max_grid * q->block * lane_bytes > kFoldMax)
            return cleanup(fail(PT_E_OOM, "RAY_DEPTH too large: the fold records of one wave per compute unit exceed 1 GiB"));
    }
    const size_t fold_bytes = (size_t)q->max_grid * q->block * lane_bytes;
    if (hipMalloc(reinterpret_cast<void**>(&q->arena), PT_PIXELS_CTL_BYTES + kCtrBytes + fold_bytes) != hipSuccess)
        return cleanup(fail(PT_E_OOM, "pixel-sample buffers: hipMalloc failed"));
    if (hipMemset(q->arena, 0, PT_PIXELS_CTL_BYTES + kCtrBytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipEventCreate(&q->e0) != hipSuccess || hipEventCreate(&q->e1) != hipSuccess)
        return cleanup(fail(PT_E_HIP, "pixel-sample set-up failed"));
    q->p.S = device_view(s, *ds);
    q->p.cam = make_cam(s);
    q->p.head = reinterpret_cast<unsigned long long*>(q->arena);
    q->p.counters = reinterpret_cast<unsigned long long*>(q->arena + PT_PIXELS_CTL_BYTES);
    q->p.fold = reinterpret_cast<uint4*>(q->arena + PT_PIXELS_CTL_BYTES + kCtrBytes);
    q->p.depth = depth;
    q->p.aux_words = aux_words;
    q->p.dfs_words = dfs_words;
    q->p.service = (uint32_t)std::min(64, std::max(1, tune_int("pixels_service", PT_PIXELS_SERVICE)));
    *out = q;
    return PT_OK;
}

int pt_pixq_run(pt_pixq* q, void* stream, uint64_t n, pt_pixel_state* dev_state, const uint32_t* dev_counts,
                uint32_t spp) {
    if (!q) return fail(PT_E_INVALID, "null pixel-sample context");
    if (n > q->max_pixels) return fail(PT_E_INVALID, "more records than the context's max_pixels");
    if (n == 0) return PT_OK;
    if (!dev_state) return fail(PT_E_INVALID, "null state buffer");
    // (the kernel moves a record as 16-B pieces, a count as a word)
    if (reinterpret_cast<uintptr_t>(dev_state) & 15u) return fail(PT_E_INVALID, "the state buffer must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(dev_counts) & 3u) return fail(PT_E_INVALID, "the count buffer must be 4-byte aligned");
    HIP_TRY(hipSetDevice(q->dev));
    // one run at a time: the control block and the fold records are the context's
    if (const int rc = settle(q)) return rc;
    pt::PixelsParams p = q->p;
    p.state = reinterpret_cast<pt::PixelRec*>(dev_state);
    p.counts = dev_counts;
    p.spp = spp;
    p.n = (uint32_t)n;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(q->max_grid, (n + q->block - 1u) / q->block);
    // records a wave reserves per pull of the work counter: an eighth of its share, from a full
    // wave to 512 (same-address atomics serialise chip-wide)
    const uint64_t waves = (uint64_t)grid * (q->block / 64u);
    p.batch = (uint32_t)std::min<uint64_t>(512u, std::max<uint64_t>(64u, n / (waves * 8u)));
    HIP_TRY(pt_launch_pixels(p, grid, q->block, static_cast<hipStream_t>(stream), q->e0, q->e1));
    q->pending = true;
    return PT_OK;
}

int pt_pixq_stats(pt_pixq* q, pt_stats* st) {
    if (!q || !st) return fail(PT_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(q->dev));
    if (const int rc = settle(q)) return rc;
    unsigned long long cc[PT_CTR_COPIES * PT_CTR_STRIDE];
    HIP_TRY(hipMemcpy(cc, q->p.counters, sizeof(cc), hipMemcpyDeviceToHost));
    unsigned long long c[kCtrs];
    for (uint32_t k = 0; k < kCtrs; ++k) {
        unsigned long long sum = 0ull;
        for (uint32_t x = 0; x < PT_CTR_COPIES; ++x) sum += cc[PT_CTR_STRIDE * x + k];
        c[k] = sum - q->seen[k];
        q->seen[k] = sum;
    }
    memset(st, 0, sizeof(*st));
    counter_stats(c, st);
    st->samples = c[PT_PIXELS_CTR_SAMPLES];
    st->kernel_ms = q->kernel_ms;
    q->kernel_ms = 0.0;
    // algorithmic bytes per counted unit, as a wavefront session reports them
    st->node_bytes = sizeof(pt::Node);
    st->prim_bytes = 48;
    st->aux_bytes = PT_AUXW * sizeof(pt::AuxSL);
    return PT_OK;
}

void pt_pixq_free(pt_pixq* q) {
    if (!q) return;
    (void)hipSetDevice(q->dev);
    if (q->pending) (void)hipEventSynchronize(q->e1);   // the last run still uses the arena
    if (q->e0) (void)hipEventDestroy(q->e0);
    if (q->e1) (void)hipEventDestroy(q->e1);
    (void)hipFree(q->arena);
    delete q;
}

int pt_sample_pixels(pt_scene* s, int device, uint64_t n, pt_pixel_state* state, const uint32_t* counts, uint32_t spp,
                     pt_stats* stats) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (n > 0 && !state) return fail(PT_E_INVALID, "null state buffer");
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return PT_OK;
    const uint64_t cap = std::min(n, kChunk);
    pt_pixq* q = nullptr;
    int rc = pt_pixq_create(s, device, cap, &q);
    if (rc) return rc;
    void* dst = nullptr;
    void* dct = nullptr;
    auto done = [&](int code) {
        (void)hipFree(dst);
        (void)hipFree(dct);
        pt_pixq_free(q);
        return code;
    };
    if (hipMalloc(&dst, cap * sizeof(pt_pixel_state)) != hipSuccess ||
        (counts && hipMalloc(&dct, cap * sizeof(uint32_t)) != hipSuccess))
        return done(fail(PT_E_HIP, "state / count buffers: hipMalloc failed"));
    for (uint64_t at = 0; at < n; at += cap) {
        const uint64_t m = std::min(cap, n - at);
        if (hipMemcpy(dst, state + at, m * sizeof(pt_pixel_state), hipMemcpyHostToDevice) != hipSuccess ||
            (counts && hipMemcpy(dct, counts + at, m * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess))
            return done(fail(PT_E_HIP, "state upload failed"));
        if ((rc = pt_pixq_run(q, nullptr, m, static_cast<pt_pixel_state*>(dst), static_cast<const uint32_t*>(dct), spp)))
            return done(rc);
        // (the null stream orders this copy after the run)
        if (hipMemcpy(state + at, dst, m * sizeof(pt_pixel_state), hipMemcpyDeviceToHost) != hipSuccess)
            return done(fail(PT_E_HIP, "state download failed"));
    }
    if (stats && (rc = pt_pixq_stats(q, stats))) return done(rc);
    return done(PT_OK);
}

}  // extern "C"
