// rayq.cpp -- the ray-query engine's host side (pt_rayq_*, pt_intersect): closest-hit queries for
// rays the caller supplies, on the scene's device copy, without a session.
#include <string.h>

#include "api_internal.h"

static_assert(sizeof(pt_ray) == sizeof(pt::RayRec) && sizeof(pt_ray_hit) == sizeof(pt::RayHit) && sizeof(pt_ray) == 24 &&
                  sizeof(pt_ray_hit) == 24,
              "ray / hit records: ABI and device layouts differ");

namespace pti {
namespace {

constexpr size_t kCtrBytes = PT_CTR_COPIES * PT_CTR_STRIDE * sizeof(unsigned long long);
constexpr uint64_t kChunk = 1ull << 22;   // pt_intersect: rays per upload / run / download
constexpr uint32_t kMaxLds = 65536u;      // LDS a workgroup may ask for

// the time of the last run's kernels, once they have finished (also: the control block is free)
int settle(pt_rayq* q) {
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

int pt_rayq_create(pt_scene* s, int device, uint64_t max_rays, pt_rayq** out) {
    if (!s || !out) return fail(PT_E_INVALID, "null argument");
    if (max_rays == 0 || max_rays >= (1ull << 32)) return fail(PT_E_INVALID, "max_rays must be in [1, 2^32)");
    int rc = check_device(device);
    if (rc) return rc;
    if ((rc = pt_scene_prepare(s))) return rc;
    DevScene* ds = nullptr;
    double up_ms = 0.0;
    if ((rc = ensure_device_scene(s, device, false, &ds, &up_ms))) return rc;
    DevProps props;
    if ((rc = device_props(device, &props))) return rc;
    auto* q = new pt_rayq();
    q->sc = s;
    q->dev = device;
    q->max_rays = max_rays;
    auto cleanup = [&](int code) {
        pt_rayq_free(q);
        return code;
    };
    // the lanes' aux stacks: as deep as the wide aux tree can need, so no query outgrows its stack
    // (Query::sp counts it in 7 bits; pt_scene_prepare rejects deeper trees)
    const uint32_t aux_words = std::min<uint32_t>(
        PT_QUERY_SP_MAX, std::max({lane_words(s, PT_TRAVERSAL_REPLAY), s->auxw_stack, 1u}));
    while (q->block > 64u && q->block * 4u * (aux_words + 1u) > kMaxLds) q->block /= 2u;
    // every workgroup a CU can hold at 8 waves per SIMD (a workgroup that starts after the work
    // counter has passed n leaves at once)
    q->max_grid = (uint32_t)props.cus * (2048u / q->block);
    const size_t bytes = PT_RAYS_CTL_BYTES + kCtrBytes + (size_t)max_rays * 4u;
    if (hipSetDevice(device) != hipSuccess) return cleanup(fail(PT_E_HIP, "hipSetDevice failed"));
    if (hipMalloc(reinterpret_cast<void**>(&q->arena), bytes) != hipSuccess)
        return cleanup(fail(PT_E_HIP, "ray-query buffers: hipMalloc failed"));
    if (hipMemset(q->arena, 0, PT_RAYS_CTL_BYTES + kCtrBytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipEventCreate(&q->e0) != hipSuccess || hipEventCreate(&q->e1) != hipSuccess)
        return cleanup(fail(PT_E_HIP, "ray-query set-up failed"));
    q->p.S = device_view(s, *ds);
    q->p.head = reinterpret_cast<unsigned long long*>(q->arena);
    q->p.exact_n = reinterpret_cast<uint32_t*>(q->arena + 8);
    q->p.counters = reinterpret_cast<unsigned long long*>(q->arena + PT_RAYS_CTL_BYTES);
    q->p.exact = reinterpret_cast<uint32_t*>(q->arena + PT_RAYS_CTL_BYTES + kCtrBytes);
    q->p.aux_words = aux_words;
    q->p.dfs_words = std::max<uint32_t>(s->max_stack, 1u);
    q->p.service = (uint32_t)std::min(64, std::max(1, tune_int("rays_service", PT_RAYS_SERVICE)));
    *out = q;
    return PT_OK;
}

int pt_rayq_run(pt_rayq* q, void* stream, uint64_t n, const pt_ray* dev_rays, pt_ray_hit* dev_hits) {
    if (!q) return fail(PT_E_INVALID, "null ray-query context");
    if (n > q->max_rays) return fail(PT_E_INVALID, "more rays than the context's max_rays");
    if (n == 0) return PT_OK;
    if (!dev_rays || !dev_hits) return fail(PT_E_INVALID, "null ray or hit buffer");
    HIP_TRY(hipSetDevice(q->dev));
    // one run at a time: the control block and the exact list are the context's
    if (const int rc = settle(q)) return rc;
    pt::RaysParams p = q->p;
    p.rays = reinterpret_cast<const pt::RayRec*>(dev_rays);
    p.hits = reinterpret_cast<pt::RayHit*>(dev_hits);
    p.n = (uint32_t)n;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(q->max_grid, (n + q->block - 1u) / q->block);
    // rays a wave reserves per pull of the work counter: an eighth of its share, from a full wave
    // to 512 (same-address atomics serialise chip-wide: one per ray-sized refill would set the rate)
    const uint64_t waves = (uint64_t)grid * (q->block / 64u);
    p.batch = (uint32_t)std::min<uint64_t>(512u, std::max<uint64_t>(64u, n / (waves * 8u)));
    HIP_TRY(pt_launch_rays(p, grid, q->block, static_cast<hipStream_t>(stream), q->e0, q->e1));
    q->pending = true;
    return PT_OK;
}

int pt_rayq_stats(pt_rayq* q, pt_stats* st) {
    if (!q || !st) return fail(PT_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(q->dev));
    if (const int rc = settle(q)) return rc;
    unsigned long long cc[PT_CTR_COPIES * PT_CTR_STRIDE];
    HIP_TRY(hipMemcpy(cc, q->p.counters, sizeof(cc), hipMemcpyDeviceToHost));
    unsigned long long c[8];
    for (uint32_t k = 0; k < 8u; ++k) {
        unsigned long long sum = 0ull;
        for (uint32_t x = 0; x < PT_CTR_COPIES; ++x) sum += cc[PT_CTR_STRIDE * x + k];
        c[k] = sum - q->seen[k];
        q->seen[k] = sum;
    }
    memset(st, 0, sizeof(*st));
    counter_stats(c, st);
    st->kernel_ms = q->kernel_ms;
    q->kernel_ms = 0.0;
    // algorithmic bytes per counted unit, as a wavefront session reports them
    st->node_bytes = sizeof(pt::Node);
    st->prim_bytes = 48;
    st->aux_bytes = PT_AUXW * sizeof(pt::AuxSL);
    return PT_OK;
}

void pt_rayq_free(pt_rayq* q) {
    if (!q) return;
    (void)hipSetDevice(q->dev);
    if (q->pending) (void)hipEventSynchronize(q->e1);   // the last run still reads the arena
    if (q->e0) (void)hipEventDestroy(q->e0);
    if (q->e1) (void)hipEventDestroy(q->e1);
    (void)hipFree(q->arena);
    delete q;
}

int pt_intersect(pt_scene* s, int device, uint64_t n, const pt_ray* rays, pt_ray_hit* hits, pt_stats* stats) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (n > 0 && (!rays || !hits)) return fail(PT_E_INVALID, "null ray or hit buffer");
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return PT_OK;
    const uint64_t cap = std::min(n, kChunk);
    pt_rayq* q = nullptr;
    int rc = pt_rayq_create(s, device, cap, &q);
    if (rc) return rc;
    void* dr = nullptr;
    void* dh = nullptr;
    auto done = [&](int code) {
        (void)hipFree(dr);
        (void)hipFree(dh);
        pt_rayq_free(q);
        return code;
    };
    if (hipMalloc(&dr, cap * sizeof(pt_ray)) != hipSuccess || hipMalloc(&dh, cap * sizeof(pt_ray_hit)) != hipSuccess)
        return done(fail(PT_E_HIP, "ray / hit buffers: hipMalloc failed"));
    for (uint64_t at = 0; at < n; at += cap) {
        const uint64_t m = std::min(cap, n - at);
        if (hipMemcpy(dr, rays + at, m * sizeof(pt_ray), hipMemcpyHostToDevice) != hipSuccess)
            return done(fail(PT_E_HIP, "ray upload failed"));
        if ((rc = pt_rayq_run(q, nullptr, m, static_cast<const pt_ray*>(dr), static_cast<pt_ray_hit*>(dh)))) return done(rc);
        // (the null stream orders this copy after the run)
        if (hipMemcpy(hits + at, dh, m * sizeof(pt_ray_hit), hipMemcpyDeviceToHost) != hipSuccess)
            return done(fail(PT_E_HIP, "hit download failed"));
    }
    if (stats && (rc = pt_rayq_stats(q, stats))) return done(rc);
    return done(PT_OK);
}

}  // extern "C"
