// rayq.cpp -- the ray-query engine's host side (pt_rayq_*, pt_intersect): closest-hit queries for
// rays the caller supplies, on the scene's device copy, without a session.
#include <string.h>

#include "api_internal.h"

static_assert(sizeof(pt_ray) == sizeof(pt::RayRec) && sizeof(pt_ray_hit) == sizeof(pt::RayHit) && sizeof(pt_ray) == 24 &&
                  sizeof(pt_ray_hit) == 24,
              "ray / hit records: ABI and device layouts differ");

using namespace pti;

extern "C" {

int pt_rayq_create(pt_scene* s, int device, uint64_t max_rays, pt_rayq** out) {
    return qctx_create(s, device, max_rays, "max_rays", out, [&](pt_rayq* q, const DevScene& ds, uint32_t cus) {
        const LaneWords w = lane_words(s);
        if (const int rc = rays_shape(q, w, cus)) return rc;
        // the arena's tail: the exact list (max_rays words)
        if (const int rc = qctx_alloc(q, PT_RAYS_CTL_BYTES, (size_t)max_rays * 4u, "ray-query", PT_E_HIP)) return rc;
        q->p.S = device_view(s, ds);
        q->p.head = reinterpret_cast<unsigned long long*>(q->arena);
        q->p.exact_n = reinterpret_cast<uint32_t*>(q->arena + 8);
        q->p.counters = q->counters;
        q->p.exact = reinterpret_cast<uint32_t*>(q->arena + PT_RAYS_CTL_BYTES + kQCtrBytes);
        q->p.aux_words = w.aux_words;
        q->p.dfs_words = w.dfs_words;
        q->p.service = (uint32_t)std::min(64, std::max(1, tune_int("rays_service", PT_RAYS_SERVICE)));
        return (int)PT_OK;
    });
}

int pt_rayq_run(pt_rayq* q, void* stream, uint64_t n, const pt_ray* dev_rays, pt_ray_hit* dev_hits) {
    if (!q) return fail(PT_E_INVALID, "null ray-query context");
    if (n > q->max_items) return fail(PT_E_INVALID, "more rays than the context's max_rays");
    if (n == 0) return PT_OK;
    if (!dev_rays || !dev_hits) return fail(PT_E_INVALID, "null ray or hit buffer");
    HIP_TRY(hipSetDevice(q->dev));
    // one run at a time: the control block and the exact list are the context's
    if (const int rc = q->t.settle()) return rc;
    pt::RaysParams p = q->p;
    p.rays = reinterpret_cast<const pt::RayRec*>(dev_rays);
    p.hits = reinterpret_cast<pt::RayHit*>(dev_hits);
    p.n = (uint32_t)n;
    const RunShape sh = qctx_shape(q, n);
    p.batch = sh.batch;
    HIP_TRY(pt_launch_rays(p, sh.grid, q->block, static_cast<hipStream_t>(stream), q->t.e0, q->t.e1));
    q->t.pending = true;
    return PT_OK;
}

int pt_rayq_stats(pt_rayq* q, pt_stats* st) { return qctx_stats(q, 8u, st); }

void pt_rayq_free(pt_rayq* q) { qctx_free(q); }

int pt_intersect(pt_scene* s, int device, uint64_t n, const pt_ray* rays, pt_ray_hit* hits, pt_stats* stats) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (n > 0 && (!rays || !hits)) return fail(PT_E_INVALID, "null ray or hit buffer");
    return run_chunks<pt_rayq>(
        s, device, n, stats, {pt_rayq_create, pt_rayq_stats, pt_rayq_free}, sizeof(pt_ray), sizeof(pt_ray_hit), PT_E_HIP,
        "ray / hit buffers: hipMalloc failed",
        [&](void* const* d, uint64_t at, uint64_t m) { return copy_up(d[0], rays + at, m * sizeof(pt_ray), "ray upload"); },
        [&](pt_rayq* q, void* const* d, uint64_t m) {
            return pt_rayq_run(q, nullptr, m, static_cast<const pt_ray*>(d[0]), static_cast<pt_ray_hit*>(d[1]));
        },
        [&](void* const* d, uint64_t at, uint64_t m) { return copy_down(hits + at, d[1], m * sizeof(pt_ray_hit), "hit download"); });
}

}  // extern "C"
