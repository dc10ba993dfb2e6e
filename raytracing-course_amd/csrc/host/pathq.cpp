// pathq.cpp -- the batch radiance engine's host side (pt_pathq_*, pt_radiance) and pt_camera_rays:
// Scene::RayTrace for rays the caller supplies, on the scene's device copy, without a session
// (DESIGN.md §4.6).
#include <string.h>

#include "api_internal.h"

static_assert(sizeof(pt_path_ray) == sizeof(pt::PathRec) && sizeof(pt_path_out) == sizeof(pt::PathOut) &&
                  sizeof(pt_path_ray) == 32 && sizeof(pt_path_out) == 16,
              "path / radiance records: ABI and device layouts differ");

using namespace pti;

extern "C" {

int pt_pathq_create(pt_scene* s, int device, uint64_t max_paths, pt_pathq** out) {
    return qctx_create(s, device, max_paths, "max_paths", out, [&](pt_pathq* q, const DevScene& ds, uint32_t cus) {
        const LaneWords w = lane_words(s);
        const uint32_t depth = s->hs.depth;   // RAY_DEPTH as prepared (pt_scene_override applies)
        // the arena's tail: the resident lanes' fold records
        size_t fold_bytes = 0;
        if (const int rc = qctx_fold_shape(q, w, cus, depth, pt_paths_occupancy, "k_paths", &fold_bytes)) return rc;
        if (const int rc = qctx_alloc(q, PT_PATHS_CTL_BYTES, fold_bytes, "path-query", PT_E_OOM)) return rc;
        q->p.S = device_view(s, ds);
        q->p.head = reinterpret_cast<unsigned long long*>(q->arena);
        q->p.counters = q->counters;
        q->p.fold = reinterpret_cast<uint4*>(q->arena + PT_PATHS_CTL_BYTES + kQCtrBytes);
        q->p.depth = depth;
        q->p.aux_words = w.aux_words;
        q->p.dfs_words = w.dfs_words;
        q->p.service = (uint32_t)std::min(64, std::max(1, tune_int("paths_service", PT_PATHS_SERVICE)));
        return (int)PT_OK;
    });
}

int pt_pathq_run(pt_pathq* q, void* stream, uint64_t n, const pt_path_ray* dev_in, pt_path_out* dev_out) {
    if (!q) return fail(PT_E_INVALID, "null path-query context");
    if (n > q->max_items) return fail(PT_E_INVALID, "more paths than the context's max_paths");
    if (n == 0) return PT_OK;
    if (!dev_in || !dev_out) return fail(PT_E_INVALID, "null path or radiance buffer");
    // (the kernel moves a record as 16-B pieces)
    if ((reinterpret_cast<uintptr_t>(dev_in) | reinterpret_cast<uintptr_t>(dev_out)) & 15u)
        return fail(PT_E_INVALID, "path and radiance buffers must be 16-byte aligned");
    HIP_TRY(hipSetDevice(q->dev));
    // one run at a time: the control block and the fold records are the context's
    if (const int rc = q->t.settle()) return rc;
    pt::PathsParams p = q->p;
    p.in = reinterpret_cast<const pt::PathRec*>(dev_in);
    p.out = reinterpret_cast<pt::PathOut*>(dev_out);
    p.n = (uint32_t)n;
    const RunShape sh = qctx_shape(q, n);
    p.batch = sh.batch;
    HIP_TRY(pt_launch_paths(p, sh.grid, q->block, static_cast<hipStream_t>(stream), q->t.e0, q->t.e1));
    q->t.pending = true;
    return PT_OK;
}

int pt_pathq_stats(pt_pathq* q, pt_stats* st) { return qctx_stats(q, 8u, st); }

void pt_pathq_free(pt_pathq* q) { qctx_free(q); }

int pt_radiance(pt_scene* s, int device, uint64_t n, const pt_path_ray* in, pt_path_out* out, pt_stats* stats) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (n > 0 && (!in || !out)) return fail(PT_E_INVALID, "null path or radiance buffer");
    return run_chunks<pt_pathq>(
        s, device, n, stats, {pt_pathq_create, pt_pathq_stats, pt_pathq_free}, sizeof(pt_path_ray), sizeof(pt_path_out),
        PT_E_HIP, "path / radiance buffers: hipMalloc failed",
        [&](void* const* d, uint64_t at, uint64_t m) { return copy_up(d[0], in + at, m * sizeof(pt_path_ray), "path upload"); },
        [&](pt_pathq* q, void* const* d, uint64_t m) {
            return pt_pathq_run(q, nullptr, m, static_cast<const pt_path_ray*>(d[0]), static_cast<pt_path_out*>(d[1]));
        },
        [&](void* const* d, uint64_t at, uint64_t m) { return copy_down(out + at, d[1], m * sizeof(pt_path_out), "radiance download"); });
}

int pt_camera_rays(pt_scene* s, uint64_t n, const float* xy, pt_ray* out) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (n > 0 && (!xy || !out)) return fail(PT_E_INVALID, "null coordinate or ray buffer");
    const pt::CamView cam = make_cam(s);
    for (uint64_t i = 0; i < n; ++i) {
        const pt::Ray r = pt::camera_ray(cam, xy[2 * i], xy[2 * i + 1]);
        out[i] = pt_ray{{r.o.x, r.o.y, r.o.z}, {r.d.x, r.d.y, r.d.z}};
    }
    return PT_OK;
}

}  // extern "C"
