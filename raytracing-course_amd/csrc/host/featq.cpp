// featq.cpp -- the first-hit feature engine's host side (pt_featq_*, pt_features) and a session's
// form of it (pt_session_features): for image-plane positions, the closest hit of the camera's
// ray and the hit primitive's scene data, on the scene's device copy.
#include <string.h>

#include "api_internal.h"

static_assert(sizeof(pt_feature) == sizeof(pt::Feature) && sizeof(pt_feature) == 64 && offsetof(pt_feature, n) == 8 &&
                  offsetof(pt_feature, interior) == 20 && offsetof(pt_feature, albedo) == 24 &&
                  offsetof(pt_feature, ior) == 36 && offsetof(pt_feature, emission) == 40 &&
                  offsetof(pt_feature, material) == 52 && offsetof(pt_feature, type) == 56 &&
                  offsetof(pt_feature, reserved) == 60 && sizeof(pt::FeatXY) == 8,
              "feature record: ABI and device layouts differ");
static_assert(offsetof(pt_feature, t) == offsetof(pt_ray_hit, t) && offsetof(pt_feature, n) == offsetof(pt_ray_hit, n) &&
                  offsetof(pt_feature, interior) == offsetof(pt_ray_hit, interior),
              "a feature record starts with its ray's hit record");

namespace pti {
namespace {

// the session's feature context and its pixels' centres, made at the first pt_session_features (a
// session that never asks has the memory and the launches it always had)
int ensure_features(pt_session* ss, uint64_t n) {
    if (ss->feat_q) return PT_OK;
    if (const int rc = ensure_export(ss)) return rc;   // (the export's first record per tile)
    pt_featq* q = nullptr;
    if (const int rc = pt_featq_create(ss->sc, ss->dev, n, &q)) return rc;
    q->p.cam = ss->cam;   // the camera the session renders with
    void* xy = nullptr;
    if (hipMalloc(&xy, n * sizeof(pt::FeatXY)) != hipSuccess) {
        pt_featq_free(q);
        return fail(PT_E_OOM, "device allocation failed (feature positions)");
    }
    pt::FeatPosParams pp;
    memset(&pp, 0, sizeof(pp));
    pp.tm = ss->tm;
    pp.n_tiles_local = ss->n_tiles_local;
    pp.tile_rec = ss->state_tile_rec;
    pp.xy = static_cast<pt::FeatXY*>(xy);
    hipError_t e = pt_launch_feats_positions(pp, ss->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ss->stream);
    if (e != hipSuccess) {
        (void)hipFree(xy);
        pt_featq_free(q);
        return fail(PT_E_HIP, std::string("feature positions: ") + hipGetErrorString(e));
    }
    ss->feat_q = q;
    ss->feat_xy = pp.xy;
    return PT_OK;
}

}  // namespace
}  // namespace pti

using namespace pti;

extern "C" {

int pt_featq_create(pt_scene* s, int device, uint64_t max_points, pt_featq** out) {
    return qctx_create(s, device, max_points, "max_points", out, [&](pt_featq* q, const DevScene& ds, uint32_t cus) {
        // the lanes' aux stacks, the workgroup, the resident grid and the arena's tail: k_rays' rules (rayq.cpp)
        const LaneWords w = lane_words(s);
        if (const int rc = rays_shape(q, w, cus)) return rc;
        if (const int rc = qctx_alloc(q, PT_RAYS_CTL_BYTES, (size_t)max_points * 4u, "feature", PT_E_OOM)) return rc;
        q->p.S = device_view(s, ds);
        q->p.cam = make_cam(s);
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

int pt_featq_run(pt_featq* q, void* stream, uint64_t n, const float* dev_xy, pt_feature* dev_out) {
    if (!q) return fail(PT_E_INVALID, "null feature context");
    if (n > q->max_items) return fail(PT_E_INVALID, "more points than the context's max_points");
    if (n == 0) return PT_OK;
    if (!dev_xy || !dev_out) return fail(PT_E_INVALID, "null position or feature buffer");
    // (the kernel reads a position as one 8-B piece and writes a record as four 16-B pieces)
    if (reinterpret_cast<uintptr_t>(dev_xy) & 7u) return fail(PT_E_INVALID, "the position buffer must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(dev_out) & 15u) return fail(PT_E_INVALID, "the feature buffer must be 16-byte aligned");
    HIP_TRY(hipSetDevice(q->dev));
    // one run at a time: the control block and the exact list are the context's
    if (const int rc = q->t.settle()) return rc;
    pt::FeatsParams p = q->p;
    p.xy = reinterpret_cast<const pt::FeatXY*>(dev_xy);
    p.out = reinterpret_cast<pt::Feature*>(dev_out);
    p.n = (uint32_t)n;
    const RunShape sh = qctx_shape(q, n);
    p.batch = sh.batch;
    HIP_TRY(pt_launch_feats(p, sh.grid, q->block, static_cast<hipStream_t>(stream), q->t.e0, q->t.e1));
    q->t.pending = true;
    return PT_OK;
}

int pt_featq_stats(pt_featq* q, pt_stats* st) { return qctx_stats(q, 8u, st); }

void pt_featq_free(pt_featq* q) { qctx_free(q); }

int pt_features(pt_scene* s, int device, uint64_t n, const float* xy, pt_feature* out, pt_stats* stats) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (n > 0 && (!xy || !out)) return fail(PT_E_INVALID, "null position or feature buffer");
    return run_chunks<pt_featq>(
        s, device, n, stats, {pt_featq_create, pt_featq_stats, pt_featq_free}, sizeof(pt::FeatXY), sizeof(pt_feature),
        PT_E_OOM, "position / feature buffers: hipMalloc failed",
        [&](void* const* d, uint64_t at, uint64_t m) { return copy_up(d[0], xy + 2 * at, m * sizeof(pt::FeatXY), "position upload"); },
        [&](pt_featq* q, void* const* d, uint64_t m) {
            return pt_featq_run(q, nullptr, m, static_cast<const float*>(d[0]), static_cast<pt_feature*>(d[1]));
        },
        [&](void* const* d, uint64_t at, uint64_t m) { return copy_down(out + at, d[1], m * sizeof(pt_feature), "feature download"); });
}

int pt_session_features(pt_session* ss, pt_feature* dev_out, uint64_t cap, pt_stats* st) {
    if (!ss) return fail(PT_E_INVALID, "null session");
    const uint64_t n = owned_pixels(ss);
    if (cap < n) return fail(PT_E_INVALID, "room for " + std::to_string(cap) + " records, the session owns " +
                                               std::to_string(n) + " pixels");
    if (st) memset(st, 0, sizeof(*st));
    if (n == 0) return PT_OK;
    if (!dev_out) return fail(PT_E_INVALID, "null feature buffer");
    if (reinterpret_cast<uintptr_t>(dev_out) & 15u) return fail(PT_E_INVALID, "the feature buffer must be 16-byte aligned");
    HIP_TRY(hipSetDevice(ss->dev));
    // (no flush_trace: the features depend on no pixel's state, a pending pass stays pending)
    if (const int rc = ensure_features(ss, n)) return rc;
    if (const int rc = pt_featq_run(ss->feat_q, ss->stream, n, reinterpret_cast<const float*>(ss->feat_xy), dev_out))
        return rc;
    // complete on return; the work is the context's to report, never the session's counters
    pt_stats mine;
    if (const int rc = pt_featq_stats(ss->feat_q, &mine)) return rc;
    if (st) *st = mine;
    return PT_OK;
}

int pt_session_features_host(pt_session* ss, pt_feature* out, uint64_t cap, pt_stats* st) {
    if (!ss) return fail(PT_E_INVALID, "null session");
    const uint64_t n = owned_pixels(ss);
    if (cap < n) return fail(PT_E_INVALID, "room for " + std::to_string(cap) + " records, the session owns " +
                                               std::to_string(n) + " pixels");
    if (n == 0) return pt_session_features(ss, nullptr, 0, st);
    if (!out) return fail(PT_E_INVALID, "null feature buffer");
    HIP_TRY(hipSetDevice(ss->dev));
    void* d = nullptr;
    if (hipMalloc(&d, n * sizeof(pt_feature)) != hipSuccess) return fail(PT_E_OOM, "device allocation failed (feature records)");
    int rc = pt_session_features(ss, static_cast<pt_feature*>(d), n, st);
    if (!rc && hipMemcpy(out, d, n * sizeof(pt_feature), hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(PT_E_HIP, "feature download failed");
    (void)hipFree(d);
    return rc;
}

}  // extern "C"
