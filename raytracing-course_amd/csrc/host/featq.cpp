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

constexpr size_t kCtrBytes = PT_CTR_COPIES * PT_CTR_STRIDE * sizeof(unsigned long long);
constexpr uint64_t kChunk = 1ull << 22;   // pt_features: points per upload / run / download
constexpr uint32_t kMaxLds = 65536u;      // LDS a workgroup may ask for

// the time of the last run's kernels, once they have finished (also: the control block is free)
int settle(pt_featq* q) {
    if (!q->pending) return PT_OK;
    HIP_TRY(hipEventSynchronize(q->e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, q->e0, q->e1));
    q->kernel_ms += ms;
    q->pending = false;
    return PT_OK;
}

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
    if (!s || !out) return fail(PT_E_INVALID, "null argument");
    if (max_points == 0 || max_points >= (1ull << 32)) return fail(PT_E_INVALID, "max_points must be in [1, 2^32)");
    int rc = check_device(device);
    if (rc) return rc;
    if ((rc = pt_scene_prepare(s))) return rc;
    DevScene* ds = nullptr;
    double up_ms = 0.0;
    if ((rc = ensure_device_scene(s, device, false, &ds, &up_ms))) return rc;
    DevProps props;
    if ((rc = device_props(device, &props))) return rc;
    auto* q = new pt_featq();
    q->sc = s;
    q->dev = device;
    q->max_points = max_points;
    auto cleanup = [&](int code) {
        pt_featq_free(q);
        return code;
    };
    // the lanes' aux stacks, the workgroup and the resident grid: k_rays' rules (rayq.cpp)
    const uint32_t aux_words = std::min<uint32_t>(
        PT_QUERY_SP_MAX, std::max({lane_words(s, PT_TRAVERSAL_REPLAY), s->auxw_stack, 1u}));
    while (q->block > 64u && q->block * 4u * (aux_words + 1u) > kMaxLds) q->block /= 2u;
    q->max_grid = (uint32_t)props.cus * (2048u / q->block);
    const size_t bytes = PT_RAYS_CTL_BYTES + kCtrBytes + (size_t)max_points * 4u;
    if (hipSetDevice(device) != hipSuccess) return cleanup(fail(PT_E_HIP, "hipSetDevice failed"));
    if (hipMalloc(reinterpret_cast<void**>(&q->arena), bytes) != hipSuccess)
        return cleanup(fail(PT_E_OOM, "feature buffers: hipMalloc failed"));
    if (hipMemset(q->arena, 0, PT_RAYS_CTL_BYTES + kCtrBytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipEventCreate(&q->e0) != hipSuccess || hipEventCreate(&q->e1) != hipSuccess)
        return cleanup(fail(PT_E_HIP, "feature set-up failed"));
    q->p.S = device_view(s, *ds);
    q->p.cam = make_cam(s);
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

int pt_featq_run(pt_featq* q, void* stream, uint64_t n, const float* dev_xy, pt_feature* dev_out) {
    if (!q) return fail(PT_E_INVALID, "null feature context");
    if (n > q->max_points) return fail(PT_E_INVALID, "more points than the context's max_points");
    if (n == 0) return PT_OK;
    if (!dev_xy || !dev_out) return fail(PT_E_INVALID, "null position or feature buffer");
    // (the kernel reads a position as one 8-B piece and writes a record as four 16-B pieces)
    if (reinterpret_cast<uintptr_t>(dev_xy) & 7u) return fail(PT_E_INVALID, "the position buffer must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(dev_out) & 15u) return fail(PT_E_INVALID, "the feature buffer must be 16-byte aligned");
    HIP_TRY(hipSetDevice(q->dev));
    // one run at a time: the control block and the exact list are the context's
    if (const int rc = settle(q)) return rc;
    pt::FeatsParams p = q->p;
    p.xy = reinterpret_cast<const pt::FeatXY*>(dev_xy);
    p.out = reinterpret_cast<pt::Feature*>(dev_out);
    p.n = (uint32_t)n;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(q->max_grid, (n + q->block - 1u) / q->block);
    // points a wave reserves per pull of the work counter: k_rays' rule (rayq.cpp)
    const uint64_t waves = (uint64_t)grid * (q->block / 64u);
    p.batch = (uint32_t)std::min<uint64_t>(512u, std::max<uint64_t>(64u, n / (waves * 8u)));
    HIP_TRY(pt_launch_feats(p, grid, q->block, static_cast<hipStream_t>(stream), q->e0, q->e1));
    q->pending = true;
    return PT_OK;
}

int pt_featq_stats(pt_featq* q, pt_stats* st) {
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

void pt_featq_free(pt_featq* q) {
    if (!q) return;
    (void)hipSetDevice(q->dev);
    if (q->pending) (void)hipEventSynchronize(q->e1);   // the last run still reads the arena
    if (q->e0) (void)hipEventDestroy(q->e0);
    if (q->e1) (void)hipEventDestroy(q->e1);
    (void)hipFree(q->arena);
    delete q;
}

int pt_features(pt_scene* s, int device, uint64_t n, const float* xy, pt_feature* out, pt_stats* stats) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (n > 0 && (!xy || !out)) return fail(PT_E_INVALID, "null position or feature buffer");
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return PT_OK;
    const uint64_t cap = std::min(n, kChunk);
    pt_featq* q = nullptr;
    int rc = pt_featq_create(s, device, cap, &q);
    if (rc) return rc;
    void* dx = nullptr;
    void* df = nullptr;
    auto done = [&](int code) {
        (void)hipFree(dx);
        (void)hipFree(df);
        pt_featq_free(q);
        return code;
    };
    if (hipMalloc(&dx, cap * sizeof(pt::FeatXY)) != hipSuccess || hipMalloc(&df, cap * sizeof(pt_feature)) != hipSuccess)
        return done(fail(PT_E_OOM, "position / feature buffers: hipMalloc failed"));
    for (uint64_t at = 0; at < n; at += cap) {
        const uint64_t m = std::min(cap, n - at);
        if (hipMemcpy(dx, xy + 2 * at, m * sizeof(pt::FeatXY), hipMemcpyHostToDevice) != hipSuccess)
            return done(fail(PT_E_HIP, "position upload failed"));
        if ((rc = pt_featq_run(q, nullptr, m, static_cast<const float*>(dx), static_cast<pt_feature*>(df)))) return done(rc);
        // (the null stream orders this copy after the run)
        if (hipMemcpy(out + at, df, m * sizeof(pt_feature), hipMemcpyDeviceToHost) != hipSuccess)
            return done(fail(PT_E_HIP, "feature download failed"));
    }
    if (stats && (rc = pt_featq_stats(q, stats))) return done(rc);
    return done(PT_OK);
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
