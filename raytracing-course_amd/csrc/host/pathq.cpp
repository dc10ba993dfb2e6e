// pathq.cpp -- the batch radiance engine's host side (pt_pathq_*, pt_radiance) and pt_camera_rays:
// Scene::RayTrace for rays the caller supplies, on the scene's device copy, without a session
// (DESIGN.md §4.6).
#include <string.h>

#include "api_internal.h"

static_assert(sizeof(pt_path_ray) == sizeof(pt::PathRec) && sizeof(pt_path_out) == sizeof(pt::PathOut) &&
                  sizeof(pt_path_ray) == 32 && sizeof(pt_path_out) == 16,
              "path / radiance records: ABI and device layouts differ");

namespace pti {
namespace {

constexpr size_t kCtrBytes = PT_CTR_COPIES * PT_CTR_STRIDE * sizeof(unsigned long long);
constexpr uint64_t kChunk = 1ull << 22;   // pt_radiance: paths per upload / run / download
constexpr uint32_t kMaxLds = 65536u;      // LDS a workgroup may ask for
// The fold area's bound: RAY_DEPTH x 16 B per resident lane.  A full grid (2,048 lanes on each of
// 256 CUs) at the bench job's RAY_DEPTH 6 takes 48 MiB, at depth 10 80 MiB; 1 GiB holds a full grid
// up to depth 128 and one wave per CU up to depth 4,096.  Beyond it the grid shrinks: the paths
// keep their rate per lane, the chip holds fewer of them.
constexpr uint64_t kFoldMax = 1ull << 30;

// the time of the last run's kernel, once it has finished (also: the control block is free)
int settle(pt_pathq* q) {
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

int pt_pathq_create(pt_scene* s, int device, uint64_t max_paths, pt_pathq** out) {
    if (!s || !out) return fail(PT_E_INVALID, "null argument");
    if (max_paths == 0 || max_paths >= (1ull << 32)) return fail(PT_E_INVALID, "max_paths must be in [1, 2^32)");
    int rc = check_device(device);
    if (rc) return rc;
    if ((rc = pt_scene_prepare(s))) return rc;
    DevScene* ds = nullptr;
    double up_ms = 0.0;
    if ((rc = ensure_device_scene(s, device, false, &ds, &up_ms))) return rc;
    DevProps props;
    if ((rc = device_props(device, &props))) return rc;
    auto* q = new pt_pathq();
    q->sc = s;
    q->dev = device;
    q->max_paths = max_paths;
    auto cleanup = [&](int code) {
        pt_pathq_free(q);
        return code;
    };
    // A lane's LDS column: the aux stack as deep as the wide aux tree can need (so no query outgrows
    // it: Query::sp counts it in 7 bits, pt_scene_prepare rejects deeper trees), or the exact DFS's
    // stack, which runs when the aux stack is dead; and the trash word
    const uint32_t aux_words = std::min<uint32_t>(
        PT_QUERY_SP_MAX, std::max({lane_words(s, PT_TRAVERSAL_REPLAY), s->auxw_stack, 1u}));
    const uint32_t dfs_words = std::max<uint32_t>(s->max_stack, 1u);
    const uint32_t words = std::max(aux_words, dfs_words) + 1u;
    while (q->block > 64u && q->block * 4u * words > kMaxLds) q->block /= 2u;
    if (q->block * 4u * words > kMaxLds) return cleanup(fail(PT_E_SCENE, "a lane's traversal stacks do not fit the LDS"));
    if (hipSetDevice(device) != hipSuccess) return cleanup(fail(PT_E_HIP, "hipSetDevice failed"));
    // the resident grid: what the compiler's registers and the LDS let a CU hold (the waves are
    // persistent: a workgroup beyond that would start when another has left, and find no work)
    int per_cu = 0;
    if (pt_paths_occupancy(q->block, (size_t)q->block * 4u * words, &per_cu) != hipSuccess || per_cu < 1)
        return cleanup(fail(PT_E_HIP, "k_paths does not fit a compute unit"));
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
    if (hipMalloc(reinterpret_cast<void**>(&q->arena), PT_PATHS_CTL_BYTES + kCtrBytes + fold_bytes) != hipSuccess)
        return cleanup(fail(PT_E_OOM, "path-query buffers: hipMalloc failed"));
    if (hipMemset(q->arena, 0, PT_PATHS_CTL_BYTES + kCtrBytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipEventCreate(&q->e0) != hipSuccess || hipEventCreate(&q->e1) != hipSuccess)
        return cleanup(fail(PT_E_HIP, "path-query set-up failed"));
    q->p.S = device_view(s, *ds);
    q->p.head = reinterpret_cast<unsigned long long*>(q->arena);
    q->p.counters = reinterpret_cast<unsigned long long*>(q->arena + PT_PATHS_CTL_BYTES);
    q->p.fold = reinterpret_cast<uint4*>(q->arena + PT_PATHS_CTL_BYTES + kCtrBytes);
    q->p.depth = depth;
    q->p.aux_words = aux_words;
    q->p.dfs_words = dfs_words;
    q->p.service = (uint32_t)std::min(64, std::max(1, tune_int("paths_service", PT_PATHS_SERVICE)));
    *out = q;
    return PT_OK;
}

int pt_pathq_run(pt_pathq* q, void* stream, uint64_t n, const pt_path_ray* dev_in, pt_path_out* dev_out) {
    if (!q) return fail(PT_E_INVALID, "null path-query context");
    if (n > q->max_paths) return fail(PT_E_INVALID, "more paths than the context's max_paths");
    if (n == 0) return PT_OK;
    if (!dev_in || !dev_out) return fail(PT_E_INVALID, "null path or radiance buffer");
    // (the kernel moves a record as 16-B pieces)
    if ((reinterpret_cast<uintptr_t>(dev_in) | reinterpret_cast<uintptr_t>(dev_out)) & 15u)
        return fail(PT_E_INVALID, "path and radiance buffers must be 16-byte aligned");
    HIP_TRY(hipSetDevice(q->dev));
    // one run at a time: the control block and the fold records are the context's
    if (const int rc = settle(q)) return rc;
    pt::PathsParams p = q->p;
    p.in = reinterpret_cast<const pt::PathRec*>(dev_in);
    p.out = reinterpret_cast<pt::PathOut*>(dev_out);
    p.n = (uint32_t)n;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(q->max_grid, (n + q->block - 1u) / q->block);
    // paths a wave reserves per pull of the work counter: an eighth of its share, from a full wave
    // to 512 (same-address atomics serialise chip-wide)
    const uint64_t waves = (uint64_t)grid * (q->block / 64u);
    p.batch = (uint32_t)std::min<uint64_t>(512u, std::max<uint64_t>(64u, n / (waves * 8u)));
    HIP_TRY(pt_launch_paths(p, grid, q->block, static_cast<hipStream_t>(stream), q->e0, q->e1));
    q->pending = true;
    return PT_OK;
}

int pt_pathq_stats(pt_pathq* q, pt_stats* st) {
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

void pt_pathq_free(pt_pathq* q) {
    if (!q) return;
    (void)hipSetDevice(q->dev);
    if (q->pending) (void)hipEventSynchronize(q->e1);   // the last run still uses the arena
    if (q->e0) (void)hipEventDestroy(q->e0);
    if (q->e1) (void)hipEventDestroy(q->e1);
    (void)hipFree(q->arena);
    delete q;
}

int pt_radiance(pt_scene* s, int device, uint64_t n, const pt_path_ray* in, pt_path_out* out, pt_stats* stats) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (n > 0 && (!in || !out)) return fail(PT_E_INVALID, "null path or radiance buffer");
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return PT_OK;
    const uint64_t cap = std::min(n, kChunk);
    pt_pathq* q = nullptr;
    int rc = pt_pathq_create(s, device, cap, &q);
    if (rc) return rc;
    void* di = nullptr;
    void* dout = nullptr;
    auto done = [&](int code) {
        (void)hipFree(di);
        (void)hipFree(dout);
        pt_pathq_free(q);
        return code;
    };
    if (hipMalloc(&di, cap * sizeof(pt_path_ray)) != hipSuccess || hipMalloc(&dout, cap * sizeof(pt_path_out)) != hipSuccess)
        return done(fail(PT_E_HIP, "path / radiance buffers: hipMalloc failed"));
    for (uint64_t at = 0; at < n; at += cap) {
        const uint64_t m = std::min(cap, n - at);
        if (hipMemcpy(di, in + at, m * sizeof(pt_path_ray), hipMemcpyHostToDevice) != hipSuccess)
            return done(fail(PT_E_HIP, "path upload failed"));
        if ((rc = pt_pathq_run(q, nullptr, m, static_cast<const pt_path_ray*>(di), static_cast<pt_path_out*>(dout))))
            return done(rc);
        // (the null stream orders this copy after the run)
        if (hipMemcpy(out + at, dout, m * sizeof(pt_path_out), hipMemcpyDeviceToHost) != hipSuccess)
            return done(fail(PT_E_HIP, "radiance download failed"));
    }
    if (stats && (rc = pt_pathq_stats(q, stats))) return done(rc);
    return done(PT_OK);
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
