// qctx.cpp -- the batch contexts' core: what pt_rayq, pt_featq, pt_pathq and pt_pixq (and, for the
// timer, pt_filtq) share on the host -- the checks and the device copy of a *_create, the lanes'
// stack words, the workgroup that fits the LDS, the resident grid under the fold area's bound, the
// arena and its events, a run's grid and batch, the statistics since the last call, the release.
// Each rule has its one statement here; the creation and the one-shot forms' chunk loop are the
// templates beside the declarations (api_internal.h).  DESIGN.md §4.5.
#include "api_internal.h"

#include "../device/pt_batch.h"

namespace pti {
namespace {

constexpr uint32_t kMaxLds = 65536u;      // LDS a workgroup may ask for
// The fold area's bound: RAY_DEPTH x 16 B per resident lane.  A full grid (2,048 lanes on each of
// 256 CUs) at the bench job's RAY_DEPTH 6 takes 48 MiB, at depth 10 80 MiB; 1 GiB holds a full grid
// up to depth 128 and one wave per CU up to depth 4,096.  Beyond it the grid shrinks: the paths
// keep their rate per lane, the chip holds fewer of them.
constexpr uint64_t kFoldMax = 1ull << 30;

}  // namespace

bool RunTimer::create() { return hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess; }

int RunTimer::settle() {
    if (!pending) return PT_OK;
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    kernel_ms += ms;
    pending = false;
    return PT_OK;
}

void RunTimer::destroy() {
    if (pending) (void)hipEventSynchronize(e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
}

int qctx_open(pt_scene* s, int device, uint64_t max_items, const char* name, DevScene** ds, uint32_t* cus) {
    if (max_items == 0 || max_items >= (1ull << 32)) return fail(PT_E_INVALID, std::string(name) + " must be in [1, 2^32)");
    int rc = check_device(device);
    if (rc) return rc;
    if ((rc = pt_scene_prepare(s))) return rc;
    double up_ms = 0.0;
    if ((rc = ensure_device_scene(s, device, false, ds, &up_ms))) return rc;
    DevProps props;
    if ((rc = device_props(device, &props))) return rc;
    *cus = (uint32_t)props.cus;
    if (hipSetDevice(device) != hipSuccess) return fail(PT_E_HIP, "hipSetDevice failed");
    return PT_OK;
}

LaneWords lane_words(const pt_scene* s) {
    return {std::min<uint32_t>(PT_QUERY_SP_MAX, std::max({lane_words(s, PT_TRAVERSAL_REPLAY), s->auxw_stack, 1u})),
            std::max<uint32_t>(s->max_stack, 1u)};
}

bool fit_block(uint32_t aux_words, uint32_t dfs_words, uint32_t* block) {
    while (*block > 64u && pt::lane_lds_bytes(*block, aux_words, dfs_words) > kMaxLds) *block /= 2u;
    return pt::lane_lds_bytes(*block, aux_words, dfs_words) <= kMaxLds;
}

int rays_shape(QueryCtx* q, LaneWords w, uint32_t cus) {
    // (the aux column alone always fits: aux_words <= PT_QUERY_SP_MAX, 64 lanes x 128 words = 32 KiB;
    // the exact kernel's one wave holds the DFS stack, 64 x 4 x (dfs_words + 1) B)
    uint32_t one_wave = 64u;
    if (!fit_block(w.aux_words, 0u, &q->block) || !fit_block(0u, w.dfs_words, &one_wave))
        return fail(PT_E_SCENE, "a lane's traversal stacks do not fit the LDS");
    q->per_cu = 2048u / q->block;
    q->max_grid = cus * q->per_cu;
    return PT_OK;
}

int fold_shape(uint32_t cus, uint32_t per_cu, uint32_t block, uint32_t depth, GridShape* out) {
    const uint64_t lane_bytes = (uint64_t)std::max(depth, 1u) * sizeof(uint4);
    uint32_t max_grid = cus * per_cu;
    if ((uint64_t)max_grid * block * lane_bytes > kFoldMax) {
        max_grid = (uint32_t)std::max<uint64_t>((uint64_t)cus, kFoldMax / (block * lane_bytes));
        while (block > 64u && (uint64_t)max_grid * block * lane_bytes > kFoldMax) block /= 2u;
        if ((uint64_t)max_grid * block * lane_bytes > kFoldMax)
            return fail(PT_E_OOM, "RAY_DEPTH too large: the fold records of one wave per compute unit exceed 1 GiB");
    }
    *out = GridShape{block, max_grid};
    return PT_OK;
}

int qctx_fold_shape(QueryCtx* q, LaneWords w, uint32_t cus, uint32_t depth,
                    hipError_t (*occupancy)(uint32_t, uint32_t, uint32_t, int*), const char* kernel, size_t* fold_bytes) {
    if (!fit_block(w.aux_words, w.dfs_words, &q->block)) return fail(PT_E_SCENE, "a lane's traversal stacks do not fit the LDS");
    int per_cu = 0;
    if (occupancy(q->block, w.aux_words, w.dfs_words, &per_cu) != hipSuccess || per_cu < 1)
        return fail(PT_E_HIP, std::string(kernel) + " does not fit a compute unit");
    GridShape g;
    if (const int rc = fold_shape(cus, (uint32_t)per_cu, q->block, depth, &g)) return rc;
    q->block = g.block;
    q->max_grid = g.max_grid;
    q->per_cu = (uint32_t)per_cu;
    *fold_bytes = (size_t)g.max_grid * g.block * std::max(depth, 1u) * sizeof(uint4);
    return PT_OK;
}

int qctx_alloc(QueryCtx* q, size_t ctl_bytes, size_t tail_bytes, const char* what, int alloc_fail_code) {
    if (hipMalloc(reinterpret_cast<void**>(&q->arena), ctl_bytes + kQCtrBytes + tail_bytes) != hipSuccess)
        return fail(alloc_fail_code, std::string(what) + " buffers: hipMalloc failed");
    if (hipMemset(q->arena, 0, ctl_bytes + kQCtrBytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess || !q->t.create())
        return fail(PT_E_HIP, std::string(what) + " set-up failed");
    q->counters = reinterpret_cast<unsigned long long*>(q->arena + ctl_bytes);
    return PT_OK;
}

RunShape qctx_shape(const QueryCtx* q, uint64_t n) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>(q->max_grid, (n + q->block - 1u) / q->block);
    const uint64_t waves = (uint64_t)grid * (q->block / 64u);
    return {grid, (uint32_t)std::min<uint64_t>(512u, std::max<uint64_t>(64u, n / (waves * 8u)))};
}

int qctx_stats(QueryCtx* q, uint32_t n_counters, pt_stats* st, unsigned long long* c) {
    if (!q || !st) return fail(PT_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(q->dev));
    if (const int rc = q->t.settle()) return rc;
    unsigned long long cc[PT_CTR_COPIES * PT_CTR_STRIDE];
    HIP_TRY(hipMemcpy(cc, q->counters, sizeof(cc), hipMemcpyDeviceToHost));
    unsigned long long mine[9];
    if (!c) c = mine;
    for (uint32_t k = 0; k < n_counters; ++k) {
        unsigned long long sum = 0ull;
        for (uint32_t x = 0; x < PT_CTR_COPIES; ++x) sum += cc[PT_CTR_STRIDE * x + k];
        c[k] = sum - q->seen[k];
        q->seen[k] = sum;
    }
    memset(st, 0, sizeof(*st));
    counter_stats(c, st);
    st->kernel_ms = q->t.kernel_ms;
    q->t.kernel_ms = 0.0;
    // algorithmic bytes per counted unit, as a wavefront session reports them
    st->node_bytes = sizeof(pt::Node);
    st->prim_bytes = 48;
    st->aux_bytes = PT_AUXW * sizeof(pt::AuxSL);
    return PT_OK;
}

void qctx_close(QueryCtx* q) {
    (void)hipSetDevice(q->dev);
    q->t.destroy();
    (void)hipFree(q->arena);
}

int copy_up(void* dev, const void* host, size_t bytes, const char* what) {
    if (hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(PT_E_HIP, std::string(what) + " failed");
    return PT_OK;
}
int copy_down(void* host, const void* dev, size_t bytes, const char* what) {
    if (hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(PT_E_HIP, std::string(what) + " failed");
    return PT_OK;
}

}  // namespace pti

extern "C" int pt_selftest_fold_shape(uint32_t cus, uint32_t per_cu, uint32_t block, uint32_t depth, uint32_t* block_out,
                                      uint32_t* grid_out) {
    if (!block_out || !grid_out) return pti::fail(PT_E_INVALID, "null argument");
    if (cus == 0u || per_cu == 0u || block < 64u || block > 1024u || (block & (block - 1u)))
        return pti::fail(PT_E_INVALID, "cus and per_cu at least 1, block a power of two in [64, 1024]");
    pti::GridShape g;
    if (const int rc = pti::fold_shape(cus, per_cu, block, depth, &g)) return rc;
    *block_out = g.block;
    *grid_out = g.max_grid;
    return PT_OK;
}
