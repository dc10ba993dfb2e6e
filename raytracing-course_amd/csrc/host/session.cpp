// session.cpp -- tile sessions (pt_session_*): one rank's pixels on one device, their
// geometry and their buffers in one allocation (both laid out without a device:
// pt_selftest_wave_plan), the megakernel pass (exact / division-form traversals),
// the device tonemap with its lost-chain check, statistics, and the tile un-interleave.
// The wavefront pass itself is rounds.cpp.
#include <stdio.h>
#include <string.h>

#include <map>
#include "api_internal.h"

namespace pti {

double wall_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int finish_pending(pt_session* ss) {
    for (auto& e : ss->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) ss->kernel_ms += ms;
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    ss->pending.clear();
    // diagnostics (PT_TUNE roundlog=1): per-launch ms of the rounds, one line per sync
    const bool log = tune_int("roundlog", 0) == 1 && !ss->pending_isect.empty();
    if (log) fprintf(stderr, "rounds_ms");
    for (const auto& e : ss->pending_isect) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.e0, e.e1) == hipSuccess) {
            ss->isect_ms += ms;
            if (e.coop) ss->coop_ms += ms;
        }
        if (log) fprintf(stderr, " %.3f", ms);
        (void)hipEventDestroy(e.e0);
        (void)hipEventDestroy(e.e1);
    }
    if (log) fprintf(stderr, "\n");
    ss->pending_isect.clear();
    // (a pass that failed midway leaves pairs without an end: not an error of the next launch)
    (void)hipGetLastError();
    return PT_OK;
}

// the window tiles dealt to `rank` (pt_kernels.h tile_owner), ascending
std::vector<uint32_t> rank_tiles(uint32_t n_tiles, uint32_t tiles_x, uint32_t rank, uint32_t world) {
    std::vector<uint32_t> v;
    v.reserve(n_tiles / world + 1);
    for (uint32_t t = 0; t < n_tiles; ++t)
        if (pt::tile_owner(t, tiles_x, world) == rank) v.push_back(t);
    return v;
}

uint64_t owned_pixels(const pt_session* ss) {
    uint64_t px = 0;
    for (uint32_t t = 0; t < ss->n_tiles_local; ++t) {
        const uint32_t gt = ss->gtiles[t];
        const uint32_t tx = gt % ss->tm.tiles_x, ty = gt / ss->tm.tiles_x;
        const uint32_t w = std::min(16u, ss->tm.ww - tx * 16u), h = std::min(16u, ss->tm.wh - ty * 16u);
        px += (uint64_t)w * h;
    }
    return px;
}

// the statistics counters, summed over their per-XCD copies (after the stream's work)
hipError_t read_counters(pt_session* ss, unsigned long long c[PT_CTR_STRIDE]) {
    unsigned long long cc[PT_CTR_COPIES * PT_CTR_STRIDE];
    // (on the session's stream: the null stream would also wait for other sessions' work)
    hipError_t e = hipMemcpyAsync(cc, ss->counters, sizeof(cc), hipMemcpyDeviceToHost, ss->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ss->stream);
    for (uint32_t k = 0; k < PT_CTR_STRIDE; ++k) c[k] = 0ull;
    if (e != hipSuccess) return e;
    for (uint32_t x = 0; x < PT_CTR_COPIES; ++x)
        for (uint32_t k = 0; k < PT_CTR_STRIDE; ++k) c[k] += cc[PT_CTR_STRIDE * x + k];
    return hipSuccess;
}

// run the coalesced trace() calls of the wavefront engine as one pass
int flush_trace(pt_session* ss) {
    if (!ss->deferred_spp) return PT_OK;
    const uint32_t spp = ss->deferred_spp;
    ss->deferred_spp = 0;
    HIP_TRY(hipSetDevice(ss->dev));
    return trace_wave(ss, spp);
}

// a scene's device copy as the kernels see it (without the megakernel's aux BVH)
pt::SceneView device_view(const pt_scene* s, const DevScene& ds) {
    pt::SceneView v;
    memset(&v, 0, sizeof(v));
    v.nodes = ds.nodes;
    v.prims = ds.prims;
    v.shade = ds.shade;
    v.planes = ds.planes;
    v.emitters = ds.emitters;
    v.n_planes = (uint32_t)s->planes.size();
    v.n_emitters = (uint32_t)s->emitters.size();
    v.inv_emitters = s->emitters.empty() ? 0.f : 1.f / (float)s->emitters.size();
    v.bg = pt::mk3(s->hs.bg[0], s->hs.bg[1], s->hs.bg[2]);
    v.box_extent = s->box_extent;
    v.anc_info = ds.anc_info;
    v.anc = ds.anc;
    set_blob(v, s, ds.blob);
    return v;
}
pt::SceneView device_view(const pt_session* ss) { return device_view(ss->sc, *ss->ds); }

// the summed counter block's shared part (a session's and a ray-query context's)
void counter_stats(const unsigned long long* c, pt_stats* st) {
    st->rays = c[pt::CTR_RAYS];
    st->node_visits = c[pt::CTR_NODES];
    st->prim_tests = c[pt::CTR_PTESTS];
    st->plane_tests = c[pt::CTR_PLANES];
    st->errors = c[pt::CTR_ERRORS];
    st->aux_visits = c[pt::CTR_AUX];
    st->fallbacks = c[pt::CTR_FALLBACKS];
    st->fallbacks_ray = c[pt::CTR_FALLBACKS_RAY];
}

namespace {

// the Z-order (Morton) code of a tile's coordinates
uint64_t morton_key(uint32_t tx, uint32_t ty) {
    uint64_t m = 0;
    for (int b = 0; b < 16; ++b)
        m |= (uint64_t)((tx >> b) & 1u) << (2 * b) | (uint64_t)((ty >> b) & 1u) << (2 * b + 1);
    return m;
}

// A session's geometry, without a device: the arguments checked, the window, its tiles and the
// rank's deal of them (tm, gtiles, n_tiles_local, n_slots), the engine, and for the wavefront
// engine `ord`, the local tiles' seeding order: sorted by the Z-order code of their coordinates
int session_geometry(pt_scene* s, const pt_session_opts* o, pt_session* ss, std::vector<uint32_t>* ord) {
    if (!s->prepared) return fail(PT_E_INVALID, "scene not prepared (call pt_scene_prepare)");
    if (o->world == 0 || o->rank >= o->world) return fail(PT_E_INVALID, "bad rank/world");
    if (s->hs.W == 0 || s->hs.H == 0) return fail(PT_E_SCENE, "zero image size");
    if ((uint64_t)s->hs.W * s->hs.H >= 2147483647ull) return fail(PT_E_SCENE, "image too large for per-pixel seeds");
    // the slot record keeps the current path's vertex count in 24 bits (pt_devutil.h PixelHot)
    if (s->hs.depth >= (1u << 24)) return fail(PT_E_SCENE, "RAY_DEPTH too large (at most 16777215)");
    pt::TileMap& tm = ss->tm;
    tm.W = s->hs.W;
    tm.H = s->hs.H;
    tm.x0 = o->win_w ? o->win_x0 : 0u;
    tm.y0 = o->win_w ? o->win_y0 : 0u;
    tm.ww = o->win_w ? o->win_w : s->hs.W;
    tm.wh = o->win_w ? o->win_h : s->hs.H;
    if (tm.ww == 0 || tm.wh == 0 || (uint64_t)tm.x0 + tm.ww > s->hs.W || (uint64_t)tm.y0 + tm.wh > s->hs.H)
        return fail(PT_E_INVALID, "window outside the image");
    tm.tiles_x = (tm.ww + 15u) / 16u;
    tm.n_tiles = tm.tiles_x * ((tm.wh + 15u) / 16u);
    tm.rank = o->rank;
    tm.world = o->world;
    ss->sc = s;
    ss->traversal = o->traversal;
    ss->depth = s->hs.depth;
    ss->gtiles = rank_tiles(tm.n_tiles, tm.tiles_x, o->rank, o->world);
    ss->n_tiles_local = (uint32_t)ss->gtiles.size();
    ss->n_slots = ss->n_tiles_local * 256u;
    ss->cam = make_cam(s);
    ss->st.depth = std::max<uint32_t>(ss->depth, 1u);
    ss->st.n_slots = ss->n_slots;
    // engine: the wavefront pipeline for the (filtered) replay traversal; the
    // megakernel for the exact DFS and the division-form replay (PT_TUNE engine=mega forces it)
    ss->wave = o->traversal == PT_TRAVERSAL_REPLAY && tune_str("engine") != "mega";
    ord->clear();
    if (ss->wave) {
        std::vector<std::pair<uint64_t, uint32_t>> key(ss->n_tiles_local);
        for (uint32_t t = 0; t < ss->n_tiles_local; ++t)
            key[t] = {morton_key(ss->gtiles[t] % tm.tiles_x, ss->gtiles[t] / tm.tiles_x), t};
        std::sort(key.begin(), key.end());
        for (const auto& k : key) ord->push_back(k.second);
    }
    return PT_OK;
}

// the wavefront pass's plan for this session's pixels and scene on a device of `cus` compute units
int session_plan(pt_session* ss, uint32_t cus) {
    if (!ss->wave) return PT_OK;
    const pt_scene* s = ss->sc;
    PlanInputs in;
    in.cus = cus;
    in.n_slots = ss->n_slots;
    in.n_tiles_local = ss->n_tiles_local;
    in.depth = ss->depth;
    in.n_planes = (uint32_t)s->planes.size();
    in.n_emitters = (uint32_t)s->emitters.size();
    in.auxw_stack = s->auxw_stack;
    in.auxsl_depth = s->auxsl_depth;
    in.max_stack = s->max_stack;
    in.n_aux = (uint32_t)s->auxsl.size();
    return plan_wave(in, &ss->plan);
}

// Every device buffer of the session in ONE allocation (sections at 256-B offsets): each
// section is declared once, as the pointer field it fills and its bytes; bind() stores the
// allocation's base + offset into every field.  `at` is the allocation's size.
struct Arena {
    size_t at = 0;
    std::vector<std::pair<void*, size_t>> fields;   // {the pointer field's address, the section's offset}
    template <class T>
    void add(T** field, size_t bytes) {
        fields.emplace_back((void*)field, at);
        at = (at + std::max<size_t>(bytes, 16) + 255) & ~(size_t)255;
    }
    void bind(unsigned char* base) const {
        for (const auto& f : fields) {
            unsigned char* p = base + f.second;
            memcpy(f.first, &p, sizeof(p));
        }
    }
};

// the session's sections, in the arena's order (`tables`: the tile table, then the seeding order)
void session_layout(pt_session* ss, size_t n_order, bool fb, uint32_t** tables, Arena& a) {
    const size_t n = std::max<size_t>(ss->n_slots, 1);
    const WavePlan& w = ss->plan;
    a.add(tables, (ss->gtiles.size() + n_order) * 4);
    a.add(&ss->st.rec, 2 * n * sizeof(uint4));
    a.add(&ss->st.fold, (size_t)ss->st.depth * n * sizeof(uint4));
    a.add(&ss->counters, 8 * PT_CTR_COPIES * PT_CTR_STRIDE);
    a.add(&ss->out, 3 * n);
    // the window's framebuffer (pt_render's device-side gather; rank 0's session)
    if (fb) a.add(&ss->fb, 3ull * ss->tm.ww * ss->tm.wh);
    if (!ss->wave) return;
    for (pt::RayQ& q : ss->fq) {
        a.add(&q.ro, n * 16);
        a.add(&q.rd, n * 16);
        a.add(&q.ri, n * 16);
    }
    a.add(&ss->fq[0].pid, 2 * n * 4);   // (both queues' halves: fq[1].pid is fq[0].pid + n)
    a.add(&ss->done.ro, n * 16);
    a.add(&ss->ex.ro, n * 16);
    a.add(&ss->done.rd, n * 16);
    a.add(&ss->ex.rd, n * 16);
    a.add(&ss->done.id, n * 4);
    a.add(&ss->carry, 2ull * w.carry_cap * w.carry_words * 4);
    a.add(&ss->ctl, 8 * PT_CTL_SET);
    a.add(&ss->endq, std::max((size_t)w.path_grid * pt::path_cmax(PT_NQ_BASE),
                              (size_t)w.full_grid * pt::path_cmax(w.full_nq)) * sizeof(uint2));
    a.add(&ss->order, (n + 2 * PT_ORDER_BUCKETS) * 4);
    if (w.early_k) {
        a.add(&ss->side.ro, (size_t)w.early_k * 16);
        a.add(&ss->side.rd, (size_t)w.early_k * 16);
        a.add(&ss->side.ri, (size_t)w.early_k * 16);
        a.add(&ss->side.pid, (size_t)w.early_k * 4);
        a.add(&ss->side_carry, (size_t)w.early_k * w.carry_words * 4);
        a.add(&ss->side_ctl, 8 * PT_CTL_SET);
    }
}

// the early launch's stream and events: made on a helper thread beside the set-up and
// the pass's first rounds (a stream's creation costs ~10 ms: neither on the set-up's
// path nor in the pass), joined where the first early launch needs them
int start_side_stream(pt_session* ss) {
    const int dev = ss->dev;
    auto make = [ss, dev] {
        ss->side_rc = hipSetDevice(dev);
        if (ss->side_rc == hipSuccess) ss->side_rc = take_stream(dev, &ss->side_stream, true);
        if (ss->side_rc == hipSuccess) ss->side_rc = hipEventCreateWithFlags(&ss->side_taken, hipEventDisableTiming);
        if (ss->side_rc == hipSuccess) ss->side_rc = hipEventCreateWithFlags(&ss->side_end, hipEventDisableTiming);
    };
    try {
        ss->side_th = std::thread(make);
    } catch (const std::system_error&) {
        // (no helper thread: made here, and the current device set back)
        make();
        if (hipSetDevice(ss->dev) != hipSuccess) return fail(PT_E_HIP, "hipSetDevice failed");
    }
    return PT_OK;
}

// a rank's packed tiles (256 pixels of 3 T each) scattered into the W x H image
template <class T>
int unpack_tiles(uint32_t W, uint32_t H, uint32_t rank, uint32_t world, const T* packed, T* img) {
    if (!packed || !img || world == 0) return fail(PT_E_INVALID, "bad argument");
    const uint32_t tiles_x = (W + 15u) / 16u, n_tiles = tiles_x * ((H + 15u) / 16u);
    uint32_t lt = 0;
    for (uint32_t gt = 0; gt < n_tiles; ++gt) {
        if (pt::tile_owner(gt, tiles_x, world) != rank) continue;
        const uint32_t tx = gt % tiles_x, ty = gt / tiles_x;
        for (uint32_t j = 0; j < 16u; ++j) {
            const uint32_t y = ty * 16u + j;
            if (y >= H) break;
            const uint32_t x0 = tx * 16u, w = std::min(16u, W - x0);
            memcpy(img + ((size_t)y * W + x0) * 3, packed + ((size_t)lt * 256u + j * 16u) * 3, (size_t)w * 3 * sizeof(T));
        }
        ++lt;
    }
    return PT_OK;
}

}  // namespace

int session_geometry_only(pt_scene* s, const pt_session_opts* o, pt_session* ss) {
    std::vector<uint32_t> ord;
    return session_geometry(s, o, ss, &ord);
}
}  // namespace pti

using namespace pti;

extern "C" {

// ------------------------------------------------------------- sessions ---
int pt_session_create(pt_scene* s, const pt_session_opts* o, pt_session** out) {
    if (!s || !o || !out) return fail(PT_E_INVALID, "null argument");
    auto* ss = new pt_session();
    std::vector<uint32_t> ord;   // wavefront: the local tiles' seeding order
    int rc = session_geometry(s, o, ss, &ord);
    if (!rc) rc = check_device(o->device);
    // the megakernel (exact / division-form traversal, PT_TUNE engine=mega) also reads the BVH2 aux
    DevScene* ds = nullptr;
    if (!rc) rc = ensure_device_scene(s, o->device, !ss->wave, &ds, &ss->upload_ms);
    if (rc) {
        delete ss;   // (nothing on a device yet)
        return rc;
    }
    ss->dev = o->device;
    ss->ds = ds;
    auto cleanup = [&](int code) {
        pt_session_free(ss);
        return code;
    };
    if (hipSetDevice(ss->dev) != hipSuccess) return cleanup(fail(PT_E_HIP, "hipSetDevice failed"));
    DevProps props;
    if ((rc = device_props(ss->dev, &props))) return cleanup(rc);
    if ((rc = session_plan(ss, (uint32_t)props.cus))) return cleanup(rc);
    if (take_stream(ss->dev, &ss->stream) != hipSuccess) return cleanup(fail(PT_E_HIP, "stream creation failed"));
    if (ss->plan.early_k && (rc = start_side_stream(ss))) return cleanup(rc);
    // the arena, and the two small host-made tables with one copy: session set-up is a
    // handful of runtime calls, whatever the pixel count
    Arena arena;
    uint32_t* tables = nullptr;
    session_layout(ss, ord.size(), o->rank == 0, &tables, arena);
    void* p = nullptr;
    if (hipMalloc(&p, arena.at) != hipSuccess) return cleanup(fail(PT_E_OOM, "device allocation failed (session buffers)"));
    ss->arena = static_cast<unsigned char*>(p);
    ss->arena_bytes = arena.at;
    arena.bind(ss->arena);
    if (ss->wave) ss->fq[1].pid = ss->fq[0].pid + std::max<size_t>(ss->n_slots, 1);
    if (!ss->gtiles.empty()) {
        std::vector<uint32_t> t(ss->gtiles);
        t.insert(t.end(), ord.begin(), ord.end());
        if (hipMemcpy(tables, t.data(), t.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            return cleanup(fail(PT_E_HIP, "tile tables upload failed"));
        ss->tm.gtile = tables;
        if (!ord.empty()) ss->tile_order = tables + ss->gtiles.size();
    }
    if (ss->wave && hipHostMalloc(&ss->ctl_host, 64) != hipSuccess)
        return cleanup(fail(PT_E_OOM, "host allocation failed (round counters)"));
    if (hipMemsetAsync(ss->counters, 0, 8 * PT_CTR_COPIES * PT_CTR_STRIDE, ss->stream) != hipSuccess) return cleanup(fail(PT_E_HIP, "memset failed"));
    if (ss->n_tiles_local) {
        pt::InitParams ip;
        ip.tm = ss->tm;
        ip.st = ss->st;
        if (pt_launch_init(ip, ss->n_tiles_local, ss->stream) != hipSuccess)
            return cleanup(fail(PT_E_HIP, "k_init launch failed"));
    }
    *out = ss;
    return PT_OK;
}

// test hook: a session's geometry, plan and arena layout for a device of `cus` compute units,
// as "key=value" lines (no device needed; o->device is ignored)
int pt_selftest_wave_plan(pt_scene* s, const pt_session_opts* o, uint32_t cus, char* buf, size_t cap) {
    if (!s || !o || !buf) return fail(PT_E_INVALID, "null argument");
    int rc = pt_scene_prepare(s);
    if (rc) return rc;
    pt_session ss;
    std::vector<uint32_t> ord;
    if ((rc = session_geometry(s, o, &ss, &ord))) return rc;
    if ((rc = session_plan(&ss, cus))) return rc;
    Arena arena;
    uint32_t* tables = nullptr;
    session_layout(&ss, ord.size(), o->rank == 0, &tables, arena);
    const std::string t = plan_text(ss.plan) + "n_slots=" + std::to_string(ss.n_slots) + "\nn_tiles_local=" +
                          std::to_string(ss.n_tiles_local) + "\narena_bytes=" + std::to_string(arena.at) +
                          "\naux_stack_words=" + std::to_string(s->auxw_stack) + "\n";
    if (t.size() + 1 > cap) return fail(PT_E_INVALID, "buffer too small");
    memcpy(buf, t.c_str(), t.size() + 1);
    return PT_OK;
}

int pt_session_layout(const pt_session* ss, uint32_t* n_tiles, uint64_t* packed_rgb_bytes) {
    if (!ss) return fail(PT_E_INVALID, "null session");
    if (n_tiles) *n_tiles = ss->n_tiles_local;
    if (packed_rgb_bytes) *packed_rgb_bytes = 3ull * ss->n_slots;
    return PT_OK;
}

int pt_session_trace(pt_session* ss, uint32_t spp) {
    if (!ss) return fail(PT_E_INVALID, "null session");
    if (spp == 0 || ss->n_tiles_local == 0) { ss->samples_done += spp; return PT_OK; }
    if (ss->wave) {
        // Consecutive calls are one pass: a pixel goes on with its next samples as soon
        // as it is done with the current ones, so only the last call waits for the
        // slowest pixel.  The pass runs at the next resolve / sync / stats.
        if (ss->deferred_spp > 0xffffffffu - spp) {
            const int rc = flush_trace(ss);
            if (rc) return rc;
        }
        ss->deferred_spp += spp;
        return PT_OK;
    }
    HIP_TRY(hipSetDevice(ss->dev));
    const DevScene& ds = *ss->ds;
    pt::TraceParams tp;
    const pt_scene* s = ss->sc;
    tp.S = device_view(ss);
    tp.S.aux = ss->traversal == PT_TRAVERSAL_EXACT ? nullptr : ds.aux;
    tp.cfg = replay_cfg(s);
    tp.cam = ss->cam;
    tp.tm = ss->tm;
    tp.st = ss->st;
    tp.counters = ss->counters;
    tp.depth = ss->depth;
    tp.spp = spp;
    tp.n_tiles_local = ss->n_tiles_local;
    tp.wg_prof = nullptr;
    // filtered node tests unless the division form was asked for
    const bool fast = ss->traversal == PT_TRAVERSAL_REPLAY;
    const std::string wgps = tune_str("wgprof");
    const char* wgp = wgps.c_str();
    if (*wgp) {
        if (!ss->wg_prof) HIP_TRY(hipMalloc(&ss->wg_prof, 32ull * std::max(ss->n_tiles_local, 1u)));
        HIP_TRY(hipMemsetAsync(ss->wg_prof, 0, 32ull * std::max(ss->n_tiles_local, 1u), ss->stream));
        tp.wg_prof = ss->wg_prof;
    }
    const uint32_t lds = 256u * 4u * lane_words(s, ss->traversal);
    if (lds > 160u * 1024u) return fail(PT_E_SCENE, "BVH too deep for the LDS traversal stack");
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, ss->stream));
    HIP_TRY(pt_launch_trace(tp, fast, lds, ss->stream));
    HIP_TRY(hipEventRecord(e1, ss->stream));
    if (tp.wg_prof) {
        // diagnostics: append this launch's per-workgroup timeline to the wgprof file
        std::vector<unsigned long long> h(4ull * ss->n_tiles_local);
        HIP_TRY(hipMemcpyAsync(h.data(), tp.wg_prof, h.size() * 8, hipMemcpyDeviceToHost, ss->stream));
        HIP_TRY(hipStreamSynchronize(ss->stream));
        if (FILE* f = fopen(wgp, "ab")) {
            fwrite(h.data(), 8, h.size(), f);
            fclose(f);
        }
    }
    ss->pending.emplace_back(e0, e1);
    ss->samples_done += spp;
    return PT_OK;
}

int pt_session_resolve(pt_session* ss, uint8_t* dev_out, float* dev_radiance) {
    if (!ss) return fail(PT_E_INVALID, "null session");
    if (ss->n_tiles_local == 0) return PT_OK;
    if (const int rc = flush_trace(ss)) return rc;
    // a ragged session (counts.cpp) divides each pixel's sum by its own count: none may be 0
    const bool ragged = ss->lag_max != 0;
    if (ragged && ss->lag_max == ss->samples_done)
        return fail(PT_E_INVALID, "an owned pixel has no sample yet: its mean is undefined (as pt_pixel_resolve refuses it)");
    HIP_TRY(hipSetDevice(ss->dev));
    pt::ResolveParams rp;
    rp.st = ss->st;
    rp.tm = ss->tm;
    rp.counters = ss->counters;
    rp.thr = ss->ds->thr;
    rp.out = dev_out ? dev_out : ss->out;
    rp.rad = dev_radiance;
    rp.samples = (uint32_t)ss->samples_done;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, ss->stream));
    if (ragged) HIP_TRY(launch_ragged_resolve(ss, rp.out, rp.rad));
    else HIP_TRY(pt_launch_resolve(rp, ss->n_tiles_local, ss->stream));
    HIP_TRY(hipEventRecord(e1, ss->stream));
    HIP_TRY(hipStreamSynchronize(ss->stream));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ss->resolve_ms += ms;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    // pixels short of (or past) the samples so far: a chain was lost -- an error, not an image
    unsigned long long c[PT_CTR_STRIDE];
    HIP_TRY(read_counters(ss, c));
    if (c[pt::CTR_SHORT] != ss->short_seen) {
        const unsigned long long k = c[pt::CTR_SHORT] - ss->short_seen;
        ss->short_seen = c[pt::CTR_SHORT];
        if (tune_int("shortlog", 0)) {
            // diagnostics: how far the short pixels are from the target, and where they are
            std::vector<uint4> rec(2ull * ss->n_slots);
            // (a ragged session: a pixel's own count lies lag[slot] below its `done` field)
            std::vector<uint32_t> lag(ss->n_slots, 0u);
            if (hipMemcpy(rec.data(), ss->st.rec, rec.size() * sizeof(uint4), hipMemcpyDeviceToHost) == hipSuccess &&
                (!ragged || hipMemcpy(lag.data(), lag_table(ss), lag.size() * 4, hipMemcpyDeviceToHost) == hipSuccess)) {
                std::map<int, uint32_t> hist;
                uint32_t shown = 0;
                for (uint32_t i = 0; i < ss->n_slots; ++i) {
                    const uint32_t done = rec[2 * i].w, nv = rec[2 * i].z >> 8;
                    if (done == rp.samples || rec[2 * i + 1].w == 0xFFFFFFFFu) continue;
                    hist[(int)done - (int)rp.samples]++;
                    if (shown++ < 8)
                        fprintf(stderr, "short: slot %u pixel %u done %u of %u nv %u\n", i, rec[2 * i + 1].w, done - lag[i],
                                rp.samples - lag[i], nv);
                }
                for (auto& h : hist) fprintf(stderr, "short: done - samples = %d: %u pixels\n", h.first, h.second);
            }
        }
        return fail(PT_E_HIP, std::to_string(k) + " pixel(s) did not take exactly " +
                                  (ragged ? std::string("their own count of") : std::to_string(rp.samples)) +
                                  " samples (a chain was lost)");
    }
    return PT_OK;
}

int pt_session_sync(pt_session* ss) {
    if (!ss) return fail(PT_E_INVALID, "null session");
    if (const int rc = flush_trace(ss)) return rc;
    HIP_TRY(hipSetDevice(ss->dev));
    HIP_TRY(hipStreamSynchronize(ss->stream));
    return finish_pending(ss);
}

int pt_session_reset(pt_session* ss) {
    if (!ss) return fail(PT_E_INVALID, "null session");
    if (const int rc = flush_trace(ss)) return rc;
    HIP_TRY(hipSetDevice(ss->dev));
    if (ss->n_tiles_local) {
        pt::InitParams ip;
        ip.tm = ss->tm;
        ip.st = ss->st;
        HIP_TRY(pt_launch_init(ip, ss->n_tiles_local, ss->stream));
    }
    HIP_TRY(clear_lag(ss));   // (a ragged session: uniform again)
    HIP_TRY(clear_marks(ss));   // (fresh pixels: no noise estimate yet)
    ss->samples_done = 0;
    return PT_OK;
}

int pt_session_read_packed(pt_session* ss, uint8_t* host_out, size_t bytes) {
    if (!ss || !host_out) return fail(PT_E_INVALID, "null argument");
    if (bytes < 3ull * ss->n_slots) return fail(PT_E_INVALID, "buffer too small");
    if (ss->n_slots == 0) return PT_OK;
    HIP_TRY(hipSetDevice(ss->dev));
    HIP_TRY(hipMemcpyAsync(host_out, ss->out, 3ull * ss->n_slots, hipMemcpyDeviceToHost, ss->stream));
    HIP_TRY(hipStreamSynchronize(ss->stream));
    return PT_OK;
}

int pt_session_stats(pt_session* ss, pt_stats* st) {
    if (!ss || !st) return fail(PT_E_INVALID, "null argument");
    int rc = pt_session_sync(ss);
    if (rc) return rc;
    unsigned long long c[PT_CTR_STRIDE];
    HIP_TRY(read_counters(ss, c));
    memset(st, 0, sizeof(*st));
    counter_stats(c, st);
    st->samples = owned_pixels(ss) * ss->samples_done - ss->lag_sum;   // (lag_sum: a ragged session's, counts.cpp)
    st->kernel_ms = ss->kernel_ms;
    st->resolve_ms = ss->resolve_ms;
    st->node_bytes = sizeof(pt::Node);
    st->prim_bytes = sizeof(pt::Prim);
    // algorithmic bytes per counted unit: wavefront query = 4-wide aux node (128 B),
    // reference node record (32 B), primitive geometry (48 B: the 64-B compact record
    // adds the precomputed triangle normal, a layout choice, not counted)
    st->aux_bytes = ss->wave ? PT_AUXW * sizeof(pt::AuxSL) : sizeof(pt::AuxNode);
    if (ss->wave) st->prim_bytes = 48;
    st->isect_ms = ss->isect_ms;
    st->isect_launches = ss->isect_launches;
    st->rounds = ss->rounds;
    st->coop_rays = c[pt::CTR_COOP_RAYS];
    st->coop_node_visits = c[pt::CTR_COOP_NODES];
    st->coop_prim_tests = c[pt::CTR_COOP_PTESTS];
    st->coop_aux_visits = c[pt::CTR_COOP_AUX];
    st->coop_ms = ss->coop_ms;
    st->coop_launches = ss->coop_launches;
    st->short_pixels = c[pt::CTR_SHORT];
    st->handed_on = c[pt::CTR_HANDON];
    for (uint32_t k = 0; k < PT_HO_N; ++k) st->handoff[k] = c[pt::CTR_HO + k];
    return PT_OK;
}

}  // extern "C"

namespace pti {
static_assert(sizeof(pt_stats) == 40 * 8,
              "pt_stats changed: give every new field its rule in merge_stats (sum, max, last value, or the render's own)");
// A rank's statistics into the render's: the counts summed, the times the slowest rank's, the record
// sizes any rank's.  (wall_ms, gather_rccl and gather_allocs are the render's own: pt_render sets them.)
void merge_stats(pt_stats& into, const pt_stats& rank) {
    into.rays += rank.rays; into.node_visits += rank.node_visits; into.prim_tests += rank.prim_tests;
    into.plane_tests += rank.plane_tests; into.samples += rank.samples; into.errors += rank.errors;
    into.aux_visits += rank.aux_visits; into.fallbacks += rank.fallbacks; into.fallbacks_ray += rank.fallbacks_ray;
    into.isect_launches += rank.isect_launches; into.rounds += rank.rounds;
    into.coop_rays += rank.coop_rays; into.coop_node_visits += rank.coop_node_visits;
    into.coop_prim_tests += rank.coop_prim_tests; into.coop_aux_visits += rank.coop_aux_visits;
    into.coop_launches += rank.coop_launches;
    into.short_pixels += rank.short_pixels; into.handed_on += rank.handed_on;
    for (int k = 0; k < PT_HO_N; ++k) into.handoff[k] += rank.handoff[k];
    into.kernel_ms = std::max(into.kernel_ms, rank.kernel_ms);
    into.resolve_ms = std::max(into.resolve_ms, rank.resolve_ms);
    into.isect_ms = std::max(into.isect_ms, rank.isect_ms);
    into.coop_ms = std::max(into.coop_ms, rank.coop_ms);
    into.node_bytes = rank.node_bytes; into.prim_bytes = rank.prim_bytes; into.aux_bytes = rank.aux_bytes;
}
}  // namespace pti

extern "C" {

void* pt_session_stream(pt_session* ss) {
    if (!ss) return nullptr;
    (void)flush_trace(ss);   // work ordered after the stream sees every trace() so far (errors: pt_last_error)
    return (void*)ss->stream;
}

void pt_session_free(pt_session* ss) {
    if (!ss) return;
    if (ss->side_th.joinable()) ss->side_th.join();
    (void)hipSetDevice(ss->dev);
    // both streams drained before any buffer goes (a side launch may still run after a
    // failed pass)
    if (ss->stream) (void)hipStreamSynchronize(ss->stream);
    if (ss->side_stream) (void)hipStreamSynchronize(ss->side_stream);
    finish_pending(ss);
    (void)hipFree(ss->arena);
    (void)hipFree(ss->rad); (void)hipFree(ss->wg_prof);
    (void)hipFree(ss->state_tile_rec); (void)hipFree(ss->state_marks);
    (void)hipFree(ss->counts_block); (void)hipFree(ss->counts_host_copy);
    (void)hipFree(ss->noise_block);
    pt_featq_free(ss->feat_q);
    (void)hipFree(ss->feat_xy);
    if (ss->ctl_host) (void)hipHostFree(ss->ctl_host);
    if (ss->prog_host) (void)hipHostFree(ss->prog_host);
    if (ss->side_taken) (void)hipEventDestroy(ss->side_taken);
    if (ss->side_end) (void)hipEventDestroy(ss->side_end);
    // back to the device's pools for the next session (no destroy/create per render)
    give_stream(ss->dev, ss->stream, false);
    give_stream(ss->dev, ss->side_stream, true);
    delete ss;
}

int pt_unpack_tiles(uint32_t W, uint32_t H, uint32_t rank, uint32_t world, const uint8_t* packed, uint8_t* rgb) {
    return unpack_tiles<uint8_t>(W, H, rank, world, packed, rgb);
}

int pt_unpack_tiles_f32(uint32_t W, uint32_t H, uint32_t rank, uint32_t world, const float* packed, float* rad) {
    return unpack_tiles<float>(W, H, rank, world, packed, rad);
}

}  // extern "C"
