// render.cpp -- Scene::Render equivalent (pt_render, a list of phases): one host thread and one
// session per GPU, the device tonemap, the framebuffer gather (one grouped ncclGather over
// xGMI to the first device, or through the host), the P6 write.
#include <stdio.h>
#include <string.h>

#include <condition_variable>
#include "api_internal.h"

namespace pti {
namespace {

void progress_bar(uint64_t done, uint64_t total, int& last) {
    // the reference prints "Loading: [ ##...   x% ]" every 10 % (src/scene.cpp:232-240)
    const int ct = total ? (int)((done * 10) / total) : 10;
    while (last < ct && last < 10) {
        ++last;
        std::string bar = "Loading: [ ";
        bar += std::string((size_t)last, '#');
        bar += std::string((size_t)(11 - last), ' ');
        bar += std::to_string(last * 10);
        bar += "% ]\n";
        fputs(bar.c_str(), stdout);
        fflush(stdout);
    }
}

// One rank of a render: its session (freed with it), its phase times (ms), how it ended -- with
// pt_last_error's text, which is its thread's -- and rank 0's progress bar
struct RankRun {
    pt_session* x = nullptr;
    double setup = 0, wait = 0, render = 0, resolve = 0;
    int rc = PT_OK;
    std::string err;
    int bar = 0;          // its last step
    RankRun() = default;
    RankRun(const RankRun&) = delete;
    ~RankRun() { pt_session_free(x); }
    void failed(int code) { rc = code; err = pt_last_error(); }
};

// RCCL communicators over devices dev0 .. dev0+n-1, created once per process and
// device set (pt_gather_init may create one ahead of the render), with the gather's
// device buffers: made by the first render that gathers over the set and kept (grown
// when a later render needs more), so consecutive renders allocate nothing
struct CommSet {
    std::vector<ncclComm_t> c;
    std::vector<uint8_t*> send;   // per device: cap bytes (its rank's packed tiles)
    uint8_t* recv = nullptr;      // first device: n x cap bytes (the gathered blocks)
    uint32_t* src = nullptr;      // first device: per window tile, its source in recv
    size_t cap = 0, src_n = 0;
};
std::mutex g_comm_mu;
std::map<std::pair<int, int>, CommSet> g_comms;
int comm_get(int dev0, int n, CommSet** out) {
    // (caller holds g_comm_mu)
    auto key = std::make_pair(dev0, n);
    auto it = g_comms.find(key);
    if (it == g_comms.end()) {
        std::vector<int> devs(n);
        for (int g = 0; g < n; ++g) devs[g] = dev0 + g;
        std::vector<ncclComm_t> c(n);
        if (!rccl().ok) return fail(PT_E_RCCL, "librccl.so.1 not loadable");
        if (rccl().CommInitAll(c.data(), n, devs.data()) != ncclSuccess) return fail(PT_E_RCCL, "ncclCommInitAll failed");
        CommSet cs;
        cs.c = c;
        cs.send.assign((size_t)n, nullptr);
        it = g_comms.emplace(key, std::move(cs)).first;
    }
    *out = &it->second;
    return PT_OK;
}

// One process driving several GPUs: the packed u8 tiles of every session are
// gathered to the first device with one grouped ncclGather over xGMI
// (communicator and buffers cached per device set), then un-tiled there by one
// kernel into the caller's framebuffer.  *allocs = the device allocations made.
int gather_rccl(const std::vector<RankRun>& ranks, int dev0, uint32_t W, uint32_t H, uint8_t* rgb,
                uint8_t* staging, uint64_t* allocs) {
    if (tune_int("inject_rccl", 0)) return fail(PT_E_RCCL, "injected RCCL gather failure (PT_TUNE inject_rccl)");
    std::lock_guard<std::mutex> lk(g_comm_mu);
    const int n = (int)ranks.size();
    CommSet* cs = nullptr;
    if (const int rc = comm_get(dev0, n, &cs)) return rc;
    size_t cap = 0;
    for (const RankRun& k : ranks) cap = std::max<size_t>(cap, 3ull * k.x->n_slots);
    cap = std::max<size_t>(cap, 16);
    if ((uint64_t)cap * n > 0xffffffffull) return fail(PT_E_INVALID, "gather buffer beyond 4 GB");
    const uint32_t tiles_x = (W + 15u) / 16u, n_tiles = tiles_x * ((H + 15u) / 16u);
    if (cap > cs->cap) {
        // (grown: the old buffers go, new ones of the size this render needs)
        for (int g = 0; g < n; ++g) {
            HIP_TRY(hipSetDevice(dev0 + g));
            if (cs->send[(size_t)g]) (void)hipFree(cs->send[(size_t)g]);
            cs->send[(size_t)g] = nullptr;
            if (g == 0 && cs->recv) (void)hipFree(cs->recv);
            if (g == 0) cs->recv = nullptr;
        }
        cs->cap = 0;
        for (int g = 0; g < n; ++g) {
            HIP_TRY(hipSetDevice(dev0 + g));
            if (hipMalloc(&cs->send[(size_t)g], cap) != hipSuccess) return fail(PT_E_OOM, "gather buffer");
            ++*allocs;
        }
        HIP_TRY(hipSetDevice(dev0));
        if (hipMalloc(&cs->recv, cap * n) != hipSuccess) return fail(PT_E_OOM, "gather buffer");
        ++*allocs;
        cs->cap = cap;
    }
    if (n_tiles > cs->src_n) {
        HIP_TRY(hipSetDevice(dev0));
        if (cs->src) (void)hipFree(cs->src);
        cs->src = nullptr;
        cs->src_n = 0;
        if (hipMalloc(&cs->src, std::max<size_t>(n_tiles, 1) * 4) != hipSuccess) return fail(PT_E_OOM, "gather buffer");
        ++*allocs;
        cs->src_n = n_tiles;
    }
    for (int g = 0; g < n; ++g) {
        HIP_TRY(hipSetDevice(dev0 + g));
        if (ranks[g].x->n_slots)
            HIP_TRY(hipMemcpyAsync(cs->send[(size_t)g], ranks[g].x->out, 3ull * ranks[g].x->n_slots, hipMemcpyDeviceToDevice,
                                   ranks[g].x->stream));
    }
    const Rccl& R = rccl();
    ncclResult_t r = R.GroupStart();
    for (int g = 0; g < n && r == ncclSuccess; ++g)
        r = R.Gather(cs->send[(size_t)g], g == 0 ? cs->recv : nullptr, cs->cap, ncclUint8, 0, cs->c[g], ranks[g].x->stream);
    if (r == ncclSuccess) r = R.GroupEnd();
    if (r != ncclSuccess) return fail(PT_E_RCCL, std::string("ncclGather: ") + R.GetErrorString(r));
    // the framebuffer on the first device: every window tile's source in the gathered blocks
    // (owner * cap + its rank among the owner's tiles * 768), un-tiled by one kernel, one copy out
    std::vector<uint32_t> src(n_tiles), seen((size_t)n, 0u);
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const uint32_t g = pt::tile_owner(t, tiles_x, (uint32_t)n);
        src[t] = (uint32_t)(g * cs->cap + seen[g]++ * 768u);
    }
    HIP_TRY(hipSetDevice(dev0));
    HIP_TRY(hipMemcpyAsync(cs->src, src.data(), n_tiles * 4ull, hipMemcpyHostToDevice, ranks[0].x->stream));
    HIP_TRY(pt_launch_untile(cs->recv, cs->src, tiles_x, W, H, staging ? staging : ranks[0].x->fb, ranks[0].x->stream));
    if (!staging) HIP_TRY(hipMemcpyAsync(rgb, ranks[0].x->fb, 3ull * W * H, hipMemcpyDeviceToHost, ranks[0].x->stream));
    for (int g = 0; g < n; ++g) {
        HIP_TRY(hipSetDevice(dev0 + g));
        HIP_TRY(hipStreamSynchronize(ranks[g].x->stream));
    }
    if (staging) memcpy(rgb, staging, 3ull * W * H);
    return PT_OK;
}

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }

// pt_render's options resolved against the scene and PT_TUNE: what every phase below reads
struct RenderPlan {
    pt_scene* const s;
    pt_render_opts o;
    uint32_t S, W, H;     // samples per pixel; the window (or the image)
    int ngpu;
    // PT_TUNE same_device=1 (test-only): the ngpu sessions and host threads all on o.device,
    // rendering at once -- the in-process multi-GPU path on one GPU; RCCL cannot place two ranks
    // on one device, so the framebuffer goes through the host.  same_device=2: the same, but the
    // ranks render one after another once every session is set up, so each rank's render time is
    // its time alone on a GPU (the per-rank phase times of PT_STATS=2 then project an ngpu-GPU run)
    const int same = tune_int("same_device", 0);
    // samples per trace call: one pass for all of them (a pass ends with its slowest
    // pixel, so every extra sync costs a tail).  The wavefront engine reports the
    // bar from inside the pass; the exact-traversal renderer takes ~20 passes.
    bool in_pass;
    uint32_t chunk;
    const bool radiance;  // the caller wants the fp32 radiance too
    RenderPlan(pt_scene* sc, const pt_render_opts* opts, bool rad) : s(sc), radiance(rad) {
        pt_render_opts_default(&o);
        if (opts) o = *opts;
        S = o.samples ? o.samples : s->hs.samples;
        W = o.win_w ? o.win_w : s->hs.W; H = o.win_w ? o.win_h : s->hs.H;
        ngpu = std::max(1, o.ngpu);
        const bool wave = o.traversal == PT_TRAVERSAL_REPLAY && tune_str("engine") != "mega";
        in_pass = o.progress && wave;
        chunk = o.spp_per_launch ? o.spp_per_launch
                : o.progress && !in_pass ? std::max(1u, (S + 19u) / 20u) : std::max(S, 1u);
    }
};

// PT_TUNE same_device=2: every session set up, then the ranks' renders one at a time, in rank
// order.  Every rank advances `turn` exactly once, failed or not -- set_up_and_wait() then
// rendered(), or never_started() for a rank without a thread -- so no waiting rank is skipped
// or left behind.  In any other mode the calls do nothing.
class Turnstile {
    const int n_;
    const bool on_;
    std::mutex mu_;
    std::condition_variable cv_;
    int set_up_ = 0, turn_ = 0;
    void advance(int set_up, int turn) {
        if (!on_) return;
        std::lock_guard<std::mutex> lk(mu_);
        set_up_ += set_up; turn_ += turn;
        cv_.notify_all();
    }
  public:
    Turnstile(int ranks, bool on) : n_(ranks), on_(on) {}
    // rank g is set up; returns once every rank is and g's turn has come: the ms waited
    double set_up_and_wait(int g) {
        if (!on_) return 0.0;
        advance(1, 0);
        const auto tw = Clock::now();
        std::unique_lock<std::mutex> lk(mu_);
        // (>=: a rank that never started has advanced `turn` ahead of its turn)
        cv_.wait(lk, [&] { return set_up_ == n_ && turn_ >= g; });
        return ms_since(tw);
    }
    void rendered() { advance(0, 1); }
    void never_started() { advance(1, 1); }
};

int rank_set_up(const RenderPlan& p, int g, RankRun& k) {
    const pt_session_opts so{p.same ? p.o.device : p.o.device + g, (uint32_t)g, (uint32_t)p.ngpu, p.o.traversal,
                             p.o.win_x0, p.o.win_y0, p.o.win_w, p.o.win_h};
    int r = pt_session_create(p.s, &so, &k.x);
    if (!r) r = pt_session_sync(k.x);   // (the session's init kernel)
    if (!r && tune_int("inject_fail", -1) == g) r = fail(PT_E_INVALID, "injected failure (PT_TUNE inject_fail)");
    return r;
}
// (diagnostics, same_device=2: the device busy before this rank's render, outside its time)
int rank_prespin(const RenderPlan& p, RankRun& k) {
    const int us = p.same == 2 ? tune_int("prespin_us", 0) : 0;
    if (us <= 0) return PT_OK;
    if (pt_launch_spin((uint32_t)us, 2048u, nullptr, k.x->stream) != hipSuccess)
        return fail(PT_E_HIP, "spin kernel launch failed");
    return pt_session_sync(k.x);
}
// the samples in chunks; rank 0 reports progress
int rank_render(const RenderPlan& p, int g, RankRun& k) {
    pt_session* x = k.x;
    if (g == 0 && p.in_pass) {
        const uint64_t total = owned_pixels(x) * p.S;
        x->on_progress = [bar = &k.bar, total](uint64_t n) { progress_bar(std::min(n, total), total, *bar); };
    }
    int r = PT_OK;
    for (uint32_t done = 0; !r && done < p.S;) {
        const uint32_t n = std::min(p.chunk, p.S - done);
        r = pt_session_trace(x, n);
        if (!r && (p.o.progress || p.ngpu > 1)) r = pt_session_sync(x);
        done += n;
        if (!r && g == 0 && p.o.progress) progress_bar(done, p.S, k.bar);
    }
    return r ? r : pt_session_sync(x);
}
// resolve on the device (tonemap + quantise into the packed 8-bit tiles)
int rank_resolve(const RenderPlan& p, RankRun& k) {
    pt_session* x = k.x;
    if (p.radiance && x->n_slots) {
        if (hipMalloc(&x->rad, 12ull * x->n_slots) != hipSuccess) return fail(PT_E_OOM, "radiance buffer");
    }
    return pt_session_resolve(x, nullptr, x->rad);
}
// One host thread per GPU sets up its session (the device's scene upload and the
// session buffers: devices in parallel) and drives it (the wavefront rounds sync
// on their own stream) through the resolve.
void run_rank(const RenderPlan& p, int g, RankRun& k, Turnstile& ts) {
    const auto t_g = Clock::now();
    int r = rank_set_up(p, g, k);
    k.setup = ms_since(t_g);
    k.wait = ts.set_up_and_wait(g);
    if (!r) r = rank_prespin(p, k);
    const auto t_r = Clock::now();
    if (!r) r = rank_render(p, g, k);
    k.render = ms_since(t_r);
    ts.rendered();
    const auto t_v = Clock::now();
    if (!r) r = rank_resolve(p, k);
    k.resolve = ms_since(t_v);
    if (r) k.failed(r);
}
void run_ranks(const RenderPlan& p, std::vector<RankRun>& ranks) {
    Turnstile ts(p.ngpu, p.same == 2);
    if (p.ngpu == 1) return run_rank(p, 0, ranks[0], ts);
    std::vector<std::thread> th;
    for (int g = 0; g < p.ngpu; ++g) {
        try {
            th.emplace_back(run_rank, std::cref(p), g, std::ref(ranks[(size_t)g]), std::ref(ts));
        } catch (const std::system_error&) {
            // a rank whose thread cannot start fails; it still counts as set up and
            // rendered, so the ranks of same_device=2 waiting for their turn go on
            ranks[(size_t)g].failed(fail(PT_E_INVALID, "cannot start the host thread of rank " + std::to_string(g)));
            ts.never_started();
        }
    }
    for (auto& t : th) t.join();
}

// A pinned staging buffer for the framebuffer's copy out (a device-to-pageable copy is staged
// by the runtime at a fraction of the link's rate), allocated on a thread of its own beside the
// render.  bytes = 0: none.  (No thread: the copy out goes through the device framebuffer.)
class Staging {
    std::thread th_;
    uint8_t* p_ = nullptr;
  public:
    explicit Staging(size_t bytes) {
        if (!bytes) return;
        try {
            th_ = std::thread([this, bytes] {
                void* q = nullptr;
                if (hipHostMalloc(&q, bytes, hipHostMallocDefault) == hipSuccess) p_ = static_cast<uint8_t*>(q);
            });
        } catch (const std::system_error&) {
        }
    }
    // the buffer, once its thread is done, or null
    uint8_t* get() { if (th_.joinable()) th_.join(); return p_; }
    ~Staging() { if (get()) (void)hipHostFree(p_); }
};

// The gather of the packed 8-bit tiles.  One session owns every tile: un-tiled on its device, one copy out
int gather_single(const RenderPlan& p, pt_session* x, uint8_t* rgb, uint8_t* staging, Clock::time_point t_gather) {
    if (!x->n_slots) return PT_OK;
    const uint32_t W = p.W, H = p.H, tiles_x = (W + 15u) / 16u;
    const double g0 = ms_since(t_gather);
    // (into the pinned staging buffer directly: the kernel's stores cross the link)
    if (hipSetDevice(x->dev) != hipSuccess ||
        pt_launch_untile(x->out, nullptr, tiles_x, W, H, staging ? staging : x->fb, x->stream) != hipSuccess ||
        (!staging && hipMemcpyAsync(rgb, x->fb, 3ull * W * H, hipMemcpyDeviceToHost, x->stream) != hipSuccess) ||
        hipStreamSynchronize(x->stream) != hipSuccess)
        return fail(PT_E_HIP, "framebuffer copy failed");
    const double g1 = ms_since(t_gather);
    if (staging) memcpy(rgb, staging, 3ull * W * H);
    if (stats_level() >= 3)
        fprintf(stderr, "gather ms: staging join %.1f untile+copy %.1f (%s) host copy %.1f\n", g0, g1 - g0,
                staging ? "kernel into pinned" : "copy engine", ms_since(t_gather) - g1);
    return PT_OK;
}
// every rank's packed tiles read back and un-tiled on the host
int gather_host(const RenderPlan& p, const std::vector<RankRun>& ranks, uint8_t* rgb) {
    for (int g = 0; g < p.ngpu; ++g) {
        pt_session* x = ranks[(size_t)g].x;
        if (!x->n_slots) continue;
        std::vector<uint8_t> packed(3ull * x->n_slots);
        if (const int rc = pt_session_read_packed(x, packed.data(), packed.size())) return rc;
        pt_unpack_tiles(p.W, p.H, (uint32_t)g, (uint32_t)p.ngpu, packed.data(), rgb);
    }
    return PT_OK;
}
// PT_GATHER_AUTO: RCCL when ngpu > 1 (host fallback with a warning, the reason in
// pt_last_error); PT_GATHER_RCCL: RCCL at any ngpu, an error if it fails;
// PT_GATHER_HOST: never RCCL.  (PT_TUNE inject_rccl=1: the AUTO fail-over at any ngpu;
// same_device: never RCCL.)  Into agg: gather_rccl and gather_allocs.
int gather_frame(const RenderPlan& p, const std::vector<RankRun>& ranks, uint8_t* rgb, Staging& staging,
                 Clock::time_point t_gather, pt_stats* agg) {
    const bool auto_rccl = p.ngpu > 1 || tune_int("inject_rccl", 0) != 0;
    const bool try_rccl = !p.same && (p.o.gather == PT_GATHER_RCCL || (p.o.gather == PT_GATHER_AUTO && auto_rccl));
    uint8_t* pinned = staging.get();
    if (try_rccl) {
        const int rc = gather_rccl(ranks, p.o.device, p.W, p.H, rgb, pinned, &agg->gather_allocs);
        agg->gather_rccl = rc == PT_OK;
        if (rc == PT_OK || p.o.gather == PT_GATHER_RCCL) return rc;
        fprintf(stderr, "pt_render: RCCL gather unavailable (%s); gathering through the host\n", pt_last_error());
    }
    return p.ngpu == 1 ? gather_single(p, ranks[0].x, rgb, pinned, t_gather) : gather_host(p, ranks, rgb);
}

// per-rank phase times (the CLI's PT_STATS=2): set-up = the device's scene upload (if
// this session did it) + the session's buffers and init kernel
int report_ranks(const std::vector<RankRun>& ranks, double gather_ms, bool rccl) {
    const int ngpu = (int)ranks.size();
    for (int g = 0; g < ngpu; ++g) {
        const RankRun& k = ranks[(size_t)g];
        pt_stats rs;
        if (const int rc = pt_session_stats(k.x, &rs)) return rc;
        fprintf(stderr, "pt_render rank %d/%d: setup_ms=%.1f scene_upload_ms=%.3f wait_ms=%.1f render_ms=%.1f "
                "resolve_ms=%.1f isect_ms=%.1f coop_ms=%.1f coop_launches=%llu rounds=%llu rays=%llu "
                "handed_on=%llu\n", g, ngpu, k.setup, k.x->upload_ms, k.wait, k.render, k.resolve, rs.isect_ms, rs.coop_ms,
                (unsigned long long)rs.coop_launches, (unsigned long long)rs.rounds,
                (unsigned long long)rs.rays, (unsigned long long)rs.handed_on);
    }
    fprintf(stderr, "pt_render gather_ms=%.1f path=%s\n", gather_ms, rccl ? "rccl" : "host");
    return PT_OK;
}

// rank g's radiance read back and un-tiled into the caller's image
int read_radiance(const RenderPlan& p, int g, const RankRun& k, float* radiance) {
    if (!k.x->n_slots) return PT_OK;
    std::vector<float> pr(3ull * k.x->n_slots);
    if (hipMemcpy(pr.data(), k.x->rad, pr.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(PT_E_HIP, "radiance readback failed");
    pt_unpack_tiles_f32(p.W, p.H, (uint32_t)g, (uint32_t)p.ngpu, pr.data(), radiance);
    return PT_OK;
}
}  // namespace
}  // namespace pti

using namespace pti;

extern "C" {

int pt_gather_init(int device, int ngpu) {
    if (ngpu < 1 || device < 0) return fail(PT_E_INVALID, "bad device range");
    if (tune_int("same_device", 0)) return PT_OK;   // (test-only mode: host gather)
    std::lock_guard<std::mutex> lk(g_comm_mu);
    CommSet* c = nullptr;
    return comm_get(device, ngpu, &c);
}

void pt_render_opts_default(pt_render_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->device = 0;
    o->ngpu = 1;
    o->traversal = PT_TRAVERSAL_REPLAY;
}

// options, refusals, staging, ranks, errors, gather, reports, radiance and stats
int pt_render(pt_scene* s, const pt_render_opts* opts, uint8_t* rgb, float* radiance, pt_stats* stats) {
    const auto t0 = Clock::now();
    if (!s) return fail(PT_E_INVALID, "null scene");
    int rc = pt_scene_prepare(s);
    if (rc) return rc;
    const RenderPlan p(s, opts, radiance != nullptr);
    if (p.o.gather == PT_GATHER_RCCL && p.same)
        return fail(PT_E_INVALID, "PT_GATHER_RCCL with PT_TUNE same_device: RCCL cannot place two ranks on one device");
    Staging staging(rgb && tune_int("staging", 1) ? 3ull * p.W * p.H : 0);
    std::vector<RankRun> ranks((size_t)p.ngpu);
    run_ranks(p, ranks);
    for (const RankRun& k : ranks)
        if (k.rc) return fail(k.rc, k.err);
    // gather the packed 8-bit tiles: over RCCL to device `o.device` when ngpu > 1, else one copy
    pt_stats agg;
    memset(&agg, 0, sizeof(agg));
    const auto t_gather = Clock::now();
    if (rgb && (rc = gather_frame(p, ranks, rgb, staging, t_gather, &agg))) return rc;
    const double gather_ms = ms_since(t_gather);
    if (stats_level() >= 2 && (rc = report_ranks(ranks, gather_ms, agg.gather_rccl != 0))) return rc;
    for (int g = 0; g < p.ngpu; ++g) {
        const RankRun& k = ranks[(size_t)g];
        if (radiance && (rc = read_radiance(p, g, k, radiance))) return rc;
        pt_stats st;
        if ((rc = pt_session_stats(k.x, &st))) return rc;
        merge_stats(agg, st);
    }
    if (p.o.progress) progress_bar(p.S, p.S, ranks[0].bar);
    agg.wall_ms = ms_since(t0);
    if (stats) *stats = agg;
    return agg.errors ? fail(PT_E_INVALID, "exactness guard tripped (a recomputed hit differs from its query's)") : PT_OK;
}

int pt_write_ppm(const char* path, uint32_t W, uint32_t H, const uint8_t* rgb) {
    if (!path || !rgb) return fail(PT_E_INVALID, "null argument");
    FILE* f = fopen(path, "wb");
    if (!f) return fail(PT_E_IO, std::string("cannot write ") + path);
    fprintf(f, "P6\n%u %u\n255\n", W, H);
    const size_t n = (size_t)W * H * 3;
    const bool ok = fwrite(rgb, 1, n, f) == n;
    if (fclose(f) != 0 || !ok) return fail(PT_E_IO, std::string("short write to ") + path);
    return PT_OK;
}

}  // extern "C"
