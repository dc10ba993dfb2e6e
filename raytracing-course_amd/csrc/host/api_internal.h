// api_internal.h -- what libpt's host units share (internal; not part of the C ABI).
//
// The C ABI of include/pt.h is implemented across these units:
//   common.cpp    errors, PT_TUNE, the RCCL loader, stream pools, device properties,
//                 the scene's device copy, pt_device_init
//   scene_api.cpp Scene::Load / InitScene equivalents: parse, reference BVH, aux BVH,
//                 the query blob (pt_scene_*)
//   session.cpp   tile sessions: set-up (geometry, arena), the megakernel pass, resolve, stats (pt_session_*)
//   wave_plan.cpp the wavefront pass's launch shapes and capacities (plan_wave: no device needed)
//   rounds.cpp    the wavefront pass: path rounds, early / final cooperative launches
//   render.cpp    Scene::Render equivalent, pt_render as its phases: the options resolved, the refusals, the
//                 pinned staging buffer, the ranks (a host thread and a session per GPU: set up, wait for
//                 its turn, render, resolve), their errors, the gather (RCCL / one session / host), the
//                 PT_STATS reports, the radiance read-back and the merged stats; PPM
//   qctx.cpp      what the batch contexts below share: set-up, launch shape, statistics, the event timer and
//                 (here, as templates) their creation and the one-shot host forms' chunk loop
//   rayq.cpp      the ray-query engine: closest-hit queries for the caller's rays (pt_rayq_*, pt_intersect)
//   featq.cpp     the first-hit feature engine: the closest hit and the hit primitive's scene data for the
//                 caller's image-plane positions, and for a session's pixel centres (pt_featq_*, pt_features,
//                 pt_session_features)
//   filtq.cpp     the guided filter of a frame: guides from the first-hit features of the pixel centres, one
//                 kernel launch per a-trous level (pt_filtq_*, pt_filter), and the same on the host
//                 (pt_selftest_filter_host)
//   pathq.cpp     the batch radiance engine: RayTrace for the caller's rays (pt_pathq_*, pt_radiance,
//                 pt_camera_rays)
//   pixq.cpp      the pixel-sample engine: Sample's loop for the caller's pixel states (pt_pixq_*,
//                 pt_sample_pixels, pt_pixel_init, pt_pixel_resolve)
//   states.cpp    a session's pixels out as pixel states and in again (pt_session_pixels / export / import),
//                 and the import's classification on the host (pt_selftest_state_slots)
//   counts.cpp    per-pixel sample counts in a session (pt_session_trace_counts / import_ragged /
//                 samples_range), and the slot -> record map on the host (pt_selftest_count_records)
//   noise.cpp     a session's own noise estimate and the adaptive step planned from it (pt_session_mark /
//                 noise / plan / refine), and the plan on the host (pt_selftest_refine_plan)
//   selftest.cpp  host execution of the device query / integrator code (one HostQuery, the twin of
//                 pt_batch.h's start_query and QStats, under every hook), and pt_selftest_math (the
//                 device code's scalar functions on the host or in k_selftest_math) (tests only; one
//                 hook, pt_selftest_wave_plan, is in session.cpp beside the set-up it reports, another,
//                 pt_selftest_fold_shape, in qctx.cpp)
#pragma once
#include "pt.h"

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

#include "../device/pt_coop.h"
#include "../device/pt_feats.h"
#include "../device/pt_filter.h"
#include "../device/pt_kernels.h"
#include "../device/pt_paths.h"
#include "../device/pt_pixels.h"
#include "../device/pt_rays.h"
#include "pt_scene.h"

#pragma GCC visibility push(hidden)

namespace pti {

// the message of the last failure on this thread (pt_last_error)
int fail(int code, const std::string& msg);
const std::string& last_error();

// PT_TUNE="key=value,..." (the keys are listed in common.cpp and INTEGRATION.md)
std::string tune_str(const char* key);
bool tune_has(const char* key);
int tune_int(const char* key, int def);
// PT_STATS=N (the CLI's phase reports): N, or 0 when unset
int stats_level();

// RCCL, loaded on first use (dlopen): only the multi-GPU gather needs it
struct Rccl {
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclGather) Gather = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool ok = false;
};
const Rccl& rccl();

// streams: per-device pools (pt_device_init makes one ahead of time; sessions take
// streams from the pools and give them back).  side = the early cooperative launch's
// stream, from a pool of greatest-priority streams (common.cpp has the reason).
hipError_t take_stream(int dev, hipStream_t* s, bool side = false);
void give_stream(int dev, hipStream_t s, bool side);

// A scene's device copy: ONE allocation holding the query blob (which also holds
// the reference nodes, primitives and ancestor lists the other kernels read:
// the views below point into it), the shading records, the plane and emitter
// lists, the gamma thresholds and k_wcamera's copy of the aux BVH's top two
// levels -- uploaded with one copy from one host image.  The BVH2 aux (the
// megakernel's traversal) is uploaded on first use only.
struct DevScene {
    unsigned char* base = nullptr;
    const pt::F4* blob = nullptr;
    const pt::Node* nodes = nullptr;
    const pt::Prim* prims = nullptr;
    const uint32_t* anc_info = nullptr;
    const uint32_t* anc = nullptr;
    const pt::Shade* shade = nullptr;
    const uint32_t* planes = nullptr;
    const uint32_t* emitters = nullptr;
    const float* thr = nullptr;
    const pt::AuxSL* top = nullptr;   // aux root entries + their child nodes' entries (k_wcamera)
    uint32_t n_top = 0;
    pt::AuxNode* aux = nullptr;       // BVH2 aux (megakernel only)
};
struct DevEntry {
    std::mutex mu;                    // this device's upload (devices upload in parallel)
    bool ready = false;
    DevScene d;
};

constexpr uint32_t kCandCap = 24;   // candidate-list words per lane (per replay pass)

// device properties, queried once per device
struct DevProps { bool ok = false; int cus = 0; char arch[64] = {0}; double props_ms = 0.0; };
int device_props(int dev, DevProps* out);
int check_device(int dev);
int ensure_device_scene(pt_scene* s, int dev, bool mega, DevScene** out, double* upload_ms);
void free_device_scene(DevScene& d);

// scene views (scene_api.cpp)
pt::ReplayCfg replay_cfg(const pt_scene* s);
uint32_t lane_words(const pt_scene* s, int traversal);
void set_blob(pt::SceneView& v, const pt_scene* s, const pt::F4* blob);
pt::SceneView host_view(const pt_scene* s, int traversal);
pt::CamView make_cam(const pt_scene* s);

// fn(begin, end, part) over [0, n) in at most `parts` contiguous chunks, one thread each
// (host preparation loops whose items are independent).  A thread that cannot be
// started leaves its chunk to the calling thread.
template <class F>
void parallel_chunks(size_t n, unsigned parts, F fn) {
    parts = std::max(1u, std::min<unsigned>(parts, (unsigned)((n + 8191) / 8192)));
    if (parts == 1) { fn((size_t)0, n, 0u); return; }
    std::vector<std::thread> th;
    std::vector<unsigned> here;
    for (unsigned k = 0; k < parts; ++k) {
        try {
            th.emplace_back(fn, n * k / parts, n * (k + 1) / parts, k);
        } catch (const std::system_error&) {
            here.push_back(k);
        }
    }
    for (unsigned k : here) fn(n * k / parts, n * (k + 1) / parts, k);
    for (auto& t : th) t.join();
}
unsigned prep_threads();

// sessions (session.cpp, rounds.cpp)
double wall_ms();
int finish_pending(pt_session* ss);
std::vector<uint32_t> rank_tiles(uint32_t n_tiles, uint32_t tiles_x, uint32_t rank, uint32_t world);
uint64_t owned_pixels(const pt_session* ss);
// a session's geometry without a device (tm -- its gtile left null --, gtiles, n_tiles_local, n_slots)
int session_geometry_only(pt_scene* s, const pt_session_opts* o, pt_session* ss);
hipError_t read_counters(pt_session* ss, unsigned long long c[PT_CTR_STRIDE]);
int flush_trace(pt_session* ss);
int trace_wave(pt_session* ss, uint32_t spp);
// states.cpp: the state-exchange buffers (made at the first use), and an import's validation of the
// caller's n records -- nothing of the session written; res: the SR_* words of pt_states.h
std::vector<uint32_t> tile_records(const pt_session* ss);   // the export's first record of every local tile
int ensure_export(pt_session* ss);
int validate_import(pt_session* ss, uint64_t n, const pt_pixel_state* dev_state, unsigned long long* res);
int check_state_pointer(const void* p);
// a device buffer of n records for the host-pointer forms
struct DevRecords {
    void* p = nullptr;
    ~DevRecords() { (void)hipFree(p); }
    int alloc(uint64_t n);
};
// counts.cpp: a ragged session's lag table (null: none yet), zeroed -- the session is uniform again;
// the resolve with every pixel's own count (a ragged session's pt_session_resolve launch)
uint32_t* lag_table(const pt_session* ss);
hipError_t clear_lag(pt_session* ss);
hipError_t launch_ragged_resolve(pt_session* ss, uint8_t* out, float* rad);
// ... the table's making (all zero) at the first ragged call, the refusal of a megakernel session, and
// the pass of an accepted set of counts -- their sum (above 0), the largest and the smallest count a
// pixel stands at after them -- with its lag bookkeeping (pt_session_trace_counts, pt_session_refine)
int ensure_lag(pt_session* ss);
int refuse_megakernel(const pt_session* ss);
int counts_pass(pt_session* ss, const uint32_t* dev_counts, unsigned long long sum, unsigned long long total_max,
                unsigned long long total_min);
// noise.cpp: every pixel's mark cleared -- no pixel has a noise estimate (no table yet: nothing to do)
hipError_t clear_marks(pt_session* ss);
pt::SceneView device_view(const pt_session* ss);
pt::SceneView device_view(const pt_scene* s, const DevScene& ds);   // ... of any device copy (rayq.cpp)
// the hand-off site named `name` (PT_HO_*: "suspend", "flush", "ringout", "exact", "side_take",
// "side_yield", "side_handon", "grow_yield", "grow_handon"), or -1
int handoff_site(const char* name);
// the summed counter block's slots CTR_RAYS .. CTR_FALLBACKS_RAY as pt_stats' rays .. fallbacks_ray
void counter_stats(const unsigned long long* c, pt_stats* st);
// a rank's pt_session_stats into a render's: every field by its rule (session.cpp, beside pt_session_stats)
void merge_stats(pt_stats& into, const pt_stats& rank);

// The wavefront pass's launch shapes and capacities (wave_plan.cpp): fixed at session creation,
// a function of the scene's tree facts, the CU count, the owned pixels and PT_TUNE.  (Run state
// and device pointers are pt_session's.)
struct WavePlan {
    uint32_t shade_grid = 0;      // (read by no launch: path rounds run k_wshade on 64 workgroups)
    uint32_t path_budget = 1024, path_ticks = 0, low_ticks = 0;
    // the full rounds' shape: query waves per workgroup (PT_TUNE nq: 2 or 3) and its grid; path_grid is
    // the grid of the NQ = 2 launches (low-chain rounds at most low_grid of it, the sparse kernel)
    uint32_t full_nq = PT_NQ_FULL, path_grid = 0, full_grid = 0;
    uint32_t carry_words = 0;     // words of a suspended query's record
    uint32_t lane_cap = 0;        // min(pixels, query lanes): what one round can suspend
    uint32_t carry_cap = 0;       // ... and what the early launch yields besides: the carry queue's entries
    bool runend_auto = false;     // path_runend follows the launch's shape (a few chains per query wave)
    uint32_t path_runend = 0, path_sparse = 0, sparse_steps = 8;
    uint32_t coop_max = 0, coop_grid = 0, coop_reserve = 0;   // cooperative engine (k_wcoop) at the end of a pass
    uint32_t coop_team = 4;       // lanes per chain in the cooperative engine (pure-coop rate, teams of
                                  // 64 / 32 / 16 / 8: 283 / 392 / 572 / 815 Mray/s; the final launch in
                                  // teams of 4 against 8, rank 0 of 1 / 8: 475.9 / 74.7 ms against
                                  // 476.3 / 79.2, means of 5 interleaved runs, profiles/r06_coop/team4)
    bool coop_order = true;       // the cooperative engine takes the pixels furthest from the target first
    uint32_t coop_grow = 0;       // the final launch's last chains handed to whole-wave teams (0: never)
    uint32_t coop_grow_mid = 0;   // ... and an earlier stage of teams of 32 (0: none)
    uint32_t round_batch = 1;     // rounds launched per count while the chains are far above the hand-over
    // early cooperative launch: once a pass's chains fall below early_at, the early_k chains
    // with the most samples left run in a cooperative launch on a second stream (early_wg
    // workgroups per CU, beside the path engine's low-chain rounds) to the end of the pass
    uint32_t early_wg = 1, early_at = 0, early_k = 0, side_team = 8;
    // k_wpath's per-trip step mix: {probe_every, probe_min, aux_extra, end_min}, and the one of
    // rounds that start with fewer than lowq chains (latency-bound: few chains per lane)
    uint32_t mix[4] = {PT_PROBE_EVERY, PT_PROBE_MIN, PT_AUX2, PT_END_MIN},
             mix_low[4] = {PT_PROBE_EVERY, PT_PROBE_MIN, PT_AUX2, PT_END_MIN_LOW};
    uint32_t lowq = 0;
    uint32_t low_grid = 0;        // path workgroups of those rounds
    // a scene beyond the cooperative engine's LDS tables (RAY_DEPTH > QC_FOLD, more than
    // QC_NPL planes or QC_NEM emitters) runs its BIG instantiation
    bool big = false;
};
struct PlanInputs {
    uint32_t cus = 0;                                     // the device's compute units
    uint32_t n_slots = 0, n_tiles_local = 0, depth = 0;   // the session's pixels and RAY_DEPTH
    uint32_t n_planes = 0, n_emitters = 0;
    uint32_t auxw_stack = 0, auxsl_depth = 0, max_stack = 0, n_aux = 0;   // the scene's tree facts (pt_scene)
};
// PT_OK, or PT_E_INVALID for a PT_TUNE value no plan has (nq)
int plan_wave(const PlanInputs& in, WavePlan* out);
// the plan as "key=value" lines, a line per field (pt_selftest_wave_plan)
std::string plan_text(const WavePlan& w);
// a path round's launch shape: query waves per workgroup, workgroups, and the chains a
// workgroup holds at most.  Full rounds (at least lowq chains, not the sparse kernel) run the
// plan's full shape; low-chain rounds, the sparse kernel and a round beside the early
// cooperative launch (`side`: its workgroup's LDS must fit beside the round's) NQ = 2.
struct PathShape { uint32_t nq, grid, cmax; };
PathShape path_shape(const WavePlan& w, uint32_t chains, bool sparse, bool side);

static_assert(pt::HO_SUSPEND == PT_HO_SUSPEND && pt::HO_FLUSH == PT_HO_FLUSH && pt::HO_RINGOUT == PT_HO_RINGOUT &&
                  pt::HO_EXACT == PT_HO_EXACT && pt::HO_SIDE_TAKE == PT_HO_SIDE_TAKE &&
                  pt::HO_SIDE_YIELD == PT_HO_SIDE_YIELD && pt::HO_SIDE_HANDON == PT_HO_SIDE_HANDON &&
                  pt::HO_GROW_YIELD == PT_HO_GROW_YIELD && pt::HO_GROW_HANDON == PT_HO_GROW_HANDON &&
                  pt::HO_N == PT_HO_N && PT_HO_N <= 12 && pt::CTR_HO + PT_HO_N <= PT_CTR_STRIDE,
              "hand-off sites: device and ABI numbering differ");

}  // namespace pti

#define HIP_TRY(expr)                                                                                 \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return pti::fail(PT_E_HIP, std::string(#expr " failed: ") + hipGetErrorString(e_));       \
    } while (0)

struct pt_scene {
    pth::HScene hs;
    bool prepared = false;
    std::vector<pth::HNode> nodes;
    uint32_t n_bvh = 0;
    std::vector<uint32_t> planes, emitters;
    std::vector<pt::Node> dnodes;
    std::vector<pt::Prim> dprims;
    std::vector<pt::Shade> dshade;
    std::vector<pt::AuxNode> aux;
    std::vector<pt::AuxSL> auxsl;
    uint32_t tree_depth = 0, max_stack = 0, aux_depth = 0, auxsl_depth = 0;
    float box_extent = 0.f;     // max |coordinate| of the reference node boxes
    std::vector<uint32_t> anc_info, anc;   // per-leaf ancestor lists (replay walk)
    std::vector<pt::F4> blob;   // the wavefront query's fetch space (pt_core.h SceneView::blob)
    uint32_t o_nodes = 0, o_aux = 0, o_ainfo = 0, o_anc = 0, o_qprim = 0, o_prim = 0, o_bundle = 0;
    uint32_t auxw_stack = 0;    // per-lane stack words of the wide aux traversal
    uint32_t aux_rshift = 0;    // leaf-range packing of the wide aux entries (annotate_aux_ranges)
    std::vector<float> regions;   // per reference node: its leaf's hit region {lo, hi} (lo > hi: unbounded)
    uint32_t aux_coarse_leaves = 0;   // leaf entries whose binary16 own box is > 4x wider than the f32 one
    float thr[256];
    // the device-only sections of the blob (byte offsets; the device copy is the blob)
    size_t i_shade = 0, i_planes = 0, i_emit = 0, i_thr = 0, i_top = 0;
    uint32_t n_top = 0;
    std::map<int, std::unique_ptr<pti::DevEntry>> dev;
    std::mutex mu;                    // the image and the device map (not the uploads)
};

struct pt_session {
    pt_scene* sc = nullptr;
    int dev = 0;
    const pti::DevScene* ds = nullptr;   // the scene's copy on this device
    double upload_ms = 0.0;         // time this session spent uploading it (0: already there)
    pt::TileMap tm{};
    uint32_t n_tiles_local = 0, n_slots = 0, depth = 0;
    pt::PixelState st{};          // per-slot records + fold records (device)
    unsigned long long* counters = nullptr;
    uint8_t* out = nullptr;
    uint8_t* fb = nullptr;            // rank 0: the window's row-major framebuffer (device)
    float* rad = nullptr;
    unsigned long long* wg_prof = nullptr;
    // wavefront engine (replay traversal): its plan, fixed at creation, and its buffers
    bool wave = false;
    pti::WavePlan plan;
    uint32_t* order = nullptr;    // 2 x 256 bucket counters + the intake order (a round's work: <= pixels)
    // the early cooperative launch (plan.early_k chains on a second stream)
    pt::RayQ side = {};           // its queue (early_k entries) ...
    uint32_t* side_carry = nullptr;   // ... its suspended queries' restart records (early_k x carry_words)
    uint32_t* side_ctl = nullptr;     // ... and its two round-counter sets
    hipStream_t side_stream = nullptr;
    hipEvent_t side_taken = nullptr, side_end = nullptr;   // its queue is taken / it has stopped
    std::thread side_th;          // makes the three above (joined before their first use)
    hipError_t side_rc = hipSuccess;
    // every device buffer below lives in one allocation (pt_session_create)
    unsigned char* arena = nullptr;
    size_t arena_bytes = 0;
    pt::RayQ fq[2] = {};          // fresh rays (n_slots each)
    pt::DoneQ done = {};          // exact-DFS results (n_slots)
    pt::RayQ ex = {};             // rays handed to the exact DFS (n_slots)
    uint32_t* carry = nullptr;    // 2 * plan.carry_cap * plan.carry_words
    uint2* endq = nullptr;        // grid * path_cmax(nq) of the larger shape: the shade waves' ended paths
    unsigned long long short_seen = 0;   // CTR_SHORT at the last resolve
    uint32_t* ctl = nullptr;      // 2 x PT_CTL_SET round counters
    uint32_t* ctl_host = nullptr; // pinned copy of one counter set
    double roundlog_t = 0.0;      // (roundlog>=2: the last round's end, host clock, and the rays by then)
    unsigned long long roundlog_rays = 0;
    uint32_t rounds = 0;
    hipStream_t stream = nullptr;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;   // the passes' event pairs (kernel_ms)
    struct LaunchEvents {
        hipEvent_t e0, e1;
        bool coop;                // a cooperative-engine launch (coop_ms)
    };
    std::vector<LaunchEvents> pending_isect;   // the rounds' launches (isect_ms)
    double kernel_ms = 0.0, resolve_ms = 0.0, isect_ms = 0.0, coop_ms = 0.0;
    uint64_t isect_launches = 0, coop_launches = 0;
    uint64_t samples_done = 0;
    uint32_t deferred_spp = 0;    // wavefront engine: trace() calls not yet run (one pass at the next sync point)
    uint32_t* tile_order = nullptr;   // local tiles in Z-order of their image position (k_wcamera)
    std::vector<uint32_t> gtiles;     // this rank's window tiles (local -> window tile), tm.gtile on the device
    // optional progress report during a pass (pt_render's bar): finished samples,
    // counted by the kernels into host-mapped memory and polled at the round syncs
    std::function<void(uint64_t)> on_progress;
    unsigned long long* prog_host = nullptr;
    unsigned long long* prog_dev = nullptr;
    pt::CamView cam{};
    int traversal = PT_TRAVERSAL_REPLAY;
    // state exchange (states.cpp), allocations of their own made at the first export / import:
    // the export's first record per local tile; the import's result block and per-slot marks
    uint32_t* state_tile_rec = nullptr;
    unsigned char* state_marks = nullptr;
    // per-pixel sample counts (counts.cpp), allocations of their own made at the first
    // ragged call: the result block with the per-slot lag table behind it -- every owned pixel's
    // `done` stands at samples_done, its own count is samples_done - lag[slot] --, and the host
    // form's copy of the caller's counts.  lag_sum / lag_max: the owned slots' lags, summed and
    // their largest (0: every pixel stands at samples_done, the session is uniform)
    unsigned char* counts_block = nullptr;
    uint32_t* counts_host_copy = nullptr;
    uint64_t lag_sum = 0;
    uint32_t lag_max = 0;
    // the session's noise estimate (noise.cpp), an allocation of its own made at the first
    // noise call: a plan's result block, every slot's mark (the sum and the count it held when marked;
    // all zero: no mark), and a word per slot for a step's counts and the host forms' outputs
    unsigned char* noise_block = nullptr;
    // first-hit features (featq.cpp), made at the first pt_session_features: a feature
    // context of the session's scene and device for its owned pixels, and their centres in the export's order
    pt_featq* feat_q = nullptr;
    pt::FeatXY* feat_xy = nullptr;
};

namespace pti {

// The events around a context's last run and the time they add up to (qctx.cpp).
struct RunTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;   // around the last run's kernels
    bool pending = false;           // ... whose time has not been added to kernel_ms yet
    double kernel_ms = 0.0;         // since the context's last *_stats
    bool create();                  // the two events (false: hipEventCreate failed)
    // the time of the last run's kernels, once they have finished (also: what the run used is free)
    int settle();
    void destroy();                 // waits for a pending run, which still uses the context's arena
};

// What every batch context is (qctx.cpp): the scene's copy on one device, one arena -- the run's
// control block | the statistics counters | the engine's own tail --, the launch shape and the run
// state.  An engine's context is this and its parameter block `p`: the view of the device copy and
// the arena's pieces, the per-run members filled by its *_run.
struct QueryCtx {
    pt_scene* sc = nullptr;
    int dev = 0;
    uint64_t max_items = 0;
    unsigned char* arena = nullptr;
    unsigned long long* counters = nullptr;   // PT_CTR_COPIES x PT_CTR_STRIDE, in the arena behind the control block
    uint32_t block = 256, max_grid = 1;   // the kernel's workgroup (its lanes' stacks fit the LDS) and the resident grid
    uint32_t per_cu = 0;   // the workgroups per compute unit the shape started from (pt_selftest_ctx_shape reports it)
    RunTimer t;
    unsigned long long seen[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // the counters at the last *_stats
};

}  // namespace pti

// rayq.cpp, k_rays: the tail is the exact list (max_items words); p's rays, hits, n, batch: per run
struct pt_rayq : pti::QueryCtx { pt::RaysParams p{}; };
// featq.cpp, k_feats: p holds the camera besides; the tail as pt_rayq's; xy, out, n, batch: per run
struct pt_featq : pti::QueryCtx { pt::FeatsParams p{}; };
// pathq.cpp, k_paths: the tail is the resident lanes' fold records, which max_grid is sized with; in, out, n, batch: per run
struct pt_pathq : pti::QueryCtx { pt::PathsParams p{}; };
// pixq.cpp, k_pixels: p holds the camera besides; the tail as pt_pathq's; state, counts, spp, n, batch: per run
struct pt_pixq : pti::QueryCtx { pt::PixelsParams p{}; };

// A filter context (filtq.cpp): a window's guides and the two colour buffers the levels alternate between.
struct pt_filtq {
    pt_scene* sc = nullptr;
    int dev = 0;
    uint32_t x0 = 0, y0 = 0, w = 0, h = 0;
    // one allocation: the guides (32 B per pixel) | two sets of 16-B colours
    unsigned char* arena = nullptr;
    const float* thr = nullptr;     // the scene's gamma thresholds on the device
    pti::RunTimer t;
    uint64_t guide_points = 0;      // traced for the guides since the last pt_filtq_stats
};

namespace pti {

// ---- the batch contexts' core (qctx.cpp): each rule of set-up, shape, statistics and the one-shot
// host forms stated once
constexpr size_t kQCtrBytes = PT_CTR_COPIES * PT_CTR_STRIDE * sizeof(unsigned long long);
// *_create's checks -- the scene, the range of `max_items` (the message names the caller's
// parameter, `name`) and the device --, then the prepared scene's copy on the device (made current)
// and its compute units
int qctx_open(pt_scene* s, int device, uint64_t max_items, const char* name, DevScene** ds, uint32_t* cus);
// A lane's stack words: the aux stack as deep as the wide aux tree can need (so no query outgrows
// it: Query::sp counts it in 7 bits, pt_scene_prepare rejects deeper trees), and the exact DFS's
struct LaneWords { uint32_t aux_words, dfs_words; };
LaneWords lane_words(const pt_scene* s);
// The widest workgroup, from *block down to 64 threads, whose lanes' LDS columns (pt_batch.h
// lane_lds_bytes) fit a workgroup's LDS; false: not even 64 lanes' do (*block is 64 then)
bool fit_block(uint32_t aux_words, uint32_t dfs_words, uint32_t* block);
// The shape of an engine without fold records (k_rays, k_feats: the lanes hold the aux stack only, the
// exact kernel's one wave the DFS stack): the block fit of both (PT_E_SCENE), and every workgroup a
// compute unit can hold at 8 waves per SIMD (a workgroup that starts after the work counter has
// passed n leaves at once); q's block, per_cu and max_grid set
int rays_shape(QueryCtx* q, LaneWords w, uint32_t cus);
// The resident grid of an engine with fold records (RAY_DEPTH x 16 B per resident lane): per_cu
// workgroups on each compute unit, unless the fold area then exceeds 1 GiB -- fewer workgroups then,
// after that narrower ones, down to one wave per compute unit; PT_E_OOM where that is still too much
struct GridShape { uint32_t block, max_grid; };
int fold_shape(uint32_t cus, uint32_t per_cu, uint32_t block, uint32_t depth, GridShape* out);
// ... for a context: the block fit (PT_E_SCENE), `occupancy` asked for `kernel` (what the compiler's
// registers and the LDS let a compute unit hold: the waves are persistent, a workgroup beyond that
// would start when another has left, and find no work), fold_shape; q's block and max_grid set, the
// fold area's size in *fold_bytes
int qctx_fold_shape(QueryCtx* q, LaneWords w, uint32_t cus, uint32_t depth,
                    hipError_t (*occupancy)(uint32_t, uint32_t, uint32_t, int*), const char* kernel, size_t* fold_bytes);
// The arena -- ctl_bytes | counters | tail_bytes --, control block and counters zeroed, and the
// timer's events.  `what` names the engine in the messages; alloc_fail_code is the code of a failed hipMalloc
int qctx_alloc(QueryCtx* q, size_t ctl_bytes, size_t tail_bytes, const char* what, int alloc_fail_code);
// A run's shape: no more workgroups than the resident grid or than n needs; and the items a wave
// reserves per pull of the work counter: an eighth of its share, from a full wave to 512
// (same-address atomics serialise chip-wide: one per item-sized refill would set the rate)
struct RunShape { uint32_t grid, batch; };
RunShape qctx_shape(const QueryCtx* q, uint64_t n);
// *_stats: the settled time and the counters' first n_counters slots, summed over the copies, since
// the last call (c, if given: those n_counters differences), as pt_stats
int qctx_stats(QueryCtx* q, uint32_t n_counters, pt_stats* st, unsigned long long* c = nullptr);
void qctx_close(QueryCtx* q);   // the pending run waited for, events and arena freed (q itself stays)

// *_create: the checks and the device copy, a new context, `fill` for the engine's own set-up
// (int fill(Q*, const DevScene&, uint32_t cus)); the context freed again where that fails
template <class Q, class Fill>
int qctx_create(pt_scene* s, int device, uint64_t max_items, const char* name, Q** out, Fill fill) {
    if (!s || !out) return fail(PT_E_INVALID, "null argument");
    DevScene* ds = nullptr;
    uint32_t cus = 0;
    int rc = qctx_open(s, device, max_items, name, &ds, &cus);
    if (rc) return rc;
    Q* q = new Q();
    q->sc = s;
    q->dev = device;
    q->max_items = max_items;
    if ((rc = fill(q, *ds, cus))) {
        qctx_close(q);
        delete q;
        return rc;
    }
    *out = q;
    return PT_OK;
}
template <class Q>
void qctx_free(Q* q) {
    if (!q) return;
    qctx_close(q);
    delete q;
}

// host <-> device copies of the one-shot forms (`what` failed: PT_E_HIP)
int copy_up(void* dev, const void* host, size_t bytes, const char* what);
int copy_down(void* host, const void* dev, size_t bytes, const char* what);

// A context kind's public calls, for run_chunks
template <class Q>
struct QueryApi {
    int (*create)(pt_scene*, int, uint64_t, Q**);
    int (*stats)(Q*, pt_stats*);
    void (*free)(Q*);
};
// The one-shot host forms (pt_intersect, pt_radiance, pt_sample_pixels, pt_features): a context
// for chunks of at most 2^22 items, two device buffers of item_bytes[k] per item (0: none, the
// pointer stays null), then per chunk `up(d, at, m)`, `run(q, d, m)` on the null stream -- which
// orders the copies around the run --, `down(d, at, m)`; the context's stats into `stats` if given.
// buf_fail / buf_msg: a failed buffer hipMalloc's code and message.
template <class Q, class Up, class Run, class Down>
int run_chunks(pt_scene* s, int device, uint64_t n, pt_stats* stats, const QueryApi<Q>& api, size_t item_bytes0,
               size_t item_bytes1, int buf_fail, const char* buf_msg, Up up, Run run, Down down) {
    constexpr uint64_t kChunk = 1ull << 22;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return PT_OK;
    const uint64_t cap = std::min(n, kChunk);
    Q* q = nullptr;
    int rc = api.create(s, device, cap, &q);
    if (rc) return rc;
    const size_t item_bytes[2] = {item_bytes0, item_bytes1};
    void* d[2] = {nullptr, nullptr};
    auto done = [&](int code) {
        (void)hipFree(d[0]);
        (void)hipFree(d[1]);
        api.free(q);
        return code;
    };
    for (int k = 0; k < 2; ++k)
        if (item_bytes[k] && hipMalloc(&d[k], cap * item_bytes[k]) != hipSuccess) return done(fail(buf_fail, buf_msg));
    for (uint64_t at = 0; at < n; at += cap) {
        const uint64_t m = std::min(cap, n - at);
        if ((rc = up(d, at, m)) || (rc = run(q, d, m)) || (rc = down(d, at, m))) return done(rc);
    }
    if (stats && (rc = api.stats(q, stats))) return done(rc);
    return done(PT_OK);
}

}  // namespace pti

#pragma GCC visibility pop
