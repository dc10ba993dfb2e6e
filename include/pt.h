/* pt.h -- C ABI of the MI355X-native hw5 path tracer (libpt.so).
 *
 * Drop-in boundary for the reference's render path.  The reference
 * (FeggieBoss/raytracing-course, hw5) has no plugin/FFI seam: its callers are
 * the CLI (hw5/run.sh:1-2 -> hw5/src/main.cpp:6-17) and the in-process trio
 *     Scene::Load(std::istream&)   hw5/include/scene.h:76, src/sceneload.cpp:112-176
 *     Scene::InitScene()           hw5/include/scene.h:78, src/scene.cpp:7-40
 *     Scene::Render(std::ostream&) hw5/include/scene.h:79, src/scene.cpp:205-252
 * Each entry point below names the reference interface it replaces.  Plain
 * pointers and sizes only; no C++/torch types cross this boundary.
 *
 * Conventions: functions return PT_OK (0) or a negative PT_E* code; the
 * message of the last failure on the calling thread is pt_last_error().
 * The caller owns every output buffer; the library owns scenes, sessions and
 * all device memory (released by pt_scene_free / pt_session_free).
 * Rendering requires a gfx950 GPU: there is no CPU fallback (PT_E_NO_GPU).
 */
#ifndef PT_H
#define PT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 6   /* 2: pt_render_opts.gather; 3: pt_stats per-engine (coop_*) fields;
                              4: pt_gather_init, and the session tile deal changed from tile
                              t -> rank t % world to tile (tx, ty) -> rank (tx + ty) % world
                              (local tiles still in ascending tile order): a driver that
                              un-interleaves packed tiles itself must use pt_unpack_tiles
                              (or ptrace.rank_tiles), not its own formula;
                              5: pt_stats.short_pixels / handed_on, and pt_session_resolve fails
                              when an owned pixel's sample count differs from the samples traced;
                              6: pt_stats.gather_allocs (the RCCL gather keeps its buffers per
                              communicator), pt_session_reset */

enum {
    PT_OK = 0,
    PT_E_INVALID = -1,   /* bad argument / state */
    PT_E_IO = -2,        /* file cannot be read / written */
    PT_E_SCENE = -3,     /* scene the reference cannot render either (no non-plane
                            primitive, bad primitive type, zero sizes) */
    PT_E_NO_GPU = -4,    /* no usable gfx950 device */
    PT_E_HIP = -5,       /* HIP runtime error */
    PT_E_RCCL = -6,      /* RCCL error (multi-GPU gather) */
    PT_E_OOM = -7
};

typedef struct pt_scene pt_scene;
typedef struct pt_session pt_session;

/* Scene::Load: parse a hw5 scene text file with the reference's exact grammar
 * and quirks.  Unknown commands produce a warning on stderr like
 * the reference (src/sceneload.cpp:170-172). */
int pt_scene_load(const char* path, pt_scene** out);
/* same, from memory (text, len bytes) */
int pt_scene_load_mem(const char* text, size_t len, pt_scene** out);

/* Scene::InitScene: std::partition of planes to the end, the reference BVH
 * (bit-faithful: same node boxes, preorder and primitive order), the emitter
 * list, and the device-side layouts.  Host-only; no GPU needed. */
int pt_scene_prepare(pt_scene* s);

/* Optional start-up of the HIP runtime on `device`: context creation and the
 * kernels' code objects (no launch).  No reference counterpart: a caller may run
 * it on a second thread while Scene::Load / InitScene parse and build on the
 * CPU, so the runtime's start-up does not add to the wall-clock (cli/main.cpp).
 * pt_render does the same work itself when it has not been done. */
int pt_device_init(int device);

/* Optional creation of the RCCL communicator that pt_render(ngpu = n, gather RCCL)
 * uses over devices device .. device+n-1 (ncclCommInitAll, cached per process).  No
 * reference counterpart (the reference renders on one host): the CLI runs it on its
 * start-up thread beside Scene::Load / InitScene, so the communicator's set-up is not
 * paid between the render and the PPM.  pt_render creates it itself otherwise. */
int pt_gather_init(int device, int ngpu);

typedef struct pt_scene_info {
    uint32_t width, height, samples, ray_depth;
    uint32_t n_prims, n_bvh_prims, n_planes, n_emitters;
    uint32_t n_nodes, tree_depth, max_stack;   /* max_stack = max pending right children */
    uint32_t n_aux_nodes, aux_depth;
    uint32_t n_warnings;
} pt_scene_info;
int pt_scene_get_info(const pt_scene* s, pt_scene_info* info);

/* Override DIMENSIONS / SAMPLES / RAY_DEPTH after loading (0 keeps the value). */
int pt_scene_override(pt_scene* s, uint32_t width, uint32_t height, uint32_t samples, uint32_t ray_depth);

/* BVH fingerprint dump (after prepare), reference layout of SURVEY §8c:
 * nodes: per node 6 f32 (min.xyz, max.xyz) + 4 u32 (left, right, first, count) = 40 B;
 * prims: per primitive u32 type + 9 f32 (a, b, c; b/c zero unless TRIANGLE) + 3 f32 pos = 52 B. */
int pt_scene_dump_bvh(const pt_scene* s, void* nodes_out, size_t nodes_bytes, void* prims_out, size_t prims_bytes);

void pt_scene_free(pt_scene* s);

/* ---------------------------------------------------------------- render */
enum {
    PT_TRAVERSAL_REPLAY = 0, /* default: candidate replay -- auxiliary BVH enumerates the reference
                                leaves the ray can reach, the reference's exact pruning is replayed
                                on their root paths only (bit-identical results) */
    PT_TRAVERSAL_EXACT = 1,  /* full reference-tree stack DFS, exact pruning semantics */
    PT_TRAVERSAL_REPLAY_DIV = 2 /* candidate replay with the reference's IEEE-division slab test at
                                   every node (the unfiltered form; same results, slower) */
};

typedef struct pt_render_opts {
    int32_t device;          /* first HIP device (default 0) */
    int32_t ngpu;            /* GPUs driven by this process (default 1); >1 = pixel tiles
                                dealt round-robin + RCCL gather of the framebuffer */
    uint32_t spp_per_launch; /* samples per kernel launch (0 = auto) */
    uint32_t samples;        /* 0 = the scene's SAMPLES */
    int32_t traversal;       /* PT_TRAVERSAL_* */
    int32_t progress;        /* 1 = print the reference's "Loading: [...]" bar to stdout */
    uint32_t win_x0, win_y0; /* optional window: render only [x0,x0+w) x [y0,y0+h) of the */
    uint32_t win_w, win_h;   /* image, keeping global-index seeds (win_w = 0: full image) */
    int32_t gather;          /* PT_GATHER_*: how the framebuffer tiles reach the caller */
} pt_render_opts;
enum {
    PT_GATHER_AUTO = 0,      /* default: RCCL (ncclGather over xGMI) when ngpu > 1, host copy if RCCL fails */
    PT_GATHER_RCCL = 1,      /* RCCL at any ngpu (also ngpu = 1: a one-rank communicator); failure is an error */
    PT_GATHER_HOST = 2       /* per-device copies through the host, never RCCL */
};
void pt_render_opts_default(pt_render_opts* o);

typedef struct pt_stats {
    uint64_t rays;           /* closest-hit queries (Scene::RayIntersection calls) */
    uint64_t node_visits;    /* BVH node records fetched */
    uint64_t prim_tests;     /* leaf primitive tests */
    uint64_t plane_tests;
    uint64_t samples;        /* pixel samples traced */
    uint64_t errors;         /* exactness guards tripped (must be 0) */
    uint64_t aux_visits;     /* auxiliary BVH node visits (replay traversal) */
    uint64_t fallbacks;      /* queries that took the exact stack DFS under replay */
    double kernel_ms;        /* sum of trace-kernel time (HIP events) */
    double resolve_ms;
    double wall_ms;          /* pt_render: upload + render + gather + tonemap */
    uint64_t node_bytes;     /* bytes of one node record / primitive record / aux node */
    uint64_t prim_bytes;
    uint64_t aux_bytes;
    uint64_t fallbacks_ray;  /* of `fallbacks`: rays with non-finite origin/direction (exact DFS by design) */
    double isect_ms;         /* wavefront engine: time of the closest-hit kernel launches (HIP events) */
    uint64_t isect_launches;
    uint64_t rounds;         /* wavefront rounds run */
    uint64_t gather_rccl;    /* 1: the multi-GPU framebuffer was gathered with RCCL (ncclGather over xGMI) */
    /* the cooperative end-of-pass engine's share of rays / node_visits / prim_tests /
       aux_visits / isect_ms / isect_launches (the rest is the path engine's) */
    uint64_t coop_rays, coop_node_visits, coop_prim_tests, coop_aux_visits;
    double coop_ms;
    uint64_t coop_launches;
    /* ABI 5: pixels found at a resolve with a sample count other than the samples traced
       (a lost chain: pt_session_resolve then fails; must be 0), and work items an early
       cooperative launch's late workgroups handed on to the next round untaken */
    uint64_t short_pixels;
    uint64_t handed_on;
    /* ABI 6: device allocations pt_render's RCCL gather made (its send / receive buffers are
       kept per communicator: 0 on every render after the first of a device set and size) */
    uint64_t gather_allocs;
    /* ABI 6: work items handed on at each place where work changes hands between the
       engines' launches, waves or queues (PT_HO_*; DESIGN.md §4 "Hand-off sites") */
    uint64_t handoff[12];
} pt_stats;
/* pt_stats.handoff sites (each has a PT_TUNE hook that forces it and one, drop=<name>, that
 * drops its items -- the resolve must then fail: INTEGRATION.md) */
enum {
    PT_HO_SUSPEND = 0,      /* path engine, round end: running queries -> the next carry queue */
    PT_HO_FLUSH = 1,        /* path engine, shade wave after the query waves left: next rays -> next fresh queue */
    PT_HO_RINGOUT = 2,      /* path engine, shade wave's exit: ray-ring leftovers -> next fresh queue */
    PT_HO_EXACT = 3,        /* path engine: a query -> the exact-DFS kernels (k_wexact, k_wshade) */
    PT_HO_SIDE_TAKE = 4,    /* early cooperative launch: the heaviest chains taken from the round's work */
    PT_HO_SIDE_YIELD = 5,   /* early launch's stop: its running chains -> the next carry queue */
    PT_HO_SIDE_HANDON = 6,  /* early launch's late workgroups: untaken items -> the next carry queue */
    PT_HO_GROW_YIELD = 7,   /* final launch's grow stop: its running chains -> the bigger teams' launch */
    PT_HO_GROW_HANDON = 8,  /* final launch's late workgroups: untaken items -> the bigger teams' launch */
    PT_HO_N = 9
};

/* Scene::Render minus the stream write: renders W*H*3 u8 (row-major, top row
 * first, exactly the reference's P6 payload) into rgb, and optionally the
 * pre-tonemap fp32 mean radiance (W*H*3) into radiance.  Either may be NULL.
 * With a window, the outputs are win_w*win_h*3 (the same pixels as a full
 * render would give there).  stats may be NULL. */
int pt_render(pt_scene* s, const pt_render_opts* opts, uint8_t* rgb, float* radiance, pt_stats* stats);

/* P6 writer of src/scene.cpp:206-208,243-251 ("P6\n{W} {H}\n255\n" + payload). */
int pt_write_ppm(const char* path, uint32_t width, uint32_t height, const uint8_t* rgb);

/* ------------------------------------------------------- sessions (tiles)
 * Progressive / sharded rendering on ONE device, used by pt_render and by
 * multi-process drivers (one process per GPU): the image is cut into 16x16
 * tiles, tile (tx, ty) belongs to rank (tx + ty) % world (diagonal stripes: every
 * rank gets every row and column of the image); a rank's tiles are kept in
 * ascending tile order (t = ty * tiles_x + tx).  The session keeps every owned
 * pixel's RNG stream and f32 sum resident in HBM, so pt_session_trace(spp)
 * continues each pixel's stream exactly as the reference's sequential spp loop. */
typedef struct pt_session_opts {
    int32_t device;
    uint32_t rank, world;
    int32_t traversal;
    uint32_t win_x0, win_y0, win_w, win_h;   /* optional window (win_w = 0: full image) */
} pt_session_opts;

int pt_session_create(pt_scene* s, const pt_session_opts* o, pt_session** out);
/* number of owned tiles and of packed output bytes (tiles*256*3) */
int pt_session_layout(const pt_session* ss, uint32_t* n_tiles, uint64_t* packed_rgb_bytes);
/* enqueue spp more samples for every owned pixel (asynchronous).  With the
 * wavefront engine consecutive calls are coalesced into ONE pass, run by the
 * next resolve / sync / stats / stream call: a pixel goes on with its next
 * samples as soon as it has finished the current ones, so only the end of the
 * coalesced pass waits for the slowest pixel.  Results are identical either way
 * (each pixel's samples stay in stream order). */
int pt_session_trace(pt_session* ss, uint32_t spp);
/* tonemap the current means (sum / samples so far) into the packed tile
 * buffer: 256*3 u8 per owned tile, pixels of a tile row-major; dev_out is a
 * device pointer on the session's device (NULL = internal buffer).
 * dev_radiance (optional, device) receives 256*3 f32 per tile. */
int pt_session_resolve(pt_session* ss, uint8_t* dev_out, float* dev_radiance);
int pt_session_sync(pt_session* ss);
/* restart every owned pixel at sample 0 (its stream re-seeded, its sum zeroed), the
 * session's buffers and counters kept: the next trace(S) renders exactly what a new
 * session would -- Scene::Render's job again without the set-up (bench.py repeats the
 * metric's 256-spp frame this way).  Runs any trace() not yet run first. */
int pt_session_reset(pt_session* ss);
/* copy the internal packed buffer to host memory (after resolve+sync) */
int pt_session_read_packed(pt_session* ss, uint8_t* host_out, size_t bytes);
/* scatter packed tiles of `rank` (world ranks) into a width*height*3 image
 * (width/height = the rendered window's size) */
int pt_unpack_tiles(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, const uint8_t* packed,
                    uint8_t* rgb);
int pt_unpack_tiles_f32(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, const float* packed,
                        float* rad);
/* counters accumulated by this session (after sync) */
int pt_session_stats(pt_session* ss, pt_stats* st);
/* HIP stream of the session (hipStream_t), for callers that order their own work after it */
void* pt_session_stream(pt_session* ss);
void pt_session_free(pt_session* ss);

/* ------------------------------------------------------- session states
 * A session's pixels as pt_pixel_state records (below, "pixel samples") and back: the hand-over
 * between the two owners of a pixel's state (additions to ABI 6: no existing struct or function
 * changed).  No reference counterpart: the reference's render cannot be interrupted.  A record a
 * session exports is byte for byte the record pt_pixq_run leaves for that pixel after the same
 * samples -- the saved-value flag in bit 31 of rng, saved = +0 when nothing is saved, samples = the
 * session's count --, so a frame may be checkpointed and resumed, moved to another number of ranks,
 * started from the caller's seeds, or traced in bulk here and refined with pt_pixq_run.
 * pt_session_stats().samples stays owned pixels x samples so far, imported samples included; the
 * work counters (rays, node_visits, ...) count this session's own tracing only. */
typedef struct pt_pixel_state pt_pixel_state;
/* pixels this session owns (inside its window) */
int pt_session_pixels(const pt_session* ss, uint64_t* n);
/* Every owned pixel as a pt_pixel_state, in slot order: the session's tiles in ascending tile
 * order, a tile's pixels row-major, pixels outside the window left out -- exactly
 * pt_session_pixels records, each with the image's global x, y.  Runs any trace() not yet run
 * first.  dev_state: 16-byte aligned device pointer on the session's device, room for cap
 * records; cap < the count: PT_E_INVALID, nothing written.  Complete on return. */
int pt_session_export(pt_session* ss, pt_pixel_state* dev_state, uint64_t cap);
/* Replace the session's pixels by the caller's states.  Records may come in any order.  A
 * record whose pixel lies in the image but is not this session's (another rank's tile, outside
 * the window) is skipped; *taken (may be NULL; written on success only) = records taken.
 * Refused with PT_E_INVALID, the session left exactly as it was, when: a record has x >= W or
 * y >= H; a taken record's rng has low 31 bits outside 1 .. 2^31-2; an owned pixel is named by no
 * record or by more than one; the taken records' `samples` are not all equal.  On success the
 * session stands at that common sample count S: the next trace(k) takes every pixel from S to
 * S + k on the imported streams, and resolve divides by S + k.  S = 0 is allowed (fresh states
 * with the caller's seeds).  A taken record's `saved` is read only when its flag is set; its sum is
 * taken as given (non-finite values too).  A session that owns no pixel takes none of any list.
 * Runs any trace() not yet run first.  Every record is checked before the first is written: the
 * records must not change during the call.  Complete on return. */
int pt_session_import(pt_session* ss, uint64_t n, const pt_pixel_state* dev_state, uint64_t* taken);
/* the same with host pointers (upload / download inside; no alignment asked) */
int pt_session_export_host(pt_session* ss, pt_pixel_state* state, uint64_t cap);
int pt_session_import_host(pt_session* ss, uint64_t n, const pt_pixel_state* state, uint64_t* taken);

/* Per-pixel sample counts: adaptive passes on the session's own engines (additions to ABI 6).
 * Pixel i of the session -- in pt_session_export's order -- takes dev_counts[i] more samples
 * (any u32; 0 leaves the pixel's state untouched, bit for bit).  n must equal pt_session_pixels.
 * Runs any trace() not yet run first, then one pass of the session's own engines; asynchronous on
 * the session's stream like a pass; dev_counts must not change before the next sync point
 * (sync / resolve / stats / export / import).  After it the session is "ragged": pixels hold
 * different sample counts.
 *   A ragged session: a pixel that has taken k samples in all holds exactly the state pt_pixq_run
 * leaves after k samples, and pt_session_export returns it byte for byte, `samples` = the pixel's
 * own count.  pt_session_trace(spp) adds spp to every pixel (and coalesces as always).
 * pt_session_resolve divides each pixel's sum by its own count, as pt_pixel_resolve does, and
 * returns PT_E_INVALID -- nothing written, the session intact -- while an owned pixel has no sample;
 * its lost-chain check is as strict as ever: every owned pixel must stand exactly at the count the
 * session expects of it (pt_stats.short_pixels counts the others).  pt_session_stats().samples is
 * the owned pixels' counts summed, imported samples included; the work counters count this
 * session's own tracing.  pt_session_reset, and a pt_session_import (which goes on refusing
 * unequal counts), leave a uniform session.
 *   Refused with PT_E_INVALID, the session left exactly as it was: n is not the session's pixel
 * count; dev_counts is NULL with n > 0; a pixel's count would pass 2^32 - 1.  A session that owns
 * no pixel accepts n = 0.  All-zero counts launch no pass and change nothing.
 *   Scope: the wavefront engines only.  A megakernel session (traversal EXACT or REPLAY_DIV, or
 * PT_TUNE engine=mega) returns PT_E_INVALID from these calls: k_trace advances by a uniform spp. */
int pt_session_trace_counts(pt_session* ss, uint64_t n, const uint32_t* dev_counts);
int pt_session_trace_counts_host(pt_session* ss, uint64_t n, const uint32_t* counts);
/* pt_session_import without the equal-`samples` rule: every other rule, and the all-or-nothing
 * refusal, as pt_session_import has them.  Each pixel goes on from its record's own count. */
int pt_session_import_ragged(pt_session* ss, uint64_t n, const pt_pixel_state* dev_state, uint64_t* taken);
int pt_session_import_ragged_host(pt_session* ss, uint64_t n, const pt_pixel_state* state, uint64_t* taken);
/* the smallest and the largest sample count of the session's pixels, trace() calls not yet run
 * included (equal: a uniform session).  Host bookkeeping: no device work, no sync point. */
int pt_session_samples_range(const pt_session* ss, uint32_t* least, uint32_t* most);

/* ------------------------------------------------------- session noise
 * The session's own estimate of where more samples are needed, and the adaptive step it plans from
 * it (additions to ABI 6: no existing struct or function changed).  No reference counterpart: the
 * reference gives every pixel the same SAMPLES.  The session remembers every owned pixel's sum at an
 * earlier count, the pixel's MARK, turns the movement of the pixel's mean since the mark into a noise
 * figure, the figures into counts by the rule below, and runs the counts as pt_session_trace_counts
 * runs them.  One pt_session_refine is one adaptive step; a loop of it until refined == 0 renders the
 * frame to a noise threshold under a sample cap.
 *   The arithmetic is f32, every operation rounded (no FMA), in this order.  A pixel now is
 * (sum[3], k), k its own count; its mark is (M[3], a), a = 0 meaning "no mark".
 *   No estimate -- a == 0 or k <= a:  noise = +inf (bits 0x7f800000).
 *   Otherwise, with mean(s, n) = (1.f / float(n)) * s as pt_pixel_resolve has it:
 *     m_c = mean(sum_c, k), p_c = mean(M_c, a)                  for c = r, g, b
 *     d  = (|m_r - p_r| + |m_g - p_g|) + |m_b - p_b|
 *     l  = (m_r + m_g) + m_b
 *     lf = l > 0x1p-10f ? l : 0x1p-10f                          (a select: a NaN l takes the floor)
 *     noise = d / sqrtf(lf)
 * so a noise is never negative: finite, +inf or NaN (a non-finite sum).
 *   Options: threshold, step, max_samples (0 = 2^32 - 1), spread.  Invalid: a NaN or negative
 * threshold, step == 0, spread > 1.
 *     hot  = noise > threshold      strict: false for NaN, true for +inf, computed or "no estimate"
 *     hot' = hot, or with spread == 1: hot, or one of the pixel's 8 neighbours that is an owned pixel
 *            of the SAME 16 x 16 tile is hot.  The rule never looks across a tile's border -- the
 *            next tile may be another rank's --, so a pixel's plan does not depend on the sharding.
 *     count = 0 if the noise is NaN; 0 if !hot'; 0 if k >= max_samples; else min(step, max_samples - k)
 *   The result: refined = pixels with count > 0; samples = the counts' sum; unmarked = owned pixels
 * with no estimate; nonfinite = owned pixels with a NaN noise; capped = pixels that are hot', not NaN,
 * and stand at k >= max_samples; worst = the largest finite noise of an owned pixel that has an
 * estimate (0: none); least, most = pt_session_samples_range after the call.
 *   Every call first runs any trace() not yet run.  mark, noise and plan are complete on return;
 * noise and plan change nothing of the session -- no mark, no lag, no `done` field.  Values are in
 * pt_session_export's order; cap = room in the buffer, below pt_session_pixels: PT_E_INVALID, nothing
 * written.  pt_session_plan's counts may be NULL (the result alone; cap is not read).
 *   pt_session_refine is the plan, then mark := now for every pixel with count > 0, then the counts'
 * pass (pt_session_trace_counts' own, asynchronous like it; one host read-back per step).  The counts
 * live in the session.  refined == 0: nothing is launched and nothing changes, marks included.  A
 * session that was never marked has no estimate anywhere: the first refine marks every pixel and gives
 * each min(step, max_samples - k), so a loop of refine alone bootstraps itself.  A pixel with count 0
 * keeps its mark and its state, so its noise is the same number at every later step: a pixel once cold
 * stays cold, and refined == 0 means the frame is done.
 *   Marks are the session's alone: pt_session_reset, pt_session_import and pt_session_import_ragged
 * clear them all (unmarked = the pixel count afterwards), and pt_session_export does not carry them.
 *   Refused with PT_E_INVALID, the session left exactly as it was: NULL options or result; invalid
 * options; a buffer too small; a megakernel session, as pt_session_trace_counts refuses it.  A session
 * that owns no pixel accepts every call and reports zeros.  No count can pass 2^32 - 1. */
typedef struct pt_refine_opts   { float threshold; uint32_t step, max_samples, spread; } pt_refine_opts;
typedef struct pt_refine_result { uint64_t refined, samples, unmarked, nonfinite, capped; float worst;
                                  uint32_t least, most; } pt_refine_result;
/* mark := now for every owned pixel */
int pt_session_mark(pt_session* ss);
/* every owned pixel's noise (dev_noise: a device pointer on the session's device, room for cap f32) */
int pt_session_noise(pt_session* ss, float* dev_noise, uint64_t cap);
int pt_session_noise_host(pt_session* ss, float* noise, uint64_t cap);
/* the step pt_session_refine would take now: every owned pixel's count and the result */
int pt_session_plan(pt_session* ss, const pt_refine_opts* o, uint32_t* dev_counts, uint64_t cap, pt_refine_result* res);
int pt_session_plan_host(pt_session* ss, const pt_refine_opts* o, uint32_t* counts, uint64_t cap, pt_refine_result* res);
/* one adaptive step */
int pt_session_refine(pt_session* ss, const pt_refine_opts* o, pt_refine_result* res);

/* ------------------------------------------------------------ ray queries
 * Scene::RayIntersection (src/scene.cpp:46-77) for the caller's own rays, bit for bit: the
 * planes, then the reference BVH with its pruning semantics (first-hit buffers, picking,
 * visibility passes).  No reference counterpart as an interface: RayIntersection is private
 * to the reference's render.  A ray is used as given (never normalised).  A hit's id is the
 * primitive's index in the prepared order -- the order of pt_scene_dump_bvh's primitives,
 * planes at the end; a miss is id = -1 with the other five words 0. */
typedef struct pt_rayq pt_rayq;
typedef struct pt_ray     { float o[3], d[3]; } pt_ray;
typedef struct pt_ray_hit { int32_t id; float t; float n[3]; uint32_t interior; } pt_ray_hit;

/* a ray-query context on `device` for runs of up to max_rays (1 .. 2^32 - 1) rays; prepares
 * the scene if needed; the scene must outlive the context */
int pt_rayq_create(pt_scene* s, int device, uint64_t max_rays, pt_rayq** out);
/* asynchronous on `stream` (a hipStream_t; NULL = the null stream); dev_rays / dev_hits are
 * device pointers on the context's device; n <= max_rays; n = 0 enqueues nothing.  One run at
 * a time per context: a run first waits (on the host) for the context's previous run. */
int pt_rayq_run(pt_rayq* q, void* stream, uint64_t n, const pt_ray* dev_rays, pt_ray_hit* dev_hits);
/* waits for the last run; fills rays, node_visits, prim_tests, plane_tests, aux_visits,
 * fallbacks, fallbacks_ray, errors (must be 0), kernel_ms and the *_bytes record sizes for the
 * runs since the last call */
int pt_rayq_stats(pt_rayq* q, pt_stats* st);
void pt_rayq_free(pt_rayq* q);
/* convenience, host pointers: uploads, runs, downloads, in chunks of at most 2^22 rays so that
 * device memory stays bounded; synchronous; stats may be NULL */
int pt_intersect(pt_scene* s, int device, uint64_t n, const pt_ray* rays, pt_ray_hit* hits, pt_stats* stats);

/* ------------------------------------------------------------ batch radiance
 * Scene::RayTrace (src/scene.cpp:83-178) for the caller's own rays, bit for bit (additions to
 * ABI 6: no existing struct or function changed).  No reference counterpart as an interface:
 * RayTrace is private to the reference's render, reachable only through the scene's one pinhole
 * camera.  One record is one call: its output is RayTrace(random, Ray{o, d}, RAY_DEPTH) with
 * `random` a fresh std::minstd_rand rnd(seed) and fresh uniform / normal distributions.
 * RAY_DEPTH is the scene's value when the context is created (pt_scene_override applies).  The
 * ray is used as given (never normalised; a non-finite ray is answered as the reference answers
 * it).  rgb is the value RayTrace returns, not a mean; rays = the path's RayIntersection calls
 * (0 when RAY_DEPTH is 0).  `reserved` is written as 0 and not read.  A caller who wants many
 * samples sends many records, with their own jitter and seeds. */
typedef struct pt_pathq pt_pathq;
typedef struct pt_path_ray  { float o[3], d[3]; uint32_t seed; uint32_t reserved; } pt_path_ray;   /* 32 B */
typedef struct pt_path_out  { float rgb[3]; uint32_t rays; } pt_path_out;                          /* 16 B */

/* a batch radiance context on `device` for runs of up to max_paths (1 .. 2^32 - 1) paths; prepares
 * the scene if needed; the scene must outlive the context.  The context holds RAY_DEPTH x 16 B of
 * device memory per resident lane (PT_E_OOM if one wave per compute unit would pass 1 GiB). */
int pt_pathq_create(pt_scene* s, int device, uint64_t max_paths, pt_pathq** out);
/* asynchronous on `stream` (a hipStream_t; NULL = the null stream); dev_in / dev_out are 16-byte
 * aligned device pointers on the context's device; n <= max_paths; n = 0 enqueues nothing.  One
 * run at a time per context: a run first waits (on the host) for the context's previous run. */
int pt_pathq_run(pt_pathq* q, void* stream, uint64_t n, const pt_path_ray* dev_in, pt_path_out* dev_out);
/* waits for the last run; fills rays, node_visits, prim_tests, plane_tests, aux_visits, fallbacks,
 * fallbacks_ray (over every vertex of every path), errors (must be 0), kernel_ms and the *_bytes
 * record sizes for the runs since the last call */
int pt_pathq_stats(pt_pathq* q, pt_stats* st);
void pt_pathq_free(pt_pathq* q);
/* convenience, host pointers: uploads, runs, downloads, in chunks of at most 2^22 paths so that
 * device memory stays bounded; synchronous; stats may be NULL */
int pt_radiance(pt_scene* s, int device, uint64_t n, const pt_path_ray* in, pt_path_out* out, pt_stats* stats);
/* Camera::GetToRay(x, y) (src/scene.cpp:180-187) for n float pixel coordinates xy[2i], xy[2i + 1]:
 * the ray a pixel sample at (x, y) starts with (the direction is not normalised).  Host only. */
int pt_camera_rays(pt_scene* s, uint64_t n, const float* xy, pt_ray* out);

/* ------------------------------------------------------------ pixel samples
 * Scene::Sample's loop (src/scene.cpp:189-200) for a list of pixels the caller supplies, bit for
 * bit (additions to ABI 6: no existing struct or function changed).  No reference counterpart as
 * an interface: Sample is private to the reference's render, which gives every pixel of the frame
 * the same SAMPLES.  Here a record is one pixel's state -- its random stream, its f32 sum and its
 * sample count --, owned by the caller: it may be run for any number of further samples, any
 * number of times, copied, stored and moved between devices and processes.  Each new sample of a
 * record is one trip of Sample's loop on the record's ONE stream, as the previous sample left it:
 *   fx = float(x) + uniform01(rnd);  fy = float(y) + uniform01(rnd);        (scene.cpp:197-198)
 *   sum = sum + RayTrace(random, cam.GetToRay(fx, fy), RAY_DEPTH);  samples++   (scene.cpp:199)
 * the sum added component by component in f32, the normal_distribution's saved value carried in
 * the record.  (At RAY_DEPTH 0 the two jitter draws still happen and the sum gets + 0.)  So a state
 * run for a and then for b samples equals, bit for bit, one run of a + b; and a fresh default-seed
 * state taken to S samples resolves to the radiance pt_render and the reference give that pixel at
 * SAMPLES = S.  A record's samples are serial, as a pixel's are in the reference: a run takes at
 * least as long as its longest record. */
typedef struct pt_pixq pt_pixq;
typedef struct pt_pixel_state {     /* 32 B; arrays 16-byte aligned */
    uint32_t rng;      /* minstd_rand state, 1 .. 2^31-2; bit 31 set = the pixel's
                          normal_distribution holds a saved value */
    float    saved;    /* that value (0 when none) */
    uint32_t x, y;     /* the pixel: sample k's ray is GetToRay(float(x)+u1, float(y)+u2) */
    float    sum[3];   /* Sample's `summary`, f32, added in the reference's order */
    uint32_t samples;  /* samples in sum */
} pt_pixel_state;

/* Host only.  n fresh states for the pixels xy[2i], xy[2i + 1]: std::minstd_rand rnd(seed) with
 * fresh distributions (no saved value), sum = 0, samples = 0.  seeds == NULL: the reference's seed
 * y * W + x (src/scene.cpp:216); else seeds[i], reduced as minstd_rand's constructor reduces it.
 * x >= W or y >= H: PT_E_INVALID. */
int pt_pixel_init(pt_scene* s, uint64_t n, const uint32_t* xy, const uint32_t* seeds, pt_pixel_state* out);
/* a pixel-sample context on `device` for runs of up to max_pixels (1 .. 2^32 - 1) records; prepares
 * the scene if needed; the scene must outlive the context.  RAY_DEPTH (pt_scene_override applies)
 * and the camera are read here.  The context holds RAY_DEPTH x 16 B of device memory per resident
 * lane (PT_E_OOM if one wave per compute unit would pass 1 GiB). */
int pt_pixq_create(pt_scene* s, int device, uint64_t max_pixels, pt_pixq** out);
/* asynchronous on `stream` (a hipStream_t; NULL = the null stream).  Record i takes dev_counts[i]
 * more samples (dev_counts == NULL: spp), and dev_state[i] is updated in place to the state after
 * them; a count of 0 leaves the record's 32 bytes untouched.  Two records that name the same pixel
 * are independent.  dev_state is a 16-byte aligned device pointer on the context's device,
 * dev_counts a device pointer to n u32; n <= max_pixels; n = 0 enqueues nothing.  One run at a
 * time per context: a run first waits (on the host) for the context's previous run. */
int pt_pixq_run(pt_pixq* q, void* stream, uint64_t n, pt_pixel_state* dev_state, const uint32_t* dev_counts,
                uint32_t spp);
/* waits for the last run; fills samples (those the runs added), rays, node_visits, prim_tests,
 * plane_tests, aux_visits, fallbacks, fallbacks_ray (over every vertex of every sample), errors
 * (must be 0), kernel_ms and the *_bytes record sizes for the runs since the last call */
int pt_pixq_stats(pt_pixq* q, pt_stats* st);
void pt_pixq_free(pt_pixq* q);
/* convenience, host pointers, `state` updated in place: uploads, runs, downloads, in chunks of at
 * most 2^22 records so that device memory stays bounded; synchronous; counts (n u32) may be NULL:
 * spp for every record; stats may be NULL */
int pt_sample_pixels(pt_scene* s, int device, uint64_t n, pt_pixel_state* state, const uint32_t* counts,
                     uint32_t spp, pt_stats* stats);
/* Host only.  Sample's return value and Render's 8-bit step for n states: mean[3i ..] =
 * 1.f / samples * sum (src/scene.cpp:201: a product with the rounded reciprocal), rgb[3i ..] = the
 * tonemap, gamma and rounding of scene.cpp:227-233, computed by the function the device resolve
 * uses.  Either output may be NULL.  A state with samples == 0: PT_E_INVALID. */
int pt_pixel_resolve(pt_scene* s, uint64_t n, const pt_pixel_state* state, float* mean, uint8_t* rgb);

/* ------------------------------------------------------------ first-hit features
 * What a position on the image plane looks at (additions to ABI 6: no existing struct or function
 * changed): the closest hit of the camera's ray through it, and the scene data of the primitive
 * that hit names -- albedo, normal and depth buffers for a filter or denoiser, a cost map,
 * picking, a G-buffer preview.  No reference counterpart as an interface.  A position is two
 * floats (x, y) in pixel units, used as given, exactly as pt_camera_rays takes them; it may lie
 * outside the frame and may be non-finite.  Its record is defined by the reference:
 *   ray = Camera::GetToRay(x, y)              (src/scene.cpp:180-187; the direction not normalised)
 *   hit = Scene::RayIntersection(ray)         (src/scene.cpp:46-77)
 * and everything else is a copy of primitives[hit.id]'s data, or of the scene's BG_COLOR: no
 * arithmetic is added, so every field agrees with the reference's bit for bit.  On a miss id = -1,
 * emission = BG_COLOR -- what RayTrace returns for that ray -- and every other word is 0.  A
 * non-finite position gives a non-finite ray, which is answered as the reference answers it. */
typedef struct pt_feature {          /* 64 B; arrays 16-byte aligned */
    int32_t  id;                     /* bytes 0..23: the pt_ray_hit of `ray`, byte for byte */
    float    t;
    float    n[3];
    uint32_t interior;
    float    albedo[3];              /* primitives[id].col */
    float    ior;                    /* primitives[id].ior, whatever the material */
    float    emission[3];            /* primitives[id].emission; on a miss: BG_COLOR */
    uint32_t material;               /* 0 diffuse, 1 metallic, 2 dielectric */
    uint32_t type;                   /* 1 plane, 2 box, 4 ellipsoid, 8 triangle; 0 = miss */
    uint32_t reserved;               /* written 0 */
} pt_feature;
typedef struct pt_featq pt_featq;

/* a feature context on `device` for runs of up to max_points (1 .. 2^32 - 1) positions; prepares
 * the scene if needed; the scene must outlive the context.  The camera is read here.  The context
 * holds 4 B of device memory per point. */
int pt_featq_create(pt_scene* s, int device, uint64_t max_points, pt_featq** out);
/* asynchronous on `stream` (a hipStream_t; NULL = the null stream); dev_xy (2 floats per point,
 * 8-byte aligned) and dev_out (16-byte aligned) are device pointers on the context's device;
 * n <= max_points; n = 0 enqueues nothing; a refusal writes nothing.  One run at a time per
 * context: a run first waits (on the host) for the context's previous run. */
int pt_featq_run(pt_featq* q, void* stream, uint64_t n, const float* dev_xy, pt_feature* dev_out);
/* waits for the last run; fills what pt_rayq_stats fills (rays = the points) for the runs since
 * the last call; errors must be 0 */
int pt_featq_stats(pt_featq* q, pt_stats* st);
void pt_featq_free(pt_featq* q);
/* convenience, host pointers: uploads, runs, downloads, in chunks of at most 2^22 points so that
 * device memory stays bounded; synchronous; stats may be NULL */
int pt_features(pt_scene* s, int device, uint64_t n, const float* xy, pt_feature* out, pt_stats* stats);

/* One record per pixel the session owns, in pt_session_export's order, for the pixel's centre
 * (float(x) + 0.5f, float(y) + 0.5f), x and y the image's global coordinates.  dev_out: a 16-byte
 * aligned device pointer with room for cap records; cap below pt_session_pixels: PT_E_INVALID,
 * nothing written (a session that owns no pixel accepts cap = 0).  Complete on return.  Works for
 * a session of any traversal or engine.  Reads nothing of the pixels' states and changes nothing
 * of the session: trace() calls not yet run stay pending, marks, lag and pt_session_stats are
 * untouched; the call's work is reported through st alone (as pt_featq_stats fills it; may be
 * NULL).  What the session needs for this -- a feature context and 8 B per owned pixel -- is made
 * at the first call. */
int pt_session_features(pt_session* ss, pt_feature* dev_out, uint64_t cap, pt_stats* st);
int pt_session_features_host(pt_session* ss, pt_feature* out, uint64_t cap, pt_stats* st);

/* Host only, after pt_scene_prepare: the scene data a hit's id names, for every primitive in the
 * prepared order (pt_scene_dump_bvh's); n must equal pt_scene_info.n_prims.  With it the id of any
 * pt_ray_hit or pt_feature resolves on the host. */
typedef struct pt_prim_shade { float albedo[3]; float ior; float emission[3]; uint32_t material; } pt_prim_shade;
int pt_scene_shade(const pt_scene* s, pt_prim_shade* out, size_t n);
/* Host only: the scene's BG_COLOR */
int pt_scene_background(const pt_scene* s, float rgb[3]);

/* ------------------------------------------------------------ guided filter
 * A feature-guided a-trous denoise of a frame (additions to ABI 6: no existing struct or function
 * changed).  No reference counterpart.  Everything is f32, every operation rounded, no FMA, in the
 * order written here: a float32 restatement agrees bit for bit (tests/_filter.py is one).
 *
 * A frame is a window w x h of the image, row-major, top row first: radiance (3 x f32 per pixel,
 * pt_render's layout), one pt_feature per pixel for the pixel's centre
 * (float(x0 + x) + 0.5f, float(y0 + y) + 0.5f), and the options below.
 *
 * The guide of a pixel (32 B): n[3], t, a[3] = albedo, cls.  cls = 0 on a miss (id < 0), otherwise
 * 1 + material + 4 * (emission[0] != 0 || emission[1] != 0 || emission[2] != 0).  n, t and a are the
 * record's words (the library's records hold zeros there on a miss).
 *
 * Constants: ga = sigma_a * sigma_a; ia = ga > 0 ? 1.f / ga : 0.f.  Per level L = 0 .. levels - 1:
 * s = 1 << L, sc = sigma_c * 2^-L, gc = sc * sc, ic = gc > 0 ? 1.f / gc : 0.f.  Per pixel p:
 * gz = sigma_z * t_p; gz = gz * gz; iz = gz > 0 ? 1.f / gz : 0.f.  (Selects: a NaN takes 0.)
 *
 * One level (level 0 reads the input, level L the output of level L - 1).  A colour is finite when
 * its three channels are.  A pixel whose own colour is not finite keeps its three words.  Otherwise,
 * with K = {1/16, 1/4, 3/8, 1/4, 1/16}, acc = (0, 0, 0) and ws = 0, the 25 taps dy = -2 .. 2 (outer),
 * dx = -2 .. 2 (inner), q = (x + dx * s, y + dy * s):
 *   the centre tap has w = 9/64;
 *   a tap outside the window, one with cls_q != cls_p and one whose colour is not finite are skipped;
 *   otherwise  d = (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z;  d = d > 0 ? d : 0;  normal_pow2
 *              times d = d * d;  wn = cls_p == 0 ? 1 : d;
 *              dz = t_p - t_q;  ez = dz * dz;
 *              ea = (da0 * da0 + da1 * da1) + da2 * da2  over a_p - a_q;  ec the same over the current
 *              level's c_p - c_q;
 *              D = ((1 + ez * iz) * (1 + ea * ia)) * (1 + ec * ic);
 *              w = (K[dy + 2] * K[dx + 2] * wn) / D;  w = w > 0 ? w : 0;
 *   a tap that is not skipped adds acc_c = acc_c + w * c_q,c and ws = ws + w.
 * Then inv = 1.f / ws (ws >= 9/64) and out_c = acc_c * inv.  The last level's output is the result;
 * its optional 8-bit form is the render's tonemap, gamma and rounding of it (pt_pixel_resolve's). */
enum { PT_FILTER_ROWMAJOR = 0,       /* the input is w * h pixels, row-major */
       PT_FILTER_TILES = 1 };        /* the input is a world-1 session's packed dev_radiance of the same
                                      * window: exactly what pt_unpack_tiles_f32(w, h, 0, 1, ..) reads */
typedef struct pt_filter_opts {
    uint32_t levels;                 /* 1 .. 8 */
    float    sigma_c, sigma_z, sigma_a;   /* each >= 0 and finite; 0 switches that weight off */
    uint32_t normal_pow2;            /* 0 .. 8 */
    uint32_t layout;                 /* PT_FILTER_*: of the input; the output is row-major either way */
} pt_filter_opts;
/* levels 3, sigma_c 1, sigma_z 0.05, sigma_a 0.1, normal_pow2 5, row-major */
void pt_filter_opts_default(pt_filter_opts* o);
typedef struct pt_filtq pt_filtq;
/* a filter context on `device` for the window (x0, y0, w, h) of the scene's image; w = 0: the full
 * image; a window outside the image, or one of more than 2^27 pixels: PT_E_INVALID.  Prepares the
 * scene if needed; the scene must outlive the context.  Computes the window's guides here, once,
 * with a feature query on the pixel centres.  The context holds 64 B of device memory per pixel. */
int pt_filtq_create(pt_scene* s, int device, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, pt_filtq** out);
/* replaces the guides by ones packed from the caller's w * h records (device, 16-byte aligned,
 * row-major); asynchronous on `stream`, after the context's previous run */
int pt_filtq_set_features(pt_filtq* q, void* stream, const pt_feature* dev_features);
/* asynchronous on `stream` (a hipStream_t; NULL = the null stream), one launch per level.  dev_in
 * (opts->layout), dev_out (w * h * 3 f32) and the optional dev_rgb (w * h * 3 u8; may be NULL) are
 * device pointers on the context's device, dev_in and dev_out 4-byte aligned.  Ranges that overlap,
 * NULL pointers and invalid options: PT_E_INVALID, nothing enqueued, nothing written.  One run at a
 * time per context: a run first waits (on the host) for the context's previous run. */
int pt_filtq_run(pt_filtq* q, void* stream, const pt_filter_opts* opts, const float* dev_in, float* dev_out,
                 uint8_t* dev_rgb);
/* waits for the last run; fills kernel_ms (the runs since the last call) and rays (the guide points
 * traced since the last call); every other field 0 */
int pt_filtq_stats(pt_filtq* q, pt_stats* st);
void pt_filtq_free(pt_filtq* q);
/* convenience, host pointers, synchronous: a context, an upload, a run, a download.  rgb may be NULL */
int pt_filter(pt_scene* s, int device, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const pt_filter_opts* opts,
              const float* in, float* out, uint8_t* rgb);

const char* pt_last_error(void);
int pt_abi_version(void);

/* ------------------------------------------------------------ test hooks
 * Host execution of the device traversal code (pt_trace.h) for CPU unit
 * tests of the stack-DFS logic, and the device code's scalar functions one by
 * one (pt_selftest_math).  Never used by pt_render. */
int pt_selftest_ray_intersection(pt_scene* s, int32_t traversal, uint32_t n, const float* rays, int32_t* ids,
                                 float* hits, uint64_t* counters8);
int pt_selftest_render_host(pt_scene* s, int32_t traversal, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                            uint32_t spp, float* radiance);
/* The query's decision step (pt_query.h q_decide) against the self-test's own plain loop
 * over the hit list, on n seeded decision states (ne <= nh <= PT_QHK, sorted lists, thresholds
 * and t's on both sides of the bounds, both values of overflow, lists full of entered hits):
 * out3 = {states, states with a slot to examine, states whose Query differs in any byte}.
 * Needs no GPU. */
int pt_selftest_decide(uint64_t seed, uint64_t n, uint64_t* out3);
/* the same n states after the decision: device < 0 the host's plain loop, device >= 0 q_decide in
 * a kernel of its own on that device, 64 consecutive states to a wave.  states (cap bytes; may be
 * NULL) takes n records of *state_bytes bytes each; counts (may be NULL) takes 4 + PT_QHK (= 10)
 * values by the plain loop: the states that left to a leaf check, with the pass done, to another
 * pass, to the exact DFS, then per slot the states whose last examined slot it was. */
int pt_selftest_decide_states(int device, uint64_t seed, uint64_t n, void* states, uint64_t cap, uint64_t* counts,
                              uint32_t* state_bytes);
/* the query blob's wide aux entries against the host-form array (pt_query.h: the last two words
 * ready-made): out5 = {entries, empty, leaf, internal, entries whose words differ from what the
 * host form's code, range and leaf ordinal give}.  Prepares the scene if needed.  Needs no GPU. */
int pt_selftest_aux_words(pt_scene* s, uint64_t* out5);
/* n batch radiance records on the host: trace_path_with over the query state machine run to
 * completion, as pt_selftest_render_host runs a pixel's samples.  Fills out (rgb, and each path's
 * rays) and counters8: the totals of rays, nodes, primitive tests, plane tests, errors, aux
 * visits, fallbacks and non-finite-ray fallbacks (the CTR_* slots).  counters8 may be NULL. */
int pt_selftest_paths_host(pt_scene* s, uint64_t n, const pt_path_ray* in, pt_path_out* out, uint64_t* counters8);
/* n pixel-sample records on the host, updated in place as pt_pixq_run updates them: camera_ray and
 * trace_path_with over the query state machine run to completion, on each record's stream.  counts
 * may be NULL (spp for every record).  counters8 as pt_selftest_paths_host fills it; the samples
 * added are the counts' sum.  Needs no GPU. */
int pt_selftest_pixels_host(pt_scene* s, uint64_t n, pt_pixel_state* state, const uint32_t* counts, uint32_t spp,
                            uint64_t* counters8);
/* n feature records on the host, as pt_featq_run writes them: camera_ray, the query state machine
 * run to completion, then the shade lookup, by the inline functions k_feats runs.  counters8 as
 * pt_selftest_paths_host fills it (rays = n); may be NULL.  Needs no GPU. */
int pt_selftest_features_host(pt_scene* s, uint64_t n, const float* xy, pt_feature* out, uint64_t* counters8);
/* pt_filtq_run's result on the host for a w x h frame: the guides packed from `features` (w * h
 * records, row-major), then the levels, by the inline functions k_filter_guides and k_filter run, on
 * one thread.  in: opts->layout; out: w * h * 3 f32.  Needs no device and no scene. */
int pt_selftest_filter_host(uint32_t w, uint32_t h, const pt_feature* features, const pt_filter_opts* opts,
                            const float* in, float* out);
/* The parse as pt_scene_load left it, before pt_scene_prepare (afterwards: PT_E_INVALID, the
 * primitives are reordered), every field as its raw bits.  out: an 80-byte header (width, height,
 * samples, ray_depth u32; fov_x, background, camera position, right, up, forward f32), then per
 * primitive in file order 100 bytes: u32 type; the three shape vectors; position; rotation x y z w;
 * colour; emission; u32 material; f32 IOR.  warnings: the "unexpected command(...)" lines in order,
 * each ended by '\n' (no NUL).  *need / *warn_need = the bytes either takes; out and warnings may be
 * NULL to ask for them alone.  Needs no GPU. */
int pt_selftest_scene_dump(const pt_scene* s, void* out, size_t cap, size_t* need, char* warnings, size_t warn_cap,
                           size_t* warn_need);
/* pt_scene_load_mem parsed in at most `stretches` (1 .. 64) stretches on as many threads, whatever
 * the text's size and the machine's thread count (pt_scene_load_mem itself uses one stretch below
 * 1 MiB, else up to 16).  cuts (may be NULL; room for cap) takes the offsets at which the stretches
 * begin and end: 0, each cut, len; *n_cuts = their number (at most stretches + 1).  Needs no GPU. */
int pt_selftest_scene_load_stretches(const char* text, size_t len, uint32_t stretches, pt_scene** out, uint64_t* cuts,
                                     uint32_t cap, uint32_t* n_cuts);
/* the 256-entry gamma threshold table used by the device tonemap */
int pt_selftest_gamma_table(const pt_scene* s, float* thr256);
/* session set-up without a device: the geometry (o's rank, world, window, traversal; o->device is
 * ignored), the wavefront pass's launch shapes and capacities on a device of `cus` compute units,
 * and the arena's layout, as "key=value" lines in buf (cap bytes; PT_E_INVALID if too small): a
 * line per plan field (mix and mix_low: four values), then n_slots, n_tiles_local, arena_bytes and
 * aux_stack_words (the scene's wide aux traversal stack, which a carry record holds).
 * Prepares the scene if needed. */
int pt_selftest_wave_plan(pt_scene* s, const pt_session_opts* o, uint32_t cus, char* buf, size_t cap);
/* a batch context's launch shape without a device: the workgroup and the resident grid of a context
 * with fold records (pt_pathq, pt_pixq) on a device of `cus` compute units that hold `per_cu`
 * workgroups of `block` threads each, at RAY_DEPTH `depth` -- per_cu * cus workgroups unless their
 * lanes' fold records (16 B x depth each) exceed 1 GiB, then fewer, then narrower ones; PT_E_OOM
 * where one wave per compute unit still exceeds it. */
int pt_selftest_fold_shape(uint32_t cus, uint32_t per_cu, uint32_t block, uint32_t depth, uint32_t* block_out,
                           uint32_t* grid_out);
/* the batch engines' workgroup for lanes whose stacks take `aux_words` (the aux stack) and `dfs_words`
 * (the exact DFS's) words, without a device: *block_aux_only as pt_rayq / pt_featq choose it (their
 * lanes hold the aux stack only, their exact kernel's one wave the DFS stack), *block_both as pt_pathq /
 * pt_pixq do before the fold area's bound (a lane's column holds the larger of the two): from 256
 * threads down to 64 until the columns fit a workgroup's 64 KiB of LDS.  *fits: bit 0 the first
 * kind accepts the stacks, bit 1 the second does (a refusal is their PT_E_SCENE). */
int pt_selftest_fit_block(uint32_t aux_words, uint32_t dfs_words, uint32_t* block_aux_only, uint32_t* block_both,
                          uint32_t* fits);
/* ... for a scene's own stack words, which it also returns.  Prepares the scene if needed. */
int pt_selftest_lane_shape(pt_scene* s, uint32_t* aux_words, uint32_t* dfs_words, uint32_t* block_aux_only,
                           uint32_t* block_both, uint32_t* fits);
/* a live batch context's launch shape: its workgroup, its resident grid, and the workgroups per
 * compute unit that shape started from (pt_rayq, pt_featq: 2,048 lanes' worth; pt_pathq, pt_pixq: the
 * kernel's occupancy).  kind names what ctx is.  Read-only. */
#define PT_CTX_RAYQ 0u
#define PT_CTX_FEATQ 1u
#define PT_CTX_PATHQ 2u
#define PT_CTX_PIXQ 3u
int pt_selftest_ctx_shape(uint32_t kind, const void* ctx, uint32_t* block, uint32_t* max_grid, uint32_t* per_cu);
/* per record the session slot it would land in, by the functions k_states_mark uses compiled
 * for the host: >= 0 slot, -1 in the image but not this session's, -2 outside the image or a
 * bad rng word (of a pixel that is this session's: another's record is -1 whatever it holds).
 * o as pt_selftest_wave_plan takes it.  Needs no GPU. */
int pt_selftest_state_slots(pt_scene* s, const pt_session_opts* o, uint64_t n, const pt_pixel_state* state,
                            int64_t* slot_out);
/* per slot of the session (o as pt_selftest_wave_plan takes it) the record of its export that holds
 * the slot's pixel -- pt_session_trace_counts' count for it --, -1 for an edge tile's padding lane,
 * by the function the count kernels use compiled for the host.  *n_slots = the session's slots;
 * rec_out has room for cap (fewer than the slots: PT_E_INVALID).  Needs no GPU. */
int pt_selftest_count_records(pt_scene* s, const pt_session_opts* o, uint64_t cap, int64_t* rec_out, uint64_t* n_slots);
/* one pt_session_trace_counts call's arithmetic on the host, for n pixels of a session whose
 * `done` fields stand at S with the pixels' counts lag[i] below it: *S2 = the pass's target (the
 * largest count after the call; past 2^32 - 1: PT_E_INVALID, nothing written), done[i] = the field
 * the pass starts pixel i from, lag_after[i] = its distance below S2 afterwards.  Needs no GPU. */
int pt_selftest_count_step(uint32_t S, uint64_t n, const uint32_t* lag, const uint32_t* counts, uint32_t* done,
                           uint32_t* lag_after, uint32_t* S2);
/* pt_session_plan on the host ("session noise" above), for the n pixels of a session (o as
 * pt_selftest_wave_plan takes it) in its export's order: `now` their states, `mark` their states when
 * marked (a record with samples == 0: no mark; only sum and samples are read).  By the functions
 * k_noise_plan runs compiled for the host, and the same in-tile neighbour rule.  noise and counts may
 * be NULL; res->least / most = the range of now's samples.  n other than the session's pixel count,
 * NULL or invalid options: PT_E_INVALID.  Needs no GPU. */
int pt_selftest_refine_plan(pt_scene* s, const pt_session_opts* o, uint64_t n, const pt_pixel_state* now,
                            const pt_pixel_state* mark, const pt_refine_opts* ro, float* noise, uint32_t* counts,
                            pt_refine_result* res);
/* The scalar building blocks of the device code (logf, the RNG streams, the normal and cosine
 * samplers, the Schlick term, the resolve's mean + tonemap + 8-bit step, IEEE divide / sqrt /
 * conversions), element by element: n records in, n records out (little-endian, packed).
 * device >= 0: one element per thread in a kernel of their own on that device; device < 0: the
 * same inline functions compiled for the host (needs no GPU).
 *   op        record in                          record out
 *   LOGF      f32 x                              f32 logf(x)
 *   RNG       u32 seed, u32 n (one n per call)   n uniform, n normal, n mixed draws (f32; 3 fresh streams)
 *   NORMAL3   u32 seed, u32 pre                  8 x 3 f32: consecutive unit normal vectors
 *   COSINE    u32 seed, u32 pre, 3 f32 normal    8 x 3 f32: consecutive cosine samples about it
 *   FRESNEL   f32 eta1, eta2, cosn               f32 reflection probability, -1 = total internal reflection
 *   RESOLVE   f32 sum, u32 samples               f32 mean, u32 8-bit value
 *   ARITH     f32 a, b, f64 a, b                 f32 a/b, sqrtf(|a|), f64 a/b, sqrt(|a|), f32 (float)a64, (float)(double)a
 * pre = normal draws made on the stream first (odd: the sampler starts with a saved value). */
enum { PT_MATH_LOGF = 0, PT_MATH_RNG = 1, PT_MATH_NORMAL3 = 2, PT_MATH_COSINE = 3, PT_MATH_FRESNEL = 4,
       PT_MATH_RESOLVE = 5, PT_MATH_ARITH = 6 };
int pt_selftest_math(int device, uint32_t op, uint64_t n, const void* in, void* out);

#ifdef __cplusplus
}
#endif
#endif /* PT_H */
