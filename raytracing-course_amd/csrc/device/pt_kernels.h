// pt_kernels.h -- kernel parameter blocks shared by the host driver and the kernels.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
#include <hip/hip_runtime_api.h>
#endif
#include <stddef.h>

#include <type_traits>

#include "pt_query.h"

namespace pt {

struct TileMap {
    uint32_t W, H;        // full image size (seeds are y*W + x, camera uses W, H)
    uint32_t x0, y0;      // rendered window origin
    uint32_t ww, wh;      // rendered window size (= W, H for a full render)
    uint32_t tiles_x;     // ceil(ww/16)
    uint32_t n_tiles;     // ceil(ww/16)*ceil(wh/16)
    uint32_t rank, world; // window tile t belongs to rank tile_owner(t, tiles_x, world)
    const uint32_t* gtile;   // device: this rank's window tiles in ascending order (local -> window tile)
};

// The deal of a window's 16x16 tiles to the ranks of a multi-GPU render: tile
// (tx, ty) belongs to rank (tx + ty) % world.  Diagonal stripes give every rank
// every column and every row of the image in equal parts; the plain t % world
// deals whole tile columns whenever tiles_x % world == 0 (1080p: 120 tiles per
// row), and the dragon's columns cost more than the walls' (rank-of-8 spread 7 %).
// A rank's local tiles are its window tiles in ascending order.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t tile_owner(uint32_t t, uint32_t tiles_x, uint32_t world) {
    return (t % tiles_x + t / tiles_x) % world;
}

// Per owned slot (256 per owned tile) one 32-B record, read and written as two
// 16-B pieces: a shade touches ONE piece (one vector load + one store instead of
// five scattered dwords), the path end the second one as well.
//   rec[2 slot]     = {rng x, rng saved (f32 bits), rng flag | vertices << 8 (24 bits), samples done}
//   rec[2 slot + 1] = {sum.r, sum.g, sum.b, global pixel index y*W + x (its seed)}
// Fold records (one 16-B record per path vertex: {idm, s1, s2, -}) are slot-major,
// fold[slot * depth + k], so a path's records share lines.
struct PixelState {
    uint4* rec;           // 2 * n_slots
    uint4* fold;          // depth * n_slots
    uint32_t n_slots;
    uint32_t depth;       // fold records per slot (>= 1)
};

struct InitParams {
    TileMap tm;
    PixelState st;
};

struct TraceParams {
    SceneView S;
    CamView cam;
    TileMap tm;
    PixelState st;
    unsigned long long* counters; // statistics counters (the CTR_* slots below)
    ReplayCfg cfg;
    uint32_t depth;
    uint32_t spp;
    uint32_t n_tiles_local;
    unsigned long long* wg_prof;  // optional per-workgroup {start, end, HW_ID, XCC_ID} (diagnostics)
};

// ---- wavefront renderer (pt_wave.h: pt_wave.hip, pt_path.hip, pt_wcoop.hip) ----
struct RayQ {                     // rays waiting for a closest-hit query
    F4* ro;                       // {o.xyz, u32 slot}
    F4* rd;                       // {d.xyz, P = closest plane t (computed by the producer)}
    int* pid;                     // the closest plane's prim (-1 none)
    F4* ri;                       // q_prep record {1/d.xyz, dl | par | exact} (computed by the producer)
};
struct DoneQ {                    // finished queries, input of the shade kernel
    F4* ro;                       // {o.xyz, u32 slot}
    F4* rd;                       // {d.xyz, -}
    uint32_t* id;                 // closest prim (the shade kernel recomputes t, n, side from it), 0xffffffff = miss
};
// how a path ended (coop_shade)
enum : uint32_t { PE_LIVE = 0u, PE_MISS = 1u, PE_CUT = 2u, PE_TERM = 3u };

// round counters: set p = ctl + PT_CTL_SET * p; the work-batch heads are one per
// XCD, each on its own 128-B line (C_HEADS + 32 x)
enum : uint32_t { C_FRESH = 0u, C_CARRY = 1u, C_DONE = 3u, C_EXACT = 4u, C_FRONT = 5u, C_BACK = 6u, C_WGDONE = 7u,
                  C_DEADLINE = 8u, C_ENDED = 9u, C_HEADS = 32u };
// C_ENDED: k_wcoop chains whose pixel reached the pass target (the final launch stops at
// side_stop_n of them to hand its last chains to whole-wave teams)
// C_WGDONE: k_wpath workgroups that have finished the round; C_DEADLINE: the round's end
// (low 32 bits of the 100-MHz realtime clock, 0 = not set yet; WaveParams::path_ticks)
#define PT_CTL_SET 288u          // words per counter set (C_HEADS + 8 x 32)
// statistics counters: one copy per XCD (PT_CTR_COPIES x PT_CTR_STRIDE u64), summed by the host
#define PT_CTR_COPIES 8u
#define PT_CTR_STRIDE 32u

struct WaveParams {
    SceneView S;
    const AuxSL* top;             // k_wcamera: the wide aux root's entries, then its inner entries' child
                                  // nodes' (entry k's child at top[PT_AUXW (1 + k)]; host form, f32)
    uint32_t n_top;               // entries in top
    uint32_t n_aux;               // wide aux entries in the blob
    CamView cam;
    TileMap tm;
    PixelState st;                // per-slot records (RNG, vertices, samples done, sum) + fold records
    RayQ fq[2];                   // fresh rays: round with parity p reads fq[p], appends to fq[1-p]
    uint32_t* cq[2];              // suspended queries (carry_words each): read cq[p], append to cq[1-p]
    uint32_t carry_cap, carry_words;
    DoneQ done;
    RayQ ex;                      // rays handed to the exact DFS this round
    uint2* endq;                  // per path workgroup path_cmax(NQ) entries: its shade wave's ended paths
                                  // {slot | miss << 31, LDS pixel-table entry}
    uint32_t* ctl;                // 2 x PT_CTL_SET round counters
    unsigned long long* counters; // statistics counters (the CTR_* slots below)
    uint32_t depth;
    uint32_t parity;
    uint32_t target;              // samples per pixel to reach in this pass
    uint32_t n_tiles_local;
    uint32_t max_stack;           // exact DFS stack words per lane
    uint32_t aux_stack;           // wide aux traversal stack words per lane (LDS)
    unsigned long long* wg_prof;  // optional (diagnostics): per isect workgroup {start, end, HW_ID, XCC_ID, steps}
    // path engine (k_wpath): chains continue inside the kernel
    uint32_t path;                // 1 (k_wshade shades the exact-DFS results only)
    uint32_t path_budget;         // loop trips a query wave keeps its chains going after the round's work ran out
    uint32_t path_ticks;          // ... or, if nonzero, 100-MHz clock ticks after the first wave found it out:
                                  // every wave of the round stops at that one time
    uint32_t path_runend;         // a round with at most this many chains runs them to the end of the pass
    unsigned long long* progress; // optional host-mapped count of finished samples (progress bar), or null
    uint32_t path_cap;            // chains a workgroup may hold (<= path_cmax(NQ))
    uint32_t lstack;              // aux stack words a query lane may use (<= PT_LSTACK; deeper: exact DFS)
    const uint32_t* tile_order;   // k_wcamera: block b seeds local tile tile_order[b] (null: tile b)
    uint32_t sparse_steps;        // steps per loop trip of the end-of-pass (sparse) kernel
    uint32_t coop_reserve;        // k_wcoop: aux stack words kept free for a depth-first descent (3 (aux depth + 2))
    // k_wpath's per-trip step mix (the host may change it per round, from the chains left)
    uint32_t probe_every;         // candidate probes every n-th trip (>= 1) ...
    uint32_t probe_min;           // ... or whenever this many lanes wait for one
    uint32_t aux_extra;           // extra aux-node steps per trip for the lanes whose next step is one
    uint32_t batch;               // k_wpath: round-queue entries a wave takes per pull (at most)
    uint32_t end_min;             // k_wpath: ended paths the shade wave folds in a batch of their own (1..64;
                                  // fewer when nothing else waits: PT_END_MIN)
    // k_wcoop's intake order (null: queue order): the round's work items by the pixels'
    // remaining samples, most first (k_coop_order); `order_cur` = its 256 bucket cursors
    uint32_t* order;
    uint32_t* order_cur;
    // k_wpath's intake through an index list (null: the queues in order): work item i of
    // the round is queue item pin[i], i < pin_n (the round after an early cooperative
    // launch took the first entries of the intake order)
    const uint32_t* pin;
    uint32_t pin_n;
    // a cooperative launch beside a path round (the early launch): it stops at a chain
    // cycle's end once side_stop counts side_stop_n finished path workgroups, and yields its
    // chains as suspended queries at their start (q_init_pre: the ray was counted when it was
    // first taken) to yield_cq (counter yield_ctr: the path round's next carry queue).  The
    // pass's final launch uses the same stop with side_stop = its own C_ENDED: once all but
    // its last chains have ended, those go to a launch of whole-wave teams
    const uint32_t* side_stop;
    uint32_t side_stop_n;
    uint32_t* yield_cq;
    uint32_t* yield_ctr;
    uint32_t side_flags;          // PT_SIDE_* test hooks of that launch (0 in every render)
    // test hook (PT_TUNE drop=<site>): 1 + the hand-off site (PT_HO_*, include/pt.h) whose
    // items are dropped instead of handed on -- their chains are lost, which the resolve
    // must report (0 in every render)
    uint32_t drop;
};
// A suspended query's record in a carry queue (WaveParams::cq, carry_words words each):
//   Query | pixel slot | the query lane's aux stack words (Query::sp of them)
// The path engine resumes a query from the whole record; the cooperative engine restarts
// it from its ray and slot alone (a query is a function of its ray), so a restart record
// -- a query at its start -- needs only those two: the ray is the Query's first member.
static_assert(offsetof(Query, ray) == 0, "a carry record starts with its query's ray");
static_assert(sizeof(Query) % 4u == 0, "a carry record is addressed in words");
constexpr uint32_t CARRY_QUERY_WORDS = (uint32_t)(sizeof(Query) / 4u);
// a record's words for an aux stack of `stack_words`, rounded to 16 B
constexpr uint32_t carry_record_words(uint32_t stack_words) {
    return (CARRY_QUERY_WORDS + 1u + stack_words + 3u) & ~3u;
}
template <class W>   // uint32_t, or const uint32_t for a record that is only read
struct CarryRec {
    template <class T>
    using As = typename std::conditional<std::is_const<W>::value, const T, T>::type;
    W* w;
    PT_HD As<Query>& query() const { return *reinterpret_cast<As<Query>*>(w); }
    PT_HD As<Ray>& ray() const { return *reinterpret_cast<As<Ray>*>(w); }
    PT_HD W& slot() const { return w[CARRY_QUERY_WORDS]; }
    PT_HD W& stack(uint32_t j) const { return w[CARRY_QUERY_WORDS + 1u + j]; }
    // The whole record of a query lane: its state, slot and the q.sp words of its aux stack
    // `stk`.  (One pointer past the Query indexed by the loops, not stack(j) per word: the
    // path engine's suspend and resume then compile to the stores and loads they always were.)
    template <class STK>
    PT_HD void suspend(const Query& q, uint32_t slot_, const STK& stk) const {
        query() = q;
        W* tail = w + CARRY_QUERY_WORDS;
        tail[0] = slot_;
        for (uint32_t j = 0; j < q.sp; ++j) tail[1u + j] = stk.get(j);
    }
    template <class STK>
    PT_HD void resume(Query& q, uint32_t& slot_, STK& stk) const {
        q = query();
        W* tail = w + CARRY_QUERY_WORDS;
        slot_ = tail[0];
        for (uint32_t k = 0; k < q.sp; ++k) stk.set(k, tail[1u + k]);
    }
};
// record k of a queue of `words`-word records
template <class W>
PT_HD CarryRec<W> carry_rec(W* queue, uint32_t k, uint32_t words) { return CarryRec<W>{queue + (size_t)k * words}; }
// A restart record, a query at its start: the whole Query (a record the path engine may
// resume: coop_restart) ...
PT_HD void carry_put_restart(CarryRec<uint32_t> r, const Query& q, uint32_t slot) {
    r.query() = q;
    r.slot() = slot;
}
// ... or its ray alone (k_side_take: only the cooperative engine reads these records, and
// it reads ray() and slot(), never query())
PT_HD void carry_put_restart(CarryRec<uint32_t> r, const Ray& ray, uint32_t slot) {
    r.ray() = ray;
    r.slot() = slot;
}

// k_wcoop beside a path round, test hooks (PT_TUNE side_late / handon): every workgroup
// behaves as one that started after the round's end (takes nothing, hands every item on);
// the untaken items are dropped instead of handed on (a lost chain: the resolve's check)
#define PT_SIDE_LATE 1u
#define PT_SIDE_NO_HANDON 2u
// the final launch's stop: side_stop (its C_ENDED) against n_total - side_stop_n
#define PT_STOP_GROW 4u
// ... test hook (PT_TUNE grow_late): that launch's odd workgroups behave as late ones
// (stop at once and hand their untaken items on, through the intake order)
#define PT_GROW_LATE 8u
// ... test hook (PT_TUNE side_stop_now): the early launch stops after its first chain cycle
// (every team then yields its chain to the next round's carry queue)
#define PT_SIDE_STOP_NOW 16u
// path rounds, test hook (PT_TUNE shade_hold): the shade wave shades nothing until every
// query wave has left (in rounds with a budget), so all it shades goes through its flush
#define PT_SHADE_HOLD 32u
#define PT_ORDER_BUCKETS 256u

// path engine geometry: NQ query waves + 1 shade wave per workgroup (a template
// parameter of the engine: k_wpath<NQ, SPARSE>); at most path_cmax(NQ) chains resident
// per workgroup (= the capacity of its ray ring).
// Two query waves per shade wave since the hit-region query made the queries
// cheaper than their shading (3 -> 2 at 4 workgroups per CU: +13 % at rank-of-1,
// +20 % at rank-of-8; 1 query wave: -8 %).  The low-chain rounds, the end-of-pass
// kernel and everything beside a cooperative launch run that shape; the full rounds may
// run NQ = 3 at 3 workgroups per CU (PT_TUNE nq): 9 query waves per CU
// against 8, at the same 3 waves per SIMD.  Measured again in round 8 (profiles/r08_nq3):
// -12 % on the bench (a rank of 1), -13 % to -18 % at rank 0 of 8 -- at the product's rate the shade wave already takes 48 items
// per batch with 2 query waves, and with 3 its batches are full (60 of 64) and the done
// rings fill (36 of 48): the shade wave sets the rate.  2 stays the default.
#define PT_NQ_BASE 2u
#ifndef PT_NQ_FULL
#define PT_NQ_FULL 2u                  // the full rounds' shape when PT_TUNE nq is not given
#endif
#ifndef PT_PATH_WAVES_PER_EU
#define PT_PATH_WAVES_PER_EU 3u        // k_wpath occupancy (waves per SIMD) the compiler is held to
#endif
// k_wpath's default step mix (WaveParams probe_every / probe_min / aux_extra)
#define PT_PROBE_EVERY 3u              // candidate probes every n-th trip (1: every trip; 2 / 4 / 8 measured
                                       // within 1 % of 3, all +8-10 % over 1)
#define PT_AUX2 1u                     // extra aux-node steps per trip for the lanes whose next step is one
                                       // (+4.5 % at rank-of-1; 167 VGPRs)
#ifndef PT_END_MIN
#define PT_END_MIN 64u                 // k_wpath: the shade wave folds ended paths in batches of their own, once
                                       // this many wait (or nothing else is there to shade); 32 / 48 measured
                                       // +3.7 % / +5.6 %, 64 +6.2 % over folding in every shade batch
#endif
#ifndef PT_END_MIN_LOW
#define PT_END_MIN_LOW 48u             // ... in the low-chain rounds (WaveParams::end_min; round 5, three
                                       // interleaved repeats against 64: rank of 8 -3 %, of 4 -1 %, of 1 +-0;
                                       // 16 / 32 no better)
#endif
#define PT_PROBE_MIN 32u               // ... or whenever this many lanes wait for one (round 5: 32 against 16,
                                       // three interleaved repeats: rank of 1 -1.2 %, of 4 -1 %, of 8 -4 %;
                                       // 24 / 40 / 48 / 64 between or worse)
#ifndef PT_CMAX
#define PT_CMAX 384u                   // (512 until round 3; the LDS pixel table took the room)
#endif
#ifndef PT_CMAX3
#define PT_CMAX3 384u                  // ... of an NQ = 3 workgroup (448 measured the same; 480 = 53,840 B ran only 2
                                       // workgroups per CU: LDS is allocated in coarser steps than a byte)
#endif
// a shape's chain capacity and its workgroups per CU (PT_PATH_WAVES_PER_EU waves on each of 4 SIMDs)
constexpr uint32_t path_cmax(uint32_t nq) { return nq == 3u ? PT_CMAX3 : PT_CMAX; }
constexpr uint32_t path_wg_per_cu(uint32_t nq) { return PT_PATH_WAVES_PER_EU * 4u / (nq + 1u); }
// The rings, the query lanes' aux stacks and the resident chains' pixel records
// live in LDS (4 workgroups of NQ = 2 per CU, or 3 of NQ = 3; pt_path.hip static_asserts the fit):
//   pixel table path_cmax(NQ) entries (16 B: RNG, vertex count, samples done -- rec[2 slot]
//              while the chain stays in the workgroup) and their free ring
//   ray ring   path_cmax(NQ) entries (54 B: ray, slot, plane t and prim, q_prep record, table entry)
//   done rings PT_DQN entries per query wave (34 B: ray, slot, closest prim, table entry),
//              flow-controlled (a finished query waits in its lane while its ring is full)
//   aux stack  PT_LSTACK words per query lane; a query that would need more takes the
//              exact DFS (none of 10^6 measured queries needed more than 11)
#define PT_DQN 48u                     // (64 until round 3; the LDS pixel table took the room)
#define PT_LSTACK 16u                  // (+1 word per lane: the stack's trash word)

// cooperative engine (k_wcoop, the end of a pass): one wave per chain, QC_WAVES
// independent waves per workgroup, per-team and per-wave LDS for the query (pt_wcoop.hip QcTeamLds, QcPoolLds)
#ifndef QC_WAVES
#define QC_WAVES 4u
#endif
#define QC_SCAP_MIN 128u           // aux stack words per team (the smallest; also the exact DFS stack)
// The engine's LDS capacities for teams of t lanes (QcTeamLds / QcPoolLds, and the host's
// admission of a scene to a team size).  Aux stack words per chain (also its leader's exact
// DFS stack): a whole-wave team's own; smaller teams share their wave's pool, this many words
// per chain (teams of 4: 64, so that their wave's pool -- 16 chains -- stays at 1,024 words)
constexpr uint32_t qc_stack_words(uint32_t t) { return t == 64u ? 448u : t == 32u ? 192u : t == 4u ? 64u : QC_SCAP_MIN; }
// ... the pool's words per wave (teams below 64)
constexpr uint32_t qc_pool_words(uint32_t t) { return qc_stack_words(t) * (64u / t); }
// ... and its items, chain << shift | node: an aux entry index must stay below 2^shift
constexpr uint32_t qc_item_shift(uint32_t t) { return 64u / t > 8u ? 28u : 29u; }
#ifndef QC_EPL
#define QC_EPL 1u                  // aux entries a team lane tests per expansion round (nodes per round:
                                   // QC_EPL x team / 4)
#endif
#define QC_FOLD 6u                 // fold records held in LDS per chain (deeper vertices: HBM fold records)
#define QC_NPL 8u                  // plane records copied to LDS per workgroup (further planes: from HBM)
#define QC_NEM 8u                  // emitter records copied to LDS per workgroup (further emitters: from HBM)
#define QC_TOPN 21u                // aux BVH nodes 0..20 (BFS order: the top three levels) copied to LDS

struct ResolveParams {
    PixelState st;
    TileMap tm;                   // which slots are pixels (the rest of a partial edge tile are not)
    const float* thr;             // 256 gamma thresholds
    uint8_t* out;                 // 3 * n_slots
    float* rad;                   // optional 3 * n_slots
    uint32_t samples;             // samples accumulated so far
    unsigned long long* counters; // statistics counters: C_SHORT counts the owned pixels whose
                                  // samples done differ from `samples` (a lost chain; must be 0)
};
// statistics counter slots (per copy, PT_CTR_STRIDE u64): pt_stats' rays .. fallbacks_ray, the
// cooperative engine's share of them (CTR_COOP_*), the resolve's short pixels, the chains handed
// on; CTR_HO + PT_HO_*: the items handed on at each hand-off site (include/pt.h PT_HO_*;
// DESIGN.md §4 "Hand-off sites")
enum : uint32_t {
    CTR_RAYS = 0u, CTR_NODES = 1u, CTR_PTESTS = 2u, CTR_PLANES = 3u, CTR_ERRORS = 4u, CTR_AUX = 5u,
    CTR_FALLBACKS = 6u, CTR_FALLBACKS_RAY = 7u, CTR_COOP_RAYS = 8u, CTR_COOP_NODES = 9u, CTR_COOP_PTESTS = 10u,
    CTR_SHORT = 11u, CTR_HANDON = 12u, CTR_COOP_AUX = 13u, CTR_HO = 16u
};
// (the 14 named slots are distinct -- together exactly bits 0-13 -- and lie below CTR_HO)
static_assert((1u << CTR_RAYS | 1u << CTR_NODES | 1u << CTR_PTESTS | 1u << CTR_PLANES | 1u << CTR_ERRORS |
               1u << CTR_AUX | 1u << CTR_FALLBACKS | 1u << CTR_FALLBACKS_RAY | 1u << CTR_COOP_RAYS |
               1u << CTR_COOP_NODES | 1u << CTR_COOP_PTESTS | 1u << CTR_SHORT | 1u << CTR_HANDON |
               1u << CTR_COOP_AUX) == (1u << 14) - 1u && 14u <= CTR_HO,
              "statistics counter slots: two names share a slot, or one reaches the hand-off sites");
// a diagnostic slot beside them (no pt_stats field: PT_TUNE roundlog=2 prints it per round): the
// path engine's finished queries that found their done ring full and were still waiting in their
// lanes when their round ended (counted where they are suspended, off the trip)
enum : uint32_t { CTR_DQ_FULL = 14u };
static_assert(CTR_DQ_FULL >= 14u && CTR_DQ_FULL < CTR_HO, "the diagnostic slot lies between the named slots and the hand-off sites");
// the hand-off sites (include/pt.h PT_HO_*, which the host checks these against)
enum : uint32_t { HO_SUSPEND = 0u, HO_FLUSH, HO_RINGOUT, HO_EXACT, HO_SIDE_TAKE, HO_SIDE_YIELD, HO_SIDE_HANDON,
                  HO_GROW_YIELD, HO_GROW_HANDON, HO_N };

}  // namespace pt

hipError_t pt_preload_kernels_base();
hipError_t pt_preload_kernels_wave();
hipError_t pt_launch_init(const pt::InitParams& p, uint32_t n_tiles, hipStream_t s);
// diagnostics (PT_TUNE prespin_us): every lane busy for `us` microseconds
hipError_t pt_launch_spin(uint32_t us, uint32_t blocks, float* sink, hipStream_t s);
// variant: bit 0 = filtered node tests + flat replay, bit 1 = XCD-banded tile order
hipError_t pt_launch_trace(const pt::TraceParams& p, bool fast, uint32_t lds_bytes, hipStream_t s);
// wavefront pipeline (pt_wave.hip, pt_path.hip, pt_wcoop.hip): start a pass (first camera ray of every
// owned pixel), then path-engine rounds
hipError_t pt_launch_wave_start(pt::WaveParams p, hipStream_t s);
// path engine round: {k_wpath, k_wexact, k_wshade (exact results)}
// sparse: the end-of-pass kernel (few chains: every step kind and several steps per trip)
// (neither this nor pt_launch_coop zeroes the round's output counter set: the pass loop does,
// once per round -- host/rounds.cpp zero_round_out)
// nq: the launch's shape, query waves per workgroup (2, or 3 -- not the sparse kernel); p.endq holds
// path_cmax(nq) entries per workgroup and p.path_cap is at most path_cmax(nq)
hipError_t pt_launch_path_round(pt::WaveParams p, uint32_t nq, uint32_t path_grid, uint32_t shade_grid, hipStream_t s,
                                bool sparse, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// the cooperative engine's intake order (WaveParams::order): the round's n work items
// counting-sorted by their pixels' remaining samples, most first
hipError_t pt_launch_coop_order(pt::WaveParams p, uint32_t n, hipStream_t s);
// the early cooperative launch's queue: the first k items of p.order (the pixels with the
// most samples left) copied into `side` -- fresh rays as they are, suspended queries as
// restart records (their ray and slot) -- whose round counters side_ctl[C_CARRY / C_FRESH]
// count them (zeroed by the caller)
hipError_t pt_launch_side_take(pt::WaveParams p, uint32_t k, pt::RayQ side, uint32_t* side_carry, uint32_t* side_ctl,
                               hipStream_t s);
// cooperative engine: one launch runs every remaining chain of the pass to its end
// team = lanes per chain (8 -- the default --, 16, 32 or 64)
// big: the scene exceeds the LDS tables (QC_FOLD / QC_NPL / QC_NEM; team 8 or 64 then)
hipError_t pt_launch_coop(pt::WaveParams p, uint32_t grid, uint32_t team, bool big, hipStream_t s,
                          hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
hipError_t pt_launch_resolve(const pt::ResolveParams& p, uint32_t n_tiles, hipStream_t s);
// the row-major ww x wh x 3 framebuffer from packed tiles: window tile t at byte src[t] of `in`
// (src null: t * 768, the packed buffer of a session that owns every tile)
hipError_t pt_launch_untile(const uint8_t* in, const uint32_t* src, uint32_t tiles_x, uint32_t ww, uint32_t wh,
                            uint8_t* fb, hipStream_t s);
