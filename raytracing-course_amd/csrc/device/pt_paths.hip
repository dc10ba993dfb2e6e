// pt_paths.hip -- the batch radiance engine: Scene::RayTrace (src/scene.cpp:83-178) for rays the
// caller supplies, one radiance record per path.  The closest-hit query is the
// path engine's (pt_query.h), the vertex and the fold are the integrator's (pt_trace.h:
// shade_vertex, fold_vertex), in trace_path_with's order; there are no pixels, sums, chains or rings.
//   k_paths   a lane per path, with refill: persistent waves, every trip advances each running
//             lane's query by one q_step; once enough lanes wait, a service step shades the
//             finished queries' vertices, folds the ended paths and takes the next ones
// A query the replay does not take (Q_EXACT: a non-finite ray, a hitting-leaf list full of entered
// hits) is answered in the service step by the exact stack DFS, on the lane's own LDS words.
#include <hip/hip_runtime.h>

#include "pt_batch.h"
#include "pt_paths.h"

namespace pt {

// a lane's path: its running query, its random stream and where it is in RayTrace's recursion
// (whose depth argument at the current ray is depth - nv)
struct PathLane {
    Query q;
    Rng R;
    uint32_t idx;     // the path's record
    uint32_t nv;      // vertices so far (fold records written)
    uint32_t nrays;   // RayIntersection calls so far
};

__device__ __forceinline__ void store_out(const PathsParams& P, uint32_t i, f3 L, uint32_t rays) {
    reinterpret_cast<uint4*>(P.out)[i] = make_uint4(f2u(L.x), f2u(L.y), f2u(L.z), rays);   // one 16-B store
}

// A lane takes path i: its record and a fresh stream.  False at RAY_DEPTH 0 (RayTrace returns
// black before it draws or intersects anything: the zeros are stored at once); true: the path's
// first ray is in `ray`
__device__ __forceinline__ bool take_path(const PathsParams& P, uint32_t i, PathLane& L, Ray& ray) {
    const uint4* rec = reinterpret_cast<const uint4*>(P.in) + 2u * (size_t)i;
    const uint4 a = rec[0], b = rec[1];
    if (P.depth == 0u) {
        store_out(P, i, mk3(0.f, 0.f, 0.f), 0u);
        return false;
    }
    ray.o = mk3(u2f(a.x), u2f(a.y), u2f(a.z));   // used as given, never normalised
    ray.d = mk3(u2f(a.w), u2f(b.x), u2f(b.y));
    L.R = rng_seed(b.z);
    L.idx = i;
    L.nv = 0u;
    L.nrays = 0u;
    return true;
}

// RayIntersection's start for the path's next ray, counted in its record
__device__ __forceinline__ void start_ray(const PathsParams& P, const Ray& ray, PathLane& L, QStats& st) {
    start_query(P.S, ray, L.q, st);
    L.nrays++;
}

// an ended path: its fold and its record
__device__ __forceinline__ void end_path(const PathsParams& P, const PathLane& L, const HbmVStore& vs, f3 leaf) {
    store_out(P, L.idx, fold_path(P.S, L.nv, vs, leaf), L.nrays);
}

// The occupancy the compiler is held to, in waves per SIMD (`make DEFS=-DPT_PATHS_WAVES_PER_EU=N`
// builds another; left to itself the compiler takes 188 VGPRs, 2 waves: the table in DESIGN.md §4.6)
#ifndef PT_PATHS_WAVES_PER_EU
#define PT_PATHS_WAVES_PER_EU 3
#endif
#define PT_PATHS_OCC __attribute__((amdgpu_waves_per_eu(PT_PATHS_WAVES_PER_EU, PT_PATHS_WAVES_PER_EU)))

#ifndef PT_PATHS_PLAIN
__global__ void __launch_bounds__(256) PT_PATHS_OCC k_paths(PathsParams P) {
    extern __shared__ uint32_t lds_stack[];
    const LaneStack ls = lane_stack(P, lds_stack);
    LdsMemN<64u> stk = ls.aux();
    HbmVStore vs = lane_fold(P);
    QStats st;
    PathLane L;
    L.q.phase = Q_DONE;
    bool have = false;        // this lane holds a path that has not ended
    WaveTake T{0u, true, 0ull};   // the wave's reservation of path indices (wave-uniform)
    // Why this loop ends, from the wave's own state alone (it waits for no other wave or workgroup
    // anywhere: the only shared word is the work counter, which is only ever added to; the fold
    // records and the LDS column are the lane's own):
    //   * a pull adds `batch` >= 64 to the work counter, so after at most n / batch + 1 pulls by
    //     all waves together every pull returns a value >= n and `more` turns false for good;
    //   * a lane that holds a path advances its query by one q_step per trip, and a query takes a
    //     finite number of steps (the state machine q_run loops over);
    //   * a path has at most RAY_DEPTH queries: each finished query's vertex raises `nv`, and the
    //     path ends at nv = RAY_DEPTH, at a miss or where the vertex ends it; the exact DFS a Q_EXACT
    //     query runs in the service step visits each reference node at most once;
    //   * a trip on which no lane runs is a service step, which gives every waiting lane its
    //     vertex -- after which the lane runs again or is empty -- and every empty lane a path
    //     while the reservation lasts, so it either starts queries, or hands out paths (the
    //     reservation shrinks, or a pull moves the counter on), or finds nothing left and leaves;
    //   * so the trips are bounded by the pulls, plus the steps of the queries of the paths the
    //     wave took.
    for (;;) {
        const bool run = have && q_running(L.q.phase);
        const unsigned long long mrun = __ballot(run);
        // The service step, once `service` lanes wait (a finished query, or empty) or none runs.
        // Not on every trip: a vertex recomputes its hit, samples and writes a fold record, a
        // taking lane tests the planes, each behind dependent loads the whole wave waits for.
        if (64u - (uint32_t)__popcll(mrun) >= P.service || mrun == 0ull) {
            Ray ray;
            bool start = false;   // this lane begins the query of `ray` below
            if (have && !run) {
                f3 leaf;
                start = lane_vertex(P.S, P.depth, L.q, L.R, L.nv, ls, vs, st, ray, leaf);
                if (!start) {
                    end_path(P, L, vs, leaf);
                    have = false;
                }
            }
            if (T.dry()) T.pull(P);
            if (T.rleft != 0u) {
                const unsigned long long m = __ballot(!have);
                const uint32_t k = lanes_below(m);
                if (!have && T.holds(k)) {
                    start = take_path(P, (uint32_t)T.item(k), L, ray);
                    have = start;
                }
                T.advance(m);
            }
            // (one copy of the planes and the set-up for the child rays and the first rays)
            if (start) start_ray(P, ray, L, st);
            if (T.spent() && __ballot(have) == 0ull) break;
        }
        if (have && q_running(L.q.phase)) q_step(P.S, L.q, st.C, stk);
    }
    st.flush(P.counters);
}
#else
// The plain form (`make DEFS=-DPT_PATHS_PLAIN`, measured against the refill form by
// tools/paths_bench.py): a lane per path, grid-stride, the whole path in the lane -- each wave as
// slow as its longest path
__global__ void __launch_bounds__(256) PT_PATHS_OCC k_paths(PathsParams P) {
    extern __shared__ uint32_t lds_stack[];
    const LaneStack ls = lane_stack(P, lds_stack);
    LdsMemN<64u> stk = ls.aux();
    HbmVStore vs = lane_fold(P);
    QStats st;
    PathLane L;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += stride) {
        Ray ray;
        if (!take_path(P, (uint32_t)i, L, ray)) continue;
        // (ends: a path has at most RAY_DEPTH queries, a query finitely many steps)
        for (;;) {
            start_ray(P, ray, L, st);
            while (q_running(L.q.phase)) q_step(P.S, L.q, st.C, stk);
            f3 leaf;
            if (lane_vertex(P.S, P.depth, L.q, L.R, L.nv, ls, vs, st, ray, leaf)) continue;
            end_path(P, L, vs, leaf);
            break;
        }
    }
    st.flush(P.counters);
}
#endif

}  // namespace pt

hipError_t pt_paths_occupancy(uint32_t block, uint32_t aux_words, uint32_t dfs_words, int* per_cu) {
    return pt::lanes_occupancy(pt::k_paths, block, aux_words, dfs_words, per_cu);
}

hipError_t pt_launch_paths(const pt::PathsParams& p, uint32_t grid, uint32_t block, hipStream_t s, hipEvent_t e0,
                           hipEvent_t e1) {
    return pt::launch_lanes(pt::k_paths, p, PT_PATHS_CTL_BYTES, grid, block, s, e0, e1);
}
