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

#include "pt_devutil.h"
#include "pt_paths.h"

namespace pt {

// the statistics a wave gathered, flushed once (one atomic per counter and wave)
struct PathStats {
    QCounts C{0u, 0u, 0u, 0u};
    uint32_t rays = 0u, err = 0u, exact = 0u, exact_ray = 0u;
    __device__ __forceinline__ void flush(unsigned long long* counters) const {
        unsigned long long* ctr = ctr_copy(counters);
        wave_add_u64(ctr + CTR_RAYS, rays);
        wave_add_u64(ctr + CTR_NODES, C.nodes);
        wave_add_u64(ctr + CTR_PTESTS, C.ptests);
        wave_add_u64(ctr + CTR_PLANES, C.planes);
        wave_add_u64(ctr + CTR_ERRORS, err);
        wave_add_u64(ctr + CTR_AUX, C.aux);
        wave_add_u64(ctr + CTR_FALLBACKS, exact);
        wave_add_u64(ctr + CTR_FALLBACKS_RAY, exact_ray);
    }
};

// a lane's path: its running query, its random stream and where it is in RayTrace's recursion
struct PathLane {
    Query q;
    Rng R;
    uint32_t idx;     // the path's record
    uint32_t nv;      // vertices so far (fold records written)
    uint32_t rem;     // RayTrace's depth argument at the current ray
    uint32_t nrays;   // RayIntersection calls so far
};

// the lane's LDS column: the query's aux stack, or (the aux stack is dead by then) the exact DFS's
struct LaneStack {
    uint32_t* base;
    uint32_t aux_words, dfs_words;
    __device__ __forceinline__ LdsMemN<64u> aux() const { return LdsMemN<64u>{base, aux_words, aux_words}; }
    __device__ __forceinline__ LdsMemN<64u> dfs() const { return LdsMemN<64u>{base, dfs_words, dfs_words}; }
};
__device__ __forceinline__ LaneStack lane_stack(const PathsParams& P, uint32_t* lds) {
    const uint32_t words = (P.aux_words > P.dfs_words ? P.aux_words : P.dfs_words) + 1u;
    // [word][lane] per wave
    return LaneStack{lds + (threadIdx.x >> 6) * 64u * words + (threadIdx.x & 63u), P.aux_words, P.dfs_words};
}
__device__ __forceinline__ HbmVStore lane_fold(const PathsParams& P) {
    return HbmVStore{P.fold + ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * P.depth};
}

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
    L.rem = P.depth;
    L.nrays = 0u;
    return true;
}

// RayIntersection's start for `ray`: the planes, then the BVH query's set-up
__device__ __forceinline__ void start_query(const PathsParams& P, const Ray& ray, PathLane& L, PathStats& st) {
    float pt;
    int pid;
    q_planes(P.S, ray, pt, pid);
    st.C.planes += P.S.n_planes;
    q_init(P.S, ray, pt, pid, L.q);
    L.nrays++;
    st.rays++;
    if (L.q.phase == Q_EXACT) st.exact_ray++;   // a non-finite ray: the exact DFS by design
}

// The vertex of a query that left Q_AUX / Q_REPLAY (trace_path_with's loop body after the query).
// The hit is recomputed from its primitive as q_run does (the probe computes t only); a Q_EXACT
// query is answered here by the exact DFS.  True: the path goes on with `ray`; false: it has
// ended with `leaf` below its nv fold records.
__device__ __forceinline__ bool path_vertex(const PathsParams& P, PathLane& L, const LaneStack& ls, HbmVStore& vs,
                                            PathStats& st, Ray& ray, f3& leaf) {
    ray = L.q.ray;
    Hit h;
    int id;
    if (L.q.phase == Q_EXACT) {
        LdsMemN<64u> xs = ls.dfs();
        id = q_exact(P.S, ray, xs, h, st.C);
        st.exact++;
    } else {
        id = L.q.res_id;
        if (id >= 0) {
            const bool ok = prim_intersect(P.S.prims[id], ray, h);
            if (!ok || f2u(h.t) != f2u(L.q.res_t)) st.err++;   // must never happen (the tests check)
        }
    }
    if (id < 0) {
        leaf = P.S.bg;
        return false;
    }
    uint32_t idm;
    float s1, s2;
    const bool cont = shade_vertex(P.S, L.R, ray, h, id, idm, s1, s2);
    vs.put(L.nv++, idm, s1, s2);   // nv < depth: a record follows a query, and a path has at most depth queries
    L.rem--;
    leaf = mk3(0.f, 0.f, 0.f);
    return cont && L.rem != 0u;
}

// an ended path: the backward fold, deepest vertex first (trace_path_with's order), and its record
__device__ __forceinline__ void end_path(const PathsParams& P, const PathLane& L, const HbmVStore& vs, f3 leaf) {
    f3 Lr = leaf;
    for (uint32_t k = L.nv; k > 0u;) {
        --k;
        uint32_t idm;
        float s1, s2;
        vs.get(k, idm, s1, s2);
        Lr = fold_vertex(P.S, Lr, idm, s1, s2);
    }
    store_out(P, L.idx, Lr, L.nrays);
}

__device__ __forceinline__ bool q_running(const Query& q) { return q.phase == Q_AUX || q.phase == Q_REPLAY; }

// The occupancy the compiler is held to, in waves per SIMD (`make DEFS=-DPT_PATHS_WAVES_PER_EU=N`
// builds another; left to itself the compiler takes 188 VGPRs, 2 waves: the table in DESIGN.md §4.6)
#ifndef PT_PATHS_WAVES_PER_EU
#define PT_PATHS_WAVES_PER_EU 3
#endif
#define PT_PATHS_OCC __attribute__((amdgpu_waves_per_eu(PT_PATHS_WAVES_PER_EU, PT_PATHS_WAVES_PER_EU)))

#ifndef PT_PATHS_PLAIN
__global__ void __launch_bounds__(256) PT_PATHS_OCC k_paths(PathsParams P) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t lane = threadIdx.x & 63u;
    const LaneStack ls = lane_stack(P, lds_stack);
    LdsMemN<64u> stk = ls.aux();
    HbmVStore vs = lane_fold(P);
    PathStats st;
    PathLane L;
    L.q.phase = Q_DONE;
    bool have = false;        // this lane holds a path that has not ended
    // the wave's reservation [rnext, rnext + rleft) of path indices, and whether the work counter
    // may still be below n (all three wave-uniform)
    unsigned long long rnext = 0ull;
    uint32_t rleft = 0u;
    bool more = true;
    // Why this loop ends, from the wave's own state alone (it waits for no other wave or workgroup
    // anywhere: the only shared word is the work counter, which is only ever added to; the fold
    // records and the LDS column are the lane's own):
    //   * a pull adds `batch` >= 64 to the work counter, so after at most n / batch + 1 pulls by
    //     all waves together every pull returns a value >= n and `more` turns false for good;
    //   * a lane that holds a path advances its query by one q_step per trip, and a query takes a
    //     finite number of steps (the state machine q_run loops over);
    //   * a path has at most RAY_DEPTH queries: each finished query's vertex lowers `rem`, and the
    //     path ends at rem = 0, at a miss or where the vertex ends it; the exact DFS a Q_EXACT
    //     query runs in the service step visits each reference node at most once;
    //   * a trip on which no lane runs is a service step, which gives every waiting lane its
    //     vertex -- after which the lane runs again or is empty -- and every empty lane a path
    //     while the reservation lasts, so it either starts queries, or hands out paths (the
    //     reservation shrinks, or a pull moves the counter on), or finds nothing left and leaves;
    //   * so the trips are bounded by the pulls, plus the steps of the queries of the paths the
    //     wave took.
    for (;;) {
        const bool run = have && q_running(L.q);
        const unsigned long long mrun = __ballot(run);
        // The service step, once `service` lanes wait (a finished query, or empty) or none runs.
        // Not on every trip: a vertex recomputes its hit, samples and writes a fold record, a
        // taking lane tests the planes, each behind dependent loads the whole wave waits for.
        if (64u - (uint32_t)__popcll(mrun) >= P.service || mrun == 0ull) {
            Ray ray;
            bool start = false;   // this lane begins the query of `ray` below
            if (have && !run) {
                f3 leaf;
                start = path_vertex(P, L, ls, vs, st, ray, leaf);
                if (!start) {
                    end_path(P, L, vs, leaf);
                    have = false;
                }
            }
            if (rleft == 0u && more) {
                // one atomic per pull, by one lane, for the whole wave
                unsigned long long got = 0ull;
                if (lane == 0u) got = atomicAdd(P.head, (unsigned long long)P.batch);
                // (lane 0's value in scalar registers: the reservation is wave-uniform)
                const unsigned long long base =
                    (unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(got >> 32)) << 32 |
                    __builtin_amdgcn_readfirstlane((uint32_t)got);
                rnext = base;
                rleft = base < P.n ? (uint32_t)(P.n - base < P.batch ? P.n - base : P.batch) : 0u;
                more = base + P.batch < P.n;
            }
            if (rleft != 0u) {
                const unsigned long long m = __ballot(!have);
                const uint32_t k = lanes_below(m);
                if (!have && k < rleft) {
                    start = take_path(P, (uint32_t)(rnext + k), L, ray);
                    have = start;
                }
                const uint32_t took = (uint32_t)__popcll(m) < rleft ? (uint32_t)__popcll(m) : rleft;
                rnext += took;
                rleft -= took;
            }
            // (one copy of the planes and the set-up for the child rays and the first rays)
            if (start) start_query(P, ray, L, st);
            if (rleft == 0u && !more && __ballot(have) == 0ull) break;
        }
        if (have && q_running(L.q)) q_step(P.S, L.q, st.C, stk);
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
    PathStats st;
    PathLane L;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += stride) {
        Ray ray;
        if (!take_path(P, (uint32_t)i, L, ray)) continue;
        // (ends: a path has at most RAY_DEPTH queries, a query finitely many steps)
        for (;;) {
            start_query(P, ray, L, st);
            while (q_running(L.q)) q_step(P.S, L.q, st.C, stk);
            f3 leaf;
            if (path_vertex(P, L, ls, vs, st, ray, leaf)) continue;
            end_path(P, L, vs, leaf);
            break;
        }
    }
    st.flush(P.counters);
}
#endif

}  // namespace pt

hipError_t pt_paths_occupancy(uint32_t block, size_t lds_bytes, int* per_cu) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, pt::k_paths, (int)block, lds_bytes);
}

hipError_t pt_launch_paths(const pt::PathsParams& p, uint32_t grid, uint32_t block, hipStream_t s, hipEvent_t e0,
                           hipEvent_t e1) {
    hipError_t e = hipMemsetAsync(p.head, 0, PT_PATHS_CTL_BYTES, s);
    if (e != hipSuccess) return e;
    if (e0 && (e = hipEventRecord(e0, s)) != hipSuccess) return e;
    const uint32_t words = (p.aux_words > p.dfs_words ? p.aux_words : p.dfs_words) + 1u;
    hipLaunchKernelGGL(pt::k_paths, dim3(grid), dim3(block), (block / 64u) * 64u * 4u * words, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return e1 ? hipEventRecord(e1, s) : hipSuccess;
}
