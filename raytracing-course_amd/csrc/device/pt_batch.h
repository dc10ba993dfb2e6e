// pt_batch.h -- what the batch engines share on the device (k_rays / k_feats through pt_rays.h's
// engine template, k_paths, k_pixels): a wave's statistics and their flush, the wave's reservation
// of items from the run's work counter, a lane's LDS column and fold records, RayIntersection's
// start, the vertex of a finished query, the backward fold, and the launch of a kernel whose lanes
// own such a column.  Each rule is stated here once; an engine's loop, its service step and the
// reasons its loop ends stay in the engine's own file.  DESIGN.md §4.5.
//
// Only the batch engines include this header: the render path's kernels (pt_path.hip, pt_wcoop.hip,
// pt_wave.hip, pt_kernels.hip) do not, and nothing here edits a header they read.
#pragma once
#include "pt_kernels.h"

namespace pt {

// The LDS of a workgroup of `block` threads whose lanes each own one column: the aux stack, or (the
// aux stack is dead by then) the exact DFS's stack, and the trash word.  One statement for the host's
// block fit, its occupancy query and the launch.
inline size_t lane_lds_bytes(uint32_t block, uint32_t aux_words, uint32_t dfs_words) {
    const uint32_t words = (aux_words > dfs_words ? aux_words : dfs_words) + 1u;
    return (size_t)(block / 64u) * 64u * 4u * words;
}

}  // namespace pt

#if defined(__HIPCC__)
#include "pt_devutil.h"

namespace pt {

// the statistics a wave gathered, flushed once (one atomic per counter and wave); returns the
// wave's counter copy, for an engine with counters of its own behind CTR_FALLBACKS_RAY
struct QStats {
    QCounts C{0u, 0u, 0u, 0u};
    uint32_t rays = 0u, err = 0u, exact = 0u, exact_ray = 0u;
    __device__ __forceinline__ unsigned long long* flush(unsigned long long* counters) const {
        unsigned long long* ctr = ctr_copy(counters);
        wave_add_u64(ctr + CTR_RAYS, rays);
        wave_add_u64(ctr + CTR_NODES, C.nodes);
        wave_add_u64(ctr + CTR_PTESTS, C.ptests);
        wave_add_u64(ctr + CTR_PLANES, C.planes);
        wave_add_u64(ctr + CTR_ERRORS, err);
        wave_add_u64(ctr + CTR_AUX, C.aux);
        wave_add_u64(ctr + CTR_FALLBACKS, exact);
        wave_add_u64(ctr + CTR_FALLBACKS_RAY, exact_ray);
        return ctr;
    }
};

// a query in this phase is advanced by the trip's q_step (in any other it waits for the service step)
__device__ __forceinline__ bool q_running(uint32_t phase) { return phase == Q_AUX || phase == Q_REPLAY; }

// A wave's reservation [rnext, rnext + rleft) of item indices, and whether the work counter may
// still be below n (all three wave-uniform).  PARAMS: head, batch (>= 64), n.  An aggregate, begun
// as WaveTake{0u, true, 0ull}: nothing reserved, the counter not yet seen.  A service step's use,
// by every lane of the wave:
//     if (T.dry()) T.pull(P);
//     if (T.rleft != 0u) {
//         const unsigned long long m = __ballot(!have);   // the empty lanes ask, in lane order
//         const uint32_t k = lanes_below(m);
//         if (!have && T.holds(k)) { ... this lane takes T.item(k) ... }
//         T.advance(m);
//     }
//     if (T.spent() && __ballot(have) == 0ull) break;
// (The members are small and take values, and the conditions stand at the call: the engines' code
// is then what it was with the three variables written out -- profiles/r26_batchcore.)
struct WaveTake {
    uint32_t rleft;
    bool more;
    unsigned long long rnext;
    // nothing reserved, and the counter may still be below n: time to pull
    __device__ __forceinline__ bool dry() const { return rleft == 0u && more; }
    // one atomic per pull, by one lane, for the whole wave
    template <class PARAMS>
    __device__ __forceinline__ void pull(const PARAMS& P) {
        unsigned long long got = 0ull;
        if ((threadIdx.x & 63u) == 0u) got = atomicAdd(P.head, (unsigned long long)P.batch);
        // (lane 0's value in scalar registers: the reservation is wave-uniform)
        const unsigned long long base =
            (unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(got >> 32)) << 32 |
            __builtin_amdgcn_readfirstlane((uint32_t)got);
        rnext = base;
        rleft = base < P.n ? (uint32_t)(P.n - base < P.batch ? P.n - base : P.batch) : 0u;
        more = base + P.batch < P.n;
    }
    // the hand-out: the k-th lane that asks gets the reservation's k-th item while it lasts ...
    __device__ __forceinline__ bool holds(uint32_t k) const { return k < rleft; }
    __device__ __forceinline__ unsigned long long item(uint32_t k) const { return rnext + k; }
    // ... and the reservation moves on by what the asking lanes `m` took
    __device__ __forceinline__ void advance(unsigned long long m) {
        const uint32_t took = (uint32_t)__popcll(m) < rleft ? (uint32_t)__popcll(m) : rleft;
        rnext += took;
        rleft -= took;
    }
    // nothing reserved and nothing left to pull: the wave leaves once no lane holds an item
    __device__ __forceinline__ bool spent() const { return rleft == 0u && !more; }
};

// the lane's LDS column: the query's aux stack, or (the aux stack is dead by then) the exact DFS's
struct LaneStack {
    uint32_t* base;
    uint32_t aux_words, dfs_words;
    __device__ __forceinline__ LdsMemN<64u> aux() const { return LdsMemN<64u>{base, aux_words, aux_words}; }
    __device__ __forceinline__ LdsMemN<64u> dfs() const { return LdsMemN<64u>{base, dfs_words, dfs_words}; }
};
template <class PARAMS>
__device__ __forceinline__ LaneStack lane_stack(const PARAMS& P, uint32_t* lds) {
    const uint32_t words = (P.aux_words > P.dfs_words ? P.aux_words : P.dfs_words) + 1u;
    // [word][lane] per wave
    return LaneStack{lds + (threadIdx.x >> 6) * 64u * words + (threadIdx.x & 63u), P.aux_words, P.dfs_words};
}
// the resident lane's fold records (PARAMS: fold, depth)
template <class PARAMS>
__device__ __forceinline__ HbmVStore lane_fold(const PARAMS& P) {
    return HbmVStore{P.fold + ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * P.depth};
}

// RayIntersection's start for `ray`: the planes, then the BVH query's set-up
__device__ __forceinline__ void start_query(const SceneView& S, const Ray& ray, Query& q, QStats& st) {
    float pt;
    int pid;
    q_planes(S, ray, pt, pid);
    st.C.planes += S.n_planes;
    q_init(S, ray, pt, pid, q);
    st.rays++;
    if (q.phase == Q_EXACT) st.exact_ray++;   // a non-finite ray: the exact DFS by design
}

// The vertex of a query that left Q_AUX / Q_REPLAY (trace_path_with's loop body after the query).
// The hit is recomputed from its primitive as q_run does (the probe computes t only); a Q_EXACT
// query is answered here by the exact DFS.  True: the path goes on with `ray`; false: it has
// ended with `leaf` below its nv fold records.  (RayTrace's depth argument at the current ray is
// depth - nv.)
__device__ __forceinline__ bool lane_vertex(const SceneView& S, uint32_t depth, const Query& q, Rng& R, uint32_t& nv,
                                            const LaneStack& ls, HbmVStore& vs, QStats& st, Ray& ray, f3& leaf) {
    ray = q.ray;
    Hit h;
    int id;
    if (q.phase == Q_EXACT) {
        LdsMemN<64u> xs = ls.dfs();
        id = q_exact(S, ray, xs, h, st.C);
        st.exact++;
    } else {
        id = q.res_id;
        if (id >= 0) {
            const bool ok = prim_intersect(S.prims[id], ray, h);
            if (!ok || f2u(h.t) != f2u(q.res_t)) st.err++;   // must never happen (the tests check)
        }
    }
    if (id < 0) {
        leaf = S.bg;
        return false;
    }
    uint32_t idm;
    float s1, s2;
    const bool cont = shade_vertex(S, R, ray, h, id, idm, s1, s2);
    vs.put(nv++, idm, s1, s2);   // nv < depth: a record follows a query, and a path has at most depth queries
    leaf = mk3(0.f, 0.f, 0.f);
    return cont && nv != depth;   // RayTrace(.., 0) = 0
}

// an ended path's value: the backward fold, deepest vertex first (trace_path_with's order)
__device__ __forceinline__ f3 fold_path(const SceneView& S, uint32_t nv, const HbmVStore& vs, f3 leaf) {
    f3 Lr = leaf;
    for (uint32_t k = nv; k > 0u;) {
        --k;
        uint32_t idm;
        float s1, s2;
        vs.get(k, idm, s1, s2);
        Lr = fold_vertex(S, Lr, idm, s1, s2);
    }
    return Lr;
}

// workgroups of `block` threads, each lane with its LDS column, that one compute unit holds of `kernel`
template <class KERNEL>
hipError_t lanes_occupancy(KERNEL kernel, uint32_t block, uint32_t aux_words, uint32_t dfs_words, int* per_cu) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kernel, (int)block,
                                                        lane_lds_bytes(block, aux_words, dfs_words));
}

// `kernel` on `s` with the lanes' LDS columns, after the memset of the run's control block (at
// p.head); e0 / e1 around the kernel
template <class KERNEL, class PARAMS>
hipError_t launch_lanes(KERNEL kernel, const PARAMS& p, uint32_t ctl_bytes, uint32_t grid, uint32_t block, hipStream_t s,
                        hipEvent_t e0, hipEvent_t e1) {
    hipError_t e = hipMemsetAsync(p.head, 0, ctl_bytes, s);
    if (e != hipSuccess) return e;
    if (e0 && (e = hipEventRecord(e0, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lane_lds_bytes(block, p.aux_words, p.dfs_words), s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return e1 ? hipEventRecord(e1, s) : hipSuccess;
}

}  // namespace pt
#endif  // __HIPCC__
