// pt_rays.hip -- the ray-query engine: Scene::RayIntersection (src/scene.cpp:46-77) for rays the
// caller supplies, one hit record per ray.  The query is the path engine's
// (pt_query.h: planes, then the auxiliary BVH and the replay of the reference's pruning), without
// pixels, chains, rings or a shade wave:
//   k_rays        a lane per ray, with refill: persistent waves, every trip advances each running
//                 lane by one q_step; once enough lanes have finished, they retire and take the
//                 next rays
//   k_rays_exact  the rays the replay does not take (Q_EXACT: non-finite components, a hitting-leaf
//                 list full of entered hits), one exact stack DFS per lane
#include <hip/hip_runtime.h>

#include "pt_devutil.h"
#include "pt_rays.h"

namespace pt {

__device__ __forceinline__ Ray load_ray(const RayRec* rays, size_t i) {
    const RayRec r = rays[i];
    Ray ray;
    ray.o = mk3(r.o[0], r.o[1], r.o[2]);   // used as given, never normalised
    ray.d = mk3(r.d[0], r.d[1], r.d[2]);
    return ray;
}

__device__ __forceinline__ void store_hit(RayHit* hits, size_t i, int id, const Hit& h) {
    RayHit o;
    const bool ok = id >= 0;
    o.id = ok ? id : -1;
    o.t = ok ? h.t : 0.f;
    o.n[0] = ok ? h.n.x : 0.f;
    o.n[1] = ok ? h.n.y : 0.f;
    o.n[2] = ok ? h.n.z : 0.f;
    o.interior = ok ? h.interior : 0u;
    hits[i] = o;
}

// the statistics a wave gathered, flushed once (one atomic per counter and wave)
struct RayStats {
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

// a lane takes ray i: the planes, then the BVH query's set-up
__device__ __forceinline__ void take_ray(const RaysParams& P, size_t i, Query& q, RayStats& st) {
    const Ray ray = load_ray(P.rays, i);
    float pt;
    int pid;
    q_planes(P.S, ray, pt, pid);
    st.C.planes += P.S.n_planes;
    q_init(P.S, ray, pt, pid, q);
    st.rays++;
    if (q.phase == Q_EXACT) st.exact_ray++;   // a non-finite ray: the exact DFS by design
}

// A query that left Q_AUX / Q_REPLAY retires (every lane of the wave calls this; `fin` = this lane
// retires ray i): a Q_EXACT ray joins the exact list, any other one stores its hit, recomputed from
// its primitive exactly as q_run does (the probe computes t only).
__device__ __forceinline__ void retire(const RaysParams& P, bool fin, size_t i, const Query& q, RayStats& st) {
    const bool ex = fin && q.phase == Q_EXACT;
    const uint32_t k = wave_append(P.exact_n, ex);
    if (ex) {
        P.exact[k] = (uint32_t)i;
        st.exact++;
    } else if (fin) {
        Hit h;
        if (q.res_id >= 0) {
            const bool ok = prim_intersect(P.S.prims[q.res_id], q.ray, h);
            if (!ok || f2u(h.t) != f2u(q.res_t)) st.err++;   // must never happen (the tests check)
        }
        store_hit(P.hits, i, q.res_id, h);
    }
}

#ifndef PT_RAYS_PLAIN
__global__ void __launch_bounds__(256) k_rays(RaysParams P) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t lane = threadIdx.x & 63u;
    // [word][lane] per wave: words 0 .. aux_words - 1, then the trash word
    LdsMemN<64u> stk{lds_stack + (threadIdx.x >> 6) * 64u * (P.aux_words + 1u) + lane, P.aux_words, P.aux_words};
    RayStats st;
    Query q;
    q.phase = Q_DONE;
    bool have = false;        // this lane holds a ray that has not retired
    size_t idx = 0;
    // the wave's reservation [rnext, rnext + rleft) of ray indices, and whether the work counter may
    // still be below n (all three wave-uniform)
    unsigned long long rnext = 0ull;
    uint32_t rleft = 0u;
    bool more = true;
    // Why this loop ends, from the wave's own state alone (it waits for no other wave or workgroup
    // anywhere: the only shared words are the work counter and the exact list's count, both only
    // ever added to):
    //   * a pull adds `batch` >= 64 to the work counter, so after at most n / batch + 1 pulls by
    //     all waves together every pull returns a value >= n and `more` turns false for good;
    //   * a lane that holds a ray advances by one q_step per trip, and a query takes a finite
    //     number of steps (the state machine q_run loops over);
    //   * a trip on which no lane runs is a service step, which retires every finished lane, so
    //     it either hands out rays (the reservation shrinks, or a pull moves the counter on) or
    //     finds nothing left and leaves;
    //   * so the trips are bounded by the pulls, plus the steps of the rays the wave took.
    for (;;) {
        const bool run = have && (q.phase == Q_AUX || q.phase == Q_REPLAY);
        const unsigned long long mrun = __ballot(run);
        // The service step, once `service` lanes wait (finished or empty) or none runs: the finished
        // lanes retire and the empty ones take rays.  Not on every trip: a retiring lane recomputes
        // its hit and a taking one tests the planes, each behind dependent loads that the whole
        // wave waits for -- a few lanes at a time, that cost as much as the trip's q_step.
        if (64u - (uint32_t)__popcll(mrun) >= P.service || mrun == 0ull) {
            const bool fin = have && !run;
            retire(P, fin, idx, q, st);
            if (fin) have = false;
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
                    idx = (size_t)(rnext + k);
                    take_ray(P, idx, q, st);
                    have = true;
                }
                const uint32_t took = (uint32_t)__popcll(m) < rleft ? (uint32_t)__popcll(m) : rleft;
                rnext += took;
                rleft -= took;
            }
            if (rleft == 0u && !more && __ballot(have) == 0ull) break;
        }
        if (have && (q.phase == Q_AUX || q.phase == Q_REPLAY)) q_step(P.S, q, st.C, stk);
    }
    st.flush(P.counters);
}
#else
// The plain form (`make DEFS=-DPT_RAYS_PLAIN`, measured against the refill form by
// tools/rays_bench.py): a lane per ray, grid-stride, each wave as slow as its slowest ray
__global__ void __launch_bounds__(256) k_rays(RaysParams P) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t lane = threadIdx.x & 63u;
    LdsMemN<64u> stk{lds_stack + (threadIdx.x >> 6) * 64u * (P.aux_words + 1u) + lane, P.aux_words, P.aux_words};
    RayStats st;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    // (a wave-uniform trip count: retire()'s append needs the whole wave)
    for (unsigned long long b = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); b < P.n; b += stride) {
        const size_t i = (size_t)(b + lane);
        const bool have = i < P.n;
        Query q;
        q.phase = Q_DONE;
        if (have) take_ray(P, i, q, st);
        while (q.phase == Q_AUX || q.phase == Q_REPLAY) q_step(P.S, q, st.C, stk);
        retire(P, have, i, q, st);
    }
    st.flush(P.counters);
}
#endif

// The exact list's rays (k_wexact's shape: 64-lane workgroups, grid-stride, the DFS stack in LDS);
// launched after every k_rays, its count read from device memory
__global__ void __launch_bounds__(64) k_rays_exact(RaysParams P) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t n = *P.exact_n;
    LdsMemN<64u> stk{lds_stack + threadIdx.x, P.dfs_words, P.dfs_words};
    RayStats st;
    for (uint32_t k = blockIdx.x * 64u + threadIdx.x; k < n; k += gridDim.x * 64u) {
        const size_t i = P.exact[k];
        const Ray ray = load_ray(P.rays, i);
        Hit h;
        const int id = q_exact(P.S, ray, stk, h, st.C);
        store_hit(P.hits, i, id, h);
    }
    st.C.planes = 0u;   // (k_rays counted these rays' plane tests when it took them)
    st.flush(P.counters);
}

}  // namespace pt

hipError_t pt_launch_rays(const pt::RaysParams& p, uint32_t grid, uint32_t block, hipStream_t s, hipEvent_t e0,
                          hipEvent_t e1) {
    hipError_t e = hipMemsetAsync(p.head, 0, PT_RAYS_CTL_BYTES, s);
    if (e != hipSuccess) return e;
    if (e0 && (e = hipEventRecord(e0, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(pt::k_rays, dim3(grid), dim3(block), (block / 64u) * 64u * 4u * (p.aux_words + 1u), s, p);
    hipLaunchKernelGGL(pt::k_rays_exact, dim3(256), dim3(64), 64u * 4u * (p.dfs_words + 1u), s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return e1 ? hipEventRecord(e1, s) : hipSuccess;
}
