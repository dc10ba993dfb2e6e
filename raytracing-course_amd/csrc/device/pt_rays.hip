// pt_rays.hip -- the ray-query engine: Scene::RayIntersection (src/scene.cpp:46-77) for rays the
// caller supplies, one hit record per ray.  The query is the path engine's
// (pt_query.h: planes, then the auxiliary BVH and the replay of the reference's pruning), without
// pixels, chains, rings or a shade wave:
//   k_rays        a lane per ray, with refill: persistent waves, every trip advances each running
//                 lane by one q_step; once enough lanes have finished, they retire and take the
//                 next rays
//   k_rays_exact  the rays the replay does not take (Q_EXACT: non-finite components, a hitting-leaf
//                 list full of entered hits), one exact stack DFS per lane
// Both are instantiations of pt_rays.h's engine templates with the job below.
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

// the ray-query job (pt_rays.h): item i is the caller's i-th ray, its record the i-th hit
struct RaysJob {
    const RaysParams& P;
    __device__ __forceinline__ Ray ray(size_t i) const { return load_ray(P.rays, i); }
    __device__ __forceinline__ void store(size_t i, int id, const Hit& h) const { store_hit(P.hits, i, id, h); }
};

#ifndef PT_RAYS_PLAIN
__global__ void __launch_bounds__(256) k_rays(RaysParams P) {
    rays_engine(P, RaysJob{P});
}
#else
// The plain form (`make DEFS=-DPT_RAYS_PLAIN`, measured against the refill form by
// tools/rays_bench.py): a lane per ray, grid-stride, each wave as slow as its slowest ray
__global__ void __launch_bounds__(256) k_rays(RaysParams P) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t lane = threadIdx.x & 63u;
    LdsMemN<64u> stk{lds_stack + (threadIdx.x >> 6) * 64u * (P.aux_words + 1u) + lane, P.aux_words, P.aux_words};
    QStats st;
    const RaysJob job{P};
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    // (a wave-uniform trip count: retire()'s append needs the whole wave)
    for (unsigned long long b = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); b < P.n; b += stride) {
        const size_t i = (size_t)(b + lane);
        const bool have = i < P.n;
        Query q;
        q.phase = Q_DONE;
        if (have) take_ray(P, job, i, q, st);
        while (q_running(q.phase)) q_step(P.S, q, st.C, stk);
        retire(P, job, have, i, q, st);
    }
    st.flush(P.counters);
}
#endif

// The exact list's rays (64-lane workgroups); launched after every k_rays
__global__ void __launch_bounds__(64) k_rays_exact(RaysParams P) {
    rays_exact_engine(P, RaysJob{P});
}

}  // namespace pt

hipError_t pt_launch_rays(const pt::RaysParams& p, uint32_t grid, uint32_t block, hipStream_t s, hipEvent_t e0,
                          hipEvent_t e1) {
    return pt::launch_rays_pair(pt::k_rays, pt::k_rays_exact, p, grid, block, s, e0, e1);
}
