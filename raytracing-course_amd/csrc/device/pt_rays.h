// pt_rays.h -- the ray-query engine's parameter block (pt_rays.hip, host/rayq.cpp): closest-hit
// queries (Scene::RayIntersection, src/scene.cpp:46-77) for rays the caller supplies -- no pixels,
// no chains, no shading.  DESIGN.md §4.5.
//
// The engine itself -- the persistent refill loop, its service step, the exact list and the
// per-wave counter flush -- is a template over a job type (rays_engine / rays_exact_engine below,
// device compiles only; the reservation, the statistics and the query's start are pt_batch.h's), so that an engine with another source of rays and another record per item
// instantiates it and does not copy it: pt_rays.hip with the caller's rays and 24-B hits,
// pt_feats.hip with the camera's rays and 64-B first-hit features.
#pragma once
#include "pt_kernels.h"

namespace pt {

// the records of include/pt.h (pt_ray, pt_ray_hit), 24 B each
struct RayRec { float o[3], d[3]; };
struct RayHit { int32_t id; float t; float n[3]; uint32_t interior; };   // a miss: id = -1, the rest 0

// A run's control block, zeroed by one memset on the run's stream before its launches:
//   u64 head     the work counter: rays [0, head) have been taken by some wave
//   u32 exact_n  rays on the exact list (k_rays_exact's count)
#define PT_RAYS_CTL_BYTES 16u
// k_rays: waiting lanes (finished or empty) at which a wave retires and refills (PT_TUNE rays_service)
#define PT_RAYS_SERVICE 32u

struct RaysParams {
    SceneView S;
    const RayRec* rays;
    RayHit* hits;
    uint32_t n;
    uint32_t batch;               // rays a wave reserves per pull of the work counter (>= 64)
    uint32_t service;             // waiting lanes (finished or empty) at which a wave retires and refills (1..64)
    unsigned long long* head;
    uint32_t* exact_n;
    uint32_t* exact;              // the exact list: indices of the rays the replay hands to the exact DFS
    unsigned long long* counters; // PT_CTR_COPIES x PT_CTR_STRIDE statistics counters (pt_kernels.h CTR_RAYS ..
                                  // CTR_FALLBACKS_RAY of each copy)
    uint32_t aux_words;           // k_rays: aux stack words per lane (LDS; + a trash word)
    uint32_t dfs_words;           // k_rays_exact: exact DFS stack words per lane (LDS; + a trash word)
};

}  // namespace pt

// k_rays then k_rays_exact on `s`, after the control block's memset; `block` = threads per k_rays
// workgroup (a multiple of 64 whose stacks fit the workgroup's LDS); e0 / e1 around the two kernels
hipError_t pt_launch_rays(const pt::RaysParams& p, uint32_t grid, uint32_t block, hipStream_t s, hipEvent_t e0,
                          hipEvent_t e1);

#if defined(__HIPCC__)
// ---- the engine (device code) ----------------------------------------------------------------
// PARAMS: a parameter block with RaysParams' run members (S, n, batch, service, head, exact_n,
// exact, counters, aux_words, dfs_words).  JOB: what an item is --
//   Ray  ray(size_t i) const                             the ray of item i
//   void store(size_t i, int id, const Hit& h) const     item i's record from its closest hit (id < 0: a miss,
//                                                        h then holds nothing)
#include "pt_batch.h"

namespace pt {

// a lane takes item i: RayIntersection's start for its ray
template <class PARAMS, class JOB>
__device__ __forceinline__ void take_ray(const PARAMS& P, const JOB& job, size_t i, Query& q, QStats& st) {
    start_query(P.S, job.ray(i), q, st);
}

// A query that left Q_AUX / Q_REPLAY retires (every lane of the wave calls this; `fin` = this lane
// retires item i): a Q_EXACT ray joins the exact list, any other one stores its record, the hit
// recomputed from its primitive exactly as q_run does (the probe computes t only).
template <class PARAMS, class JOB>
__device__ __forceinline__ void retire(const PARAMS& P, const JOB& job, bool fin, size_t i, const Query& q,
                                       QStats& st) {
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
        job.store(i, q.res_id, h);
    }
}

// a lane per item, with refill: persistent waves, every trip advances each running lane by one
// q_step; once enough lanes have finished, they retire and take the next items.  The workgroup's
// dynamic LDS: (blockDim.x / 64) x 64 x (aux_words + 1) words.
template <class PARAMS, class JOB>
__device__ __forceinline__ void rays_engine(const PARAMS& P, const JOB& job) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t lane = threadIdx.x & 63u;
    // [word][lane] per wave: words 0 .. aux_words - 1, then the trash word
    LdsMemN<64u> stk{lds_stack + (threadIdx.x >> 6) * 64u * (P.aux_words + 1u) + lane, P.aux_words, P.aux_words};
    QStats st;
    Query q;
    q.phase = Q_DONE;
    bool have = false;        // this lane holds a ray that has not retired
    size_t idx = 0;
    WaveTake T{0u, true, 0ull};   // the wave's reservation of item indices (wave-uniform)
    // Why this loop ends, from the wave's own state alone (it waits for no other wave or workgroup
    // anywhere: the only shared words are the work counter and the exact list's count, both only
    // ever added to):
    //   * a pull adds `batch` >= 64 to the work counter, so after at most n / batch + 1 pulls by
    //     all waves together every pull returns a value >= n and `more` turns false for good;
    //   * a lane that holds a ray advances by one q_step per trip, and a query takes a finite
    //     number of steps (the state machine q_run loops over);
    //   * a trip on which no lane runs is a service step, which retires every finished lane, so
    //     it either hands out items (the reservation shrinks, or a pull moves the counter on) or
    //     finds nothing left and leaves;
    //   * so the trips are bounded by the pulls, plus the steps of the rays the wave took.
    for (;;) {
        const bool run = have && q_running(q.phase);
        const unsigned long long mrun = __ballot(run);
        // The service step, once `service` lanes wait (finished or empty) or none runs: the finished
        // lanes retire and the empty ones take items.  Not on every trip: a retiring lane recomputes
        // its hit and a taking one tests the planes, each behind dependent loads that the whole
        // wave waits for -- a few lanes at a time, that cost as much as the trip's q_step.
        if (64u - (uint32_t)__popcll(mrun) >= P.service || mrun == 0ull) {
            const bool fin = have && !run;
            retire(P, job, fin, idx, q, st);
            if (fin) have = false;
            if (T.dry()) T.pull(P);
            if (T.rleft != 0u) {
                const unsigned long long m = __ballot(!have);
                const uint32_t k = lanes_below(m);
                if (!have && T.holds(k)) {
                    idx = (size_t)T.item(k);
                    take_ray(P, job, idx, q, st);
                    have = true;
                }
                T.advance(m);
            }
            if (T.spent() && __ballot(have) == 0ull) break;
        }
        if (have && q_running(q.phase)) q_step(P.S, q, st.C, stk);
    }
    st.flush(P.counters);
}

// The exact list's items (k_wexact's shape: 64-lane workgroups, grid-stride, the DFS stack in LDS:
// 64 x (dfs_words + 1) words); launched after every run of rays_engine, its count read from device memory
template <class PARAMS, class JOB>
__device__ __forceinline__ void rays_exact_engine(const PARAMS& P, const JOB& job) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t n = *P.exact_n;
    LdsMemN<64u> stk{lds_stack + threadIdx.x, P.dfs_words, P.dfs_words};
    QStats st;
    for (uint32_t k = blockIdx.x * 64u + threadIdx.x; k < n; k += gridDim.x * 64u) {
        const size_t i = P.exact[k];
        const Ray ray = job.ray(i);
        Hit h;
        const int id = q_exact(P.S, ray, stk, h, st.C);
        job.store(i, id, h);
    }
    st.C.planes = 0u;   // (the refill loop counted these rays' plane tests when it took them)
    st.flush(P.counters);
}

// The engine's two kernels on `s`, after the control block's memset: `engine` (rays_engine) on
// `grid` workgroups of `block` threads, then `exact` (rays_exact_engine); e0 / e1 around the two
template <class KERNEL, class PARAMS>
hipError_t launch_rays_pair(KERNEL engine, KERNEL exact, const PARAMS& p, uint32_t grid, uint32_t block, hipStream_t s,
                            hipEvent_t e0, hipEvent_t e1) {
    hipError_t e = hipMemsetAsync(p.head, 0, PT_RAYS_CTL_BYTES, s);
    if (e != hipSuccess) return e;
    if (e0 && (e = hipEventRecord(e0, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(engine, dim3(grid), dim3(block), (block / 64u) * 64u * 4u * (p.aux_words + 1u), s, p);
    hipLaunchKernelGGL(exact, dim3(256), dim3(64), 64u * 4u * (p.dfs_words + 1u), s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return e1 ? hipEventRecord(e1, s) : hipSuccess;
}

}  // namespace pt
#endif  // __HIPCC__
