// pt_rays.h -- the ray-query engine's parameter block (pt_rays.hip, host/rayq.cpp): closest-hit
// queries (Scene::RayIntersection, src/scene.cpp:46-77) for rays the caller supplies -- no pixels,
// no chains, no shading.  DESIGN.md §4.5.
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
