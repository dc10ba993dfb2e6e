// pt_paths.h -- the batch radiance engine's parameter block (pt_paths.hip, host/pathq.cpp):
// Scene::RayTrace (src/scene.cpp:83-178) for rays the caller supplies, one radiance record per
// path -- no pixels, no camera, no sums.  DESIGN.md §4.6.
#pragma once
#include "pt_kernels.h"

namespace pt {

// the records of include/pt.h (pt_path_ray 32 B, pt_path_out 16 B)
struct PathRec { float o[3], d[3]; uint32_t seed, reserved; };
struct PathOut { float rgb[3]; uint32_t rays; };

// A run's control block, zeroed by one memset on the run's stream before its launch:
//   u64 head     the work counter: paths [0, head) have been taken by some wave
#define PT_PATHS_CTL_BYTES 16u
// k_paths: waiting lanes (finished query or empty) at which a wave runs its service step
// (PT_TUNE paths_service; 48 is the best measured value: the table in DESIGN.md §4.6)
#define PT_PATHS_SERVICE 48u

struct PathsParams {
    SceneView S;
    const PathRec* in;
    PathOut* out;
    uint32_t n;
    uint32_t depth;               // RAY_DEPTH: a path's closest-hit queries at most, and its fold records
    uint32_t batch;               // paths a wave reserves per pull of the work counter (>= 64)
    uint32_t service;             // waiting lanes at which a wave runs its service step (1..64)
    unsigned long long* head;
    uint4* fold;                  // fold records, `depth` per resident lane slot (HbmVStore's layout):
                                  // fold[(workgroup * threads + thread) * depth + vertex]
    unsigned long long* counters; // PT_CTR_COPIES x PT_CTR_STRIDE statistics counters (CTR_RAYS .. CTR_FALLBACKS_RAY)
    uint32_t aux_words;           // aux stack words per lane ...
    uint32_t dfs_words;           // ... and exact DFS stack words per lane: both on the lane's one LDS
                                  // column of max(aux_words, dfs_words) + 1 words (the last: the trash word)
};

}  // namespace pt

// workgroups of `block` threads, each lane with its LDS column (pt_batch.h lane_lds_bytes), that one
// compute unit holds of k_paths
hipError_t pt_paths_occupancy(uint32_t block, uint32_t aux_words, uint32_t dfs_words, int* per_cu);
// k_paths on `s`, after the control block's memset; `block` = threads per workgroup (a multiple of 64
// whose stacks fit the workgroup's LDS), `grid` at most the workgroups the fold area was sized for;
// e0 / e1 around the kernel
hipError_t pt_launch_paths(const pt::PathsParams& p, uint32_t grid, uint32_t block, hipStream_t s, hipEvent_t e0,
                           hipEvent_t e1);
