// pt_pixels.h -- the pixel-sample engine's records and parameter block (pt_pixels.hip,
// host/pixq.cpp): Scene::Sample's loop (src/scene.cpp:189-203) for pixels the caller lists, each
// with its own number of further samples, its state handed in and out.  DESIGN.md §4.7.
#pragma once
#include "pt_kernels.h"

namespace pt {

// the record of include/pt.h (pt_pixel_state, 32 B), moved as two 16-B pieces:
//   piece 0 = {rng, saved, x, y}   piece 1 = {sum.r, sum.g, sum.b, samples}
struct PixelRec { uint32_t rng; float saved; uint32_t x, y; float sum[3]; uint32_t samples; };
#define PT_PIXEL_SAVED_BIT 0x80000000u   // in rng: the normal_distribution holds `saved`

// a record's stream, and the two words a stream goes back as (saved = 0 when none, so that a
// state has one encoding however it was reached)
PT_HD Rng pixel_rng(uint32_t rng, float saved) {
    Rng R;
    R.x = rng & ~PT_PIXEL_SAVED_BIT;
    R.saved = saved;
    R.saved_ok = rng >> 31;
    return R;
}
PT_HD uint32_t pixel_rng_word(const Rng& R) { return R.x | (R.saved_ok ? PT_PIXEL_SAVED_BIT : 0u); }
PT_HD float pixel_rng_saved(const Rng& R) { return R.saved_ok ? R.saved : 0.f; }

// A run's control block, zeroed by one memset on the run's stream before its launch:
//   u64 head     the work counter: records [0, head) have been taken by some wave
#define PT_PIXELS_CTL_BYTES 16u
// k_pixels: waiting lanes (finished query or empty) at which a wave runs its service step
// (PT_TUNE pixels_service; k_paths' value: the table in DESIGN.md §4.7)
#define PT_PIXELS_SERVICE 48u
// the samples counter's slot in the context's statistics counters, after CTR_RAYS .. CTR_FALLBACKS_RAY
// (the context's counters are its own: no session reads them)
#define PT_PIXELS_CTR_SAMPLES 8u

struct PixelsParams {
    SceneView S;
    CamView cam;
    PixelRec* state;              // n records, updated in place
    const uint32_t* counts;       // n further samples per record, or null: `spp` for every record
    uint32_t spp;
    uint32_t n;
    uint32_t depth;               // RAY_DEPTH: a path's closest-hit queries at most, and its fold records
    uint32_t batch;               // records a wave reserves per pull of the work counter (>= 64)
    uint32_t service;             // waiting lanes at which a wave runs its service step (1..64)
    unsigned long long* head;
    uint4* fold;                  // fold records, `depth` per resident lane slot (HbmVStore's layout):
                                  // fold[(workgroup * threads + thread) * depth + vertex]
    unsigned long long* counters; // PT_CTR_COPIES x PT_CTR_STRIDE statistics counters (CTR_RAYS ..
                                  // CTR_FALLBACKS_RAY, PT_PIXELS_CTR_SAMPLES)
    uint32_t aux_words;           // aux stack words per lane ...
    uint32_t dfs_words;           // ... and exact DFS stack words per lane: both on the lane's one LDS
                                  // column of max(aux_words, dfs_words) + 1 words (the last: the trash word)
};

}  // namespace pt

// workgroups of `block` threads, each lane with its LDS column (pt_batch.h lane_lds_bytes), that one
// compute unit holds of k_pixels
hipError_t pt_pixels_occupancy(uint32_t block, uint32_t aux_words, uint32_t dfs_words, int* per_cu);
// k_pixels on `s`, after the control block's memset; `block` = threads per workgroup (a multiple of 64
// whose stacks fit the workgroup's LDS), `grid` at most the workgroups the fold area was sized for;
// e0 / e1 around the kernel
hipError_t pt_launch_pixels(const pt::PixelsParams& p, uint32_t grid, uint32_t block, hipStream_t s, hipEvent_t e0,
                            hipEvent_t e1);
