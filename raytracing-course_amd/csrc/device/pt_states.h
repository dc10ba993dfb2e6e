// pt_states.h -- a session's pixels as caller-owned pixel states (pt_states.hip, host/states.cpp):
// the slot a record lands in and the record a slot leaves as.  Host and device compile the same
// functions (pt_selftest_state_slots runs them without a device).  DESIGN.md §4.8.
#pragma once
#include "pt_kernels.h"
#include "pt_pixels.h"

namespace pt {

// what a record is to a session (a slot index otherwise)
enum : int64_t { STATE_FOREIGN = -1, STATE_OUTSIDE = -2, STATE_BAD_RNG = -3 };

// minstd_rand's states: 1 .. 2^31 - 2 (bit 31 is the record's saved-value flag)
PT_HD bool state_rng_ok(uint32_t rng) {
    const uint32_t x = rng & ~PT_PIXEL_SAVED_BIT;
    return x >= 1u && x <= 0x7ffffffeu;
}

// window tile gt's place in a rank's ascending tile list (gt is one of its n_local entries)
PT_HD uint32_t state_local_tile(const uint32_t* gtile, uint32_t n_local, uint32_t gt) {
    uint32_t lo = 0u, hi = n_local;
    while (lo + 1u < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (gtile[mid] <= gt) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The slot of the session (tm, its n_local tiles) that the record of pixel (x, y) with stream word
// `rng` belongs in, or: STATE_OUTSIDE, not a pixel of the image; STATE_FOREIGN, a pixel of the
// image that is not this session's (outside its window, or another rank's tile); STATE_BAD_RNG,
// this session's pixel with a stream word no minstd_rand has.
PT_HD int64_t state_slot(const TileMap& tm, uint32_t n_local, uint32_t x, uint32_t y, uint32_t rng) {
    if (x >= tm.W || y >= tm.H) return STATE_OUTSIDE;
    if (x < tm.x0 || y < tm.y0 || x - tm.x0 >= tm.ww || y - tm.y0 >= tm.wh) return STATE_FOREIGN;
    const uint32_t wx = x - tm.x0, wy = y - tm.y0;
    const uint32_t gt = (wy >> 4) * tm.tiles_x + (wx >> 4);
    if (n_local == 0u || tile_owner(gt, tm.tiles_x, tm.world) != tm.rank) return STATE_FOREIGN;
    if (!state_rng_ok(rng)) return STATE_BAD_RNG;
    const uint32_t lt = state_local_tile(tm.gtile, n_local, gt);
    return (int64_t)lt * 256 + (int64_t)((wy & 15u) * 16u + (wx & 15u));
}

// pixels per row of window tile gt (the right edge's tiles are narrower)
PT_HD uint32_t state_tile_width(const TileMap& tm, uint32_t gt) {
    const uint32_t x = (gt % tm.tiles_x) * 16u;
    return tm.ww - x < 16u ? tm.ww - x : 16u;
}

// A slot's record pair (pt_kernels.h PixelState) from a record's two pieces and back.  One
// encoding: the flag in bit 31 of rng, saved = +0 when nothing is saved.
PT_HD void state_to_slot(uint4 a, uint4 b, uint32_t W, uint4& hot, uint4& sum) {
    const uint32_t flag = a.x >> 31;
    hot = make_uint4(a.x & ~PT_PIXEL_SAVED_BIT, flag ? a.y : 0u, flag, b.w);   // (no vertices: a sample boundary)
    sum = make_uint4(b.x, b.y, b.z, a.w * W + a.z);
}
PT_HD void slot_to_state(uint4 hot, uint4 sum, uint32_t x, uint32_t y, uint4& a, uint4& b) {
    const uint32_t flag = hot.z & 1u;
    a = make_uint4(hot.x | (flag ? PT_PIXEL_SAVED_BIT : 0u), flag ? hot.y : 0u, x, y);
    b = make_uint4(sum.x, sum.y, sum.z, hot.w);
}

// an import's result block (u64 words, zeroed with the mark array before k_states_mark)
enum : uint32_t {
    SR_TAKEN = 0u,      // records that are this session's pixels, with a good stream word
    SR_OUTSIDE = 1u,    // records outside the image
    SR_BAD_RNG = 2u,    // this session's pixels with a bad stream word
    SR_MAX = 3u,        // the taken records' largest `samples` ...
    SR_NMIN = 4u,       // ... and the complement of their smallest (so that zero is "none yet")
    SR_MISMARKED = 5u,  // owned slots named by no taken record or by more than one
    SR_LAG_SUM = 6u,    // a ragged import's write (pt_counts.hip): the taken records' distances below SR_MAX, summed
    SR_WORDS = 8u
};

struct StatesParams {
    TileMap tm;
    PixelState st;
    uint32_t n_tiles_local;
    const uint32_t* tile_rec;     // per local tile: the export's first record of that tile
    PixelRec* state;              // the caller's records (export: written; import: read)
    unsigned long long n;         // import: records
    uint32_t* mark;               // import: per slot, the taken records that name it
    unsigned long long* res;      // import: SR_* words
    const uint32_t* lag;          // export: per slot, what its pixel's count lies below `done` (pt_counts.h; null: nothing)
};

}  // namespace pt

hipError_t pt_launch_states_export(const pt::StatesParams& p, hipStream_t s);
hipError_t pt_launch_states_mark(const pt::StatesParams& p, hipStream_t s);
hipError_t pt_launch_states_check(const pt::StatesParams& p, hipStream_t s);
hipError_t pt_launch_states_write(const pt::StatesParams& p, hipStream_t s);
