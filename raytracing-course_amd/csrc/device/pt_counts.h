// pt_counts.h -- per-pixel sample counts in a session (pt_counts.hip, host/counts.cpp): the record
// of an export that a slot's pixel is, and the arithmetic of the lag table.  Host and device compile
// the same functions (pt_selftest_count_records runs them without a device).  DESIGN.md §4.9.
//
// The engines compare a pixel's `done` field with the pass's one target.  A ragged session keeps
// every owned pixel's `done` at one virtual count S (pt_session::samples_done) and the pixel's
// distance below it in lag[slot]: the pixel has taken S - lag[slot] samples.  S is the largest
// count of any owned pixel, so the smallest lag is 0 and S overflows only when a pixel's count does.
#pragma once
#include "pt_states.h"

namespace pt {

// The record of a session's export (pt_states.hip k_states_export's order: the tiles ascending, a
// tile's pixels row-major, the pixels an edge tile lacks left out) that holds slot `lane` of local
// tile `tile`, or -1 for a padding lane.  tile_rec: the first record of every local tile.
PT_HD int64_t count_record(const TileMap& tm, const uint32_t* tile_rec, uint32_t tile, uint32_t lane) {
    const uint32_t gt = tm.gtile[tile];
    const uint32_t wx = (gt % tm.tiles_x) * 16u + (lane & 15u), wy = (gt / tm.tiles_x) * 16u + (lane >> 4);
    if (gt >= tm.n_tiles || wx >= tm.ww || wy >= tm.wh) return -1;
    return (int64_t)tile_rec[tile] + (int64_t)((lane >> 4) * state_tile_width(tm, gt) + (lane & 15u));
}

// a pixel's count so far, and after `count` more samples (64 bits: past 2^32 - 1 the call is refused)
PT_HD uint32_t count_taken(uint32_t S, uint32_t lag) { return S - lag; }
PT_HD unsigned long long count_total(uint32_t S, uint32_t lag, uint32_t count) {
    return (unsigned long long)count_taken(S, lag) + count;
}
// Before a pass to the target S2 (the largest count_total of the session's pixels) in which the pixel
// takes `count` samples: its `done` field -- the engines run it from there to S2 --, and its lag after
// the pass, when every `done` stands at S2.
PT_HD uint32_t count_done_before(uint32_t S2, uint32_t count) { return S2 - count; }
PT_HD uint32_t count_lag_after(uint32_t S2, uint32_t S, uint32_t lag, uint32_t count) {
    return S2 - (uint32_t)count_total(S, lag, count);
}

// a trace_counts call's result block (u64 words, zeroed before k_counts_scan)
enum : uint32_t {
    CR_MAX_TOTAL = 0u,   // the largest count_total: the pass's target, or past 2^32 - 1 a refusal
    CR_NMIN_TOTAL = 1u,  // the complement of the smallest count_total
    CR_SUM = 2u,         // the counts' sum (0: nothing to do)
    CR_WORDS = 4u
};

struct CountsParams {
    TileMap tm;
    PixelState st;
    uint32_t n_tiles_local;
    const uint32_t* tile_rec;     // per local tile: the export's first record of that tile
    const uint32_t* counts;       // trace_counts: per record, in export order
    uint32_t* lag;                // per slot (padding lanes: 0)
    unsigned long long* res;      // trace_counts: CR_* words; import: the SR_* words of pt_states.h
    uint32_t S, S2;               // the session's virtual count before and after the call
    const PixelRec* state;        // import: the caller's records
    unsigned long long n;
    // resolve
    const float* thr;             // 256 gamma thresholds
    uint8_t* out;                 // 3 * n_slots
    float* rad;                   // optional 3 * n_slots
    unsigned long long* counters; // statistics counters (CTR_SHORT)
};

}  // namespace pt

hipError_t pt_launch_counts_scan(const pt::CountsParams& p, hipStream_t s);
hipError_t pt_launch_counts_bias(const pt::CountsParams& p, hipStream_t s);
hipError_t pt_launch_counts_import(const pt::CountsParams& p, hipStream_t s);
hipError_t pt_launch_counts_resolve(const pt::CountsParams& p, hipStream_t s);
