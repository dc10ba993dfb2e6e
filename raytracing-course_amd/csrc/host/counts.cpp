// counts.cpp -- per-pixel sample counts in a session (pt_session_trace_counts, pt_session_import_ragged
// and their host-pointer forms, pt_session_samples_range), and the hooks that run their arithmetic
// without a device.  The engines compare a pixel's `done` with a pass's one target;
// a ragged session keeps every owned pixel's `done` at one virtual count, ss->samples_done, and the
// pixel's distance below it in a per-slot lag table.  A call validates before it writes: k_counts_scan
// only reduces, the host reads its result, and k_counts_bias and the pass run after an acceptance alone.
#include <string.h>

#include "api_internal.h"
#include "../device/pt_counts.h"

namespace pti {
namespace {

constexpr size_t kResBytes = 256;   // the result block (CR_WORDS u64), the lag table behind it
static_assert(pt::CR_WORDS * 8u <= kResBytes, "the counts' result block outgrew its section");

}  // namespace

// the lag table, made (all zero: a uniform session) at the first ragged call -- a session that makes
// none has the arena, the set-up and the launches it always had
int ensure_lag(pt_session* ss) {
    if (ss->counts_block) return PT_OK;
    void* p = nullptr;
    const size_t bytes = kResBytes + (size_t)ss->n_slots * 4;
    if (hipMalloc(&p, bytes) != hipSuccess) return fail(PT_E_OOM, "device allocation failed (lag table)");
    if (hipMemsetAsync(p, 0, bytes, ss->stream) != hipSuccess) {
        (void)hipFree(p);
        return fail(PT_E_HIP, "memset failed (lag table)");
    }
    ss->counts_block = static_cast<unsigned char*>(p);
    return PT_OK;
}

int refuse_megakernel(const pt_session* ss) {
    if (ss->wave) return PT_OK;
    return fail(PT_E_INVALID, "per-pixel sample counts need the wavefront engines: this session runs the megakernel "
                              "(traversal EXACT or REPLAY_DIV, or PT_TUNE engine=mega), and k_trace advances by a uniform spp");
}

namespace {

pt::CountsParams params(const pt_session* ss) {
    pt::CountsParams p;
    memset(&p, 0, sizeof(p));
    p.tm = ss->tm;
    p.st = ss->st;
    p.n_tiles_local = ss->n_tiles_local;
    p.tile_rec = ss->state_tile_rec;
    p.lag = lag_table(ss);
    p.res = reinterpret_cast<unsigned long long*>(ss->counts_block);
    p.S = p.S2 = (uint32_t)ss->samples_done;
    return p;
}

// what both forms of trace_counts refuse before they touch the device
int check_counts(const pt_session* ss, uint64_t n, const uint32_t* counts) {
    if (!ss) return fail(PT_E_INVALID, "null session");
    if (const int rc = refuse_megakernel(ss)) return rc;
    const uint64_t owned = owned_pixels(ss);
    if (n != owned)
        return fail(PT_E_INVALID, std::to_string(n) + " counts, the session owns " + std::to_string(owned) + " pixels");
    if (n > 0 && !counts) return fail(PT_E_INVALID, "null counts");
    return PT_OK;
}

}  // namespace

uint32_t* lag_table(const pt_session* ss) {
    return ss->counts_block ? reinterpret_cast<uint32_t*>(ss->counts_block + kResBytes) : nullptr;
}

hipError_t clear_lag(pt_session* ss) {
    ss->lag_sum = 0;
    ss->lag_max = 0;
    if (!ss->counts_block) return hipSuccess;
    return hipMemsetAsync(lag_table(ss), 0, (size_t)ss->n_slots * 4, ss->stream);
}

// An accepted set of counts (their sum above 0; total_max / total_min: the largest and the smallest
// count a pixel stands at after them): every pixel's `done` at S2 - its count, the engines run them all
// to S2 = total_max.  The lag table and the export table exist.
int counts_pass(pt_session* ss, const uint32_t* dev_counts, unsigned long long sum, unsigned long long total_max,
                unsigned long long total_min) {
    if (total_max > 0xffffffffull)
        return fail(PT_E_INVALID, "a pixel would stand at " + std::to_string(total_max) + " samples: past 2^32 - 1");
    pt::CountsParams p = params(ss);
    p.counts = dev_counts;
    p.S2 = (uint32_t)total_max;
    HIP_TRY(pt_launch_counts_bias(p, ss->stream));
    const uint64_t owned = owned_pixels(ss), taken = owned * p.S - ss->lag_sum;   // (the pixels' samples so far)
    if (const int rc = trace_wave(ss, p.S2 - p.S)) return rc;
    ss->lag_sum = owned * p.S2 - (taken + sum);
    ss->lag_max = p.S2 - (uint32_t)total_min;
    return PT_OK;
}

hipError_t launch_ragged_resolve(pt_session* ss, uint8_t* out, float* rad) {
    pt::CountsParams p = params(ss);
    p.thr = ss->ds->thr;
    p.out = out;
    p.rad = rad;
    p.counters = ss->counters;
    return pt_launch_counts_resolve(p, ss->stream);
}

}  // namespace pti

using namespace pti;

extern "C" {

int pt_session_trace_counts(pt_session* ss, uint64_t n, const uint32_t* dev_counts) {
    if (const int rc = check_counts(ss, n, dev_counts)) return rc;
    if (const int rc = flush_trace(ss)) return rc;
    if (n == 0) return PT_OK;   // (a session without pixels)
    HIP_TRY(hipSetDevice(ss->dev));
    if (const int rc = ensure_export(ss)) return rc;
    if (const int rc = ensure_lag(ss)) return rc;
    pt::CountsParams p = params(ss);
    p.counts = dev_counts;
    // the counts' reductions ...
    HIP_TRY(hipMemsetAsync(p.res, 0, pt::CR_WORDS * 8u, ss->stream));
    HIP_TRY(pt_launch_counts_scan(p, ss->stream));
    unsigned long long res[pt::CR_WORDS];
    HIP_TRY(hipMemcpyAsync(res, p.res, sizeof(res), hipMemcpyDeviceToHost, ss->stream));
    HIP_TRY(hipStreamSynchronize(ss->stream));
    // ... and only then a write.  Nothing of the session has changed so far.
    if (res[pt::CR_SUM] == 0ull) return PT_OK;
    return counts_pass(ss, dev_counts, res[pt::CR_SUM], res[pt::CR_MAX_TOTAL], ~res[pt::CR_NMIN_TOTAL]);
}

int pt_session_trace_counts_host(pt_session* ss, uint64_t n, const uint32_t* counts) {
    if (const int rc = check_counts(ss, n, counts)) return rc;
    if (n == 0) return pt_session_trace_counts(ss, 0, nullptr);
    HIP_TRY(hipSetDevice(ss->dev));
    if (!ss->counts_host_copy) {
        void* p = nullptr;
        if (hipMalloc(&p, n * 4) != hipSuccess) return fail(PT_E_OOM, "device allocation failed (counts)");
        ss->counts_host_copy = static_cast<uint32_t*>(p);
    }
    // (on the session's stream: behind the kernels of an earlier call that read the copy)
    HIP_TRY(hipMemcpyAsync(ss->counts_host_copy, counts, n * 4, hipMemcpyHostToDevice, ss->stream));
    HIP_TRY(hipStreamSynchronize(ss->stream));
    return pt_session_trace_counts(ss, n, ss->counts_host_copy);
}

int pt_session_import_ragged(pt_session* ss, uint64_t n, const pt_pixel_state* dev_state, uint64_t* taken) {
    if (!ss) return fail(PT_E_INVALID, "null session");
    if (const int rc = refuse_megakernel(ss)) return rc;
    if (n > 0) {
        if (const int rc = check_state_pointer(dev_state)) return rc;
    }
    if (const int rc = flush_trace(ss)) return rc;
    if (ss->n_tiles_local == 0) {   // no pixel to replace: every record is someone else's
        if (taken) *taken = 0;
        return PT_OK;
    }
    if (n == 0) return fail(PT_E_INVALID, "no record for the session's " + std::to_string(owned_pixels(ss)) + " pixels");
    HIP_TRY(hipSetDevice(ss->dev));
    unsigned long long res[pt::SR_WORDS];
    if (const int rc = validate_import(ss, n, dev_state, res)) return rc;
    if (const int rc = ensure_lag(ss)) return rc;
    // the write: `done` at the records' largest count, each record's distance below it in the lag table
    const uint32_t smax = (uint32_t)res[pt::SR_MAX], smin = ~(uint32_t)res[pt::SR_NMIN];
    pt::CountsParams p = params(ss);
    p.state = reinterpret_cast<const pt::PixelRec*>(dev_state);
    p.n = n;
    p.S2 = smax;
    p.res = reinterpret_cast<unsigned long long*>(ss->state_marks);   // (the import's SR_* block, zeroed by the validation)
    HIP_TRY(pt_launch_counts_import(p, ss->stream));
    HIP_TRY(clear_marks(ss));   // (new states: no noise estimate yet)
    unsigned long long lag_sum = 0;
    HIP_TRY(hipMemcpyAsync(&lag_sum, p.res + pt::SR_LAG_SUM, 8, hipMemcpyDeviceToHost, ss->stream));
    HIP_TRY(hipStreamSynchronize(ss->stream));
    ss->samples_done = smax;
    ss->lag_sum = lag_sum;
    ss->lag_max = smax - smin;
    if (taken) *taken = res[pt::SR_TAKEN];
    return PT_OK;
}

int pt_session_import_ragged_host(pt_session* ss, uint64_t n, const pt_pixel_state* state, uint64_t* taken) {
    if (!ss) return fail(PT_E_INVALID, "null session");
    if (const int rc = refuse_megakernel(ss)) return rc;
    if (n > 0 && !state) return fail(PT_E_INVALID, "null state buffer");
    // (a session without pixels takes none, an empty list is refused: neither needs a copy)
    if (n == 0 || ss->n_tiles_local == 0) return pt_session_import_ragged(ss, 0, nullptr, taken);
    HIP_TRY(hipSetDevice(ss->dev));
    DevRecords d;
    if (const int rc = d.alloc(n)) return rc;
    HIP_TRY(hipMemcpy(d.p, state, n * sizeof(pt_pixel_state), hipMemcpyHostToDevice));
    return pt_session_import_ragged(ss, n, static_cast<const pt_pixel_state*>(d.p), taken);
}

int pt_session_samples_range(const pt_session* ss, uint32_t* least, uint32_t* most) {
    if (!ss || !least || !most) return fail(PT_E_INVALID, "null argument");
    *most = (uint32_t)(ss->samples_done + ss->deferred_spp);
    *least = *most - ss->lag_max;
    return PT_OK;
}

// test hook: the record of an export that every slot of a session is (-1: a padding lane), by the
// function the count kernels run
int pt_selftest_count_records(pt_scene* s, const pt_session_opts* o, uint64_t cap, int64_t* rec_out, uint64_t* n_slots) {
    if (!s || !o || !n_slots) return fail(PT_E_INVALID, "null argument");
    int rc = pt_scene_prepare(s);
    if (rc) return rc;
    pt_session ss;
    if ((rc = session_geometry_only(s, o, &ss))) return rc;
    *n_slots = ss.n_slots;
    if (ss.n_slots > cap || (ss.n_slots > 0 && !rec_out)) return fail(PT_E_INVALID, "room for fewer records than slots");
    pt::TileMap tm = ss.tm;
    tm.gtile = ss.gtiles.data();
    const std::vector<uint32_t> at = tile_records(&ss);
    for (uint32_t slot = 0; slot < ss.n_slots; ++slot)
        rec_out[slot] = pt::count_record(tm, at.data(), slot / 256u, slot % 256u);
    return PT_OK;
}

// test hook: one trace_counts call's arithmetic for n pixels at the virtual count S -- k_counts_scan's
// target S2 (PT_E_INVALID past 2^32 - 1; untouched outputs), k_counts_bias's `done` and lag
int pt_selftest_count_step(uint32_t S, uint64_t n, const uint32_t* lag, const uint32_t* counts, uint32_t* done,
                           uint32_t* lag_after, uint32_t* S2) {
    if (n > 0 && (!lag || !counts || !done || !lag_after)) return fail(PT_E_INVALID, "null argument");
    if (!S2) return fail(PT_E_INVALID, "null argument");
    unsigned long long top = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (lag[i] > S) return fail(PT_E_INVALID, "a lag above the virtual count");
        top = std::max(top, pt::count_total(S, lag[i], counts[i]));
    }
    if (top > 0xffffffffull) return fail(PT_E_INVALID, "a pixel would pass 2^32 - 1 samples");
    *S2 = (uint32_t)top;
    for (uint64_t i = 0; i < n; ++i) {
        done[i] = pt::count_done_before(*S2, counts[i]);
        lag_after[i] = pt::count_lag_after(*S2, S, lag[i], counts[i]);
    }
    return PT_OK;
}

}  // extern "C"
