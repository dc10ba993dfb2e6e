// states.cpp -- a session's pixels as caller-owned pixel states (pt_session_pixels / export / import
// and their host-pointer forms), and the hook that runs the import's classification without a
// device.  An import validates every record before it writes one: k_states_mark and
// k_states_check only count, the host reads their result, and k_states_write runs after an
// acceptance alone -- a refused import has touched the mark array and nothing of the session.
#include <string.h>

#include "api_internal.h"
#include "../device/pt_states.h"

namespace pti {

// the export's first record of every local tile (edge tiles hold fewer than 256 pixels)
std::vector<uint32_t> tile_records(const pt_session* ss) {
    std::vector<uint32_t> at(ss->n_tiles_local);
    uint32_t px = 0;
    for (uint32_t t = 0; t < ss->n_tiles_local; ++t) {
        const uint32_t gt = ss->gtiles[t], ty = gt / ss->tm.tiles_x;
        at[t] = px;
        px += pt::state_tile_width(ss->tm, gt) * std::min(16u, ss->tm.wh - ty * 16u);
    }
    return at;
}

// the session's state-exchange buffers, made at its first export / import (a session that does
// neither has the arena, the set-up and the launches it always had)
int ensure_export(pt_session* ss) {
    if (ss->state_tile_rec || ss->n_tiles_local == 0) return PT_OK;
    const std::vector<uint32_t> at = tile_records(ss);
    void* p = nullptr;
    if (hipMalloc(&p, at.size() * 4) != hipSuccess) return fail(PT_E_OOM, "device allocation failed (state export table)");
    if (hipMemcpy(p, at.data(), at.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p);
        return fail(PT_E_HIP, "state export table upload failed");
    }
    ss->state_tile_rec = static_cast<uint32_t*>(p);
    return PT_OK;
}

namespace {
constexpr size_t kResBytes = 256;   // the result block (SR_WORDS u64), the mark array behind it
static_assert(pt::SR_WORDS * 8u <= kResBytes, "the import's result block outgrew its section");
int ensure_import(pt_session* ss) {
    if (ss->state_marks || ss->n_tiles_local == 0) return PT_OK;
    void* p = nullptr;
    if (hipMalloc(&p, kResBytes + (size_t)ss->n_slots * 4) != hipSuccess)
        return fail(PT_E_OOM, "device allocation failed (state import marks)");
    ss->state_marks = static_cast<unsigned char*>(p);
    return PT_OK;
}

pt::StatesParams params(const pt_session* ss, pt_pixel_state* state, uint64_t n) {
    pt::StatesParams p;
    memset(&p, 0, sizeof(p));
    p.tm = ss->tm;
    p.st = ss->st;
    p.n_tiles_local = ss->n_tiles_local;
    p.tile_rec = ss->state_tile_rec;
    p.state = reinterpret_cast<pt::PixelRec*>(state);
    p.n = n;
    p.lag = lag_table(ss);
    if (ss->state_marks) {
        p.res = reinterpret_cast<unsigned long long*>(ss->state_marks);
        p.mark = reinterpret_cast<uint32_t*>(ss->state_marks + kResBytes);
    }
    return p;
}

}  // namespace

int check_state_pointer(const void* p) {
    if (!p) return fail(PT_E_INVALID, "null state buffer");
    // (the kernels move a record as 16-B pieces)
    if (reinterpret_cast<uintptr_t>(p) & 15u) return fail(PT_E_INVALID, "the state buffer must be 16-byte aligned");
    return PT_OK;
}

int DevRecords::alloc(uint64_t n) {
    if (hipMalloc(&p, std::max<uint64_t>(n, 1) * sizeof(pt_pixel_state)) != hipSuccess)
        return fail(PT_E_OOM, "device allocation failed (state records)");
    return PT_OK;
}

// An import's validation (the session has pixels, n > 0, its device current): every record classified
// and counted, every owned slot's marks checked, the result on the host.  Nothing of the session has
// changed when it returns, whatever it returns.
int validate_import(pt_session* ss, uint64_t n, const pt_pixel_state* dev_state, unsigned long long* res) {
    if (const int rc = ensure_import(ss)) return rc;
    const pt::StatesParams p = params(ss, const_cast<pt_pixel_state*>(dev_state), n);
    HIP_TRY(hipMemsetAsync(ss->state_marks, 0, kResBytes + (size_t)ss->n_slots * 4, ss->stream));
    HIP_TRY(pt_launch_states_mark(p, ss->stream));
    HIP_TRY(pt_launch_states_check(p, ss->stream));
    HIP_TRY(hipMemcpyAsync(res, p.res, pt::SR_WORDS * 8u, hipMemcpyDeviceToHost, ss->stream));
    HIP_TRY(hipStreamSynchronize(ss->stream));
    if (res[pt::SR_OUTSIDE])
        return fail(PT_E_INVALID, std::to_string(res[pt::SR_OUTSIDE]) + " record(s) name a pixel outside the image");
    if (res[pt::SR_BAD_RNG])
        return fail(PT_E_INVALID, std::to_string(res[pt::SR_BAD_RNG]) + " record(s) of the session's pixels have an rng " +
                                      "word outside 1 .. 2^31-2");
    if (res[pt::SR_MISMARKED])
        return fail(PT_E_INVALID, std::to_string(res[pt::SR_MISMARKED]) + " of the session's pixels are named by no " +
                                      "record or by more than one");
    return PT_OK;
}

}  // namespace pti

using namespace pti;

extern "C" {

int pt_session_pixels(const pt_session* ss, uint64_t* n) {
    if (!ss || !n) return fail(PT_E_INVALID, "null argument");
    *n = owned_pixels(ss);
    return PT_OK;
}

int pt_session_export(pt_session* ss, pt_pixel_state* dev_state, uint64_t cap) {
    if (!ss) return fail(PT_E_INVALID, "null session");
    const uint64_t n = owned_pixels(ss);
    if (cap < n) return fail(PT_E_INVALID, "room for " + std::to_string(cap) + " records, the session owns " +
                                               std::to_string(n) + " pixels");
    if (n == 0) return PT_OK;
    if (const int rc = check_state_pointer(dev_state)) return rc;
    if (const int rc = flush_trace(ss)) return rc;
    HIP_TRY(hipSetDevice(ss->dev));
    if (const int rc = ensure_export(ss)) return rc;
    HIP_TRY(pt_launch_states_export(params(ss, dev_state, n), ss->stream));
    HIP_TRY(hipStreamSynchronize(ss->stream));
    return PT_OK;
}

int pt_session_import(pt_session* ss, uint64_t n, const pt_pixel_state* dev_state, uint64_t* taken) {
    if (!ss) return fail(PT_E_INVALID, "null session");
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
    // validate, and only then a write
    unsigned long long res[pt::SR_WORDS];
    if (const int rc = validate_import(ss, n, dev_state, res)) return rc;
    const pt::StatesParams p = params(ss, const_cast<pt_pixel_state*>(dev_state), n);
    const uint32_t smax = (uint32_t)res[pt::SR_MAX], smin = ~(uint32_t)res[pt::SR_NMIN];
    if (smin != smax)
        return fail(PT_E_INVALID, "the records' sample counts differ (" + std::to_string(smin) + " .. " +
                                      std::to_string(smax) + "): a session's pixels share one count " +
                                      "(pt_session_import_ragged takes them)");
    HIP_TRY(pt_launch_states_write(p, ss->stream));
    HIP_TRY(clear_lag(ss));   // (a ragged session: uniform again)
    HIP_TRY(clear_marks(ss));   // (new states: no noise estimate yet)
    HIP_TRY(hipStreamSynchronize(ss->stream));
    ss->samples_done = smax;
    if (taken) *taken = res[pt::SR_TAKEN];
    return PT_OK;
}

int pt_session_export_host(pt_session* ss, pt_pixel_state* state, uint64_t cap) {
    if (!ss) return fail(PT_E_INVALID, "null session");
    const uint64_t n = owned_pixels(ss);
    if (cap < n) return fail(PT_E_INVALID, "room for " + std::to_string(cap) + " records, the session owns " +
                                               std::to_string(n) + " pixels");
    if (n == 0) return PT_OK;
    if (!state) return fail(PT_E_INVALID, "null state buffer");
    HIP_TRY(hipSetDevice(ss->dev));
    DevRecords d;
    if (const int rc = d.alloc(n)) return rc;
    if (const int rc = pt_session_export(ss, static_cast<pt_pixel_state*>(d.p), n)) return rc;
    HIP_TRY(hipMemcpy(state, d.p, n * sizeof(pt_pixel_state), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_session_import_host(pt_session* ss, uint64_t n, const pt_pixel_state* state, uint64_t* taken) {
    if (!ss) return fail(PT_E_INVALID, "null session");
    if (n > 0 && !state) return fail(PT_E_INVALID, "null state buffer");
    // (a session without pixels takes none, an empty list is refused: neither needs a copy)
    if (n == 0 || ss->n_tiles_local == 0) return pt_session_import(ss, 0, nullptr, taken);
    HIP_TRY(hipSetDevice(ss->dev));
    DevRecords d;
    if (const int rc = d.alloc(n)) return rc;
    HIP_TRY(hipMemcpy(d.p, state, n * sizeof(pt_pixel_state), hipMemcpyHostToDevice));
    return pt_session_import(ss, n, static_cast<const pt_pixel_state*>(d.p), taken);
}

// test hook: the import's classification on the host, by the functions k_states_mark runs
int pt_selftest_state_slots(pt_scene* s, const pt_session_opts* o, uint64_t n, const pt_pixel_state* state,
                            int64_t* slot_out) {
    if (!s || !o) return fail(PT_E_INVALID, "null argument");
    if (n > 0 && (!state || !slot_out)) return fail(PT_E_INVALID, "null state or slot buffer");
    int rc = pt_scene_prepare(s);
    if (rc) return rc;
    pt_session ss;
    if ((rc = session_geometry_only(s, o, &ss))) return rc;
    pt::TileMap tm = ss.tm;
    tm.gtile = ss.gtiles.data();
    for (uint64_t i = 0; i < n; ++i) {
        const int64_t slot = pt::state_slot(tm, ss.n_tiles_local, state[i].x, state[i].y, state[i].rng);
        slot_out[i] = slot >= 0 ? slot : slot == pt::STATE_FOREIGN ? -1 : -2;
    }
    return PT_OK;
}

}  // extern "C"
