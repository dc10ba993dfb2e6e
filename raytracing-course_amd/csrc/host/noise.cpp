// noise.cpp -- a session's own noise estimate and the adaptive step it plans from it (pt_session_mark /
// noise / plan / refine and the host-pointer forms), and the hook that runs a plan without a device
// (DESIGN.md §4.10).  The session remembers every pixel's sum at an earlier count, its mark, in a
// per-slot table of its own; pt_noise.h turns the movement since into a noise figure and the figures
// into counts.  A step validates before it writes: k_noise_plan only reads the session, the host reads
// its result, and k_noise_commit, k_counts_bias and the pass run after an acceptance alone.
#include <string.h>

#include "api_internal.h"
#include "../device/pt_noise.h"

namespace pti {
namespace {

constexpr size_t kResBytes = 256;   // the result block (NR_WORDS u64), the mark table behind it, then the count words
static_assert(pt::NR_WORDS * 8u <= kResBytes, "the plan's result block outgrew its section");

uint4* mark_table(const pt_session* ss) { return reinterpret_cast<uint4*>(ss->noise_block + kResBytes); }
// a word per slot: a step's counts, and what a host-pointer form brings back
uint32_t* count_words(const pt_session* ss) {
    return reinterpret_cast<uint32_t*>(ss->noise_block + kResBytes + (size_t)ss->n_slots * 16);
}

// the block, made (the marks all zero: no pixel has one) at the first noise call of a session that has
// pixels -- a session that makes none has the arena, the set-up and the launches it always had
int ensure_noise(pt_session* ss) {
    if (ss->noise_block) return PT_OK;
    void* p = nullptr;
    const size_t bytes = kResBytes + (size_t)ss->n_slots * 20;
    if (hipMalloc(&p, bytes) != hipSuccess) return fail(PT_E_OOM, "device allocation failed (mark table)");
    if (hipMemsetAsync(p, 0, bytes, ss->stream) != hipSuccess) {
        (void)hipFree(p);
        return fail(PT_E_HIP, "memset failed (mark table)");
    }
    ss->noise_block = static_cast<unsigned char*>(p);
    return PT_OK;
}

pt::NoiseParams params(const pt_session* ss) {
    pt::NoiseParams p;
    memset(&p, 0, sizeof(p));
    p.tm = ss->tm;
    p.st = ss->st;
    p.n_tiles_local = ss->n_tiles_local;
    p.tile_rec = ss->state_tile_rec;
    p.lag = lag_table(ss);
    p.mark = mark_table(ss);
    p.res = reinterpret_cast<unsigned long long*>(ss->noise_block);
    p.S = (uint32_t)ss->samples_done;
    return p;
}

pt::NoiseOpts kernel_opts(const pt_refine_opts* o) {
    return pt::NoiseOpts{o->threshold, o->step, pt::noise_cap(o->max_samples), o->spread};
}

int check_opts(const pt_refine_opts* o, const pt_refine_result* r) {
    if (!o || !r) return fail(PT_E_INVALID, "null options or result");
    if (!pt::noise_opts_ok(o->threshold, o->step, o->spread))
        return fail(PT_E_INVALID, "refine options: the threshold must be a number >= 0, the step above 0, spread 0 or 1");
    return PT_OK;
}

// what every call does before its own work: the refusals that need no device, the trace() calls not yet
// run, and -- for a session that has pixels -- its device made current and the tables the kernels read
int enter(pt_session* ss, uint64_t cap, bool cap_matters) {
    if (!ss) return fail(PT_E_INVALID, "null session");
    if (const int rc = refuse_megakernel(ss)) return rc;
    const uint64_t n = owned_pixels(ss);
    if (cap_matters && cap < n)
        return fail(PT_E_INVALID, "room for " + std::to_string(cap) + " values, the session owns " + std::to_string(n) +
                                      " pixels");
    if (const int rc = flush_trace(ss)) return rc;
    if (n == 0) return PT_OK;
    HIP_TRY(hipSetDevice(ss->dev));
    if (const int rc = ensure_export(ss)) return rc;
    return ensure_noise(ss);
}

// k_noise_plan and its result on the host.  o == null: the noise alone.  Nothing of the session changes.
int run_plan(pt_session* ss, const pt_refine_opts* o, float* dev_noise, uint32_t* dev_counts,
             unsigned long long res[pt::NR_WORDS]) {
    pt::NoiseParams p = params(ss);
    p.noise = dev_noise;
    p.counts = dev_counts;
    if (o) {
        p.o = kernel_opts(o);
        p.classify = 1u;
        HIP_TRY(hipMemsetAsync(p.res, 0, pt::NR_WORDS * 8u, ss->stream));
    }
    HIP_TRY(pt_launch_noise_plan(p, ss->stream));
    if (o) HIP_TRY(hipMemcpyAsync(res, p.res, pt::NR_WORDS * 8u, hipMemcpyDeviceToHost, ss->stream));
    HIP_TRY(hipStreamSynchronize(ss->stream));
    return PT_OK;
}

void fill_result(const pt_session* ss, const unsigned long long res[pt::NR_WORDS], pt_refine_result* r) {
    memset(r, 0, sizeof(*r));
    r->refined = res[pt::NR_REFINED];
    r->samples = res[pt::NR_SAMPLES];
    r->unmarked = res[pt::NR_UNMARKED];
    r->nonfinite = res[pt::NR_NONFINITE];
    r->capped = res[pt::NR_CAPPED];
    r->worst = pt::u2f((uint32_t)res[pt::NR_WORST]);
    (void)pt_session_samples_range(ss, &r->least, &r->most);
}

}  // namespace

hipError_t clear_marks(pt_session* ss) {
    if (!ss->noise_block) return hipSuccess;
    return hipMemsetAsync(mark_table(ss), 0, (size_t)ss->n_slots * 16, ss->stream);
}

}  // namespace pti

using namespace pti;

extern "C" {

int pt_session_mark(pt_session* ss) {
    if (const int rc = enter(ss, 0, false)) return rc;
    if (ss->n_tiles_local == 0) return PT_OK;
    HIP_TRY(pt_launch_noise_mark(params(ss), ss->stream));
    HIP_TRY(hipStreamSynchronize(ss->stream));
    return PT_OK;
}

int pt_session_noise(pt_session* ss, float* dev_noise, uint64_t cap) {
    if (ss && !dev_noise && owned_pixels(ss) > 0) return fail(PT_E_INVALID, "null noise buffer");
    if (const int rc = enter(ss, cap, true)) return rc;
    if (ss->n_tiles_local == 0) return PT_OK;
    return run_plan(ss, nullptr, dev_noise, nullptr, nullptr);
}

int pt_session_noise_host(pt_session* ss, float* noise, uint64_t cap) {
    if (ss && !noise && owned_pixels(ss) > 0) return fail(PT_E_INVALID, "null noise buffer");
    if (const int rc = enter(ss, cap, true)) return rc;
    if (ss->n_tiles_local == 0) return PT_OK;
    float* d = reinterpret_cast<float*>(count_words(ss));
    if (const int rc = run_plan(ss, nullptr, d, nullptr, nullptr)) return rc;
    HIP_TRY(hipMemcpyAsync(noise, d, owned_pixels(ss) * 4, hipMemcpyDeviceToHost, ss->stream));
    HIP_TRY(hipStreamSynchronize(ss->stream));
    return PT_OK;
}

int pt_session_plan(pt_session* ss, const pt_refine_opts* o, uint32_t* dev_counts, uint64_t cap, pt_refine_result* r) {
    if (const int rc = check_opts(o, r)) return rc;
    if (const int rc = enter(ss, cap, dev_counts != nullptr)) return rc;
    unsigned long long res[pt::NR_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ss->n_tiles_local) {
        if (const int rc = run_plan(ss, o, nullptr, dev_counts, res)) return rc;
    }
    fill_result(ss, res, r);
    return PT_OK;
}

int pt_session_plan_host(pt_session* ss, const pt_refine_opts* o, uint32_t* counts, uint64_t cap, pt_refine_result* r) {
    if (const int rc = check_opts(o, r)) return rc;
    if (const int rc = enter(ss, cap, counts != nullptr)) return rc;
    unsigned long long res[pt::NR_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ss->n_tiles_local) {
        uint32_t* d = counts ? count_words(ss) : nullptr;
        if (const int rc = run_plan(ss, o, nullptr, d, res)) return rc;
        if (counts) {
            HIP_TRY(hipMemcpyAsync(counts, d, owned_pixels(ss) * 4, hipMemcpyDeviceToHost, ss->stream));
            HIP_TRY(hipStreamSynchronize(ss->stream));
        }
    }
    fill_result(ss, res, r);
    return PT_OK;
}

int pt_session_refine(pt_session* ss, const pt_refine_opts* o, pt_refine_result* r) {
    if (const int rc = check_opts(o, r)) return rc;
    if (const int rc = enter(ss, 0, false)) return rc;
    unsigned long long res[pt::NR_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ss->n_tiles_local) {
        // the plan, its counts in the session's own words ...
        if (const int rc = run_plan(ss, o, nullptr, count_words(ss), res)) return rc;
    }
    // ... and only then a write.  Nothing of the session has changed so far.
    if (res[pt::NR_REFINED]) {
        if (const int rc = ensure_lag(ss)) return rc;
        pt::NoiseParams p = params(ss);
        p.counts = count_words(ss);
        HIP_TRY(pt_launch_noise_commit(p, ss->stream));   // mark := now where the pixel takes samples
        // (no count passes 2^32 - 1: a pixel's is at most max_samples - its own)
        if (const int rc = counts_pass(ss, p.counts, res[pt::NR_SAMPLES], res[pt::NR_MAX_TOTAL], ~res[pt::NR_NMIN_TOTAL]))
            return rc;
    }
    fill_result(ss, res, r);
    return PT_OK;
}

// test hook: a plan on the host, by the functions k_noise_plan runs and the same in-tile neighbour rule
int pt_selftest_refine_plan(pt_scene* s, const pt_session_opts* so, uint64_t n, const pt_pixel_state* now,
                            const pt_pixel_state* mark, const pt_refine_opts* o, float* noise, uint32_t* counts,
                            pt_refine_result* r) {
    if (!s || !so) return fail(PT_E_INVALID, "null argument");
    if (const int rc = check_opts(o, r)) return rc;
    int rc = pt_scene_prepare(s);
    if (rc) return rc;
    pt_session ss;
    if ((rc = session_geometry_only(s, so, &ss))) return rc;
    const uint64_t owned = owned_pixels(&ss);
    if (n != owned)
        return fail(PT_E_INVALID, std::to_string(n) + " records, the session owns " + std::to_string(owned) + " pixels");
    if (n > 0 && (!now || !mark)) return fail(PT_E_INVALID, "null state buffer");
    pt::TileMap tm = ss.tm;
    tm.gtile = ss.gtiles.data();
    const std::vector<uint32_t> at = tile_records(&ss);
    const pt::NoiseOpts ko = kernel_opts(o);
    memset(r, 0, sizeof(*r));
    uint32_t least = 0xffffffffu, most = 0u;
    for (uint32_t tile = 0; tile < ss.n_tiles_local; ++tile) {
        int64_t rec[256];
        float nz[256];
        bool est[256];
        unsigned long long hot[4] = {0ull, 0ull, 0ull, 0ull};
        for (uint32_t lane = 0; lane < 256u; ++lane) {
            const int64_t i = rec[lane] = pt::count_record(tm, at.data(), tile, lane);
            if (i < 0) continue;
            est[lane] = pt::noise_has_estimate(now[i].samples, mark[i].samples);
            nz[lane] = pt::noise_of(now[i].sum, now[i].samples, mark[i].sum, mark[i].samples);
            if (pt::noise_hot(nz[lane], ko.threshold)) hot[lane >> 6] |= 1ull << (lane & 63u);
        }
        for (uint32_t lane = 0; lane < 256u; ++lane) {
            const int64_t i = rec[lane];
            if (i < 0) continue;
            const bool hot2 = ko.spread ? pt::noise_spread(hot, lane) : ((hot[lane >> 6] >> (lane & 63u)) & 1ull) != 0ull;
            const pt::NoisePixel px = pt::noise_pixel(nz[lane], est[lane], hot2, now[i].samples, ko);
            if (noise) noise[i] = px.noise;
            if (counts) counts[i] = px.count;
            r->refined += px.count ? 1u : 0u;
            r->samples += px.count;
            r->unmarked += px.unmarked ? 1u : 0u;
            r->nonfinite += px.nan ? 1u : 0u;
            r->capped += px.capped ? 1u : 0u;
            r->worst = pt::u2f(std::max(pt::f2u(r->worst), pt::noise_worst_bits(px.noise, est[lane])));
            least = std::min(least, now[i].samples);
            most = std::max(most, now[i].samples);
        }
    }
    r->least = n ? least : 0u;
    r->most = most;
    return PT_OK;
}

}  // extern "C"
