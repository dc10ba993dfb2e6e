// rounds.cpp -- the wavefront pass of a session.  trace_wave is the loop of DESIGN.md §4:
// k_wcamera seeds the pass, then every iteration runs either the final cooperative stage
// (coop_final: teams of 4, then whole-wave teams, to the end of the pass) or path rounds
// (path_round: k_wpath -> k_wexact -> k_wshade; a low-chain round beside the early
// cooperative launch on the side stream, side_launch) and the count of what is left
// (count_round).  PT_TUNE is read once per pass (PassTune); each diagnostic is a function.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include "api_internal.h"

// a step that returns a PT_* code (HIP_TRY: one that returns a hipError_t)
#define TRY(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)

namespace pti {
namespace {

// The PT_TUNE keys a pass uses, read once per pass, where one is made (every tune_* call
// parses the environment string again)
struct PassTune {
    const bool has_cap = tune_has("cap"), shade_hold = tune_int("shade_hold", 0) != 0;
    const bool grow_late = tune_int("grow_late", 0) != 0, side_late = tune_int("side_late", 0) != 0;
    const bool side_stop_now = tune_int("side_stop_now", 0) != 0, handon = tune_int("handon", 1) != 0;
    const bool cprof = tune_has("cprof");   // -DPT_CPROF builds: per-phase cycles on stderr
    const bool dupcheck = tune_int("dupcheck", 0) != 0;
    const int cap = tune_int("cap", 0), batch = tune_int("batch", 32), lstack = tune_int("lstack", (int)PT_LSTACK);
    const int roundlog = tune_int("roundlog", 0);
    const std::string drop = tune_str("drop"), wgprof = tune_str("wgprof");
};

// the pass's parameter block from the session
int fill_params(pt_session* ss, uint32_t spp, const PassTune& t, pt::WaveParams& wp) {
    const pt_scene* s = ss->sc;
    memset(&wp, 0, sizeof(wp));
    wp.S = device_view(ss);
    wp.top = ss->ds->top;
    wp.n_top = ss->ds->n_top;
    wp.n_aux = (uint32_t)s->auxsl.size();
    wp.cam = ss->cam;
    wp.tm = ss->tm;
    wp.st = ss->st;
    wp.fq[0] = ss->fq[0];
    wp.fq[1] = ss->fq[1];
    wp.done = ss->done;
    wp.ex = ss->ex;
    wp.endq = ss->endq;
    wp.cq[0] = ss->carry;
    wp.cq[1] = ss->carry + (size_t)ss->plan.carry_cap * ss->plan.carry_words;
    wp.carry_cap = ss->plan.carry_cap;
    wp.carry_words = ss->plan.carry_words;
    wp.ctl = ss->ctl;
    wp.counters = ss->counters;
    wp.depth = ss->depth;
    wp.target = (uint32_t)(ss->samples_done + spp);
    wp.n_tiles_local = ss->n_tiles_local;
    wp.max_stack = std::max<uint32_t>(s->max_stack, 1u);
    wp.aux_stack = std::max<uint32_t>(s->auxw_stack, 1u);
    wp.path = 1u;
    wp.path_budget = ss->plan.path_budget;
    wp.path_ticks = ss->plan.path_ticks;
    // (path_runend and path_cap: per round, from its launch's shape -- path_round)
    wp.tile_order = ss->tile_order;
    wp.sparse_steps = ss->plan.sparse_steps;
    wp.coop_reserve = ss->plan.coop_reserve;
    // round-queue entries a query wave takes per pull: 32 (64 before round 3's low-chain
    // rounds): a workgroup fills closer to its chain cap in finer pulls; rank-of-1 / 2 / 4 / 8,
    // two calls: +0.5 / +0.5 / +3.5 / +3 % (8 and 16 the same at ranks of 1-4; profiles/r03_lowq)
    wp.batch = (uint32_t)std::min(64, std::max(1, t.batch));
    wp.end_min = ss->plan.mix[3];
    // aux stack words per query lane (PT_TUNE lstack=N < PT_LSTACK: tests of the exact-DFS
    // hand-over of queries that outgrow it)
    wp.lstack = std::min<uint32_t>(PT_LSTACK, (uint32_t)std::max(1, t.lstack));
    // test hooks: PT_TUNE shade_hold=1 (path rounds: the shade wave waits for the query waves to
    // leave), drop=<site> (the items of one hand-off site are lost: the resolve must fail)
    wp.side_flags = t.shade_hold ? PT_SHADE_HOLD : 0u;
    wp.drop = 0u;
    if (!t.drop.empty()) {
        const int site = handoff_site(t.drop.c_str());
        if (site < 0) return fail(PT_E_INVALID, "PT_TUNE drop=" + t.drop + ": no such hand-off site");
        wp.drop = 1u + (uint32_t)site;
    }
    if (ss->on_progress && !ss->prog_host) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&ss->prog_host), 8, hipHostMallocMapped | hipHostMallocCoherent));
        *ss->prog_host = 0ull;
        HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&ss->prog_dev), ss->prog_host, 0));
    }
    wp.progress = ss->on_progress ? ss->prog_dev : nullptr;
    return PT_OK;
}

// A launch's timing event pair, registered where it is created (finish_pending reads and
// destroys it: a failed step after this leaks nothing), and the launch counted
int launch_events(pt_session* ss, bool coop, hipEvent_t& e0, hipEvent_t& e1) {
    ss->pending_isect.push_back({nullptr, nullptr, coop});
    HIP_TRY(hipEventCreate(&ss->pending_isect.back().e0));
    HIP_TRY(hipEventCreate(&ss->pending_isect.back().e1));
    e0 = ss->pending_isect.back().e0;
    e1 = ss->pending_isect.back().e1;
    ss->isect_launches++;
    if (coop) ss->coop_launches++;
    return PT_OK;
}

// The one zeroing of a round's output counter set (set 1 - p of ctl; the launchers zero
// nothing).  The rule: a set is zeroed exactly once per round, on the session's stream,
// before anything that may write to it is enqueued -- for a round with a side launch,
// before side_taken is recorded, since the side launch yields into this set from the
// side stream (a second zeroing after that point would lose those yields).  The side
// launch's own sets (side_ctl) are zeroed once in side_launch; pt_launch_wave_start
// zeroes both sets of ctl at the start of a pass.
hipError_t zero_round_out(pt_session* ss, uint32_t p) {
    return hipMemsetAsync(ss->ctl + PT_CTL_SET * (1u - p), 0, 4u * PT_CTL_SET, ss->stream);
}

// The end-of-round count: counter set p (the next round's input) on the host, the
// progress report polled while the stream drains.  Returns with ctl_host valid and
// within the carry queue.
int count_round(pt_session* ss, uint32_t p) {
    HIP_TRY(hipMemcpyAsync(ss->ctl_host, ss->ctl + PT_CTL_SET * p, 8, hipMemcpyDeviceToHost, ss->stream));
    if (ss->on_progress) {
        // report the finished samples while the rounds run
        hipError_t e;
        while ((e = hipStreamQuery(ss->stream)) == hipErrorNotReady) {
            ss->on_progress(__atomic_load_n(ss->prog_host, __ATOMIC_RELAXED));
            std::this_thread::sleep_for(std::chrono::microseconds(500));
        }
        HIP_TRY(e);
    }
    HIP_TRY(hipStreamSynchronize(ss->stream));
    if (ss->ctl_host[pt::C_CARRY] > ss->plan.carry_cap) return fail(PT_E_HIP, "carry queue overflow (a lost chain)");
    return PT_OK;
}

// ---- diagnostics ---------------------------------------------------------------
// the per-workgroup profile buffer of cprof / wgprof, its first `bytes` zeroed
int arm_wg_prof(pt_session* ss, pt::WaveParams& wp, size_t bytes) {
    if (!ss->wg_prof) HIP_TRY(hipMalloc(&ss->wg_prof, 512ull * ss->plan.path_grid));
    HIP_TRY(hipMemsetAsync(ss->wg_prof, 0, bytes, ss->stream));
    wp.wg_prof = ss->wg_prof;
    return PT_OK;
}
// cprof (-DPT_CPROF builds): a cooperative launch's per-phase cycles on stderr
int report_cprof(pt_session* ss, pt::WaveParams& wp, uint32_t team, uint32_t chains, uint32_t grid, hipEvent_t i0,
                 hipEvent_t i1) {
    unsigned long long cp[64];
    HIP_TRY(hipMemcpyAsync(cp, wp.wg_prof, 512, hipMemcpyDeviceToHost, ss->stream));
    HIP_TRY(hipStreamSynchronize(ss->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, i0, i1));
    const double cyc = (double)std::max(1ull, cp[5] + cp[6]) / (64.0 / team);
    fprintf(stderr, "coop T=%u chains %u grid %u: %.2f ms, chain cycles %llu, chains %llu; cycles per chain "
            "cycle: expand %.0f cand %.0f decide %.0f shade %.0f nextray %.0f; wave lifetime %.0f\n",
            team, chains, grid, ms, cp[5], cp[6], cp[0] / cyc, cp[1] / cyc, cp[2] / cyc, cp[3] / cyc,
            cp[4] / cyc, (double)cp[7] / (grid * (double)QC_WAVES));
    // chains ending per 2^20-cycle bucket of their wave's lifetime
    fprintf(stderr, "coop chain ends per 2^20 cycles:");
    for (int i = 16; i < 64; ++i) fprintf(stderr, " %llu", cp[i]);
    fprintf(stderr, "\n");
    wp.wg_prof = nullptr;
    return PT_OK;
}
// wgprof: a path round's counts on stderr, its workgroup timelines (32 u64 each) appended to the file
int report_wgprof(pt_session* ss, const pt::WaveParams& wp, uint32_t p, const char* path) {
    uint32_t cnt[2][8];
    HIP_TRY(hipMemcpyAsync(cnt[0], ss->ctl + PT_CTL_SET * p, 32, hipMemcpyDeviceToHost, ss->stream));
    HIP_TRY(hipMemcpyAsync(cnt[1], ss->ctl + PT_CTL_SET * (1u - p), 32, hipMemcpyDeviceToHost, ss->stream));
    HIP_TRY(hipStreamSynchronize(ss->stream));
    fprintf(stderr, "round %u: in fresh %u carry %u -> out fresh %u carry %u exact %u\n", ss->rounds,
            cnt[0][pt::C_FRESH], cnt[0][pt::C_CARRY], cnt[1][pt::C_FRESH], cnt[1][pt::C_CARRY],
            cnt[1][pt::C_EXACT]);
    std::vector<unsigned long long> h(64ull * ss->plan.path_grid);
    HIP_TRY(hipMemcpyAsync(h.data(), wp.wg_prof, h.size() * 8, hipMemcpyDeviceToHost, ss->stream));
    HIP_TRY(hipStreamSynchronize(ss->stream));
    if (FILE* f = fopen(path, "ab")) {
        fwrite(h.data(), 8, h.size(), f);
        fclose(f);
    }
    return PT_OK;
}
// roundlog >= 2: each round's chains, kind, wall time and rays (roundlog=3: also how
// far behind the pass target the unfinished pixels are); `chains` 0 = the pass's start
int report_round(pt_session* ss, int level, uint32_t target, uint32_t chains, bool side, bool sparse = false) {
    if (!chains) HIP_TRY(hipStreamSynchronize(ss->stream));
    const double now = wall_ms();
    unsigned long long c[PT_CTR_STRIDE];
    HIP_TRY(read_counters(ss, c));
    const unsigned long long rays = c[pt::CTR_RAYS];
    if (chains) {
        const double ms = now - ss->roundlog_t;
        const PathShape sh = path_shape(ss->plan, chains, sparse, side);
        // (dq_full: the session's finished queries so far suspended while their done ring was full)
        fprintf(stderr, "round %u chains %u -> %u+%u (%s%s, nq %u x %u) %.2f ms rays %llu %.0f Mray/s dq_full %llu", ss->rounds,
                chains, ss->ctl_host[pt::C_FRESH], ss->ctl_host[pt::C_CARRY], chains < ss->plan.lowq ? "low" : "full",
                side ? "+side" : "", sh.nq, sh.grid, ms, rays - ss->roundlog_rays, (rays - ss->roundlog_rays) / ms / 1e3,
                c[pt::CTR_DQ_FULL]);
        if (level == 3) {
            std::vector<uint4> rec(2ull * ss->n_slots);
            HIP_TRY(hipMemcpy(rec.data(), ss->st.rec, rec.size() * sizeof(uint4), hipMemcpyDeviceToHost));
            std::vector<uint32_t> lag;
            for (uint32_t i = 0; i < ss->n_slots; ++i)
                if (rec[2 * i].w < target) lag.push_back(target - rec[2 * i].w);
            std::sort(lag.begin(), lag.end());
            const size_t m = lag.size();
            fprintf(stderr, "; unfinished %zu lag p50 %u p90 %u p99 %u max %u", m, m ? lag[m / 2] : 0u,
                    m ? lag[m * 9 / 10] : 0u, m ? lag[m * 99 / 100] : 0u, m ? lag[m - 1] : 0u);
        }
        fprintf(stderr, "\n");
    }
    ss->roundlog_rays = rays;
    ss->roundlog_t = chains ? wall_ms() : now;
    return PT_OK;
}
// dupcheck: every slot at most once in the next round's work (fresh rays + carry, set p)
int check_dups(pt_session* ss, const pt::WaveParams& wp, uint32_t p, uint32_t chains, bool side) {
    const uint32_t nf = ss->ctl_host[pt::C_FRESH], nc = ss->ctl_host[pt::C_CARRY];
    std::vector<pt::F4> ro(nf);
    std::vector<uint32_t> cw((size_t)nc * ss->plan.carry_words);
    if (nf) HIP_TRY(hipMemcpy(ro.data(), wp.fq[p].ro, nf * sizeof(pt::F4), hipMemcpyDeviceToHost));
    if (nc) HIP_TRY(hipMemcpy(cw.data(), wp.cq[p], cw.size() * 4, hipMemcpyDeviceToHost));
    std::vector<uint8_t> seen(ss->n_slots, 0);
    uint32_t dup = 0, bad = 0;
    auto see = [&](uint32_t slot) {
        if (slot >= ss->n_slots) { ++bad; return; }
        if (seen[slot]++) ++dup;
    };
    for (uint32_t i = 0; i < nf; ++i) see(pt::f2u(ro[i].w));
    for (uint32_t i = 0; i < nc; ++i) see(pt::carry_rec(cw.data(), i, ss->plan.carry_words).slot());
    if (dup || bad)
        fprintf(stderr, "dupcheck: round %u (%s%s) fresh %u carry %u: %u duplicate slot(s), %u out of range\n",
                ss->rounds, chains < ss->plan.lowq ? "low" : "full", side ? "+side" : "", nf, nc, dup, bad);
    return PT_OK;
}

// ---- the pass's stages ---------------------------------------------------------
// The final cooperative stage: the cooperative engine runs every remaining chain to the
// end of the pass.  A launch of teams of 4 (the default) stops once all but ss->plan.coop_grow
// of its chains have ended and hands those -- the pass's slowest, whose chain cycle sets
// the launch's end -- to a launch of whole-wave teams (the shortest cycle).
// (a scene beyond the engine's LDS tables runs the BIG instantiation: teams of 8 or 64)
int coop_final(pt_session* ss, const PassTune& t, pt::WaveParams& wp, uint32_t& p, uint32_t chains) {
    const bool big = ss->plan.big;
    uint32_t team = big && ss->plan.coop_team != 64u ? 8u : ss->plan.coop_team;
    for (;;) {
        // the next stage: teams of 4 or 8 -> (coop_grow_mid, from 8) teams of 32 -> (coop_grow) whole waves
        uint32_t keep = 0u, next_team = 64u;
        if (team == 8u && !big && ss->plan.coop_grow_mid > ss->plan.coop_grow && chains > ss->plan.coop_grow_mid) {
            keep = ss->plan.coop_grow_mid;
            next_team = 32u;
        } else if (team != 64u && ss->plan.coop_grow && chains > ss->plan.coop_grow) {
            keep = ss->plan.coop_grow;
        }
        // (the chains still running at the stop, at most `keep`, go to the next carry
        // queue: never more than it holds)
        keep = std::min(keep, ss->plan.carry_cap);
        const bool grow = keep != 0u;
        // (test hook grow_late: its late workgroups hand on every item they find
        // untaken, up to all of the launch's -- within the carry queue only)
        const bool grow_late = grow && t.grow_late;
        if (grow_late && chains > ss->plan.carry_cap)
            return fail(PT_E_INVALID, "PT_TUNE grow_late: more chains than the carry queue holds");
        wp.parity = p;
        hipEvent_t i0, i1;
        TRY(launch_events(ss, true, i0, i1));
        HIP_TRY(zero_round_out(ss, p));
        const uint32_t per_wg = QC_WAVES * (64u / team);   // chains per workgroup
        const uint32_t grid = std::max(1u, std::min(ss->plan.coop_grid, (chains + per_wg - 1u) / per_wg));
        if (t.cprof) TRY(arm_wg_prof(ss, wp, 512));
        if (ss->plan.coop_order) {
            const size_t cap = std::min<size_t>(std::max<size_t>(ss->n_slots, 1),
                                                std::max<uint32_t>(ss->plan.coop_max, 1u));
            if (chains > cap) return fail(PT_E_HIP, "cooperative intake order: more chains than entries");
            wp.order_cur = ss->order;
            wp.order = ss->order + 2 * PT_ORDER_BUCKETS;
            HIP_TRY(pt_launch_coop_order(wp, chains, ss->stream));
        }
        pt::WaveParams cp_ = wp;
        if (grow) {
            // stop at the chain cycle after all but coop_grow chains have ended (its own
            // C_ENDED); the rest go to the next launch's input as suspended queries
            uint32_t* out = ss->ctl + PT_CTL_SET * (1u - p);
            cp_.side_stop = out + pt::C_ENDED;
            cp_.side_stop_n = keep;            // (against the launch's own item count: before
            cp_.side_flags = PT_STOP_GROW |     //  the first count, `chains` is the slot count)
                             (grow_late ? PT_GROW_LATE : 0u);
            cp_.yield_cq = wp.cq[1u - p];
            cp_.yield_ctr = out + pt::C_CARRY;
        }
        HIP_TRY(pt_launch_coop(cp_, grid, team, big, ss->stream, i0, i1));
        wp.order = wp.order_cur = nullptr;
        if (t.cprof) TRY(report_cprof(ss, wp, team, chains, grid, i0, i1));
        ss->rounds++;
        p ^= 1u;
        TRY(count_round(ss, p));
        const uint32_t left = ss->ctl_host[pt::C_CARRY] + ss->ctl_host[pt::C_FRESH];
        if (left == 0u) return PT_OK;
        if (!grow) return fail(PT_E_HIP, "cooperative engine left chains behind");
        // the last chains: bigger teams
        chains = left;
        team = next_team;
        if (t.roundlog >= 2) fprintf(stderr, "coop grow: %u chains to teams of %u\n", left, team);
    }
}

// The early cooperative launch, beside a low-chain round: the round's heaviest
// chains (most samples left) run in a cooperative launch on the second stream while
// the path round runs the others (through wp.pin); the launch stops at a chain cycle's
// end once the round's path workgroups have all finished, its chains yielded to the
// next round's carry queue, and the next round starts when both are done.
// (test hook side_late: the launch is deferred -- side_launch_late runs it after the path
// round, on its stream: every workgroup one that started after the round's end)
struct SideLate {
    bool on = false;
    pt::WaveParams sp;
    uint32_t grid = 0;
};
// k = the chains it takes (> 0); the round's output set is zero already (zero_round_out)
int side_launch(pt_session* ss, const PassTune& t, pt::WaveParams& wp, uint32_t p, uint32_t chains, uint32_t k,
                bool sparse, SideLate& late) {
    const uint32_t path_grid = path_shape(ss->plan, chains, sparse, true).grid;   // (the round's workgroups: path_round)
    if (ss->side_th.joinable()) {
        ss->side_th.join();
        if (ss->side_rc != hipSuccess) return fail(PT_E_HIP, "side stream creation failed");
    }
    if (!ss->side_stream && take_stream(ss->dev, &ss->side_stream, true) != hipSuccess)
        return fail(PT_E_HIP, "stream creation failed");
    wp.parity = p;
    wp.order_cur = ss->order;
    wp.order = ss->order + 2 * PT_ORDER_BUCKETS;
    HIP_TRY(pt_launch_coop_order(wp, chains, ss->stream));
    HIP_TRY(hipMemsetAsync(ss->side_ctl, 0, 8 * PT_CTL_SET, ss->stream));   // (both of its sets, once)
    HIP_TRY(pt_launch_side_take(wp, k, ss->side, ss->side_carry, ss->side_ctl, ss->stream));
    // (the round's output counters, its finished-workgroup count among them, were zeroed
    // before this point: the side launch may look at them and yield into them from here on)
    if (!ss->side_taken) HIP_TRY(hipEventCreateWithFlags(&ss->side_taken, hipEventDisableTiming));
    if (!ss->side_end) HIP_TRY(hipEventCreateWithFlags(&ss->side_end, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ss->side_taken, ss->stream));
    HIP_TRY(hipStreamWaitEvent(ss->side_stream, ss->side_taken, 0));
    uint32_t* out = ss->ctl + PT_CTL_SET * (1u - p);
    pt::WaveParams sp = wp;
    sp.fq[0] = ss->side;
    sp.cq[0] = ss->side_carry;
    sp.ctl = ss->side_ctl;
    sp.parity = 0u;
    sp.order = sp.order_cur = nullptr;
    sp.pin = nullptr;
    sp.side_stop = out + pt::C_WGDONE;
    sp.side_stop_n = path_grid;
    sp.yield_cq = wp.cq[1u - p];
    sp.yield_ctr = out + pt::C_CARRY;
    sp.side_flags = (t.side_late ? PT_SIDE_LATE : 0u) | (t.side_stop_now ? PT_SIDE_STOP_NOW : 0u) |
                    (t.handon ? 0u : PT_SIDE_NO_HANDON);
    hipEvent_t i0, i1;
    TRY(launch_events(ss, true, i0, i1));
    const uint32_t grid = ss->plan.early_wg * (ss->plan.coop_grid / 8u);
    if (t.side_late) {
        late.on = true;
        late.sp = sp;
        late.grid = grid;
        HIP_TRY(hipEventRecord(i0, ss->stream));   // (timed with the round)
        HIP_TRY(hipEventRecord(i1, ss->stream));
    } else {
        HIP_TRY(pt_launch_coop(sp, grid, ss->plan.side_team, ss->plan.big, ss->side_stream, i0, i1));
        HIP_TRY(hipEventRecord(ss->side_end, ss->side_stream));
    }
    // the path round takes the other chains: items k .. chains of the order
    wp.pin = wp.order + k;
    wp.pin_n = chains - k;
    wp.order = wp.order_cur = nullptr;
    return PT_OK;
}
int side_launch_late(pt_session* ss, const SideLate& late) {
    // (it yields into the round's output counters, zeroed before the round was enqueued)
    HIP_TRY(pt_launch_coop(late.sp, late.grid, ss->plan.side_team, ss->plan.big, ss->stream));
    HIP_TRY(hipEventRecord(ss->side_end, ss->stream));
    return PT_OK;
}

// one path round (its output set zeroed by the caller): k_wpath -> k_wexact -> k_wshade
int path_round(pt_session* ss, const PassTune& t, pt::WaveParams& wp, uint32_t p, uint32_t chains, bool sparse) {
    wp.parity = p;
    if (!t.wgprof.empty()) TRY(arm_wg_prof(ss, wp, 512ull * ss->plan.path_grid));
    hipEvent_t i0, i1;
    TRY(launch_events(ss, false, i0, i1));
    const PathShape sh = path_shape(ss->plan, chains, sparse, wp.pin != nullptr);   // (pin: beside the early launch)
    const bool low = chains < ss->plan.lowq;
    wp.path_ticks = low ? ss->plan.low_ticks : ss->plan.path_ticks;
    const uint32_t* m = low ? ss->plan.mix_low : ss->plan.mix;
    wp.probe_every = m[0];
    wp.probe_min = m[1];
    wp.aux_extra = m[2];
    wp.end_min = m[3];
    // the session's grid of this shape (a low-chain round runs fewer workgroups of it)
    const uint32_t shape_grid = sh.nq == PT_NQ_BASE ? ss->plan.path_grid : ss->plan.full_grid;
    wp.path_runend = ss->plan.runend_auto ? shape_grid * sh.nq * 4u : ss->plan.path_runend;
    // Chains a workgroup may hold: 5/8 of the pixels' fair share, within
    // [256, the shape's capacity].  Below the share, about a third of the chains wait in
    // the queue and go to whichever workgroup drains first, instead of every
    // workgroup filling to its share and the costly ones finishing last
    // (1920x1080 on 1,024 workgroups: rank of 4 -> 319 instead of 478, +1 % over
    // three alternating pairs; ranks of 1 and 2 stay at 512, a rank of 8 at 256).
    // A low-chain round's workgroups take the whole capacity.
    {
        const uint64_t share = ((uint64_t)ss->n_slots + shape_grid - 1) / std::max(1u, shape_grid);
        wp.path_cap = (uint32_t)std::min<uint64_t>(sh.cmax, std::max<uint64_t>(256u, share * 5u / 8u));
    }
    if (low && ss->plan.low_grid) wp.path_cap = sh.cmax;
    if (t.has_cap) wp.path_cap = std::min<uint32_t>(sh.cmax, (uint32_t)std::max(64, t.cap));   // (an explicit cap=N stays)
    HIP_TRY(pt_launch_path_round(wp, sh.nq, sh.grid, 64u, ss->stream, sparse, i0, i1));
    wp.pin = nullptr;   // (only the round beside the early launch skips its chains)
    return PT_OK;
}

}  // namespace

int trace_wave(pt_session* ss, uint32_t spp) {
    const PassTune t;
    pt::WaveParams wp;
    TRY(fill_params(ss, spp, t, wp));
    ss->pending.emplace_back(nullptr, nullptr);   // (registered where they are created: finish_pending destroys them)
    HIP_TRY(hipEventCreate(&ss->pending.back().first));
    HIP_TRY(hipEventCreate(&ss->pending.back().second));
    const hipEvent_t e0 = ss->pending.back().first, e1 = ss->pending.back().second;
    HIP_TRY(hipEventRecord(e0, ss->stream));
    HIP_TRY(pt_launch_wave_start(wp, ss->stream));
    if (t.roundlog >= 2) TRY(report_round(ss, t.roundlog, wp.target, 0u, false));
    // rounds until no fresh ray and no suspended query is left; counts are
    // checked every few rounds (empty rounds are cheap, syncs are not free)
    // (the first round is counted alone: it ends once the pass's work is handed out, and
    // the cooperative engine may take over right after it)
    uint32_t p = 0, batch = ss->plan.coop_max ? 1u : 4u;
    // end-of-pass kernel when the chains of the last counted round are few; before
    // the first count, the pass's pixels (at most one chain each) decide
    bool sparse = ss->n_slots < ss->plan.path_sparse;
    // the cooperative engine once the chains are few (before the first count: the pixels)
    uint32_t chains = ss->n_slots;
    bool counted = false;
    for (uint32_t guard = 0;; ++guard) {
        if (chains <= ss->plan.coop_max) {
            TRY(coop_final(ss, t, wp, p, chains));
            break;
        }
        // the early launch's chains
        // (only after a count: before the first one `chains` is the slot count, not the
        // queue's, and every pixel has the same samples left)
        const bool early = ss->plan.early_k && counted && chains < ss->plan.early_at;
        const uint32_t k = early ? std::min(ss->plan.early_k, chains / 4u) : 0u;
        if (k) batch = 1u;   // (the next round reads what the side launch yields)
        SideLate late;
        for (uint32_t r = 0; r < batch; ++r) {
            HIP_TRY(zero_round_out(ss, p));
            if (k) TRY(side_launch(ss, t, wp, p, chains, k, sparse, late));
            TRY(path_round(ss, t, wp, p, chains, sparse));
            if (late.on) TRY(side_launch_late(ss, late));
            if (!t.wgprof.empty()) TRY(report_wgprof(ss, wp, p, t.wgprof.c_str()));
            ss->rounds++;
            p ^= 1u;
        }
        // (a side launch yields into this round's output: the count waits for it)
        if (k) HIP_TRY(hipStreamWaitEvent(ss->stream, ss->side_end, 0));
        TRY(count_round(ss, p));
        if (t.roundlog >= 2) TRY(report_round(ss, t.roundlog, wp.target, chains, k != 0u, sparse));
        if (t.dupcheck) TRY(check_dups(ss, wp, p, chains, k != 0u));
        if (ss->ctl_host[pt::C_FRESH] == 0u && ss->ctl_host[pt::C_CARRY] == 0u) break;
        if (guard > 100000u) return fail(PT_E_HIP, "wavefront rounds did not drain");
        chains = ss->ctl_host[pt::C_FRESH] + ss->ctl_host[pt::C_CARRY];
        counted = true;
        // near the cooperative hand-over every round is counted (the tail's rounds take ms)
        batch = chains > 4096u && chains > 4u * ss->plan.coop_max ? ss->plan.round_batch : (chains > 4096u ? 1u : 2u);
        sparse = chains < ss->plan.path_sparse;
    }
    HIP_TRY(hipEventRecord(e1, ss->stream));
    ss->samples_done += spp;
    return PT_OK;
}

}  // namespace pti
