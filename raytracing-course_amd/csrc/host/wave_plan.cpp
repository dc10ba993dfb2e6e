// wave_plan.cpp -- the wavefront pass's launch shapes and capacities (WavePlan): a function of
// the scene's tree facts, the device's CU count, the session's pixels and PT_TUNE.  No HIP
// call, no session, no scene: the CPU suite runs it through pt_selftest_wave_plan.
#include "api_internal.h"

namespace pti {

int plan_wave(const PlanInputs& in, WavePlan* out) {
    WavePlan w;
    const uint32_t cus = in.cus;
    const size_t n = std::max<size_t>(in.n_slots, 1);
    w.shade_grid = std::min<uint32_t>(cus * 8u, std::max(1u, in.n_tiles_local));
    // path engine: NQ query waves + 1 shade wave per workgroup, as many workgroups
    // per CU as its waves-per-SIMD occupancy holds (4 SIMDs per CU)
    w.path_budget = (uint32_t)std::max(1, tune_int("budget", (int)w.path_budget));
    // rounds end at one time for every wave (budget_us after the work ran out; 0: each
    // wave after `budget` trips of its own, also the mode of an explicit budget=N alone)
    // (at most 10 s: the device compares 32-bit clock differences as signed)
    w.path_ticks = (uint32_t)std::min(10000000, std::max(0, tune_int("budget_us", tune_has("budget") ? 0 : 2500))) * 100u;
    // ... and the low-chain rounds' deadline: 5 ms (fewer rounds, each of which re-sorts and
    // re-takes the early launch's heaviest chains; with coop_grow 16 per CU, one GPU call,
    // 3 repeats of every rank (tools/gpu_r5_ab.sh, profiles/r05_ab): rank of 8 mean 83.5 ->
    // 80.2 ms per 256-spp pass, rank of 4 139.9 -> 137.6, of 2 259.2 -> 255.6, one GPU
    // 488.8 -> 486.3); with budget_us=0 (trip budgets) the path rounds' mode
    // (lowq_budget_us=0: trip budgets in those rounds, as budget_us=0 for every round)
    w.low_ticks = tune_has("lowq_budget_us")
                      ? (uint32_t)std::min(10000000, std::max(0, tune_int("lowq_budget_us", 5000))) * 100u
                      : w.path_ticks == 0 ? 0u : 500000u;
    // (the full rounds' shape, PT_TUNE nq: 2, or 3 query waves per shade wave at 3 workgroups per CU)
    if (tune_has("nq")) {
        const std::string v = tune_str("nq");
        if (v != "2" && v != "3")
            return fail(PT_E_INVALID, "PT_TUNE nq=" + v + ": no such shape (2 or 3 query waves per workgroup)");
        w.full_nq = v == "3" ? 3u : 2u;
    }
    w.path_grid = cus * (uint32_t)std::max(1, tune_int("wg_per_cu", (int)pt::path_wg_per_cu(PT_NQ_BASE)));
    w.full_grid = cus * (uint32_t)std::max(1, tune_int("wg_per_cu", (int)pt::path_wg_per_cu(w.full_nq)));
    // the query lanes of the larger launch
    const uint64_t lanes = std::max<uint64_t>((uint64_t)w.path_grid * PT_NQ_BASE, (uint64_t)w.full_grid * w.full_nq) * 64u;
    // suspended-query records (pt_kernels.h CarryRec: Query | slot | aux stack).  Only a
    // query lane suspends (one query at round end), and a pixel has at most one ray
    // in flight, so a round appends at most min(pixels, query lanes) of them: the
    // carry queue can never overflow.  The exact-DFS hand-over queues (ex, done, hid)
    // do NOT have that bound: a lane that hands its ray over goes on with another
    // chain of the round's supply, so a round can hand over a ray of every chain --
    // at most one per pixel (a chain that leaves for k_wexact leaves the round).
    // They hold n entries.
    w.carry_words = pt::carry_record_words(std::max<uint32_t>(in.auxw_stack, 1u));
    w.lane_cap = (uint32_t)std::min<uint64_t>(n, lanes);
    // a round whose chains are this few runs them to the end of the pass (a few
    // per query wave of its launch, 4: rebalancing them costs more rounds than it saves)
    w.runend_auto = !tune_has("runend");
    w.path_runend = (uint32_t)std::max(0, tune_int("runend", 0));
    // rounds with fewer chains than this run the end-of-pass (sparse) kernel (its own shape's lanes)
    w.path_sparse = (uint32_t)std::max(0, tune_int("sparse", (int)(w.path_grid * PT_NQ_BASE * 32u)));
    w.sparse_steps = (uint32_t)std::max(1, tune_int("sparse_steps", (int)w.sparse_steps));
    // a round whose chains are at most this many runs the cooperative engine (one
    // wave per chain) to the end of the pass; it needs a wave's aux stack to hold
    // a depth-first descent below its expansion limit, and lane 0's exact DFS stack
    // 49,152 on the 256-CU part (2 query waves per shade wave, hit-region query; rank-of-4 /
    // rank-of-8 per GPU, teams of 8, two runs each: 32 k 2,758-2,782 / 2,348-2,396, 49 k
    // 2,754-2,774 / 2,377-2,421, 65 k 2,731-2,763 / 2,318-2,338, 98 k 2,695-2,699 / 2,220-2,324,
    // 131 k 2,599-2,603 / 2,358-2,430 Mray/s)
    w.coop_max = (uint32_t)std::max(0, tune_int("coop", (int)(cus * 192u)));
    w.coop_grid = cus * 8u;
    // (a depth-first descent below the expansion limit adds at most 3 entries per level)
    const uint32_t reserve = 3u * (in.auxsl_depth + 2u);
    // a team size's stacks hold this tree (the engine's capacities: pt_kernels.h qc_*): the
    // expansion (its own stack, or for teams of 4 the wave's pool) a depth-first descent
    // below the reserve, and the leader's exact DFS (its stack, or its slice of the pool)
    // the whole tree (and for teams below 64 the pool's items, chain << shift | node, hold
    // every aux entry index)
    auto stack_ok = [&](uint32_t expand, uint32_t dfs) { return expand >= reserve + 64u && in.max_stack <= dfs; };
    auto team_ok = [&](uint32_t t) {
        if (t < 64u && in.n_aux >= (1ull << pt::qc_item_shift(t))) return false;
        return stack_ok(t == 4u ? pt::qc_pool_words(t) : pt::qc_stack_words(t), pt::qc_stack_words(t));
    };
    w.coop_team = (uint32_t)tune_int("coop_team", (int)w.coop_team);
    if (w.coop_team != 4u && w.coop_team != 8u && w.coop_team != 16u && w.coop_team != 32u) w.coop_team = 64u;
    if (!team_ok(w.coop_team)) w.coop_team = 64u;   // deep trees: whole-wave teams
    // (paths deeper than QC_FOLD keep their further fold records in HBM, planes and
    // emitters beyond QC_NPL / QC_NEM come from HBM: no scene limit besides the stacks)
    if (!stack_ok(pt::qc_stack_words(64u), pt::qc_stack_words(64u)))
        w.coop_max = 0;
    else w.coop_reserve = reserve;
    // with the cooperative engine the path engine never runs a round to the end:
    // its rounds stay budget-limited, so the host sees the chains fall below coop_max
    if (w.coop_max && w.runend_auto) {
        w.path_runend = 0;
        w.runend_auto = false;
    }
    // ... and the end-of-pass (sparse) path kernel, whose rounds are long, never runs
    // above the hand-over
    if (w.coop_max && !tune_has("sparse")) w.path_sparse = std::min(w.path_sparse, w.coop_max);
    w.round_batch = (uint32_t)std::max(1, tune_int("round_batch", (int)w.round_batch));
    w.coop_order = tune_int("coop_order", 1) != 0;
    // the final launch's last chains to whole-wave teams: 16 per CU (4 per CU measured within
    // the spread of 0; 16 with the 5-ms low-round deadline above: see low_ticks)
    w.coop_grow = (uint32_t)std::max(0, tune_int("coop_grow", (int)(cus * 16u)));
    // ... and, before that, its last coop_grow_mid chains to teams of 32 (0: no such stage; a
    // tree too deep for the teams-of-32 stack skips it)
    w.coop_grow_mid = (uint32_t)std::max(0, tune_int("coop_grow_mid", 0));
    if (!stack_ok(pt::qc_stack_words(32u), pt::qc_stack_words(32u))) w.coop_grow_mid = 0u;
    // Early cooperative launch (teams of side_team lanes, QC_WAVES waves per workgroup):
    // the low-chain rounds leave each CU room for one more workgroup, which the heaviest
    // chains use from then on instead of waiting for the final hand-over
    w.early_wg = (uint32_t)std::max(1, tune_int("early_wg", 1));
    w.early_at = (uint32_t)std::max(0, tune_int("early_at", (int)(cus * 768u)));
    w.early_k = (uint32_t)std::max(0, tune_int("early", 1));
    // lanes per chain of that launch: 4 (default: 16 chains per wave, its pooled query keeps
    // a wave's lanes busy with half as many lanes per chain; rank 0 of 8 73.5-75.2 ms against
    // 76.4-83.1 with teams of 8, of 4 130.4-132.0 against 131.1-133.7, of 1 472-476 against
    // 476-480: profiles/r06_coop/team4), 8, 16, 32 or 64
    // (a scene beyond the LDS tables has only the teams-of-8 BIG instantiation)
    w.big = in.depth > QC_FOLD || in.n_planes > QC_NPL || in.n_emitters > QC_NEM;
    const int st = tune_int("side_team", 4);
    w.side_team = !w.big && (st == 4 || st == 16 || st == 32 || st == 64) ? (uint32_t)st : 8u;
    if (!team_ok(w.side_team)) w.side_team = team_ok(8u) ? 8u : 64u;
    if (w.early_k == 1u) w.early_k = cus * w.early_wg * QC_WAVES * (64u / w.side_team);   // early=1: what it holds
    if (!w.coop_max || (w.coop_team != 8u && w.coop_team != 4u) || w.side_team == 64u) w.early_k = 0;
    // a round's carry output also takes the early launch's yielded chains
    w.carry_cap = (uint32_t)std::min<uint64_t>(n, (uint64_t)w.lane_cap + w.early_k);
    static const char* keys[4] = {"probe_every", "probe_min", "aux_extra", "end_min"};
    static const char* lkeys[4] = {"lowq_probe_every", "lowq_probe_min", "lowq_aux_extra", "lowq_end_min"};
    for (int i = 0; i < 4; ++i) {
        const int lo = i == 0 || i == 3 ? 1 : 0;
        w.mix[i] = (uint32_t)std::max(lo, tune_int(keys[i], (int)w.mix[i]));
        // (the low rounds' end_min has a default of its own; the others follow the full rounds')
        w.mix_low[i] = (uint32_t)std::max(lo, tune_int(lkeys[i], (int)(i == 3 ? w.mix_low[i] : w.mix[i])));
    }
    w.mix[3] = std::min<uint32_t>(w.mix[3], 64u);
    w.mix_low[3] = std::min<uint32_t>(w.mix_low[3], 64u);
    // Rounds that start with fewer than 768 chains per CU run on 2 path workgroups
    // per CU (PT_CMAX chains each) instead of 4: with that few chains the rounds are
    // bound by each chain's latency, and a query trip's instruction stream shares its
    // SIMD with fewer waves.  Rank-of-1 / 2 / 4 / 8 (rank 0, three interleaved
    // repeats, profiles/r03_lowq): +2.3 / +2 / +4 / +3-10 %; 150 k / 250 k chains
    // within 1 % at ranks of 1-4, and 300 k (every round of a rank of 8, the first
    // included) -25 % at rank-of-8.
    w.lowq = (uint32_t)std::max(0, tune_int("lowq", (int)(cus * 768u)));
    w.low_grid = std::min(w.path_grid, cus * (uint32_t)std::max(1, tune_int("lowq_wg", 2)));
    *out = w;
    return PT_OK;
}

PathShape path_shape(const WavePlan& w, uint32_t chains, bool sparse, bool side) {
    if (chains < w.lowq && w.low_grid) return {PT_NQ_BASE, w.low_grid, pt::path_cmax(PT_NQ_BASE)};
    if (sparse || side || w.full_nq == PT_NQ_BASE) return {PT_NQ_BASE, w.path_grid, pt::path_cmax(PT_NQ_BASE)};
    return {w.full_nq, w.full_grid, pt::path_cmax(w.full_nq)};
}

std::string plan_text(const WavePlan& w) {
    const std::pair<const char*, uint32_t> kv[] = {
        {"shade_grid", w.shade_grid},   {"path_budget", w.path_budget}, {"path_ticks", w.path_ticks},
        {"low_ticks", w.low_ticks},     {"full_nq", w.full_nq},         {"path_grid", w.path_grid},
        {"full_grid", w.full_grid},     {"carry_words", w.carry_words}, {"lane_cap", w.lane_cap},
        {"carry_cap", w.carry_cap},     {"runend_auto", w.runend_auto}, {"path_runend", w.path_runend},
        {"path_sparse", w.path_sparse}, {"sparse_steps", w.sparse_steps}, {"coop_max", w.coop_max},
        {"coop_grid", w.coop_grid},     {"coop_reserve", w.coop_reserve}, {"coop_team", w.coop_team},
        {"coop_order", w.coop_order},   {"coop_grow", w.coop_grow},     {"coop_grow_mid", w.coop_grow_mid},
        {"round_batch", w.round_batch}, {"early_wg", w.early_wg},       {"early_at", w.early_at},
        {"early_k", w.early_k},         {"side_team", w.side_team},     {"lowq", w.lowq},
        {"low_grid", w.low_grid},       {"big", w.big}};
    std::string t;
    for (const auto& e : kv) t += std::string(e.first) + "=" + std::to_string(e.second) + "\n";
    for (const uint32_t* m : {w.mix, w.mix_low}) {
        t += m == w.mix ? "mix=" : "mix_low=";
        for (int i = 0; i < 4; ++i) t += std::to_string(m[i]) + (i < 3 ? "," : "\n");
    }
    return t;
}

}  // namespace pti
