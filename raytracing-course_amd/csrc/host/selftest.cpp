// selftest.cpp -- host execution of the device query and integrator code (pt_query.h,
// pt_coop.h, pt_trace.h) for the CPU tests, and pt_selftest_math: the device code's scalar
// functions element by element, on the host or on a device (pt_selftest.h); never used by pt_render.
#include <stdio.h>
#include <string.h>

#include <array>
#include "api_internal.h"
#include "../device/pt_selftest.h"

namespace pti {
namespace {
struct HostStack {
    std::vector<uint32_t> v;
    uint32_t cap = 0xffffffffu;
    void setc(uint32_t i, uint32_t x, bool c) { if (c) set(i, x); }
    void set(uint32_t i, uint32_t x) { if (v.size() <= i) v.resize(i + 1); v[i] = x; }
    uint32_t get(uint32_t i) const { return v[i]; }
};
struct HostVStore {
    std::vector<uint32_t> v;
    void put(uint32_t k, uint32_t idm, float s1, float s2) {
        if (v.size() < 3 * (k + 1)) v.resize(3 * (k + 1));
        v[3 * k] = idm; v[3 * k + 1] = pt::f2u(s1); v[3 * k + 2] = pt::f2u(s2);
    }
    void get(uint32_t k, uint32_t& idm, float& s1, float& s2) const {
        idm = v[3 * k]; s1 = pt::u2f(v[3 * k + 1]); s2 = pt::u2f(v[3 * k + 2]);
    }
};
// The host twin of start_query and QStats (pt_batch.h): a closest-hit query run to completion on
// this thread's stack, and what the device counts of it -- the query's QCounts added to `C` (the
// guard bit masked out of `planes`), the guard itself (C.errs), the queries that took the exact DFS
// and, of those, the non-finite rays.  trace_path_with counts a path's rays and calls the object;
// a hook that runs single queries calls query().
enum QEngine { QE_RUN, QE_COOP, QE_TRIP };   // q_run | qc_query (pt_coop.h) | q_run_trip, the path engine's trips
struct HostQuery {
    const pt::SceneView& V;
    const QEngine engine;
    const uint32_t aux_extra;       // QE_TRIP: extra aux-node steps per trip
    const bool count_nonfinite;     // false: exact_ray stays 0 (a hook whose engine has no such counter)
    const bool log;                 // PT_TUNE qstats: a record per query in qlog
    HostStack stk;
    pt::Counts C{};
    uint64_t exact_ray = 0;
    uint64_t diag[3] = {0, 0, 0};   // PT_QDIAG: queries, aux steps, range-test steps
    std::vector<std::array<uint32_t, 4>> qlog;
    explicit HostQuery(const pt::SceneView& v, QEngine e = QE_RUN, uint32_t extra = 1u, bool nonfinite = true,
                       bool qstats = false)
        : V(v), engine(e), aux_extra(extra), count_nonfinite(nonfinite), log(qstats) {}

    int operator()(const pt::Ray& r, pt::Hit& h, pt::Counts& cc) {
        pt::QCounts Q{};
        uint32_t ex = 0;
        const int id = engine == QE_COOP   ? pt::qc_query(V, r, stk, h, Q, ex)
                       : engine == QE_TRIP ? pt::q_run_trip(V, r, stk, h, Q, ex, aux_extra)
                                           : pt::q_run(V, r, stk, h, Q, ex);
        if (Q.planes & 0x80000000u) cc.errs |= 4u;   // recomputed hit differs (verdict())
        cc.nodes += Q.nodes; cc.ptests += Q.ptests; cc.planes += Q.planes & 0x7fffffffu; cc.aux += Q.aux;
        cc.fallbacks += ex;
        const float w = count_nonfinite ? pt::q_prep(V, r).w : 0.f;
        if (w != w) exact_ray++;   // a non-finite ray (q_init_pre: Q_EXACT from the start)
#ifdef PT_QDIAG
        diag[0]++; diag[1] += Q.aux; diag[2] += Q.aux_ranges;
        if (log) qlog.push_back({Q.aux, Q.rc_acc | (Q.rc_rej << 16), Q.rc_walk, Q.cands | (Q.passes << 16)});
#else
        if (log) qlog.push_back({Q.aux, Q.nodes, Q.ptests | (ex << 31), 0u});
#endif
        return id;
    }
    int query(const pt::Ray& r, pt::Hit& h) { C.rays++; return (*this)(r, h, C); }
    // the guard's "must never happen"
    int verdict() const { return C.errs ? fail(PT_E_INVALID, "recomputed closest hit differs from the query's") : PT_OK; }
    // counters8 (null: none asked for): the slots CTR_RAYS .. CTR_FALLBACKS_RAY, as QStats::flush fills them
    void pack(uint64_t* counters8) const {
        if (!counters8) return;
        uint64_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        c[pt::CTR_RAYS] = C.rays; c[pt::CTR_NODES] = C.nodes; c[pt::CTR_PTESTS] = C.ptests; c[pt::CTR_PLANES] = C.planes;
        c[pt::CTR_ERRORS] = C.errs; c[pt::CTR_AUX] = C.aux; c[pt::CTR_FALLBACKS] = C.fallbacks;
        c[pt::CTR_FALLBACKS_RAY] = exact_ray;
        memcpy(counters8, c, sizeof(c));
    }
    // make DEFS=-DPT_QDIAG: the line of n threads' queries
    static void qdiag(const HostQuery* q, size_t n) {
#ifdef PT_QDIAG
        uint64_t a[3] = {0, 0, 0};
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) a[k] += q[i].diag[k];
        fprintf(stderr, "qdiag: %llu rays, %llu aux steps, %llu of a lane that needs the range test\n",
                (unsigned long long)a[0], (unsigned long long)a[1], (unsigned long long)a[2]);
#endif
    }
};
// PT_TUNE qengine=coop (and, where the hook has it, =trip) as the query's engine
QEngine tuned_engine(bool with_trip) {
    const std::string e = tune_str("qengine");
    return e == "coop" ? QE_COOP : with_trip && e == "trip" ? QE_TRIP : QE_RUN;
}
// the general body of q_exec_aux on this thread for the holder's life (pt_query.h)
struct ForceGeneral {
    const bool was;
    explicit ForceGeneral(bool on) : was(pt::q_force_general()) { pt::q_force_general() = on; }
    ~ForceGeneral() { pt::q_force_general() = was; }
};
// q_decide stated as the plain loop over the list, apart from pt_query.h's text: the reference
// pt_selftest_decide holds q_decide to, on the host and on the device, whatever form it takes
// there (profiles/r29_decide measured a slot-indexed one).  Host only.
void q_decide_loop(pt::Query& q) {
    while (q.ne < q.nh) {
        q.cand = pt::q_sel(q.hidx, q.ne, 0xffffffffu);
        if (!(fminf(q.P, q.bt) >= pt::q_sel(q.hacc, q.ne, PT_INF))) {
            q.walk = pt::R_CAND;
            q.phase = pt::Q_REPLAY;
            return;
        }
        pt::q_record_entered(q);
    }
    pt::q_pass_done(q);
}
// n seeded decision states (a lane in phase Q_DECIDE): ne <= nh <= PT_QHK, hidx sorted with
// 0xffffffff in the empty slots, the t's, thresholds, P and bt from a few values and their
// neighbours, so that ties and +inf are common and hacc lies on both sides of min(P, bt);
// overflow takes both values, and one state in 32 has a list full of entered hits with
// overflow set (the Q_EXACT exit)
struct DecideStates {
    uint64_t x;
    explicit DecideStates(uint64_t seed) : x(seed * 0x9e3779b97f4a7c15ull + 0x2545f4914f6cdd1dull) {}
    uint32_t rnd() {   // xorshift64*
        x ^= x >> 12; x ^= x << 25; x ^= x >> 27;
        return (uint32_t)((x * 0x2545f4914f6cdd1dull) >> 32);
    }
    float val() {
        static const float base[8] = {0.5f, 1.f, 1.f, 2.f, 3.5f, PT_INF, INFINITY, 0.f};
        const float v = base[rnd() & 7u];
        const uint32_t k = rnd() % 5u;   // the value, a neighbour, or its negative
        return k == 0u ? nextafterf(v, INFINITY) : k == 1u ? nextafterf(v, -INFINITY) : k == 2u ? -v : v;
    }
    pt::Query next() {
        pt::Query q;
        memset(&q, 0, sizeof(q));
        const bool full = (rnd() & 31u) == 0u;
        const uint32_t nh = full ? (uint32_t)PT_QHK : rnd() % (PT_QHK + 1u);
        const uint32_t ne = full ? nh : (rnd() & 3u) ? 0u : rnd() % (nh + 1u);
        uint32_t idx = rnd() % 1000u;
        q.lb = idx;
        for (uint32_t k = 0; k < PT_QHK; ++k) {
            idx += 1u + rnd() % 50u;
            q.hidx[k] = k < nh ? idx : 0xffffffffu;
            q.ht[k] = val();
            q.hacc[k] = (rnd() & 3u) ? val() : (rnd() & 1u) ? INFINITY : -INFINITY;
            q.hid[k] = (int)(rnd() % 100000u);
            if (k + 1u == ne) q.lb = idx + 1u;
        }
        q.nh = nh;
        q.ne = ne;
        q.P = val();
        q.bt = (rnd() & 1u) ? PT_INF : val();
        q.res_t = val();
        q.res_id = (int)(rnd() % 100000u) - 1;
        q.phase = pt::Q_DECIDE;
        q.walk = rnd() % 3u;
        q.overflow = full ? 1u : rnd() & 1u;
        q.par = rnd() & 1u;
        q.sp = rnd() & 127u;
        q.node = rnd();
        q.cand = rnd();
        q.li = rnd();
        return q;
    }
};
}  // namespace
}  // namespace pti

using namespace pti;

extern "C" {

int pt_selftest_ray_intersection(pt_scene* s, int32_t traversal, uint32_t n, const float* rays, int32_t* ids,
                                 float* hits, uint64_t* counters8) {
    int rc = pt_scene_prepare(s);
    if (rc) return rc;
    const pt::SceneView V = host_view(s, traversal);
    const pt::ReplayCfg cfg = replay_cfg(s);
    // qengine=coop | mega | trip (the trips with PT_TUNE aux_extra extra aux-node steps each); the
    // non-finite rays are not counted here (CTR_FALLBACKS_RAY stays 0)
    const bool mega = tune_str("qengine") == "mega";   // the megakernel's FAST query (k_trace<true>)
    HostQuery q(V, tuned_engine(true), (uint32_t)std::max(0, tune_int("aux_extra", 1)), false);
    // qforms=general: the general q_exec_aux body on every step of this call
    const ForceGeneral forced(tune_str("qforms") == "general");
    for (uint32_t i = 0; i < n; ++i) {
        pt::Ray r;
        r.o = pt::mk3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
        r.d = pt::mk3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
        pt::Hit h;
        int id;
        if (traversal != PT_TRAVERSAL_REPLAY) {
            id = pt::ray_intersection<false>(V, cfg, r, q.stk, h, q.C);
        } else if (mega) {
            id = pt::ray_intersection<true>(V, cfg, r, q.stk, h, q.C);
        } else {
            id = q.query(r, h);
            if ((rc = q.verdict())) return rc;
        }
        ids[i] = id;
        const bool ok = id != -1;
        hits[5 * i] = ok ? h.t : 0.f;
        hits[5 * i + 1] = ok ? h.n.x : 0.f;
        hits[5 * i + 2] = ok ? h.n.y : 0.f;
        hits[5 * i + 3] = ok ? h.n.z : 0.f;
        hits[5 * i + 4] = ok ? (h.interior ? 1.f : 0.f) : 0.f;
    }
    HostQuery::qdiag(&q, 1);
    q.pack(counters8);
    // the exact DFS alone on this stack: it must have stayed within the words the device forms give it
    if (traversal == PT_TRAVERSAL_EXACT && q.stk.v.size() > std::max<uint32_t>(s->max_stack, 1u))
        return fail(PT_E_INVALID, "the exact DFS used more stack words than max_stack");
    return PT_OK;
}

int pt_selftest_decide(uint64_t seed, uint64_t n, uint64_t* out3) {
    if (!out3) return fail(PT_E_INVALID, "null argument");
    // q_decide_loop is the reference: q_decide must agree on every state in every byte of the Query
    DecideStates gen(seed);
    uint64_t examined = 0, bad = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const pt::Query q = gen.next();
        pt::Query a = q, b = q;
        q_decide_loop(a);
        pt::q_decide(b);
        if (memcmp(&a, &b, sizeof(a))) bad++;
        if (q.ne < q.nh) examined++;
    }
    out3[0] = n;
    out3[1] = examined;
    out3[2] = bad;
    return PT_OK;
}

int pt_selftest_decide_states(int device, uint64_t seed, uint64_t n, void* states, uint64_t cap, uint64_t* counts,
                              uint32_t* state_bytes) {
    if (state_bytes) *state_bytes = (uint32_t)sizeof(pt::Query);
    if (n == 0) return PT_OK;
    if (n > (1ull << 24)) return fail(PT_E_INVALID, "more than 2^24 states");
    if (states && cap < n * sizeof(pt::Query)) return fail(PT_E_INVALID, "state buffer too small");
    std::vector<pt::Query> st((size_t)n);
    DecideStates gen(seed);
    uint64_t c[4 + PT_QHK] = {0};
    for (uint64_t i = 0; i < n; ++i) {
        const pt::Query q = gen.next();
        pt::Query a = q;
        q_decide_loop(a);
        // the exit, and the last slot the loop examined (none: the lane came with ne == nh)
        c[a.phase == pt::Q_REPLAY ? 0 : a.phase == pt::Q_DONE ? 1 : a.phase == pt::Q_AUX ? 2 : 3]++;
        if (a.phase == pt::Q_REPLAY) c[4 + a.ne]++;
        else if (a.ne > q.ne) c[4 + a.ne - 1u]++;
        st[(size_t)i] = device < 0 ? a : q;
    }
    if (counts) memcpy(counts, c, sizeof(c));
    if (device >= 0) {
        if (const int rc = check_device(device)) return rc;
        HIP_TRY(hipSetDevice(device));
        void* buf = nullptr;
        const size_t bytes = (size_t)n * sizeof(pt::Query);
        HIP_TRY(hipMalloc(&buf, bytes));
        hipError_t e = hipMemcpy(buf, st.data(), bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = pt_launch_selftest_decide(n, buf, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(st.data(), buf, bytes, hipMemcpyDeviceToHost);
        (void)hipFree(buf);
        if (e != hipSuccess) return fail(PT_E_HIP, std::string("pt_selftest_decide_states: ") + hipGetErrorString(e));
    }
    if (states) memcpy(states, st.data(), (size_t)n * sizeof(pt::Query));
    return PT_OK;
}

int pt_selftest_aux_words(pt_scene* s, uint64_t* out5) {
    if (!s || !out5) return fail(PT_E_INVALID, "null argument");
    if (const int rc = pt_scene_prepare(s)) return rc;
    // every entry of the blob's aux section against the host-form array: the item (w7) and the
    // leaf index / range (w6) the former {range, code} pair gave, and the ordinal against the
    // bundle it names (its header holds the reference leaf)
    const size_t n = s->auxsl.size();
    if (s->blob.size() * 16 < (size_t)s->o_aux + n * sizeof(pt::AuxSL)) return fail(PT_E_INVALID, "no aux section");
    const pt::AuxSL* blob = reinterpret_cast<const pt::AuxSL*>(reinterpret_cast<const unsigned char*>(s->blob.data()) + s->o_aux);
    uint64_t empty = 0, leaf = 0, inner = 0, bad = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t code = pt::f2u(s->auxsl[i].b.w), range = pt::f2u(s->auxsl[i].b.z);
        const uint32_t w6 = pt::f2u(blob[i].b.z), w7 = pt::f2u(blob[i].b.w);
        if (code == 0xffffffffu) {
            empty++;
            if (w7 != 0xffffffffu) bad++;
        } else if (code & 0x80000000u) {
            // the old formula: item = PT_LEAFQ | rng, lidx = code & 0x7fffffff, with rng the leaf's
            // ordinal: leaves are numbered in the array's order, and bundle `ordinal` holds the leaf
            const uint32_t ord = (uint32_t)leaf++;
            const size_t bo = (size_t)s->o_bundle / 16 + 6u * (size_t)ord + 3u;
            const bool named = bo < s->blob.size() && pt::f2u(s->blob[bo].x) == (code & 0x7fffffffu);
            if (w7 != (PT_LEAFQ | ord) || w7 == 0xffffffffu || w6 != (code & 0x7fffffffu) || !named) bad++;
        } else {
            inner++;
            if (w7 != code || w6 != range) bad++;
        }
    }
    out5[0] = n; out5[1] = empty; out5[2] = leaf; out5[3] = inner; out5[4] = bad;
    return PT_OK;
}

int pt_selftest_render_host(pt_scene* s, int32_t traversal, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                            uint32_t spp, float* radiance) {
    int rc = pt_scene_prepare(s);
    if (rc) return rc;
    const pt::SceneView V = host_view(s, traversal);
    const pt::ReplayCfg cfg = replay_cfg(s);
    const pt::CamView cam = make_cam(s);
    const uint32_t S = spp ? spp : s->hs.samples;
    const uint32_t nt = std::max(1u, std::thread::hardware_concurrency());
    // diagnostics: PT_TUNE qstats=<file> dumps per-query {aux visits, node tests, prim tests, exact} (u32 x4)
    const std::string qpath = tune_str("qstats");
    const bool mega = tune_str("qengine") == "mega";   // the megakernel's FAST query (k_trace<true>)
    // a thread's query: the wavefront engine's (pt_query.h state machine) or qengine=coop's, run to completion
    std::vector<HostQuery> qs(nt, HostQuery(V, tuned_engine(false), 1u, false, !qpath.empty()));
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < nt; ++t) {
        th.emplace_back([&, t]() {
            HostQuery& q = qs[t];
            HostVStore vs;
            for (uint64_t k = t; k < (uint64_t)w * h; k += nt) {
                const uint32_t x = x0 + (uint32_t)(k % w), y = y0 + (uint32_t)(k / w);
                pt::Rng R = pt::rng_seed(y * s->hs.W + x);
                pt::f3 sum = pt::mk3(0.f, 0.f, 0.f);
                for (uint32_t i = 0; i < S; ++i) {
                    const float fx = (float)x + pt::rng_uniform(R);
                    const float fy = (float)y + pt::rng_uniform(R);
                    const pt::Ray ray = pt::camera_ray(cam, fx, fy);
                    if (traversal != PT_TRAVERSAL_REPLAY)
                        sum = sum + pt::trace_path<false>(V, cfg, ray, s->hs.depth, R, q.stk, vs, q.C);
                    else if (mega)
                        sum = sum + pt::trace_path<true>(V, cfg, ray, s->hs.depth, R, q.stk, vs, q.C);
                    else
                        sum = sum + pt::trace_path_with(V, q, ray, s->hs.depth, R, vs, q.C);
                }
                radiance[3 * k] = pt::sample_mean(sum.x, S);
                radiance[3 * k + 1] = pt::sample_mean(sum.y, S);
                radiance[3 * k + 2] = pt::sample_mean(sum.z, S);
            }
        });
    }
    for (auto& x : th) x.join();
    HostQuery::qdiag(qs.data(), qs.size());
    if (!qpath.empty())
        if (FILE* f = fopen(qpath.c_str(), "wb")) {
            for (const HostQuery& q : qs) fwrite(q.qlog.data(), 16, q.qlog.size(), f);
            fclose(f);
        }
    for (const HostQuery& q : qs)
        if ((rc = q.verdict())) return rc;
    return PT_OK;
}

int pt_selftest_paths_host(pt_scene* s, uint64_t n, const pt_path_ray* in, pt_path_out* out, uint64_t* counters8) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (n > 0 && (!in || !out)) return fail(PT_E_INVALID, "null path or radiance buffer");
    int rc = pt_scene_prepare(s);
    if (rc) return rc;
    const pt::SceneView V = host_view(s, PT_TRAVERSAL_REPLAY);
    HostQuery q(V);   // the batch radiance engine's query
    HostVStore vs;
    for (uint64_t i = 0; i < n; ++i) {
        pt::Ray ray;
        ray.o = pt::mk3(in[i].o[0], in[i].o[1], in[i].o[2]);
        ray.d = pt::mk3(in[i].d[0], in[i].d[1], in[i].d[2]);
        pt::Rng R = pt::rng_seed(in[i].seed);
        const uint64_t rays0 = q.C.rays;
        const pt::f3 L = pt::trace_path_with(V, q, ray, s->hs.depth, R, vs, q.C);
        out[i] = pt_path_out{{L.x, L.y, L.z}, (uint32_t)(q.C.rays - rays0)};
    }
    q.pack(counters8);
    return q.verdict();
}

int pt_selftest_pixels_host(pt_scene* s, uint64_t n, pt_pixel_state* state, const uint32_t* counts, uint32_t spp,
                            uint64_t* counters8) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (n > 0 && !state) return fail(PT_E_INVALID, "null state buffer");
    int rc = pt_scene_prepare(s);
    if (rc) return rc;
    const pt::SceneView V = host_view(s, PT_TRAVERSAL_REPLAY);
    const pt::CamView cam = make_cam(s);
    HostQuery q(V);   // the pixel-sample engine's query
    HostVStore vs;
    for (uint64_t i = 0; i < n; ++i) {
        pt_pixel_state& P = state[i];
        const uint32_t count = counts ? counts[i] : spp;
        if (count == 0u) continue;   // (not a byte of the record changes)
        pt::Rng R = pt::pixel_rng(P.rng, P.saved);
        pt::f3 sum = pt::mk3(P.sum[0], P.sum[1], P.sum[2]);
        // Sample's loop body (src/scene.cpp:197-199) on the record's stream
        for (uint32_t k = 0; k < count; ++k) {
            const float fx = (float)P.x + pt::rng_uniform(R);
            const float fy = (float)P.y + pt::rng_uniform(R);
            const pt::Ray ray = pt::camera_ray(cam, fx, fy);
            sum = sum + pt::trace_path_with(V, q, ray, s->hs.depth, R, vs, q.C);
        }
        P.rng = pt::pixel_rng_word(R);
        P.saved = pt::pixel_rng_saved(R);
        P.sum[0] = sum.x; P.sum[1] = sum.y; P.sum[2] = sum.z;
        P.samples += count;
    }
    q.pack(counters8);
    return q.verdict();
}

int pt_selftest_features_host(pt_scene* s, uint64_t n, const float* xy, pt_feature* out, uint64_t* counters8) {
    if (!s) return fail(PT_E_INVALID, "null scene");
    if (n > 0 && (!xy || !out)) return fail(PT_E_INVALID, "null position or feature buffer");
    int rc = pt_scene_prepare(s);
    if (rc) return rc;
    const pt::SceneView V = host_view(s, PT_TRAVERSAL_REPLAY);
    const pt::CamView cam = make_cam(s);
    HostQuery q(V);
    for (uint64_t i = 0; i < n; ++i) {
        // k_feats' job on one thread: the position's ray, its query, the record from the hit
        pt::Hit h;
        const int id = q.query(pt::camera_ray(cam, xy[2 * i], xy[2 * i + 1]), h);
        pt::Feature f;
        pt::feature_fill(V, id, h, f);
        memcpy(out + i, &f, sizeof(f));
    }
    q.pack(counters8);
    return q.verdict();
}

int pt_selftest_fit_block(uint32_t aux_words, uint32_t dfs_words, uint32_t* block_aux_only, uint32_t* block_both,
                          uint32_t* fits) {
    if (!block_aux_only || !block_both || !fits) return fail(PT_E_INVALID, "null argument");
    QueryCtx rays;   // k_rays' / k_feats' rule on one compute unit: nothing but the shape is touched
    const bool ok_rays = rays_shape(&rays, LaneWords{aux_words, dfs_words}, 1u) == PT_OK;
    uint32_t both = 256u;   // k_paths' / k_pixels' rule (qctx_fold_shape's first step)
    const bool ok_both = fit_block(aux_words, dfs_words, &both);
    *block_aux_only = rays.block;
    *block_both = both;
    *fits = (ok_rays ? 1u : 0u) | (ok_both ? 2u : 0u);
    return PT_OK;
}

int pt_selftest_lane_shape(pt_scene* s, uint32_t* aux_words, uint32_t* dfs_words, uint32_t* block_aux_only,
                           uint32_t* block_both, uint32_t* fits) {
    if (!s || !aux_words || !dfs_words) return fail(PT_E_INVALID, "null argument");
    if (const int rc = pt_scene_prepare(s)) return rc;
    const LaneWords w = lane_words(s);
    *aux_words = w.aux_words;
    *dfs_words = w.dfs_words;
    return pt_selftest_fit_block(w.aux_words, w.dfs_words, block_aux_only, block_both, fits);
}

int pt_selftest_ctx_shape(uint32_t kind, const void* ctx, uint32_t* block, uint32_t* max_grid, uint32_t* per_cu) {
    if (!ctx || !block || !max_grid || !per_cu) return fail(PT_E_INVALID, "null argument");
    const QueryCtx* q = kind == PT_CTX_RAYQ    ? static_cast<const QueryCtx*>(static_cast<const pt_rayq*>(ctx))
                        : kind == PT_CTX_FEATQ ? static_cast<const QueryCtx*>(static_cast<const pt_featq*>(ctx))
                        : kind == PT_CTX_PATHQ ? static_cast<const QueryCtx*>(static_cast<const pt_pathq*>(ctx))
                        : kind == PT_CTX_PIXQ  ? static_cast<const QueryCtx*>(static_cast<const pt_pixq*>(ctx))
                                               : nullptr;
    if (!q) return fail(PT_E_INVALID, "unknown context kind");
    *block = q->block;
    *max_grid = q->max_grid;
    *per_cu = q->per_cu;
    return PT_OK;
}

int pt_selftest_gamma_table(const pt_scene* s, float* thr256) {
    if (!s || !s->prepared || !thr256) return fail(PT_E_INVALID, "scene not prepared");
    memcpy(thr256, s->thr, sizeof(s->thr));
    return PT_OK;
}

// pt_scene_load_mem in at most `stretches` stretches, and where they begin and end
int pt_selftest_scene_load_stretches(const char* text, size_t len, uint32_t stretches, pt_scene** out, uint64_t* cuts,
                                     uint32_t cap, uint32_t* n_cuts) {
    if (!out || !n_cuts || (!text && len) || stretches == 0 || stretches > 64) return fail(PT_E_INVALID, "bad argument");
    const std::vector<size_t> cut = pth::scene_stretch_cuts(text, len, stretches);
    *n_cuts = (uint32_t)cut.size();
    if (cuts) {
        if (cap < cut.size()) return fail(PT_E_INVALID, "cuts buffer too small");
        for (size_t i = 0; i < cut.size(); ++i) cuts[i] = cut[i];
    }
    auto* s = new pt_scene();
    try {
        pth::parse_scene_stretches(text, len, s->hs, stretches);
    } catch (const std::exception& e) {
        delete s;
        return fail(PT_E_SCENE, e.what());
    }
    *out = s;
    return PT_OK;
}

// the parse as Scene::Load leaves it (before pt_scene_prepare reorders the primitives)
int pt_selftest_scene_dump(const pt_scene* s, void* out, size_t cap, size_t* need, char* warnings, size_t warn_cap,
                           size_t* warn_need) {
    if (!s || !need || !warn_need) return fail(PT_E_INVALID, "null argument");
    if (s->prepared) return fail(PT_E_INVALID, "scene already prepared: its primitives are no longer in load order");
    const pth::HScene& h = s->hs;
    *need = 80 + 100 * h.prims.size();
    *warn_need = 0;
    for (const std::string& w : h.warnings) *warn_need += w.size() + 1;
    if (out) {
        if (cap < *need) return fail(PT_E_INVALID, "dump buffer too small");
        auto* b = static_cast<unsigned char*>(out);
        const uint32_t u[4] = {h.W, h.H, h.samples, h.depth};
        memcpy(b, u, 16); memcpy(b + 16, &h.fov_x, 4); memcpy(b + 20, h.bg, 12); memcpy(b + 32, h.cam_pos, 12);
        memcpy(b + 44, h.cam_right, 12); memcpy(b + 56, h.cam_up, 12); memcpy(b + 68, h.cam_fwd, 12);
        b += 80;
        for (const pth::HPrim& p : h.prims) {
            memcpy(b, &p.type, 4); memcpy(b + 4, p.a, 12); memcpy(b + 16, p.b, 12); memcpy(b + 28, p.c, 12);
            memcpy(b + 40, p.pos, 12); memcpy(b + 52, p.rot, 16); memcpy(b + 68, p.col, 12);
            memcpy(b + 80, p.emis, 12); memcpy(b + 92, &p.mat, 4); memcpy(b + 96, &p.ior, 4);
            b += 100;
        }
    }
    if (warnings) {
        if (warn_cap < *warn_need) return fail(PT_E_INVALID, "warnings buffer too small");
        for (const std::string& w : h.warnings) {
            memcpy(warnings, w.data(), w.size());
            warnings[w.size()] = '\n';
            warnings += w.size() + 1;
        }
    }
    return PT_OK;
}

static_assert(pt::MATH_LOGF == PT_MATH_LOGF && pt::MATH_RNG == PT_MATH_RNG && pt::MATH_NORMAL3 == PT_MATH_NORMAL3 &&
                  pt::MATH_COSINE == PT_MATH_COSINE && pt::MATH_FRESNEL == PT_MATH_FRESNEL &&
                  pt::MATH_RESOLVE == PT_MATH_RESOLVE && pt::MATH_ARITH == PT_MATH_ARITH && pt::MATH_N == 7u,
              "math ops: device and ABI numbering differ");

int pt_selftest_math(int device, uint32_t op, uint64_t n, const void* in, void* out) {
    if (op >= pt::MATH_N) return fail(PT_E_INVALID, "unknown math op");
    if (n == 0) return PT_OK;
    if (!in || !out) return fail(PT_E_INVALID, "null argument");
    if (n > (1ull << 26)) return fail(PT_E_INVALID, "more than 2^26 elements");
    // RNG: one output length for the whole call, the first element's
    uint32_t rng_n = 0;
    if (op == pt::MATH_RNG) {
        const pt::MathSeedIn* I = static_cast<const pt::MathSeedIn*>(in);
        rng_n = I[0].pre;
        if (rng_n == 0 || rng_n > 65536u) return fail(PT_E_INVALID, "RNG: 1 .. 65536 draws per stream");
        for (uint64_t i = 1; i < n; ++i)
            if (I[i].pre != rng_n) return fail(PT_E_INVALID, "RNG: every element asks for the same number of draws");
    }
    const size_t in_bytes = (size_t)n * pt::math_in_bytes(op), out_bytes = (size_t)n * pt::math_out_bytes(op, rng_n);
    if (in_bytes > (1ull << 31) || out_bytes > (1ull << 31)) return fail(PT_E_INVALID, "more than 2 GiB of records");
    float thr[256] = {0.f};
    if (op == pt::MATH_RESOLVE) pth::build_gamma_thresholds(thr);
    if (device < 0) {
        parallel_chunks((size_t)n, std::min(16u, std::max(1u, std::thread::hardware_concurrency())),
                        [&](size_t b, size_t e, unsigned) {
                            for (size_t i = b; i < e; ++i) pt::math_one(op, i, in, out, thr, rng_n);
                        });
        return PT_OK;
    }
    if (const int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    unsigned char* buf = nullptr;   // in | out | thr, each 256-B aligned
    const size_t o_out = (in_bytes + 255u) & ~(size_t)255u, o_thr = o_out + ((out_bytes + 255u) & ~(size_t)255u);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&buf), o_thr + sizeof(thr)));
    hipError_t e = hipMemcpy(buf, in, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + o_thr, thr, sizeof(thr), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = pt_launch_selftest_math(op, n, buf, buf + o_out, reinterpret_cast<const float*>(buf + o_thr), rng_n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, buf + o_out, out_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) return fail(PT_E_HIP, std::string("pt_selftest_math: ") + hipGetErrorString(e));
    return PT_OK;
}

}  // extern "C"
