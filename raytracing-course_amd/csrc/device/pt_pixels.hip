// pt_pixels.hip -- the pixel-sample engine: Scene::Sample's loop (src/scene.cpp:189-203) for
// pixels the caller lists, each record with its own number of further samples on its own random
// stream, the state read and written in place.  Per new sample: the two jitter
// draws and the camera ray (camera_sample), RayTrace as k_paths runs it (pt_query.h's closest-hit
// query; pt_trace.h's shade_vertex and fold_vertex, in trace_path_with's order), sum = sum + that,
// samples + 1 -- all on the record's one stream, which the next sample finds as this one left it.
//   k_pixels  a lane per record, with refill: persistent waves, every trip advances each running
//             lane's query by one q_step; once enough lanes wait, a service step shades the
//             finished queries' vertices, folds the ended paths into their records' sums, starts
//             those records' next samples and takes new records
// A record's samples are serial (as a pixel's are in the reference): a run takes at least as long
// as its longest record.  A query the replay does not take (Q_EXACT) is answered in the service
// step by the exact stack DFS, on the lane's own LDS words.
#include <hip/hip_runtime.h>

#include "pt_batch.h"
#include "pt_pixels.h"
#include "pt_wave.h"

namespace pt {

// the wave's statistics, and the samples its records finished
struct PixelStats : QStats {
    uint32_t samples = 0u;
    __device__ __forceinline__ void flush(unsigned long long* counters) const {
        wave_add_u64(QStats::flush(counters) + PT_PIXELS_CTR_SAMPLES, samples);
    }
};

// a lane's record: its running query, its stream, its pixel and where it is in Sample's loop and
// in RayTrace's recursion (whose depth argument at the current ray is depth - nv).  The sum and
// the sample count stay in the record's second piece in memory: the lane owns the record for the
// run, and a path end is rare next to a trip.
struct PixelLane {
    Query q;
    Rng R;
    uint32_t idx;     // the record
    uint32_t x, y;    // its pixel
    uint32_t left;    // samples still to finish, the running one included
    uint32_t nv;      // the running sample's vertices so far (fold records written)
};

// a record's two 16-B pieces
__device__ __forceinline__ uint4* rec_piece(const PixelsParams& P, uint32_t i, uint32_t k) {
    return reinterpret_cast<uint4*>(P.state) + 2u * (size_t)i + k;
}
// piece 0 goes back: the stream as the record's last sample left it
__device__ __forceinline__ void store_stream(const PixelsParams& P, uint32_t i, const Rng& R, uint32_t x, uint32_t y) {
    *rec_piece(P, i, 0u) = make_uint4(pixel_rng_word(R), f2u(pixel_rng_saved(R)), x, y);   // one 16-B store
}
__device__ __forceinline__ uint32_t rec_count(const PixelsParams& P, uint32_t i) {
    return P.counts ? P.counts[i] : P.spp;
}
// Sample's loop body at RAY_DEPTH 0, `count` times: the jitter draws happen, RayTrace returns
// black before it draws or intersects anything, and the sum gets + 0
__device__ __forceinline__ void depth0_samples(const PixelsParams& P, Rng& R, uint32_t x, uint32_t y, uint32_t count,
                                               f3& sum) {
    for (uint32_t k = 0u; k < count; ++k) {
        (void)camera_sample(P.cam, R, x, y);
        sum = sum + mk3(0.f, 0.f, 0.f);
    }
}

// An ended path's value (fold_path) into its record: summary = summary + RayTrace(..) (src/scene.cpp:199), and the sample counted.
// One 16-B load and one 16-B store of the record's second piece, which no other lane touches.
__device__ __forceinline__ void add_sample(const PixelsParams& P, uint32_t i, f3 Lr) {
    uint4* p = rec_piece(P, i, 1u);
    const uint4 b = *p;
    const f3 sum = mk3(u2f(b.x), u2f(b.y), u2f(b.z)) + Lr;
    *p = make_uint4(f2u(sum.x), f2u(sum.y), f2u(sum.z), b.w + 1u);
}

// The occupancy the compiler is held to, in waves per SIMD (`make DEFS=-DPT_PIXELS_WAVES_PER_EU=N`
// builds another; 0 leaves the choice to the compiler: the table in DESIGN.md §4.7)
#ifndef PT_PIXELS_WAVES_PER_EU
#define PT_PIXELS_WAVES_PER_EU 3
#endif
#if PT_PIXELS_WAVES_PER_EU > 0
#define PT_PIXELS_OCC __attribute__((amdgpu_waves_per_eu(PT_PIXELS_WAVES_PER_EU, PT_PIXELS_WAVES_PER_EU)))
#else
#define PT_PIXELS_OCC
#endif

#ifndef PT_PIXELS_PLAIN
__global__ void __launch_bounds__(256) PT_PIXELS_OCC k_pixels(PixelsParams P) {
    extern __shared__ uint32_t lds_stack[];
    const LaneStack ls = lane_stack(P, lds_stack);
    LdsMemN<64u> stk = ls.aux();
    HbmVStore vs = lane_fold(P);
    PixelStats st;
    PixelLane L;
    L.q.phase = Q_DONE;
    bool have = false;        // this lane holds a record with samples left
    WaveTake T{0u, true, 0ull};   // the wave's reservation of record indices (wave-uniform)
    // Why this loop ends, from the wave's own state alone (it waits for no other wave or workgroup
    // anywhere: the only shared word is the work counter, which is only ever added to; a record,
    // the fold records and the LDS column are one lane's own):
    //   * a pull adds `batch` >= 64 to the work counter, so after at most n / batch + 1 pulls by
    //     all waves together every pull returns a value >= n and `more` turns false for good;
    //   * a lane that holds a record advances its query by one q_step per trip, and a query takes a
    //     finite number of steps (the state machine q_run loops over);
    //   * a path has at most RAY_DEPTH queries: each finished query's vertex raises `nv`, and the
    //     path ends at nv = RAY_DEPTH, at a miss or where the vertex ends it; the exact DFS a
    //     Q_EXACT query runs in the service step visits each reference node at most once;
    //   * a record has finitely many samples: `left` is its count (< 2^32) when the lane takes it,
    //     every ended path lowers it by one, and nothing raises it; at left = 0 the record is
    //     written back and the lane is empty -- a lane takes a new record only then, so it never
    //     holds two, and a record with count 0 (or any record at RAY_DEPTH 0, whose samples are a
    //     bounded loop of jitter draws) is finished where it is taken;
    //   * a trip on which no lane runs is a service step, which gives every waiting lane its
    //     vertex -- after which the lane runs again (the child ray, or its record's next sample)
    //     or is empty -- and every empty lane a record while the reservation lasts, so it either
    //     starts queries, or hands out records (the reservation shrinks, or a pull moves the
    //     counter on), or finds nothing left and leaves;
    //   * so the trips are bounded by the pulls, plus the steps of the queries of the samples of
    //     the records the wave took.
    for (;;) {
        const bool run = have && q_running(L.q.phase);
        const unsigned long long mrun = __ballot(run);
        // The service step, once `service` lanes wait (a finished query, or empty) or none runs.
        // Not on every trip: a vertex recomputes its hit, samples and writes a fold record, a
        // taking lane tests the planes, each behind dependent loads the whole wave waits for.
        if (64u - (uint32_t)__popcll(mrun) >= P.service || mrun == 0ull) {
            Ray ray;
            bool start = false;   // this lane begins the query of `ray` below ...
            bool first = false;   // ... a sample's first: `ray` is the camera ray still to be drawn
            if (have && !run) {
                f3 leaf;
                start = lane_vertex(P.S, P.depth, L.q, L.R, L.nv, ls, vs, st, ray, leaf);
                if (!start) {
                    add_sample(P, L.idx, fold_path(P.S, L.nv, vs, leaf));
                    st.samples++;
                    if (--L.left != 0u) {
                        start = first = true;
                    } else {
                        store_stream(P, L.idx, L.R, L.x, L.y);
                        have = false;
                    }
                }
            }
            if (T.dry()) T.pull(P);
            if (T.rleft != 0u) {
                const unsigned long long m = __ballot(!have);
                const uint32_t k = lanes_below(m);
                if (!have && T.holds(k)) {
                    // the next record: its first piece and its count (count 0: not a byte of it changes)
                    const uint32_t i = (uint32_t)T.item(k);
                    const uint32_t count = rec_count(P, i);
                    if (count != 0u) {
                        const uint4 a = *rec_piece(P, i, 0u);
                        L.R = pixel_rng(a.x, u2f(a.y));
                        L.x = a.z;
                        L.y = a.w;
                        if (P.depth != 0u) {
                            L.idx = i;
                            L.left = count;
                            have = start = first = true;
                        } else {
                            uint4* p = rec_piece(P, i, 1u);
                            const uint4 b = *p;
                            f3 sum = mk3(u2f(b.x), u2f(b.y), u2f(b.z));
                            depth0_samples(P, L.R, L.x, L.y, count, sum);
                            *p = make_uint4(f2u(sum.x), f2u(sum.y), f2u(sum.z), b.w + count);
                            store_stream(P, i, L.R, L.x, L.y);
                            st.samples += count;
                        }
                    }
                }
                T.advance(m);
            }
            // (one copy of the jitter and camera ray for the records' first and later samples, and
            // one of the planes and the set-up for the child rays and the camera rays)
            if (first) {
                // (the camera block read here, not held in SGPRs across the persistent loop)
                const PixelsParams& K = karg<PixelsParams>();
                ray = camera_sample(K.cam, L.R, L.x, L.y);
                L.nv = 0u;
            }
            if (start) start_query(P.S, ray, L.q, st);
            if (T.spent() && __ballot(have) == 0ull) break;
        }
        if (have && q_running(L.q.phase)) q_step(P.S, L.q, st.C, stk);
    }
    st.flush(P.counters);
}
#else
// The plain form (`make DEFS=-DPT_PIXELS_PLAIN`, measured against the refill form by
// tools/pixels_bench.py): a lane per record, grid-stride, the whole record in the lane -- each
// wave as slow as its longest record
__global__ void __launch_bounds__(256) PT_PIXELS_OCC k_pixels(PixelsParams P) {
    extern __shared__ uint32_t lds_stack[];
    const LaneStack ls = lane_stack(P, lds_stack);
    LdsMemN<64u> stk = ls.aux();
    HbmVStore vs = lane_fold(P);
    PixelStats st;
    Query q;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += stride) {
        const uint32_t count = rec_count(P, (uint32_t)i);
        if (count == 0u) continue;
        const uint4 a = *rec_piece(P, (uint32_t)i, 0u), b = *rec_piece(P, (uint32_t)i, 1u);
        Rng R = pixel_rng(a.x, u2f(a.y));
        f3 sum = mk3(u2f(b.x), u2f(b.y), u2f(b.z));
        if (P.depth == 0u) depth0_samples(P, R, a.z, a.w, count, sum);
        // (ends: a record has `count` samples, a path at most RAY_DEPTH queries, a query finitely many steps)
        for (uint32_t k = 0u; k < count && P.depth != 0u; ++k) {
            Ray ray = camera_sample(P.cam, R, a.z, a.w);
            uint32_t nv = 0u;
            for (;;) {
                start_query(P.S, ray, q, st);
                while (q_running(q.phase)) q_step(P.S, q, st.C, stk);
                f3 leaf;
                if (lane_vertex(P.S, P.depth, q, R, nv, ls, vs, st, ray, leaf)) continue;
                sum = sum + fold_path(P.S, nv, vs, leaf);
                break;
            }
        }
        st.samples += count;
        *rec_piece(P, (uint32_t)i, 1u) = make_uint4(f2u(sum.x), f2u(sum.y), f2u(sum.z), b.w + count);
        store_stream(P, (uint32_t)i, R, a.z, a.w);
    }
    st.flush(P.counters);
}
#endif

}  // namespace pt

hipError_t pt_pixels_occupancy(uint32_t block, uint32_t aux_words, uint32_t dfs_words, int* per_cu) {
    return pt::lanes_occupancy(pt::k_pixels, block, aux_words, dfs_words, per_cu);
}

hipError_t pt_launch_pixels(const pt::PixelsParams& p, uint32_t grid, uint32_t block, hipStream_t s, hipEvent_t e0,
                            hipEvent_t e1) {
    return pt::launch_lanes(pt::k_pixels, p, PT_PIXELS_CTL_BYTES, grid, block, s, e0, e1);
}
