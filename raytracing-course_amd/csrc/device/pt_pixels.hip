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

#include "pt_pixels.h"
#include "pt_wave.h"

namespace pt {

// the statistics a wave gathered, flushed once (one atomic per counter and wave)
struct PixelStats {
    QCounts C{0u, 0u, 0u, 0u};
    uint32_t rays = 0u, err = 0u, exact = 0u, exact_ray = 0u, samples = 0u;
    __device__ __forceinline__ void flush(unsigned long long* counters) const {
        unsigned long long* ctr = ctr_copy(counters);
        wave_add_u64(ctr + CTR_RAYS, rays);
        wave_add_u64(ctr + CTR_NODES, C.nodes);
        wave_add_u64(ctr + CTR_PTESTS, C.ptests);
        wave_add_u64(ctr + CTR_PLANES, C.planes);
        wave_add_u64(ctr + CTR_ERRORS, err);
        wave_add_u64(ctr + CTR_AUX, C.aux);
        wave_add_u64(ctr + CTR_FALLBACKS, exact);
        wave_add_u64(ctr + CTR_FALLBACKS_RAY, exact_ray);
        wave_add_u64(ctr + PT_PIXELS_CTR_SAMPLES, samples);
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

// the lane's LDS column: the query's aux stack, or (the aux stack is dead by then) the exact DFS's
struct PixelStack {
    uint32_t* base;
    uint32_t aux_words, dfs_words;
    __device__ __forceinline__ LdsMemN<64u> aux() const { return LdsMemN<64u>{base, aux_words, aux_words}; }
    __device__ __forceinline__ LdsMemN<64u> dfs() const { return LdsMemN<64u>{base, dfs_words, dfs_words}; }
};
__device__ __forceinline__ PixelStack pixel_stack(const PixelsParams& P, uint32_t* lds) {
    const uint32_t words = (P.aux_words > P.dfs_words ? P.aux_words : P.dfs_words) + 1u;
    // [word][lane] per wave
    return PixelStack{lds + (threadIdx.x >> 6) * 64u * words + (threadIdx.x & 63u), P.aux_words, P.dfs_words};
}
__device__ __forceinline__ HbmVStore pixel_fold(const PixelsParams& P) {
    return HbmVStore{P.fold + ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * P.depth};
}

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

// RayIntersection's start for `ray`: the planes, then the BVH query's set-up
__device__ __forceinline__ void start_query(const PixelsParams& P, const Ray& ray, Query& q, PixelStats& st) {
    float pt;
    int pid;
    q_planes(P.S, ray, pt, pid);
    st.C.planes += P.S.n_planes;
    q_init(P.S, ray, pt, pid, q);
    st.rays++;
    if (q.phase == Q_EXACT) st.exact_ray++;   // a non-finite ray: the exact DFS by design
}

// The vertex of a query that left Q_AUX / Q_REPLAY (trace_path_with's loop body after the query).
// The hit is recomputed from its primitive as q_run does (the probe computes t only); a Q_EXACT
// query is answered here by the exact DFS.  True: the path goes on with `ray`; false: it has
// ended with `leaf` below its nv fold records.
__device__ __forceinline__ bool sample_vertex(const PixelsParams& P, const Query& q, Rng& R, uint32_t& nv,
                                              const PixelStack& ls, HbmVStore& vs, PixelStats& st, Ray& ray, f3& leaf) {
    ray = q.ray;
    Hit h;
    int id;
    if (q.phase == Q_EXACT) {
        LdsMemN<64u> xs = ls.dfs();
        id = q_exact(P.S, ray, xs, h, st.C);
        st.exact++;
    } else {
        id = q.res_id;
        if (id >= 0) {
            const bool ok = prim_intersect(P.S.prims[id], ray, h);
            if (!ok || f2u(h.t) != f2u(q.res_t)) st.err++;   // must never happen (the tests check)
        }
    }
    if (id < 0) {
        leaf = P.S.bg;
        return false;
    }
    uint32_t idm;
    float s1, s2;
    const bool cont = shade_vertex(P.S, R, ray, h, id, idm, s1, s2);
    vs.put(nv++, idm, s1, s2);   // nv < depth: a record follows a query, and a path has at most depth queries
    leaf = mk3(0.f, 0.f, 0.f);
    return cont && nv != P.depth;   // RayTrace(.., 0) = 0
}

// an ended path's value: the backward fold, deepest vertex first (trace_path_with's order)
__device__ __forceinline__ f3 fold_sample(const PixelsParams& P, uint32_t nv, const HbmVStore& vs, f3 leaf) {
    f3 Lr = leaf;
    for (uint32_t k = nv; k > 0u;) {
        --k;
        uint32_t idm;
        float s1, s2;
        vs.get(k, idm, s1, s2);
        Lr = fold_vertex(P.S, Lr, idm, s1, s2);
    }
    return Lr;
}
// ... into its record: summary = summary + RayTrace(..) (src/scene.cpp:199), and the sample counted.
// One 16-B load and one 16-B store of the record's second piece, which no other lane touches.
__device__ __forceinline__ void add_sample(const PixelsParams& P, uint32_t i, f3 Lr) {
    uint4* p = rec_piece(P, i, 1u);
    const uint4 b = *p;
    const f3 sum = mk3(u2f(b.x), u2f(b.y), u2f(b.z)) + Lr;
    *p = make_uint4(f2u(sum.x), f2u(sum.y), f2u(sum.z), b.w + 1u);
}

__device__ __forceinline__ bool q_running(const Query& q) { return q.phase == Q_AUX || q.phase == Q_REPLAY; }

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
    const uint32_t lane = threadIdx.x & 63u;
    const PixelStack ls = pixel_stack(P, lds_stack);
    LdsMemN<64u> stk = ls.aux();
    HbmVStore vs = pixel_fold(P);
    PixelStats st;
    PixelLane L;
    L.q.phase = Q_DONE;
    bool have = false;        // this lane holds a record with samples left
    // the wave's reservation [rnext, rnext + rleft) of record indices, and whether the work counter
    // may still be below n (all three wave-uniform)
    unsigned long long rnext = 0ull;
    uint32_t rleft = 0u;
    bool more = true;
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
        const bool run = have && q_running(L.q);
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
                start = sample_vertex(P, L.q, L.R, L.nv, ls, vs, st, ray, leaf);
                if (!start) {
                    add_sample(P, L.idx, fold_sample(P, L.nv, vs, leaf));
                    st.samples++;
                    if (--L.left != 0u) {
                        start = first = true;
                    } else {
                        store_stream(P, L.idx, L.R, L.x, L.y);
                        have = false;
                    }
                }
            }
            if (rleft == 0u && more) {
                // one atomic per pull, by one lane, for the whole wave
                unsigned long long got = 0ull;
                if (lane == 0u) got = atomicAdd(P.head, (unsigned long long)P.batch);
                // (lane 0's value in scalar registers: the reservation is wave-uniform)
                const unsigned long long base =
                    (unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(got >> 32)) << 32 |
                    __builtin_amdgcn_readfirstlane((uint32_t)got);
                rnext = base;
                rleft = base < P.n ? (uint32_t)(P.n - base < P.batch ? P.n - base : P.batch) : 0u;
                more = base + P.batch < P.n;
            }
            if (rleft != 0u) {
                const unsigned long long m = __ballot(!have);
                const uint32_t k = lanes_below(m);
                if (!have && k < rleft) {
                    // the next record: its first piece and its count (count 0: not a byte of it changes)
                    const uint32_t i = (uint32_t)(rnext + k);
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
                const uint32_t took = (uint32_t)__popcll(m) < rleft ? (uint32_t)__popcll(m) : rleft;
                rnext += took;
                rleft -= took;
            }
            // (one copy of the jitter and camera ray for the records' first and later samples, and
            // one of the planes and the set-up for the child rays and the camera rays)
            if (first) {
                // (the camera block read here, not held in SGPRs across the persistent loop)
                const PixelsParams& K = karg<PixelsParams>();
                ray = camera_sample(K.cam, L.R, L.x, L.y);
                L.nv = 0u;
            }
            if (start) start_query(P, ray, L.q, st);
            if (rleft == 0u && !more && __ballot(have) == 0ull) break;
        }
        if (have && q_running(L.q)) q_step(P.S, L.q, st.C, stk);
    }
    st.flush(P.counters);
}
#else
// The plain form (`make DEFS=-DPT_PIXELS_PLAIN`, measured against the refill form by
// tools/pixels_bench.py): a lane per record, grid-stride, the whole record in the lane -- each
// wave as slow as its longest record
__global__ void __launch_bounds__(256) PT_PIXELS_OCC k_pixels(PixelsParams P) {
    extern __shared__ uint32_t lds_stack[];
    const PixelStack ls = pixel_stack(P, lds_stack);
    LdsMemN<64u> stk = ls.aux();
    HbmVStore vs = pixel_fold(P);
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
                start_query(P, ray, q, st);
                while (q_running(q)) q_step(P.S, q, st.C, stk);
                f3 leaf;
                if (sample_vertex(P, q, R, nv, ls, vs, st, ray, leaf)) continue;
                sum = sum + fold_sample(P, nv, vs, leaf);
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

hipError_t pt_pixels_occupancy(uint32_t block, size_t lds_bytes, int* per_cu) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, pt::k_pixels, (int)block, lds_bytes);
}

hipError_t pt_launch_pixels(const pt::PixelsParams& p, uint32_t grid, uint32_t block, hipStream_t s, hipEvent_t e0,
                            hipEvent_t e1) {
    hipError_t e = hipMemsetAsync(p.head, 0, PT_PIXELS_CTL_BYTES, s);
    if (e != hipSuccess) return e;
    if (e0 && (e = hipEventRecord(e0, s)) != hipSuccess) return e;
    const uint32_t words = (p.aux_words > p.dfs_words ? p.aux_words : p.dfs_words) + 1u;
    hipLaunchKernelGGL(pt::k_pixels, dim3(grid), dim3(block), (block / 64u) * 64u * 4u * words, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return e1 ? hipEventRecord(e1, s) : hipSuccess;
}
