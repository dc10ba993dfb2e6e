// pt_noise.hip -- a session's own noise estimate: the kernels that remember every
// pixel's sum at an earlier count, turn its movement since into a noise figure, and plan an adaptive
// step from the figures.  The step itself is pt_counts.hip's k_counts_bias and the ordinary pass.
//
//   k_noise_mark      per owned slot: mark := (sum, own count), one 16-B store
//   k_noise_plan      per owned slot: its noise from its sum, its lag and its mark; the tile's hot
//                     flags exchanged through LDS (four ballots, one barrier) for the neighbour rule;
//                     noise and / or count out by record; the result words and the three words
//                     k_counts_scan would make of these counts, summed per lane over the workgroup's
//                     tiles and then one atomic per wave and quantity.  It only reads the session.
//   k_noise_commit    per owned slot whose accepted count is above 0, after the host has read the
//                     plan: mark := (sum, own count)
//
// A slot per lane and a tile per workgroup (the plan: per trip of a workgroup), as k_init,
// k_counts_scan and k_resolve.  Bandwidth-bound:
// 36 B read per slot (sum, lag, mark), at most 8 B written per record.
#include <hip/hip_runtime.h>

#include "pt_devutil.h"
#include "pt_noise.h"

namespace pt {

__device__ __forceinline__ unsigned long long noise_wave_max(unsigned long long v) {
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ void noise_wave_atomic_max(unsigned long long* dst, unsigned long long v) {
    v = noise_wave_max(v);
    if ((threadIdx.x & 63u) == 0u && v != 0ull) atomicMax(dst, v);
}

// a slot's own count (a session that was never ragged has no lag table)
__device__ __forceinline__ uint32_t noise_taken(const NoiseParams& P, uint32_t slot) {
    return count_taken(P.S, P.lag ? P.lag[slot] : 0u);
}

__global__ void __launch_bounds__(256) k_noise_mark(NoiseParams P) {
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (count_record(P.tm, P.tile_rec, blockIdx.x, threadIdx.x) < 0) return;
    const uint4 sum = P.st.rec[2u * slot + 1u];
    P.mark[slot] = make_uint4(sum.x, sum.y, sum.z, noise_taken(P, slot));
}

__global__ void __launch_bounds__(256) k_noise_plan(NoiseParams P) {
    // two sets of the tile's hot words: a tile's ballots land while a slow wave still reads the last tile's
    __shared__ unsigned long long hot_words[2][4];
    // a lane's share of the result, summed over the workgroup's tiles
    uint32_t refined = 0u, unmarked = 0u, nonfinite = 0u, capped = 0u, worst = 0u;
    unsigned long long samples = 0ull, total_max = 0ull, total_nmin = 0ull;
    // (whole workgroups stay in the loop: the ballot, the barrier and the reductions are over every lane;
    // a padding lane reads its slot like any other -- the tables have n_slots entries -- and adds nothing)
    uint32_t set = 0u;
    for (uint32_t tile = blockIdx.x; tile < P.n_tiles_local; tile += gridDim.x, set ^= 1u) {
        const uint32_t slot = tile * 256u + threadIdx.x;
        const int64_t rec = count_record(P.tm, P.tile_rec, tile, threadIdx.x);
        const bool own = rec >= 0;
        const uint4 sw = P.st.rec[2u * slot + 1u];
        const uint4 mw = P.mark[slot];
        const uint32_t lag = P.lag ? P.lag[slot] : 0u, k = count_taken(P.S, lag), a = mw.w;
        const float sum[3] = {u2f(sw.x), u2f(sw.y), u2f(sw.z)}, msum[3] = {u2f(mw.x), u2f(mw.y), u2f(mw.z)};
        const bool estimate = noise_has_estimate(k, a);
        const float noise = noise_of(sum, k, msum, a);
        if (own && P.noise) P.noise[rec] = noise;
        if (!P.classify) continue;   // (uniform: the noise alone)
        const bool hot = own && noise_hot(noise, P.o.threshold);
        const unsigned long long ballot = __ballot(hot);
        if ((threadIdx.x & 63u) == 0u) hot_words[set][threadIdx.x >> 6] = ballot;
        __syncthreads();
        bool hot2 = hot;
        if (P.o.spread) {
            const unsigned long long w[4] = {hot_words[set][0], hot_words[set][1], hot_words[set][2], hot_words[set][3]};
            hot2 = own && noise_spread(w, threadIdx.x);
        }
        if (!own) continue;
        const NoisePixel px = noise_pixel(noise, estimate, hot2, k, P.o);
        if (P.counts) P.counts[rec] = px.count;
        refined += px.count ? 1u : 0u;
        samples += px.count;
        unmarked += px.unmarked ? 1u : 0u;
        nonfinite += px.nan ? 1u : 0u;
        capped += px.capped ? 1u : 0u;
        const uint32_t wb = noise_worst_bits(noise, estimate);
        worst = wb > worst ? wb : worst;
        // k_counts_scan's words for these counts (the complement of a total is never 0: a total is a u32)
        const unsigned long long total = count_total(P.S, lag, px.count);
        total_max = total > total_max ? total : total_max;
        total_nmin = ~total > total_nmin ? ~total : total_nmin;
    }
    if (!P.classify) return;
    // one atomic per wave and quantity for the whole launch: same-address atomics from the whole chip
    // serialise (pt_devutil.h xcc_id), and a wave per tile would make eight of them per 64 pixels
    wave_add_u64(P.res + NR_REFINED, refined);
    wave_add_u64(P.res + NR_SAMPLES, samples);
    wave_add_u64(P.res + NR_UNMARKED, unmarked);
    wave_add_u64(P.res + NR_NONFINITE, nonfinite);
    wave_add_u64(P.res + NR_CAPPED, capped);
    noise_wave_atomic_max(P.res + NR_WORST, worst);
    noise_wave_atomic_max(P.res + NR_MAX_TOTAL, total_max);
    noise_wave_atomic_max(P.res + NR_NMIN_TOTAL, total_nmin);
}

__global__ void __launch_bounds__(256) k_noise_commit(NoiseParams P) {
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    const int64_t rec = count_record(P.tm, P.tile_rec, blockIdx.x, threadIdx.x);
    if (rec < 0 || P.counts[rec] == 0u) return;
    const uint4 sum = P.st.rec[2u * slot + 1u];
    P.mark[slot] = make_uint4(sum.x, sum.y, sum.z, noise_taken(P, slot));
}

}  // namespace pt

// ---------------------------------------------------------------- launchers
hipError_t pt_launch_noise_mark(const pt::NoiseParams& p, hipStream_t s) {
    hipLaunchKernelGGL(pt::k_noise_mark, dim3(p.n_tiles_local), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t pt_launch_noise_plan(const pt::NoiseParams& p, hipStream_t s) {
    // (a workgroup takes every kPlanGrid-th tile: four workgroups per compute unit of an MI355X)
    constexpr uint32_t kPlanGrid = 1024u;
    hipLaunchKernelGGL(pt::k_noise_plan, dim3(p.n_tiles_local < kPlanGrid ? p.n_tiles_local : kPlanGrid), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t pt_launch_noise_commit(const pt::NoiseParams& p, hipStream_t s) {
    hipLaunchKernelGGL(pt::k_noise_commit, dim3(p.n_tiles_local), dim3(256), 0, s, p);
    return hipGetLastError();
}
