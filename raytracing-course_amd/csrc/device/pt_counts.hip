// pt_counts.hip -- per-pixel sample counts in a session: the kernels around the
// ordinary pass that make its one target mean a count of each pixel's own.
//
//   k_counts_scan     per owned slot: its record's count; the largest and the smallest total the
//                     pixels would stand at, and the counts' sum (one atomic per wave and quantity)
//   k_counts_bias     per owned slot, after the host has read the scan: done = S2 - count, so that
//                     the pass to S2 runs the pixel for `count` samples; the slot's lag after it
//   k_counts_import   record -> slot as k_states_write, `done` at the records' largest count S2 and
//                     the record's distance below it in the lag table
//   k_counts_resolve  k_resolve with every pixel's own count, S - lag (the lost-chain check unchanged)
//
// A slot per lane and a tile per workgroup, as k_init and k_resolve; a record piece moved as one
// 16-B vector access.  Nothing here is on a pass's path: the engines run unchanged between them.
#include <hip/hip_runtime.h>

#include "pt_counts.h"
#include "pt_devutil.h"

namespace pt {

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ void __launch_bounds__(256) k_counts_scan(CountsParams P) {
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    const int64_t rec = count_record(P.tm, P.tile_rec, blockIdx.x, threadIdx.x);
    const bool own = rec >= 0;
    const uint32_t count = own ? P.counts[rec] : 0u;
    const unsigned long long total = own ? count_total(P.S, P.lag[slot], count) : 0ull;
    // (whole waves: the reductions are over 64 lanes)
    const unsigned long long tmax = wave_max_u64(total), nmin = wave_max_u64(own ? ~total : 0ull);
    wave_add_u64(P.res + CR_SUM, (unsigned long long)count);
    if ((threadIdx.x & 63u) == 0u && nmin != 0ull) {   // (a wave of padding lanes alone: nothing)
        atomicMax(P.res + CR_MAX_TOTAL, tmax);
        atomicMax(P.res + CR_NMIN_TOTAL, nmin);
    }
}

__global__ void __launch_bounds__(256) k_counts_bias(CountsParams P) {
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    const int64_t rec = count_record(P.tm, P.tile_rec, blockIdx.x, threadIdx.x);
    if (rec < 0) return;
    const uint32_t count = P.counts[rec];
    uint4 hot = P.st.rec[2u * slot];
    hot.w = count_done_before(P.S2, count);
    P.st.rec[2u * slot] = hot;
    P.lag[slot] = count_lag_after(P.S2, P.S, P.lag[slot], count);
}

__global__ void __launch_bounds__(256) k_counts_import(CountsParams P) {
    // (whole waves stay in the loop: wave_add_u64 is over 64 lanes)
    const unsigned long long rounds = (P.n + 255ull) / 256ull;
    for (unsigned long long r = blockIdx.x; r < rounds; r += gridDim.x) {
        const unsigned long long i = r * 256ull + threadIdx.x;
        uint32_t lag = 0u;
        if (i < P.n) {
            const uint4* rec = reinterpret_cast<const uint4*>(P.state + i);
            const uint4 a = rec[0];
            const int64_t slot = state_slot(P.tm, P.n_tiles_local, a.z, a.w, a.x);
            if (slot >= 0) {
                uint4 hot, sum;
                state_to_slot(a, rec[1], P.tm.W, hot, sum);
                lag = P.S2 - hot.w;   // (hot.w: the record's samples, at most S2, their maximum)
                hot.w = P.S2;
                P.st.rec[2u * (uint32_t)slot] = hot;
                P.st.rec[2u * (uint32_t)slot + 1u] = sum;
                P.lag[(uint32_t)slot] = lag;
            }
        }
        wave_add_u64(P.res + SR_LAG_SUM, (unsigned long long)lag);
    }
}

__global__ void __launch_bounds__(256) k_counts_resolve(CountsParams P) {
    __shared__ float thr[256];
    thr[threadIdx.x] = P.thr[threadIdx.x];
    __syncthreads();
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    // k_resolve's lost-chain check: every owned pixel's `done` at the session's virtual count
    uint32_t px, py;
    const bool pix = slot_pixel(P.tm, blockIdx.x, threadIdx.x, px, py);
    wave_add_u64(ctr_copy(P.counters) + CTR_SHORT, pix && load_hot(P.st, slot).done != P.S ? 1ull : 0ull);
    // (a padding lane's lag is 0 and its sum 0: S >= 1 here, the host refuses a pixel without samples)
    const uint32_t samples = count_taken(P.S, P.lag[slot]);
    const f3 s = load_sum(P.st, slot);
    const float sum[3] = {s.x, s.y, s.z};
    float m[3];
    uint8_t* o = P.out + (size_t)slot * 3u;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)resolve_channel(sum[c], samples, thr, m[c]);
    if (P.rad) {
#pragma unroll
        for (int c = 0; c < 3; ++c) P.rad[(size_t)slot * 3u + c] = m[c];
    }
}

}  // namespace pt

// ---------------------------------------------------------------- launchers
hipError_t pt_launch_counts_scan(const pt::CountsParams& p, hipStream_t s) {
    hipLaunchKernelGGL(pt::k_counts_scan, dim3(p.n_tiles_local), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t pt_launch_counts_bias(const pt::CountsParams& p, hipStream_t s) {
    hipLaunchKernelGGL(pt::k_counts_bias, dim3(p.n_tiles_local), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t pt_launch_counts_import(const pt::CountsParams& p, hipStream_t s) {
    const unsigned long long wgs = (p.n + 255ull) / 256ull;
    hipLaunchKernelGGL(pt::k_counts_import, dim3((uint32_t)(wgs < 2048ull ? wgs : 2048ull)), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t pt_launch_counts_resolve(const pt::CountsParams& p, hipStream_t s) {
    hipLaunchKernelGGL(pt::k_counts_resolve, dim3(p.n_tiles_local), dim3(256), 0, s, p);
    return hipGetLastError();
}
