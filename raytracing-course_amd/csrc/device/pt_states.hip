// pt_states.hip -- a session's pixels out as pixel states and in again.
//
//   k_states_export  slot -> record: every owned pixel's state, in slot order without the edge
//                    tiles' padding lanes
//   k_states_mark    per record: whose it is (pt_states.h state_slot); a taken record marks its slot;
//                    the taken records' count and sample range, the refusals' counts
//   k_states_check   per owned slot: marked exactly once?
//   k_states_write   record -> slot, the taken records (after the host has read the checks' result)
//
// One record or slot per lane, a record moved as two 16-B pieces.  Nothing here is on a render's path.
#include <hip/hip_runtime.h>

#include "pt_devutil.h"
#include "pt_states.h"

namespace pt {

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ void __launch_bounds__(256) k_states_export(StatesParams P) {
    const uint32_t tile = blockIdx.x, lane = threadIdx.x;
    uint32_t x, y;
    if (!slot_pixel(P.tm, tile, lane, x, y)) return;
    const uint32_t slot = tile * 256u + lane;
    const uint32_t w = state_tile_width(P.tm, P.tm.gtile[tile]);
    uint4 a, b;
    slot_to_state(P.st.rec[2u * slot], P.st.rec[2u * slot + 1u], x, y, a, b);
    if (P.lag) b.w -= P.lag[slot];   // (a ragged session: `done` is the session's virtual count)
    uint4* out = reinterpret_cast<uint4*>(P.state + ((size_t)P.tile_rec[tile] + (lane >> 4) * w + (lane & 15u)));
    out[0] = a;
    out[1] = b;
}

__global__ void __launch_bounds__(256) k_states_mark(StatesParams P) {
    // (whole waves stay in the loop: the reductions below are over 64 lanes)
    const unsigned long long rounds = (P.n + 255ull) / 256ull;
    for (unsigned long long r = blockIdx.x; r < rounds; r += gridDim.x) {
        const unsigned long long i = r * 256ull + threadIdx.x;
        int64_t slot = STATE_FOREIGN;
        uint32_t samples = 0u;
        if (i < P.n) {
            const uint4* rec = reinterpret_cast<const uint4*>(P.state + i);
            const uint4 a = rec[0];
            slot = state_slot(P.tm, P.n_tiles_local, a.z, a.w, a.x);
            if (slot >= 0) {
                samples = rec[1].w;
                atomicAdd(P.mark + (uint32_t)slot, 1u);
            }
        }
        const bool take = slot >= 0;
        const unsigned long long taken = wave_sum_u64(take ? 1ull : 0ull);
        const unsigned long long outside = wave_sum_u64(slot == STATE_OUTSIDE ? 1ull : 0ull);
        const unsigned long long bad = wave_sum_u64(slot == STATE_BAD_RNG ? 1ull : 0ull);
        const uint32_t smax = wave_max_u32(take ? samples : 0u);
        const uint32_t nmin = wave_max_u32(take ? ~samples : 0u);
        if ((threadIdx.x & 63u) == 0u) {
            if (taken) {
                atomicAdd(P.res + SR_TAKEN, taken);
                atomicMax(P.res + SR_MAX, (unsigned long long)smax);
                atomicMax(P.res + SR_NMIN, (unsigned long long)nmin);
            }
            if (outside) atomicAdd(P.res + SR_OUTSIDE, outside);
            if (bad) atomicAdd(P.res + SR_BAD_RNG, bad);
        }
    }
}

__global__ void __launch_bounds__(256) k_states_check(StatesParams P) {
    uint32_t x, y;
    const bool own = slot_pixel(P.tm, blockIdx.x, threadIdx.x, x, y);
    wave_add_u64(P.res + SR_MISMARKED, own && P.mark[blockIdx.x * 256u + threadIdx.x] != 1u ? 1ull : 0ull);
}

__global__ void __launch_bounds__(256) k_states_write(StatesParams P) {
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < P.n; i += gridDim.x * 256ull) {
        const uint4* rec = reinterpret_cast<const uint4*>(P.state + i);
        const uint4 a = rec[0];
        const int64_t slot = state_slot(P.tm, P.n_tiles_local, a.z, a.w, a.x);
        if (slot < 0) continue;
        uint4 hot, sum;
        state_to_slot(a, rec[1], P.tm.W, hot, sum);
        P.st.rec[2u * (uint32_t)slot] = hot;
        P.st.rec[2u * (uint32_t)slot + 1u] = sum;
    }
}

}  // namespace pt

// ---------------------------------------------------------------- launchers
namespace {
// workgroups for n records: a record per lane, grid-stride past 2,048 workgroups
uint32_t record_grid(unsigned long long n) { return (uint32_t)((n + 255ull) / 256ull < 2048ull ? (n + 255ull) / 256ull : 2048ull); }
}  // namespace

hipError_t pt_launch_states_export(const pt::StatesParams& p, hipStream_t s) {
    hipLaunchKernelGGL(pt::k_states_export, dim3(p.n_tiles_local), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t pt_launch_states_mark(const pt::StatesParams& p, hipStream_t s) {
    hipLaunchKernelGGL(pt::k_states_mark, dim3(record_grid(p.n)), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t pt_launch_states_check(const pt::StatesParams& p, hipStream_t s) {
    hipLaunchKernelGGL(pt::k_states_check, dim3(p.n_tiles_local), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t pt_launch_states_write(const pt::StatesParams& p, hipStream_t s) {
    hipLaunchKernelGGL(pt::k_states_write, dim3(record_grid(p.n)), dim3(256), 0, s, p);
    return hipGetLastError();
}
