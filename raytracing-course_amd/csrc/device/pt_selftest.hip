// pt_selftest.hip -- k_selftest_math: pt_selftest_math's operations on the device, one element
// per thread (pt_selftest.h math_one: the functions of pt_core.h / pt_trace.h the render kernels
// call, compiled here with the same flags), and k_selftest_decide: pt_query.h's q_decide on
// decision states the host made, a state per lane.  Tests only; never used by pt_render.
#include <hip/hip_runtime.h>

#include "pt_query.h"
#include "pt_selftest.h"

namespace pt {

__global__ void __launch_bounds__(256) k_selftest_math(uint32_t op, uint64_t n, const void* in, void* out,
                                                       const float* thr, uint32_t rng_n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) math_one(op, i, in, out, thr, rng_n);
}

// q_decide on n states, 64 consecutive ones to a wave: the lanes of a wave sit at different
// slots, so the wave-uniform exit and the per-slot selects run with every mix of live lanes
__global__ void __launch_bounds__(256) k_selftest_decide(uint64_t n, Query* st) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) {
        Query q = st[i];
        q_decide(q);
        st[i] = q;
    }
}

}  // namespace pt

extern "C++" {
hipError_t pt_launch_selftest_math(uint32_t op, uint64_t n, const void* in, void* out, const float* thr,
                                   uint32_t rng_n, hipStream_t s) {
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks == 0u || blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt::k_selftest_math, dim3((uint32_t)blocks), dim3(256), 0, s, op, n, in, out, thr, rng_n);
    return hipGetLastError();
}
hipError_t pt_launch_selftest_decide(uint64_t n, void* states, hipStream_t s) {
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks == 0u || blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt::k_selftest_decide, dim3((uint32_t)blocks), dim3(256), 0, s, n, static_cast<pt::Query*>(states));
    return hipGetLastError();
}
}
