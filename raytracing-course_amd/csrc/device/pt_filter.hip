// pt_filter.hip -- the guided filter of a frame: pt_filter.h's functions over a window.
//
//   k_filter_centres   the centres of a run of window pixels (the positions of the guides' feature query)
//   k_filter_guides    pt_feature -> 32-B guide: 64 B in and 32 B out per lane, in 16-B pieces
//   k_filter<IN, LAST> one level, one pixel per lane.  IN: the level reads the context's 16-B colours
//                      (0), or the caller's 12-B pixels row-major (1) or in packed tiles (2); LAST: it
//                      writes the caller's 12-B pixels (and the optional 8-bit form), not the context's.
//
// The direct form: a workgroup is a 16 x 16 pixel tile and a wave four rows of it, so that one tap of a
// wave reads four runs of 16 neighbours -- 4 x 512 B of guides and 4 x 256 B of colours, whole lines --
// and the 25 taps of neighbouring lanes fall on the same lines, served by L1 / L2.  A level reads 48 B
// per pixel once from memory (a 32-B guide, a 16-B colour) and writes 16.
#include <hip/hip_runtime.h>

#include "pt_devutil.h"
#include "pt_filter.h"

namespace pt {

__global__ void __launch_bounds__(256) k_filter_centres(FilterGuideParams P) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n) return;
    P.xy[i] = filter_centre(P.x0, P.y0, P.w, P.first + i);
}

__global__ void __launch_bounds__(256) k_filter_guides(FilterGuideParams P) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n) return;
    Feature f;
    const uint4* src = P.feat[i].w;
    f.w[0] = src[0];
    f.w[1] = src[1];
    f.w[2] = src[2];
    f.w[3] = src[3];
    FilterGuide g;
    filter_guide(f, g);
    uint4* dst = P.guides[P.first + i].w;
    dst[0] = g.w[0];
    dst[1] = g.w[1];
}

template <int IN>
struct FilterSrcOf;
template <>
struct FilterSrcOf<0> {
    using type = FilterSrcLevel;
    static __device__ __forceinline__ type make(const FilterParams& P) { return type{P.src, P.w}; }
};
template <>
struct FilterSrcOf<1> {
    using type = FilterSrcRows;
    static __device__ __forceinline__ type make(const FilterParams& P) { return type{P.in, P.w}; }
};
template <>
struct FilterSrcOf<2> {
    using type = FilterSrcTiles;
    static __device__ __forceinline__ type make(const FilterParams& P) { return type{P.in, P.tiles_x}; }
};

template <int IN, bool LAST>
__global__ void __launch_bounds__(256) k_filter(FilterParams P) {
    const uint32_t x = blockIdx.x * 16u + (threadIdx.x & 15u), y = blockIdx.y * 16u + (threadIdx.x >> 4);
    if (x >= P.w || y >= P.h) return;
    const FilterColour c = filter_pixel(FilterSrcOf<IN>::make(P), P.guides, P.w, P.h, x, y, P.lv);
    const uint32_t i = y * P.w + x;
    if (LAST) {
        float* o = P.out + 3u * i;
        o[0] = c.r;
        o[1] = c.g;
        o[2] = c.b;
        if (P.rgb) {
            uint8_t* b = P.rgb + 3u * i;
            b[0] = (uint8_t)quantize_gamma(aces1(c.r), P.thr);
            b[1] = (uint8_t)quantize_gamma(aces1(c.g), P.thr);
            b[2] = (uint8_t)quantize_gamma(aces1(c.b), P.thr);
        }
    } else {
        P.dst[i] = filter_pack(c);
    }
}

}  // namespace pt

// ---------------------------------------------------------------- launchers
hipError_t pt_launch_filter_centres(const pt::FilterGuideParams& p, hipStream_t s) {
    if (p.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt::k_filter_centres, dim3((p.n + 255u) / 256u), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t pt_launch_filter_guides(const pt::FilterGuideParams& p, hipStream_t s) {
    if (p.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt::k_filter_guides, dim3((p.n + 255u) / 256u), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t pt_launch_filter_level(const pt::FilterParams& p, uint32_t in_kind, bool last, hipStream_t s) {
    const dim3 grid((p.w + 15u) / 16u, (p.h + 15u) / 16u), block(256);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    switch (in_kind * 2u + (last ? 1u : 0u)) {
        case 0u: hipLaunchKernelGGL((pt::k_filter<0, false>), grid, block, 0, s, p); break;
        case 1u: hipLaunchKernelGGL((pt::k_filter<0, true>), grid, block, 0, s, p); break;
        case 2u: hipLaunchKernelGGL((pt::k_filter<1, false>), grid, block, 0, s, p); break;
        case 3u: hipLaunchKernelGGL((pt::k_filter<1, true>), grid, block, 0, s, p); break;
        case 4u: hipLaunchKernelGGL((pt::k_filter<2, false>), grid, block, 0, s, p); break;
        case 5u: hipLaunchKernelGGL((pt::k_filter<2, true>), grid, block, 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
