// pt_feats.hip -- the first-hit feature engine: for positions on the image plane, the closest hit
// of the camera's ray and the hit primitive's scene data, one 64-B record per position
// (DESIGN.md §4.11).  The engine is the ray-query engine's (pt_rays.h: the refill loop, the service
// step, the exact list, the counter flush) with another job:
//   k_feats            item i's ray is camera_ray(cam, xy[i]), computed in registers by the lane
//                      that takes it; a lane that retires fetches the primitive's shading record
//                      and writes the feature
//   k_feats_exact      the same for the exact list's items (non-finite positions among them)
//   k_feats_positions  a session's positions: every owned pixel's centre, in its export's order
#include <hip/hip_runtime.h>

#include "pt_devutil.h"
#include "pt_feats.h"

namespace pt {

struct FeatsJob {
    const SceneView& S;
    const CamView& cam;
    const FeatXY* xy;
    Feature* out;
    __device__ __forceinline__ Ray ray(size_t i) const {
        const FeatXY p = xy[i];
        return camera_ray(cam, p.x, p.y);
    }
    __device__ __forceinline__ void store(size_t i, int id, const Hit& h) const {
        Feature f;
        feature_fill(S, id, h, f);
        uint4* o = out[i].w;
        o[0] = f.w[0];
        o[1] = f.w[1];
        o[2] = f.w[2];
        o[3] = f.w[3];
    }
};

__global__ void __launch_bounds__(256) k_feats(FeatsParams P) {
    rays_engine(P, FeatsJob{P.S, P.cam, P.xy, P.out});
}

__global__ void __launch_bounds__(64) k_feats_exact(FeatsParams P) {
    rays_exact_engine(P, FeatsJob{P.S, P.cam, P.xy, P.out});
}

// slot -> record (pt_counts.h count_record), slot -> pixel (slot_pixel): the two maps the export uses
__global__ void __launch_bounds__(256) k_feats_positions(FeatPosParams P) {
    const uint32_t tile = blockIdx.x, lane = threadIdx.x;
    if (tile >= P.n_tiles_local) return;
    uint32_t x, y;
    if (!slot_pixel(P.tm, tile, lane, x, y)) return;
    const int64_t rec = count_record(P.tm, P.tile_rec, tile, lane);
    if (rec < 0) return;
    P.xy[rec] = feature_centre(x, y);
}

}  // namespace pt

hipError_t pt_launch_feats(const pt::FeatsParams& p, uint32_t grid, uint32_t block, hipStream_t s, hipEvent_t e0,
                           hipEvent_t e1) {
    return pt::launch_rays_pair(pt::k_feats, pt::k_feats_exact, p, grid, block, s, e0, e1);
}

hipError_t pt_launch_feats_positions(const pt::FeatPosParams& p, hipStream_t s) {
    if (p.n_tiles_local == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt::k_feats_positions, dim3(p.n_tiles_local), dim3(256), 0, s, p);
    return hipGetLastError();
}
