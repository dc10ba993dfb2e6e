// pt_feats.h -- the first-hit feature engine's records and parameter block (pt_feats.hip,
// host/featq.cpp): for image-plane positions the caller supplies, the closest hit of
// Camera::GetToRay(x, y) (src/scene.cpp:180-187) and the scene data of the primitive it names --
// no pixels, no chains, no shading.  DESIGN.md §4.11.
//
// A record is a copy of the hit and of scene data: feature_fill adds no arithmetic.  Host and
// device compile the same function (pt_selftest_features_host runs it without a device).
#pragma once
#include "pt_counts.h"
#include "pt_rays.h"

namespace pt {

// the record of include/pt.h (pt_feature), 64 B, moved as four 16-B pieces:
//   {id, t, n.x, n.y} {n.z, interior, albedo.rg} {albedo.b, ior, emission.rg} {emission.b, material, type, 0}
struct Feature { uint4 w[4]; };

// a position, 8 B: pixel units, used as given (pt_camera_rays' xy)
struct alignas(8) FeatXY { float x, y; };

// The feature record of a closest hit (id < 0: a miss, h holds nothing): the hit as store_hit
// writes it, then primitives[id]'s shading record and type, word for word; a miss carries
// BG_COLOR as its emission -- what RayTrace returns for the ray -- and 0 everywhere else.
PT_HD void feature_fill(const SceneView& S, int id, const Hit& h, Feature& f) {
    if (id < 0) {
        f.w[0] = make_uint4(0xffffffffu, 0u, 0u, 0u);
        f.w[1] = make_uint4(0u, 0u, 0u, 0u);
        f.w[2] = make_uint4(0u, 0u, f2u(S.bg.x), f2u(S.bg.y));
        f.w[3] = make_uint4(f2u(S.bg.z), 0u, 0u, 0u);
        return;
    }
    const Shade sh = S.shade[id];
    const uint32_t type = f2u(S.prims[id].p0.w);
    f.w[0] = make_uint4((uint32_t)id, f2u(h.t), f2u(h.n.x), f2u(h.n.y));
    f.w[1] = make_uint4(f2u(h.n.z), h.interior, f2u(sh.s0.x), f2u(sh.s0.y));
    f.w[2] = make_uint4(f2u(sh.s0.z), f2u(sh.s0.w), f2u(sh.s1.x), f2u(sh.s1.y));
    f.w[3] = make_uint4(f2u(sh.s1.z), f2u(sh.s1.w), type, 0u);
}

// RaysParams' run members (pt_rays.h: the engine's PARAMS), with the camera and the positions as the
// source and the feature records as the sink
struct FeatsParams {
    SceneView S;
    CamView cam;
    const FeatXY* xy;
    Feature* out;
    uint32_t n;
    uint32_t batch;
    uint32_t service;
    unsigned long long* head;
    uint32_t* exact_n;
    uint32_t* exact;
    unsigned long long* counters;
    uint32_t aux_words;
    uint32_t dfs_words;
};

// a session's positions: every owned pixel's centre, in its export's order
struct FeatPosParams {
    TileMap tm;
    uint32_t n_tiles_local;
    const uint32_t* tile_rec;     // per local tile: the export's first record of that tile
    FeatXY* xy;                   // one per owned pixel
};

// the centre of pixel (x, y), global image coordinates
PT_HD FeatXY feature_centre(uint32_t x, uint32_t y) { return FeatXY{(float)x + 0.5f, (float)y + 0.5f}; }

}  // namespace pt

// k_feats then k_feats_exact on `s`, after the control block's memset (pt_launch_rays' contract)
hipError_t pt_launch_feats(const pt::FeatsParams& p, uint32_t grid, uint32_t block, hipStream_t s, hipEvent_t e0,
                           hipEvent_t e1);
// k_feats_positions: a workgroup per local tile
hipError_t pt_launch_feats_positions(const pt::FeatPosParams& p, hipStream_t s);
