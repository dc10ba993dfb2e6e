// pt_wave.h -- what the wavefront kernels share (pt_wave.hip, pt_path.hip, pt_wcoop.hip).
//
// A pass advances every owned pixel by `target` samples (src/scene.cpp:
// 189-203) through rounds of launches on one stream:
//
//   k_wcamera   (pass start, pt_wave.hip) the first sample's 2 jitter draws and
//               camera ray (src/scene.cpp:180-199) of every pixel -> fresh queue
//   round r (parity p):
//     k_wpath   (pt_path.hip) the path engine: persistent query waves + a shade
//               wave per workgroup; a pixel's chain (its one ray in flight)
//               keeps going inside the kernel; once the round's work is used
//               up, running queries are suspended (state + LDS stack to the
//               carry queue) and resume next round
//     k_wexact  (pt_wave.hip) the rare rays handed to the exact stack DFS
//     k_wshade  (pt_wave.hip) shades k_wexact's results: the vertex (shade_vertex:
//               material logic and random draws) and its fold record, then either
//               the child ray, or -- path over -- the backward fold into the pixel
//               sum and the next sample's camera ray
//   end of a pass: k_wcoop (pt_wcoop.hip), the cooperative engine -- a team of
//               lanes per remaining chain
//
// Every pixel has at most one ray in flight and consumes its random stream
// in the reference order (jitter, then vertex by vertex), so results are
// bit-identical however the rounds interleave pixels.  The host loops rounds
// until the fresh and carry queues are empty.  Compiled with
// -ffp-contract=off (pt_core.h).
#pragma once
#include <hip/hip_runtime.h>

#include "pt_devutil.h"
#include "pt_kernels.h"
#include "pt_coop.h"
#include "pt_query.h"
#include "pt_wprof.h"

namespace pt {

// enqueue a fresh ray with its plane result (RayIntersection's plane loop)
__device__ __forceinline__ void push_ray(const WaveParams& P, const RayQ& Q, uint32_t qi, const Ray& ray,
                                         uint32_t slot) {
    float pt;
    int pid;
    q_planes(P.S, ray, pt, pid);
    Q.ro[qi] = F4{ray.o.x, ray.o.y, ray.o.z, u2f(slot)};
    Q.rd[qi] = F4{ray.d.x, ray.d.y, ray.d.z, pt};
    Q.pid[qi] = pid;
    Q.ri[qi] = q_prep(P.S, ray);
}

// The pixel slot of a round's work item gi: carry record gi (pt_kernels.h CarryRec) below
// n_carry, else fresh ray gi - n_carry (its slot in ro.w)
__device__ __forceinline__ uint32_t work_item_slot(const WaveParams& P, uint32_t gi, uint32_t n_carry) {
    return gi < n_carry ? carry_rec(P.cq[P.parity], gi, P.carry_words).slot() : f2u(P.fq[P.parity].ro[gi - n_carry].w);
}

// A value the optimiser must treat as new at this point: a loop-invariant expression
// built from it (a per-lane address) is then not hoisted into a VGPR held across the
// whole persistent loop, where it would spill
template <class T>
__device__ __forceinline__ T opaque_v(T v) { asm volatile("" : "+v"(v)); return v; }
// The launch's parameter block read where it is used: scalar loads from the kernarg
// segment at each use (its pointer is opaque there, so nothing is hoisted), for the
// parameters of a persistent loop's rare branches, which would otherwise hold SGPRs
// (and spill them to VGPR lanes) for the loop's whole life.  Its callers' kernels
// (k_wpath, k_wshade, k_wcoop) take the block as their only argument, at offset 0.
template <class K>
__device__ __forceinline__ const K& karg() {
#if defined(__HIP_DEVICE_COMPILE__)
    auto p = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *reinterpret_cast<const K*>(p);
#else
    __builtin_unreachable();   // (host pass: never called)
#endif
}
// a pixel's next camera sample, its jitter draws and camera ray (src/scene.cpp:189-196):
// x = pix % W, y = pix / W
__device__ __forceinline__ Ray camera_sample(const CamView& cam, Rng& R, uint32_t x, uint32_t y) {
    const float fx = (float)x + rng_uniform(R);
    const float fy = (float)y + rng_uniform(R);
    return camera_ray(cam, fx, fy);
}

// One finished query of a pixel's chain in two steps, the pixel record `hot` (RNG, vertex
// count, samples done) in registers -- wherever it lives: HBM (shade_item, for k_wshade) or
// a path workgroup's LDS table (pt_path.hip vertex_item / end_item).  A pixel has one
// chain, and its next sample starts only from end_step, so its operations keep their order.
// vertex_step: the vertex (src/scene.cpp:91-177) and its fold record; true with `ray` (which
// enters as the query ray) = the child ray, or false when the path ended -- the miss, or the
// vertex ends it --, `miss` telling how.
template <class EM>
__device__ __forceinline__ bool vertex_step(const WaveParams& P, const EM& em, PixelHot& hot, uint32_t slot, Ray& ray,
                                            uint32_t hid, bool& miss) {
    uint32_t nv = hot.nv;
    Rng R = hot.R;
    bool live = false;
    miss = hid == 0xffffffffu;
    if (!miss) {
        // the closest hit's t, normal and side: recomputed from its primitive
        // (the query's own test, same operations -> same bits)
        Hit h;
        (void)prim_intersect(P.S.prims[hid], ray, h);
        uint32_t idm;
        float s1, s2;
        const bool cont = shade_vertex_e(P.S, em, P.S.shade[hid], R, ray, h, (int)hid, idm, s1, s2);
        HbmVStore vs = fold_store(P.st, slot);
        vs.put(nv, idm, s1, s2);
        ++nv;
        live = cont && nv < P.depth;   // RayTrace(.., 0) = 0
    }
    hot.nv = nv;
    hot.R = R;
    return live;
}
// end_step: an ended path's backward fold into the pixel sum (deepest vertex first,
// src/scene.cpp:198 sum += ...) and the next sample's jitter draws and camera ray; false =
// the pixel has reached this pass's target.
__device__ __forceinline__ bool end_step(const WaveParams& P, PixelHot& hot, uint32_t slot, bool miss, Ray& ray) {
    Rng R = hot.R;
    uint32_t pix;
    const f3 sum = fold_path(P.st, P.S.shade, slot, hot.nv, miss ? P.S.bg : mk3(0.f, 0.f, 0.f), pix);
    store_sum(P.st, slot, sum, pix);
    hot.done += 1u;
    hot.nv = 0u;
    bool emit = false;
    if (hot.done < P.target) {
        // (the camera block read here, not held in SGPRs across a persistent loop)
        const WaveParams& K = karg<WaveParams>();
        ray = camera_sample(K.cam, R, pix % K.tm.W, pix / K.tm.W);
        emit = true;
    }
    hot.R = R;
    return emit;
}
// Both for a record in HBM: one 16-B load, one 16-B store.  Returns true with `ray` set to
// the chain's next ray (the child, or the next sample's camera ray); `sdone` returns
// whether a sample of the pixel ended here.
template <class EM>
__device__ __forceinline__ bool shade_item(const WaveParams& P, const EM& em, uint32_t slot, Ray& ray, uint32_t hid,
                                           bool& sdone) {
    PixelHot hot = load_hot(P.st, slot);
    bool miss;
    bool emit = vertex_step(P, em, hot, slot, ray, hid, miss);
    sdone = !emit;
    if (sdone) emit = end_step(P, hot, slot, miss, ray);
    store_hot(P.st, slot, hot);
    return emit;
}

#define PT_SUSPENDED 0xfffffffeu   // done.id of a query suspended to the next round

// LDS accessors with the address space spelled out (a reference to a __shared__ member is a
// generic pointer, which the compiler may otherwise lower to flat instructions)
#if defined(__HIP_DEVICE_COMPILE__)
#define PT_LDS __attribute__((address_space(3)))
#else
#define PT_LDS
#endif
__device__ __forceinline__ uint32_t lds_read(const uint32_t& v) { return *(const volatile PT_LDS uint32_t*)&v; }
__device__ __forceinline__ void lds_write(uint32_t& v, uint32_t x) { *(volatile PT_LDS uint32_t*)&v = x; }
template <class T>
__device__ __forceinline__ T lds_get(const T* a, uint32_t i) { return ((const PT_LDS T*)a)[i]; }
template <class T>
__device__ __forceinline__ void lds_put(T* a, uint32_t i, const T& v) { ((PT_LDS T*)a)[i] = v; }

}  // namespace pt

// launchers shared between the wavefront units (host side)
hipError_t pt_launch_exact_shade(const pt::WaveParams& p, uint32_t shade_grid, hipStream_t s);
hipError_t pt_preload_kernels_path();
hipError_t pt_preload_kernels_coop();
