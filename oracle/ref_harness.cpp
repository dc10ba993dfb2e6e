// ref_harness.cpp -- fixture dumper linked against the UNMODIFIED reference
// hw5 sources (see oracle/build_ref.sh; the reference headers are included
// under a private->public define so that private members can be read; the
// reference TUs themselves are compiled untouched).  Test infrastructure only: it
// generates the golden vectors under tests/golden/ that pin oracle/pt_oracle.cpp
// and, through it, the HIP renderer.  Nothing here is shipped or timed.
//
// Modes (all outputs little-endian binary, written to the given path):
//   bvh    <scene> <nodes.bin> <prims.bin>
//          node array after Scene::InitScene (hw5/src/scene.cpp:7-21,
//          hw5/src/bvh.cpp:99-179): per node 6 f32 (min.xyz,max.xyz) +
//          4 u32 (left,right,first,count); primitive order: per primitive
//          u32 type + 9 f32 (dop_data, dop_data1, dop_data2 -- the latter two
//          zero unless TRIANGLE) + 3 f32 pos.
//   render <scene> <out.ppm> <radiance.f32> [x0 y0 w h [ystride]]
//          restates Scene::Render's per-pixel loop (hw5/src/scene.cpp:205-252)
//          around the reference's own Scene::Sample, additionally saving the
//          pre-tonemap fp32 mean radiance.  With a window, only those pixels
//          are rendered (seeds stay the global index y*W+x), the PPM is the
//          window crop; with ystride, the window's h rows are y0, y0+ystride, ...
//          Load+InitScene and render times go to stderr (bench.py cpu_baseline).
//   rng    <seed> <n> <out.bin>
//          libstdc++ minstd_rand + uniform_real<float> + normal<float> streams
//          exactly as hw5/src/scene.cpp:216-223 builds them: n uniforms, then
//          n normals from a fresh engine, then a mixed u/n pattern.
//   trav   <scene> <nrays> <seed> <out.bin>
//          random rays -> reference Scene::RayIntersection (scene.cpp:46-77)
//          and BVH_t::Intersect with INF bound (bvh.cpp:181-225).
//   rays   <scene> <rays.f32> <out.bin>
//          the caller's rays (n x 6 f32: origin, direction, used as they are) through the
//          same two calls; the record per ray is trav's.
//   parse  <scene> <out.bin>
//          Scene::Load alone (src/sceneload.cpp:112-176; no InitScene, which aborts on
//          plane-only and type-less scenes), every field as its raw bits.  Header (80 B):
//          width, height, samples, ray_depth u32; fov_x, background, cam.pos, cam.right,
//          cam.up, cam.forward f32.  Then per primitive in file order a 100-byte record:
//          u32 type; dop_data, dop_data1, dop_data2 (the latter two zero unless TRIANGLE); pos; rotator as operator>> extracts
//          it (x y z w); col; emission (f32 each); u32 material; f32 ior.  The reference
//          gives several of these fields no initial value (Scene's and Camera's members,
//          a Primitive's type, pos and dop_data*).  So that the dump is a function of the
//          file alone, the Scene is built in zero-filled storage and the stack below the
//          call is zero-filled first: such a field reads 0 unless a line wrote it.  The
//          reference's "unexpected command(...)" lines go to stderr as they are.
// Standard and glm headers first, so that only the reference's own classes
// see the access override below.
#include <algorithm>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <istream>
#include <memory>
#include <optional>
#include <random>
#include <sstream>
#include <string>
#include <thread>
#include <variant>
#include <vector>
#include <omp.h>
#define GLM_ENABLE_EXPERIMENTAL
#include <glm/vec3.hpp>
#include <glm/gtc/quaternion.hpp>
#include <glm/gtx/norm.hpp>
#define private public
#include "scene.h"
#undef private

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <vector>

static void put_u32(std::ofstream& o, uint32_t v) { o.write(reinterpret_cast<const char*>(&v), 4); }
static void put_f32(std::ofstream& o, float v) { o.write(reinterpret_cast<const char*>(&v), 4); }
static void put_i32(std::ofstream& o, int32_t v) { o.write(reinterpret_cast<const char*>(&v), 4); }

static void load(Scene& s, const char* path) {
    std::ifstream in(path);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    s.Load(in);
    s.InitScene();
}

static int mode_bvh(int argc, char** argv) {
    if (argc < 5) return 2;
    Scene s;
    load(s, argv[2]);
    std::ofstream on(argv[3], std::ios::binary), op(argv[4], std::ios::binary);
    for (const NODE_t& n : s.scene_bvh.nodes) {
        put_f32(on, n.aabb.aabb_min.x); put_f32(on, n.aabb.aabb_min.y); put_f32(on, n.aabb.aabb_min.z);
        put_f32(on, n.aabb.aabb_max.x); put_f32(on, n.aabb.aabb_max.y); put_f32(on, n.aabb.aabb_max.z);
        put_u32(on, n.left_child); put_u32(on, n.right_child);
        put_u32(on, n.first_primitive_id); put_u32(on, n.primitive_count);
    }
    for (const Primitive& p : s.primitives) {
        put_u32(op, (uint32_t)p.primitive_type);
        const bool tri = p.primitive_type == PRIMITIVE_TYPE::TRIANGLE;
        put_f32(op, p.dop_data.x); put_f32(op, p.dop_data.y); put_f32(op, p.dop_data.z);
        put_f32(op, tri ? p.dop_data1.x : 0.f); put_f32(op, tri ? p.dop_data1.y : 0.f); put_f32(op, tri ? p.dop_data1.z : 0.f);
        put_f32(op, tri ? p.dop_data2.x : 0.f); put_f32(op, tri ? p.dop_data2.y : 0.f); put_f32(op, tri ? p.dop_data2.z : 0.f);
        put_f32(op, p.pos.x); put_f32(op, p.pos.y); put_f32(op, p.pos.z);
    }
    return 0;
}

// zero the stack that Scene::Load's frames will occupy (through a volatile pointer, so
// that the stores stay).  What a field without an initial value then reads is still the
// compiler's choice of stack slots: the fixtures regenerate byte-identically with the
// compiler and flags of oracle/build_ref.sh, and tests/_loader_cases.py keeps its cases to
// fields that a line of the file wrote, or that read this zero with that build.
__attribute__((noinline)) static void zero_stack_below() {
    volatile unsigned char pad[1 << 16];
    for (size_t i = 0; i < sizeof(pad); ++i) pad[i] = 0;
}

static void put_v3(std::ofstream& o, const glm::vec3& v) { put_f32(o, v.x); put_f32(o, v.y); put_f32(o, v.z); }

static int mode_parse(int argc, char** argv) {
    if (argc < 4) return 2;
    std::ifstream in(argv[2], std::ios::binary);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    // zero-filled storage, written through a volatile pointer: the constructor's own
    // stores are then the only other ones the fields see before Load
    void* mem = std::aligned_alloc(alignof(Scene) < 64 ? 64 : alignof(Scene), (sizeof(Scene) + 63) / 64 * 64);
    if (!mem) return 1;
    {
        volatile unsigned char* b = static_cast<volatile unsigned char*>(mem);
        for (size_t i = 0; i < sizeof(Scene); ++i) b[i] = 0;
    }
    Scene* sp = new (mem) Scene;
    Scene& s = *sp;
    zero_stack_below();
    s.Load(in);
    std::ofstream o(argv[3], std::ios::binary);
    put_u32(o, s.cam.width); put_u32(o, s.cam.height); put_u32(o, s.samples); put_u32(o, s.ray_depth);
    put_f32(o, s.cam.fov_x);
    put_v3(o, s.background.rgb); put_v3(o, s.cam.pos); put_v3(o, s.cam.right); put_v3(o, s.cam.up);
    put_v3(o, s.cam.forward);
    for (const Primitive& p : s.primitives) {
        uint32_t type, mat;
        static_assert(sizeof(p.primitive_type) == 4 && sizeof(p.material) == 4, "enum width");
        std::memcpy(&type, &p.primitive_type, 4);
        std::memcpy(&mat, &p.material, 4);
        put_u32(o, type);
        // (dop_data1 and dop_data2 of anything but a TRIANGLE are never written by the reference and
        // lie in a temporary whose stack slots hold other objects before it: 0, as mode bvh dumps them)
        const bool tri = p.primitive_type == PRIMITIVE_TYPE::TRIANGLE;
        const glm::vec3 zero{0.f, 0.f, 0.f};
        put_v3(o, p.dop_data); put_v3(o, tri ? p.dop_data1 : zero); put_v3(o, tri ? p.dop_data2 : zero);
        put_v3(o, p.pos);
        put_f32(o, p.rotator.x); put_f32(o, p.rotator.y); put_f32(o, p.rotator.z); put_f32(o, p.rotator.w);
        put_v3(o, p.col.rgb); put_v3(o, p.emission.rgb);
        put_u32(o, mat);
        put_f32(o, p.ior);
    }
    o.close();
    if (!o) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
    sp->~Scene();
    std::free(mem);
    return 0;
}

static double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static int mode_render(int argc, char** argv) {
    if (argc < 5) return 2;
    Scene s;
    const double t0 = now_s();
    load(s, argv[2]);
    const double t1 = now_s();
    // threads as the reference sets them (hw5/src/scene.cpp:212), unless REF_THREADS
    // names the host's usable CPU share (bench.py cpu_baseline)
    const char* rt = std::getenv("REF_THREADS");
    const int threads = rt && *rt ? std::atoi(rt) : (int)std::thread::hardware_concurrency();
    omp_set_num_threads(threads);
    const unsigned W = s.cam.width, H = s.cam.height;
    unsigned x0 = 0, y0 = 0, w = W, h = H, ystride = 1;
    if (argc >= 9) {
        x0 = (unsigned)std::atoi(argv[5]); y0 = (unsigned)std::atoi(argv[6]);
        w = (unsigned)std::atoi(argv[7]); h = (unsigned)std::atoi(argv[8]);
    }
    if (argc >= 10) ystride = (unsigned)std::max(1, std::atoi(argv[9]));   // rows y0, y0+ystride, ...
    std::vector<float> rad((size_t)w * h * 3);
    std::vector<unsigned char> rgb((size_t)w * h * 3);
    #pragma omp parallel for schedule(dynamic)
    for (long long k = 0; k < (long long)w * h; ++k) {
        const unsigned x = x0 + (unsigned)(k % w), y = y0 + (unsigned)(k / w) * ystride;
        const unsigned i = y * W + x;
        std::minstd_rand rnd(i);
        std::uniform_real_distribution<float> uniform01{0.f, 1.f};
        std::normal_distribution<float> normal01{0.f, 1.f};
        RANDOM_t random{rnd, uniform01, normal01};
        Color c = s.Sample(random, x, y);
        rad[k * 3 + 0] = c.r(); rad[k * 3 + 1] = c.g(); rad[k * 3 + 2] = c.b();
        Color t = GammaCorrected(AcesTonemap(c));
        unsigned char* u = t.toUInts();
        rgb[k * 3 + 0] = u[0]; rgb[k * 3 + 1] = u[1]; rgb[k * 3 + 2] = u[2];
        delete[] u;
    }
    const double t2 = now_s();
    std::fprintf(stderr, "ref_harness: load_init_s=%.6f render_s=%.6f threads=%d hardware_concurrency=%u\n", t1 - t0,
                 t2 - t1, threads, std::thread::hardware_concurrency());
    std::ofstream out(argv[3], std::ios::binary);
    out << "P6\n" << w << " " << h << "\n" << 255 << "\n";
    out.write(reinterpret_cast<const char*>(rgb.data()), (std::streamsize)rgb.size());
    std::ofstream orad(argv[4], std::ios::binary);
    orad.write(reinterpret_cast<const char*>(rad.data()), (std::streamsize)(rad.size() * 4));
    return 0;
}

static int mode_rng(int argc, char** argv) {
    if (argc < 5) return 2;
    const unsigned seed = (unsigned)std::strtoul(argv[2], nullptr, 10);
    const int n = std::atoi(argv[3]);
    std::ofstream o(argv[4], std::ios::binary);
    {
        std::minstd_rand rnd(seed);
        std::uniform_real_distribution<float> u{0.f, 1.f};
        for (int k = 0; k < n; ++k) put_f32(o, u(rnd));
    }
    {
        std::minstd_rand rnd(seed);
        std::normal_distribution<float> g{0.f, 1.f};
        for (int k = 0; k < n; ++k) put_f32(o, g(rnd));
    }
    {
        // mixed pattern: draw kind decided by a fixed bit pattern
        std::minstd_rand rnd(seed);
        std::uniform_real_distribution<float> u{0.f, 1.f};
        std::normal_distribution<float> g{0.f, 1.f};
        for (int k = 0; k < n; ++k) {
            const bool use_u = ((k * 2654435761u) >> 7) & 1u;
            put_f32(o, use_u ? u(rnd) : g(rnd));
        }
    }
    return 0;
}

// one 72-byte record: the ray, then RayIntersection's and BVH_t::Intersect's answers
static void put_trav_record(std::ofstream& o, Scene& s, const Ray& r) {
    ray_intersection_t a = s.RayIntersection(r);
    ray_intersection_t b = s.scene_bvh.Intersect(s.primitives, r, INF);
    put_f32(o, r.o.x); put_f32(o, r.o.y); put_f32(o, r.o.z);
    put_f32(o, r.d.x); put_f32(o, r.d.y); put_f32(o, r.d.z);
    for (const ray_intersection_t* q : {&a, &b}) {
        put_i32(o, q->id);
        const bool h = q->id != -1;
        put_f32(o, h ? q->isec.t : 0.f);
        put_f32(o, h ? q->isec.normal.x : 0.f); put_f32(o, h ? q->isec.normal.y : 0.f);
        put_f32(o, h ? q->isec.normal.z : 0.f);
        put_u32(o, h ? (uint32_t)q->isec.interior : 0u);
    }
}

static int mode_trav(int argc, char** argv) {
    if (argc < 6) return 2;
    Scene s;
    load(s, argv[2]);
    const int nrays = std::atoi(argv[3]);
    std::mt19937 gen((unsigned)std::strtoul(argv[4], nullptr, 10));
    std::uniform_real_distribution<float> U(0.f, 1.f);
    std::normal_distribution<float> N(0.f, 1.f);
    std::ofstream o(argv[5], std::ios::binary);
    // scene extent from the root box (planes excluded from the BVH)
    const AABB_t& root = s.scene_bvh.nodes[0].aabb;
    for (int k = 0; k < nrays; ++k) {
        Ray r;
        if (k & 1) {
            // from the camera through a random pixel (unnormalised, as GetToRay)
            r = s.cam.GetToRay(U(gen) * s.cam.width, U(gen) * s.cam.height);
        } else {
            // from a random point of the (slightly grown) root box, random direction
            glm::vec3 p;
            for (int a = 0; a < 3; ++a) {
                const float lo = root.aabb_min[a], hi = root.aabb_max[a];
                const float ext = hi - lo;
                p[a] = lo - 0.25f * ext + 1.5f * ext * U(gen);
            }
            glm::vec3 d{N(gen), N(gen), N(gen)};
            if (k % 7 == 2) d.x = 0.f;  // exercise zero direction components
            if (k % 11 == 4) d.y = -0.f;
            r = Ray(p, glm::normalize(d));
        }
        put_trav_record(o, s, r);
    }
    return 0;
}

static int mode_rays(int argc, char** argv) {
    if (argc < 5) return 2;
    Scene s;
    load(s, argv[2]);
    std::ifstream in(argv[3], std::ios::binary);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[3]); return 1; }
    std::ofstream o(argv[4], std::ios::binary);
    float f[6];
    while (in.read(reinterpret_cast<char*>(f), sizeof f))
        put_trav_record(o, s, Ray(glm::vec3{f[0], f[1], f[2]}, glm::vec3{f[3], f[4], f[5]}));
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: ref_harness bvh|parse|render|rng|trav|rays ...\n"); return 2; }
    const std::string m = argv[1];
    int rc = 2;
    if (m == "bvh") rc = mode_bvh(argc, argv);
    else if (m == "render") rc = mode_render(argc, argv);
    else if (m == "rng") rc = mode_rng(argc, argv);
    else if (m == "trav") rc = mode_trav(argc, argv);
    else if (m == "rays") rc = mode_rays(argc, argv);
    else if (m == "parse") rc = mode_parse(argc, argv);
    if (rc == 2) std::fprintf(stderr, "bad arguments for mode %s\n", m.c_str());
    return rc;
}
