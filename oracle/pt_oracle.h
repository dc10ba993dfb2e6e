/* pt_oracle.h -- C API of the CPU restatement (TEST INFRASTRUCTURE ONLY).
 * See pt_oracle.cpp.  Loaded by tests/ (ctypes), __graft_entry__.smoke() and
 * bench.py's cpu_baseline leg; never by the product library. */
#ifndef PT_ORACLE_H
#define PT_ORACLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef struct oracle_scene oracle_scene;
oracle_scene* oracle_load(const char* path);
void oracle_free(oracle_scene* o);
/* load_scene alone on (text, len), no init_scene: the parse in ref_harness parse's layout (80-byte
 * header + 100 bytes per primitive in file order).  Returns the bytes the dump takes; writes it
 * where out has room for them (cap).  warnings (may be NULL) takes the "unexpected command(...)"
 * lines, each ended by '\n', up to warn_cap bytes; *warn_need = their size. */
uint64_t oracle_parse_dump(const char* text, uint64_t len, void* out, uint64_t cap, char* warnings, uint64_t warn_cap,
                           uint64_t* warn_need);
int oracle_info(const oracle_scene* o, uint32_t* out8);
int oracle_dump_bvh(const oracle_scene* o, void* nodes_out, void* prims_out);
int oracle_render(oracle_scene* o, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t spp,
                  int nthreads, uint8_t* rgb, float* rad, uint64_t* counters);
/* oracle_render + the vertex census: census[n_prims * 10] u64, per primitive id {diffuse,
 * metallic, total internal reflection, Fresnel reflection, refraction} x {outside, interior} */
int oracle_render_census(oracle_scene* o, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t spp,
                         int nthreads, uint8_t* rgb, float* rad, uint64_t* counters, uint64_t* census);
/* per primitive id 6 u32: type, material, IOR bits, emissive, moved, rotated */
int oracle_prim_info(const oracle_scene* o, uint32_t* out);
int oracle_ray_intersection(const oracle_scene* o, uint32_t n, const float* rays, int32_t* ids, float* hit);
int oracle_rng(uint32_t seed, uint32_t n, float* out);
/* the integrator's scalar building blocks, element by element (see pt_oracle.cpp) */
void oracle_logf(uint64_t n, const float* x, float* out);
uint64_t oracle_logf_mismatches(uint64_t n, const float* x, const float* got);
void oracle_fresnel(uint64_t n, const float* in, float* out);
void oracle_normal_vecs(uint64_t n, const uint32_t* in, float* out);
void oracle_sample_cosine(uint64_t n, const void* in, float* out);
void oracle_tonemap(uint32_t n, const float* rad, uint8_t* rgb);
void oracle_gamma_u8(uint32_t n, const float* v, uint8_t* out);
uint64_t oracle_check_gamma_table(const float* thr);
#ifdef __cplusplus
}
#endif
#endif
