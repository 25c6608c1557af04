// The hot path: per-pixel path tracing on gfx950 (MI355X).
//
// Replaces   render<<<(W/8+1,H/8+1),(8,8)>>>   gpu-version/main.cu:72-105
//            ray_color                         gpu-version/main.cu:17-70  (semantics:
//                                              cmake-cpu-version/main.cpp:13-43)
//            hittable_list::hit + sphere/rect/cylinder::hit   gpu-version/object.cuh
//            material::scatter / emitted       gpu-version/material.cuh
//            camera::get_ray                   cmake-cpu-version/camera.h:32-39
//            curand XORWOW per-pixel state     -> Philox-seeded xorshift128 per (pixel, sample) (philox.h)
//
// Shape of the kernel
//   * 256-thread workgroup = 4 wave64; the grid only fills the chip (persistent waves) and
//     every wave pulls work items -- an 8x8 pixel tile x 64 sample indices -- from one
//     global counter.  A work-item (lane) owns ONE PATH at a time and runs its whole
//     bounce loop (get_color), exactly as the reference's thread does for its pixel.
//   * lanes stay converged across bounces: every iteration of the main loop is one
//     closest-hit query for all live lanes over a wave-uniform primitive loop.  A lane
//     whose path ended adds the radiance to its pixel and immediately takes the next
//     (pixel, sample) item of the tile's pool -- __ballot of the idle lanes, mbcnt for
//     the rank, a wave-uniform cursor -- so no lane waits for the slowest pixel of the
//     tile; the loop leaves on !__any(active) with the pool empty.
//     (variant bit 0 restores strict ownership: a lane only takes samples of its own
//     pixel.  Results are identical; it is kept to measure what the pool buys.)
//   * that hand-off is legal because the per-pixel sum is exact: each fp32 sample is
//     added as 64-bit fixed point (2^-24), in LDS per tile, then one 64-bit global
//     atomic per pixel and channel; a second kernel converts to the fp32 framebuffer
//     with fully coalesced stores.
//   * the primitive tables the inner loop reads ("hot" part of the scene image,
//     device_scene.h) are copied into LDS once per workgroup; all lanes read the same
//     record (broadcast ds_read_b128), four spheres are fetched one batch ahead of use.
//     No virtual calls, no pointer chasing; cold data (1/r, material records) stays in
//     global memory / L2 and is read once per bounce.
//   * the list is not scanned blindly: after the few big spheres, clusters of 8 spheres are
//     tested only when some lane's ray reaches the cluster's bounding box (aabb.hpp slab test
//     per lane + one __ballot), with a per-lane margin that covers the fp32 error of the
//     sphere test so that the closest hit -- and the framebuffer -- stay bit-identical to the
//     full scan (variant bit 4 is the full scan).
//   * arithmetic: fp32, every fused multiply-add explicit (-ffp-contract=off), IEEE
//     sqrt and divide, so results are bit-identical to the scalar restatement the
//     tests check against.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "device_scene.h"
#include "philox.h"
#include "rt_env.h"
#include "rt_media.h"
#include "rt_motion.h"
#include "rt_trig.h"
#include "shard.h"
#include "../../include/rtmi.h"

// minimum resident waves per SIMD the register allocator must leave room for (8 <=> 64 VGPRs)
#ifndef RT_WAVES_PER_SIMD
#define RT_WAVES_PER_SIMD 7
#endif
// ... of the light-sampling kernels (render_nee_kernel): the shadow phase keeps eight more values alive per lane
#ifndef RT_NEE_WAVES_PER_SIMD
#define RT_NEE_WAVES_PER_SIMD 6
#endif
// Wave priority (s_setprio) of the sections of an iteration.  Seven waves share a SIMD's issue port; a wave in the closest-hit
// query is a chain of short dependent steps (LDS reads, compares, branches) that wants its slot the moment its data is there,
// a wave in the seeding or in the rejection loop is a long run of independent vector instructions that can fill any gap.
// With every section at priority 0 the frame takes 131.5 ms; query + hit record + pixel accumulation at 2, scatter step /
// camera ray at 1, refill and rejection loop at 0: 127.2 ms (-3.3 %).  Measured: walk alone at 1 / 2 / 3: 129.7 / 130.1 /
// 129.5; query set-up + walk at 1: 128.6; + hit record and accumulation: 127.6; + scatter at 1: 127.4; the rejection loop
// or the refill raised instead: 131.6 / 128.8; the walk LOWERED: 133.4.  Re-measured on round 3's kernel (121.8 ms): the refill at
// 1 -- level with the scatter step -- 121.0 (-0.6 %, three alternations on one box), at 2: 122.2; the rejection loop at 1: 123.5;
// the walk and the hit record at 3 on top of that: 120.5 against 120.9 (means of five alternations; the walk alone at 3: 120.8, the
// query set-up at 3 as well: 121.05, at 1: 121.1, the scatter step at 2: 120.6).
#ifndef RT_PRIO_Q
#define RT_PRIO_Q 2  /* query set-up: prefix spheres, grid entry */
#endif
#ifndef RT_PRIO_W
#define RT_PRIO_W 3  /* grid walk */
#endif
#ifndef RT_PRIO_H
#define RT_PRIO_H 3  /* from the end of the walk to the refill: other primitives, hit record, pixel accumulation */
#endif
#ifndef RT_PRIO_F
#define RT_PRIO_F 1  /* refill (seeding, jitter) */
#endif
#ifndef RT_PRIO_R
#define RT_PRIO_R 0  /* rejection loop */
#endif
#ifndef RT_PRIO_S
#define RT_PRIO_S 1  /* after the rejection loop: scatter step, camera ray, ray tail */
#endif
// 1: the rejection loop draws three values per attempt for every lane and selects the state to keep (no inner branch)
// candidate predicate of a sphere test: a real root that is not behind the origin (as two nested branches: evaluated without
// short-circuit -- three compares, one branch -- it measured 146.5 against 145.5 ms)
#define RT_CAND(disc, hb, cc) (!((disc) < 0.0f) && !((hb) >= 0.0f && (cc) >= 0.0f))

namespace rtmi {

static constexpr float kTMin = 0.001f;  // main.cu:45 / main.cpp:22
static_assert(RT_FIX_BITS == RT_ACC_FIX_BITS, "the kernel's pixel sums and the ABI's scale");

// ---------------------------------------------------------------- RNG
struct LaneRng {
    Xor128 g;
    uint32_t draws;
};

__device__ __forceinline__ void rng_start(LaneRng &r, uint32_t pixel, uint32_t sample, uint32_t k0, uint32_t k1) {
    // The key schedule (k + r W for the ten rounds) is wave-uniform and loop-invariant, so the compiler computes the twenty
    // words once per launch -- and then, out of scalar registers, keeps them in the lanes of a spill VGPR and fetches
    // them with v_readlane (plus hazard nops) in every seeding.  Behind this barrier the key is a fresh scalar of the
    // iteration, and the schedule is two s_add per round.
    asm volatile("" : "+s"(k0), "+s"(k1));
    r.g = xor128_seed(pixel, sample, k0, k1);
}

template <bool COUNT>
__device__ __forceinline__ float rng_next(LaneRng &r) {
    const uint32_t w = xor128_next(r.g);
    if (COUNT) r.draws++;
    return (float)(w >> 8) * (1.0f / 16777216.0f);
}

template <bool COUNT>
__device__ __forceinline__ float rng_pm1(LaneRng &r) {  // random_double(-1, 1): -1 + 2 xi
    // xi = k 2^-24 with a 24-bit integer k: 2 xi and -1 + 2 xi are exact in fp32 (multiples of 2^-23 in [-1, 1)), so
    // one fused multiply-add returns the very value of the checker's three operations (convert, scale, shift)
    const uint32_t w = xor128_next(r.g);
    if (COUNT) r.draws++;
    return fmaf((float)(w >> 8), 1.0f / 8388608.0f, -1.0f);
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return fmaf(ax, bx, fmaf(ay, by, az * bz));
}

// IEEE-correct fp32 square root, bit for bit what sqrtf() returns.  hipcc expands sqrtf() to v_sqrt_f32 (1 ulp) plus the
// one-step correction below, wrapped in a scaling for arguments below 2^-96 (v_sqrt_f32 flushes denormals) and a fix-up for
// 0 and inf: 17 instructions.  The arguments of this kernel (discriminants, squared lengths) are ordinary numbers, so the
// wrapping only runs -- through sqrtf() itself -- when some lane of the wave really holds such an argument: 11 instructions
// otherwise.  The kernel takes ~10 square roots per iteration of its main loop.
__device__ __forceinline__ float rt_sqrtf(float x) {
    // [2^-96, inf): one unsigned compare on the bit pattern (negative numbers and NaN fall outside as well)
    if (__builtin_expect((uint32_t)(__float_as_uint(x) - 0x0f800000u) >= (0x7f800000u - 0x0f800000u), 0)) return sqrtf(x);
    const float s = __builtin_amdgcn_sqrtf(x);
    const float s_dn = __uint_as_float(__float_as_uint(s) - 1u), s_up = __uint_as_float(__float_as_uint(s) + 1u);
    const float r_dn = fmaf(-s_dn, s, x), r_up = fmaf(-s_up, s, x);
    float r = r_dn <= 0.0f ? s_dn : s;
    r = r_up > 0.0f ? s_up : r;
    return r;
}

// number of set bits of a lane mask as a 32-bit SCALAR (popcll's result is compared as a 64-bit value, for which the
// scalar unit has no ordered compare: the comparison then runs on the vector ALU, once per pass of the walk's loops)
__device__ __forceinline__ int mask_count(unsigned long long m) {
    return __builtin_amdgcn_readfirstlane(__builtin_popcount((uint32_t)m) + __builtin_popcount((uint32_t)(m >> 32)));
}

// checker_texture::value, texture.cuh:44-52: sign of sin(10x)sin(10y)sin(10z) as the
// parity of floor(10x/pi) + floor(10y/pi) + floor(10z/pi); zero factor -> even
__device__ __forceinline__ bool checker_odd(float px, float py, float pz) {
    const float inv_pi = 0.318309886183790671538f;
    float tx = 10.0f * px, ty = 10.0f * py, tz = 10.0f * pz;
    int kx = (int)floorf(tx * inv_pi), ky = (int)floorf(ty * inv_pi), kz = (int)floorf(tz * inv_pi);
    bool zero = (tx == 0.0f) || (ty == 0.0f) || (tz == 0.0f);
    return !zero && (((kx + ky + kz) & 1) != 0);
}

// a x b, one fused multiply-add per component (the checker uses the same form)
__device__ __forceinline__ void cross3(float ax, float ay, float az, float bx, float by, float bz, float &cx, float &cy, float &cz) {
    cx = fmaf(ay, bz, -(az * by));
    cy = fmaf(az, bx, -(ax * bz));
    cz = fmaf(ax, by, -(ay * bx));
}

// image texture, taichi-version/material.py:137-144: texel[int(frac(u) * rows)][int(frac(v) * cols)] / 255
__device__ __forceinline__ void image_texel(const float4 *__restrict__ image, const float4 q1, float u, float v, float &r, float &g,
                                            float &b) {
    const int rows = __float_as_int(q1.y), cols = __float_as_int(q1.z);
    const int x = min((int)((u - floorf(u)) * (float)rows), rows - 1);
    const int y = min((int)((v - floorf(v)) * (float)cols), cols - 1);
    const uint32_t w = reinterpret_cast<const uint32_t *>(image)[__float_as_int(q1.x) + x * cols + y];
    r = (float)(w & 255u) / 255.0f, g = (float)((w >> 8) & 255u) / 255.0f, b = (float)((w >> 16) & 255u) / 255.0f;
}

// original list index of a grouped primitive id (cold tables), for the tie rule
__device__ __forceinline__ int list_index_of(const RenderParams &P, const float4 *__restrict__ image, int id) {
    if (id < P.ns) return __float_as_int(image[P.off_sph_cold + id].z);
    if (id < P.ns + P.nr) return __float_as_int(image[P.off_rect_cold + (id - P.ns)].y);
    if (id < P.ns + P.nr + P.nc) return __float_as_int(image[P.off_cyl_cold + 4 * (id - P.ns - P.nr) + 3].y);
    return __float_as_int(image[P.off_tri_cold + 2 * (id - P.ns - P.nr - P.nc)].y);
}

// radiance sample -> 64-bit fixed point with RT_FIX_BITS (24) fractional bits, round to nearest even;
// NaN -> 0, magnitude clamped to RT_FIX_CLAMP (2^16).  |sample| <= 2^16 and at most 2^23 samples per pixel
// (checked by the host) keep every pixel sum below 2^39 < 2^63 / 2^24: the integer sums never wrap.
__device__ __forceinline__ unsigned long long radiance_to_fixed(float v) {
    // |v| < 128 (every sample that is not a look straight into a bright emitter): v * 2^24 is exact (a power of two)
    // and below 2^31, so round-to-nearest-even and a 32-bit convert give llrint((double)v * 2^24); sign-extended
    if (fabsf(v) < 128.0f) return (unsigned long long)(long long)(int)rintf(v * 16777216.0f);
    if (!(fabsf(v) <= RT_FIX_CLAMP)) v = (v != v) ? 0.0f : copysignf(RT_FIX_CLAMP, v);
    // the general case without fp64: |v| = hi + frac with hi = trunc(|v|) (v_cvt_u32_f32; the
    // subtraction of the integer part is exact), frac * 2^24 < 2^24 is exact in fp32 arithmetic before the
    // rounding, and rounding it to nearest even rounds the whole value to nearest even because hi * 2^24 is
    // an even integer.
    const float a = fabsf(v);
    const uint32_t hi = (uint32_t)a;
    const float frac = a - (float)hi;
    const uint32_t lo = (uint32_t)rintf(frac * 16777216.0f);
    const unsigned long long m = ((unsigned long long)hi << RT_FIX_BITS) + lo;
    return v < 0.0f ? 0ull - m : m;
}

// ---------------------------------------------------------------- light sampling (render_nee_kernel)
static constexpr float kPi = 3.14159265358979323846f, kInvPi = 0.318309886183790671538f;

// density of the reference's fuzzy-metal direction d = r + f s (s uniform in the unit ball, |r| = 1) at the unit direction w:
// the part of the ray t w, t > 0, inside the ball of radius f around r, weighted by t^2 -- (t1^3 - t0^3) / (4 pi f^3) with the
// roots t0,1 of |t w - r|^2 = f^2 and t0 clamped at 0; as (t1 - t0)(t1^2 + t1 t0 + t0^2), which does not cancel at small f
__device__ __forceinline__ float metal_pdf(float wx, float wy, float wz, float rx, float ry, float rz, float f) {
    const float wr = dot3(wx, wy, wz, rx, ry, rz);
    const float disc = fmaf(wr, wr, fmaf(f, f, -1.0f));
    if (!(disc >= 0.0f)) return 0.0f;
    const float sq = sqrtf(disc);
    const float t1 = wr + sq;
    if (!(t1 > 0.0f)) return 0.0f;
    const float t0 = fmaxf(wr - sq, 0.0f);
    return (t1 - t0) * fmaf(t1, t1, fmaf(t1, t0, t0 * t0)) * (0.25f * kInvPi) / (f * f * f);
}

// 1 - cos of the half-angle of the cone a sphere of squared radius r2 subtends at squared distance c2 > r2 (stable for small cones)
__device__ __forceinline__ float cone_one_minus_cos(float r2, float c2) {
    const float q = r2 / c2;
    return q / (1.0f + sqrtf(fmaxf(0.0f, 1.0f - q)));
}

// ---------------------------------------------------------------- kernel
// POOL:     idle lanes take the next (pixel, sample) item of the wave's tile (default)
//           / false: a lane only renders samples of its own pixel (ablation: the north_star's literal lane-per-pixel shape)
// SCALAR:   nothing is staged in LDS: every table is read from global memory -- wave-uniform reads through
//           the scalar cache (SGPR operands), per-lane reads through the vector L1/L2.  The mode for scenes
//           whose tables would crowd out occupancy or not fit the 160 KB at all.
// CULL:     the candidate search of the closest-hit query.  Every search is conservative with respect to the fp32 error of
//           the primitive tests, so the closest hit -- and the framebuffer -- equal the reference's linear scan bit for bit.
//           5  uniform grid over the clustered spheres, COMPACT tables (16-bit list entries, one word per cell): sphere-only
//              scenes whose tables fit LDS beside full occupancy.  Every lane walks the cells its ray crosses front to back.
//           6  the same for a grid one cell high (a sheet of spheres on the ground: RTIOW): the walk has no y axis
//           7  the same walk over the WIDE tables (32-bit list entries, two words per cell, up to 1023 cells per axis): every
//              other scene.  Its cells also list the rectangles, cylinders and triangles (taichi-version/bvh.py:109-199
//              indexes every hittable): a lane tests what its cells list; only the oversized primitives (the RTIOW ground,
//              a room's walls) are tested for every query
//           8  the walk of 7 over wide tables with NESTED cells (rt_scene_set_nested_grid): a cell that clustered geometry
//              overfills carries a sub-grid, which the lane walks while its ray is inside the cell.  Tables in global memory only
//           ablations (RTMI_ABLATIONS builds): 3 range tables, 2 two-level box hierarchy per lane (round 1's default), 1 wave
//           votes per cluster box (aabb.hpp:15-29 + __any), 0 no culling: the reference's linear hittable_list scan
// EXT:      the Taichi renderer's extras -- triangles (taichi-version/hittable.py:38-71) and image textures read at the
//           hit record's (u, v) (material.py:137-144).  Only the builds for scenes that use them carry the code: it
//           costs the kernel its register budget (86 spilled VGPRs instead of 23) whether a scene uses it or not.
// SPH:      the scene holds spheres only (RTIOW, the 3-sphere scene): no rectangle / cylinder / triangle code, no dispatch
//           on the winner's type -- and, what pays, a dozen fewer launch values and loop-invariant masks competing for scalar
//           registers (the surplus of those lives in the lanes of a spill VGPR: one v_readlane per use).  The compact-table
//           kernels (CULL 5, 6) are built this way only.
// NEE:      light sampling (rt_scene_set_light_sampling): one light sample per eligible vertex, combined with the BSDF sample
//           by multiple importance sampling (power heuristic).  The sample's visibility is a SHADOW PHASE of the lane: the
//           lane's next query is the shadow ray (same origin, best_t starting below 1, any hit occludes); then the lane
//           adds the sample's contribution and restores its continuation.  Only render_nee_kernel carries it.
template <bool COUNT, bool POOL, bool SCALAR, int CULL, bool EXT, bool SPH>
__global__ __launch_bounds__(256, RT_WAVES_PER_SIMD) void render_kernel(const RenderParams P, const float4 *__restrict__ image,
                                                     unsigned long long *__restrict__ acc,
                                                     unsigned int *__restrict__ queue,
                                                     DevCounters *__restrict__ counters) {
    constexpr bool NEE = false, AOV = false, ENV = false, MEDIA = false, MOTION = false;
#include "render_body.h"
}

// light sampling (NEE): the general layouts with triangles and image textures -- the linear scan (CULL 0) and the wide grid
// walk (CULL 7) with its tables in LDS or in global memory (SCALAR)
template <bool SCALAR, int CULL>
__global__ __launch_bounds__(256, RT_NEE_WAVES_PER_SIMD) void render_nee_kernel(const RenderParams P, const float4 *__restrict__ image,
                                                         unsigned long long *__restrict__ acc,
                                                         unsigned int *__restrict__ queue,
                                                         DevCounters *__restrict__ counters) {
    constexpr bool COUNT = false, POOL = true, EXT = true, SPH = false, NEE = true, AOV = false, ENV = false, MEDIA = false, MOTION = false;
#include "render_body.h"
}

// nested grid (rt_scene_set_nested_grid): the global-memory walk over wide tables with nested cells (CULL 8), plain and with
// triangles / image textures, and its counting build.  A kernel of its own, like the light-sampling one: the render_kernel
// instances of a product build stay the eight they were.
template <bool COUNT, bool EXT>
__global__ __launch_bounds__(256, RT_WAVES_PER_SIMD) void render_nested_kernel(const RenderParams P, const float4 *__restrict__ image,
                                                            unsigned long long *__restrict__ acc,
                                                            unsigned int *__restrict__ queue,
                                                            DevCounters *__restrict__ counters) {
    constexpr bool POOL = true, SCALAR = true, SPH = false, NEE = false, AOV = false, ENV = false, MEDIA = false, MOTION = false;
    constexpr int CULL = 8;
#include "render_body.h"
}

// first-hit feature passes (rt_render_hip_feature): a sample runs as in render_kernel up to its first closest-hit query -- same
// stream, jitter, lens draw, camera ray and walk -- and there adds the feature P.feature selects (a launch value) in place of
// radiance.  One query per sample, so the general builds (triangles, image textures) serve every scene: the linear scan (CULL 0),
// the wide grid walk (7) and the nested walk (8), tables in LDS or in global memory (SCALAR).
template <bool SCALAR, int CULL>
__global__ __launch_bounds__(256, RT_WAVES_PER_SIMD) void render_feature_kernel(const RenderParams P, const float4 *__restrict__ image,
                                                             unsigned long long *__restrict__ acc,
                                                             unsigned int *__restrict__ queue,
                                                             DevCounters *__restrict__ counters) {
    constexpr bool COUNT = false, POOL = true, EXT = true, SPH = false, NEE = false, AOV = true, ENV = false, MEDIA = false, MOTION = false;
#include "render_body.h"
}

#if !defined(RT_ENV_TU) && !defined(RT_MEDIA_TU) && !defined(RT_MOTION_TU)  // (render_env.hip, render_media.hip and render_motion.hip include this file for the helpers above and define their own kernels)
// fixed-point pixel sums -> fp32 framebuffer (rgb_sum[(row*W + x)*3 + c]); every store
// instruction writes 256 contiguous bytes
__global__ __launch_bounds__(256) void finalize_kernel(const unsigned long long *__restrict__ acc,
                                                       float *__restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)((double)(long long)acc[i] * (1.0 / 16777216.0));
}

#endif  // RT_ENV_TU, RT_MEDIA_TU, RT_MOTION_TU

#if defined(RT_ENV_TU) || defined(RT_MEDIA_TU) || defined(RT_MOTION_TU)
#elif defined(RT_ISA_ONLY)
// tools/isa_stats.py: one instance alone (RT_ISA_ONLY = its template arguments), compiled to assembly in seconds
template __global__ void render_kernel<RT_ISA_ONLY>(const RenderParams, const float4 *__restrict__, unsigned long long *__restrict__,
                                                    unsigned int *__restrict__, DevCounters *__restrict__);
#elif defined(RT_ISA_ONLY_NEE)
// ... and one light-sampling instance (RT_ISA_ONLY_NEE = SCALAR, CULL)
template __global__ void render_nee_kernel<RT_ISA_ONLY_NEE>(const RenderParams, const float4 *__restrict__, unsigned long long *__restrict__,
                                                            unsigned int *__restrict__, DevCounters *__restrict__);
#elif defined(RT_ISA_ONLY_NESTED)
// ... and one nested-grid instance (RT_ISA_ONLY_NESTED = COUNT, EXT)
template __global__ void render_nested_kernel<RT_ISA_ONLY_NESTED>(const RenderParams, const float4 *__restrict__, unsigned long long *__restrict__,
                                                                  unsigned int *__restrict__, DevCounters *__restrict__);
#elif defined(RT_ISA_ONLY_AOV)
// ... and one feature instance (RT_ISA_ONLY_AOV = SCALAR, CULL)
template __global__ void render_feature_kernel<RT_ISA_ONLY_AOV>(const RenderParams, const float4 *__restrict__, unsigned long long *__restrict__,
                                                                unsigned int *__restrict__, DevCounters *__restrict__);
#else
// ---------------------------------------------------------------- launchers used by render_host.hip
// X(variant id, POOL, SCALAR, CULL, SPH).  The host resolves variant 0 to one of the five PRODUCT instances:
//    2  compact grid one cell high, tables in LDS (RTIOW)         6  compact grid, 3-D walk, tables in LDS (sphere-only scenes)
//   36  wide grid tables in LDS (scenes with other primitives)   44  wide grid tables in global memory (large scenes)
//   16  no culling -- the reference's linear hittable_list scan: what a scene of a handful of primitives of several types runs
//       (nothing is listed in a grid there; sample_scene.json 54 ms against 79 ms for 36 with its empty grid), and the
//       definition every other kernel's image is held to
// and 36, 44 and 16 also exist with EXT (triangles, image textures): eight render_kernel instances in a product build
// (make ABLATIONS=0), beside the light-sampling kernels and variant 52, the nested-grid walk (render_nested_kernel: scenes with
// the nested grid on and a cell to nest; plain and EXT in every build, its counting build with RTMI_ABLATIONS).  The default build (RTMI_ABLATIONS=1: tests, bench.py) adds the measurement variants -- same image, bit for
// bit -- and the counting kernels:
//    1  variant 6 with strict one-lane-per-pixel ownership       40  variant 6 with its tables in global memory
//   17  variant 16 with strict ownership                         24  variant 16 with its tables in global memory
//   32  wave-level cluster votes      64  per-lane cluster lists through the two-level box hierarchy (round 1's default)
//  128  per-lane cluster lists through the range tables (first half of round 2)
#define RT_PRODUCT_TABLE(X)          \
    X(2, true, false, 6, true)       \
    X(6, true, false, 5, true)       \
    X(36, true, false, 7, false)     \
    X(44, true, true, 7, false)      \
    X(16, true, false, 0, false)
#define RT_PRODUCT_EXT_TABLE(X)      \
    X(36, true, false, 7, false)     \
    X(44, true, true, 7, false)      \
    X(16, true, false, 0, false)
#if RTMI_ABLATIONS
#define RT_ABLATION_TABLE(X)         \
    X(1, false, false, 5, true)      \
    X(40, true, true, 5, true)       \
    X(17, false, false, 0, false)    \
    X(24, true, true, 0, false)      \
    X(32, true, false, 1, false)     \
    X(64, true, false, 2, false)     \
    X(128, true, false, 3, false)
#define RT_ABLATION_EXT_TABLE(X) X(24, true, true, 0, false)
// counting kernels (rt_render_hip_count): X(variant, SCALAR, CULL, EXT, SPH)
#define RT_COUNT_TABLE(X)            \
    X(6, false, 5, false, true)      \
    X(36, false, 7, true, false)     \
    X(44, true, 7, true, false)      \
    X(64, false, 2, false, false)    \
    X(128, false, 3, false, false)
#else
#define RT_ABLATION_TABLE(X)
#define RT_ABLATION_EXT_TABLE(X)
#define RT_COUNT_TABLE(X)
#endif
// light-sampling kernels (render_nee_kernel, every build): X(variant, SCALAR, CULL) -- the layouts of variant 0's general scenes
#define RT_NEE_TABLE(X) \
    X(36, false, 7)     \
    X(44, true, 7)      \
    X(16, false, 0)
// feature kernels (render_feature_kernel, every build): X(layout, SCALAR, CULL) -- the layouts of variant 0's general scenes, the
// nested walk, and the linear scan over global memory (24) for compact-table scenes whose scan tables do not fit LDS
#define RT_FEATURE_TABLE(X) \
    X(36, false, 7)         \
    X(44, true, 7)          \
    X(16, false, 0)         \
    X(24, true, 0)          \
    X(52, true, 8)
#define RT_VARIANT_TABLE(X) RT_PRODUCT_TABLE(X) RT_ABLATION_TABLE(X)
#define RT_EXT_TABLE(X) RT_PRODUCT_EXT_TABLE(X) RT_ABLATION_EXT_TABLE(X)

constexpr unsigned kNestedVariant = 52;  // render_nested_kernel

bool has_ablations() { return RTMI_ABLATIONS != 0; }

// launches the instance of a RESOLVED variant (never 0); false: no such build
bool launch_render(const RenderParams &P, const void *image, unsigned long long *acc, unsigned int *queue,
                   DevCounters *counters, size_t lds_bytes, unsigned grid, hipStream_t stream, unsigned variant, bool ext) {
    const float4 *img = (const float4 *)image;
    const dim3 g(grid), t(256);
    if (variant == kNestedVariant) {
        if (counters) {
#if RTMI_ABLATIONS
            hipLaunchKernelGGL((render_nested_kernel<true, true>), g, t, lds_bytes, stream, P, img, acc, queue, counters);
            return true;
#else
            return false;
#endif
        }
        DevCounters *no_counters = nullptr;
        if (ext) hipLaunchKernelGGL((render_nested_kernel<false, true>), g, t, lds_bytes, stream, P, img, acc, queue, no_counters);
        else hipLaunchKernelGGL((render_nested_kernel<false, false>), g, t, lds_bytes, stream, P, img, acc, queue, no_counters);
        return true;
    }
    if (counters) {
#define RT_LAUNCH_COUNT(V, SCALAR, CULL, EXT, SPH)                                                                                         \
    if (variant == V) {                                                                                                                     \
        hipLaunchKernelGGL((render_kernel<true, true, SCALAR, CULL, EXT, SPH>), g, t, lds_bytes, stream, P, img, acc, queue, counters);   \
        return true;                                                                                                                        \
    }
        RT_COUNT_TABLE(RT_LAUNCH_COUNT)
#undef RT_LAUNCH_COUNT
        return false;
    }
    DevCounters *none = nullptr;
    if (ext) {
#define RT_LAUNCH_EXT(V, POOL, SCALAR, CULL, SPH)                                                                                          \
    if (variant == V) {                                                                                                                     \
        hipLaunchKernelGGL((render_kernel<false, POOL, SCALAR, CULL, true, false>), g, t, lds_bytes, stream, P, img, acc, queue, none);   \
        return true;                                                                                                                        \
    }
        RT_EXT_TABLE(RT_LAUNCH_EXT)
#undef RT_LAUNCH_EXT
        return false;
    }
#define RT_LAUNCH(V, POOL, SCALAR, CULL, SPH)                                                                                              \
    if (variant == V) {                                                                                                                     \
        hipLaunchKernelGGL((render_kernel<false, POOL, SCALAR, CULL, false, SPH>), g, t, lds_bytes, stream, P, img, acc, queue, none);    \
        return true;                                                                                                                        \
    }
    RT_VARIANT_TABLE(RT_LAUNCH)
#undef RT_LAUNCH
    return false;
}

// launches the light-sampling kernel of a layout (16, 36 or 44); false: no such build
bool launch_render_nee(const RenderParams &P, const void *image, unsigned long long *acc, unsigned int *queue, size_t lds_bytes,
                       unsigned grid, hipStream_t stream, unsigned variant) {
    const float4 *img = (const float4 *)image;
    DevCounters *none = nullptr;
#define RT_LAUNCH_NEE(V, SCALAR, CULL)                                                                                   \
    if (variant == V) {                                                                                                   \
        hipLaunchKernelGGL((render_nee_kernel<SCALAR, CULL>), dim3(grid), dim3(256), lds_bytes, stream, P, img, acc, queue, none); \
        return true;                                                                                                      \
    }
    RT_NEE_TABLE(RT_LAUNCH_NEE)
#undef RT_LAUNCH_NEE
    return false;
}

// launches the feature kernel of a layout (RT_FEATURE_TABLE); false: no such build
bool launch_render_feature(const RenderParams &P, const void *image, unsigned long long *acc, unsigned int *queue, size_t lds_bytes,
                           unsigned grid, hipStream_t stream, unsigned layout) {
    const float4 *img = (const float4 *)image;
    DevCounters *none = nullptr;
#define RT_LAUNCH_AOV(V, SCALAR, CULL)                                                                                        \
    if (layout == V) {                                                                                                         \
        hipLaunchKernelGGL((render_feature_kernel<SCALAR, CULL>), dim3(grid), dim3(256), lds_bytes, stream, P, img, acc, queue, none); \
        return true;                                                                                                           \
    }
    RT_FEATURE_TABLE(RT_LAUNCH_AOV)
#undef RT_LAUNCH_AOV
    return false;
}

int blocks_per_cu_feature(unsigned layout, size_t lds_bytes) {
    int n = 0;
    hipError_t e = hipErrorInvalidValue;
#define RT_OCC_AOV(V, SCALAR, CULL) \
    if (layout == V) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_feature_kernel<SCALAR, CULL>, 256, lds_bytes);
    RT_FEATURE_TABLE(RT_OCC_AOV)
#undef RT_OCC_AOV
    return (e == hipSuccess && n > 0) ? n : 4;
}

bool variant_has_nee(unsigned variant) {
#define RT_HAS_NEE(V, SCALAR, CULL) \
    if (variant == V) return true;
    RT_NEE_TABLE(RT_HAS_NEE)
#undef RT_HAS_NEE
    return false;
}

int blocks_per_cu_nee(unsigned variant, size_t lds_bytes) {
    int n = 0;
    hipError_t e = hipErrorInvalidValue;
#define RT_OCC_NEE(V, SCALAR, CULL) \
    if (variant == V) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_nee_kernel<SCALAR, CULL>, 256, lds_bytes);
    RT_NEE_TABLE(RT_OCC_NEE)
#undef RT_OCC_NEE
    return (e == hipSuccess && n > 0) ? n : 4;
}

// resident workgroups per CU of a variant at this dynamic-LDS size (advisory; an over-estimate only
// leaves late workgroups that find the queue empty)
int blocks_per_cu(unsigned variant, bool count, size_t lds_bytes, bool ext) {
    int n = 0;
    hipError_t e = hipErrorInvalidValue;
    if (variant == kNestedVariant) {
#if RTMI_ABLATIONS
        if (count) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_nested_kernel<true, true>, 256, lds_bytes);
#endif
        if (!count && ext) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_nested_kernel<false, true>, 256, lds_bytes);
        if (!count && !ext) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_nested_kernel<false, false>, 256, lds_bytes);
    } else if (count) {
#define RT_OCC_COUNT(V, SCALAR, CULL, EXT, SPH) \
    if (variant == V) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_kernel<true, true, SCALAR, CULL, EXT, SPH>, 256, lds_bytes);
        RT_COUNT_TABLE(RT_OCC_COUNT)
#undef RT_OCC_COUNT
    } else if (ext) {
#define RT_OCC_EXT(V, POOL, SCALAR, CULL, SPH) \
    if (variant == V) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_kernel<false, POOL, SCALAR, CULL, true, false>, 256, lds_bytes);
        RT_EXT_TABLE(RT_OCC_EXT)
#undef RT_OCC_EXT
    } else {
#define RT_OCC(V, POOL, SCALAR, CULL, SPH) \
    if (variant == V) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_kernel<false, POOL, SCALAR, CULL, false, SPH>, 256, lds_bytes);
        RT_VARIANT_TABLE(RT_OCC)
#undef RT_OCC
    }
    return (e == hipSuccess && n > 0) ? n : 4;
}

// candidate search of a variant (the CULL template argument): decides how much of the hot table is staged; -1: no such build
int variant_cull_mode(unsigned variant) {
    if (variant == kNestedVariant) return 8;
#define RT_MODE(V, POOL, SCALAR, CULL, SPH) \
    if (variant == V) return CULL;
    RT_VARIANT_TABLE(RT_MODE)
#undef RT_MODE
    return -1;
}

// does the variant have a build with triangles and image textures?
bool variant_has_ext(unsigned variant) {
    if (variant == kNestedVariant) return true;
#define RT_HAS_EXT(V, POOL, SCALAR, CULL, SPH) \
    if (variant == V) return true;
    RT_EXT_TABLE(RT_HAS_EXT)
#undef RT_HAS_EXT
    return false;
}

bool variant_has_count(unsigned variant) {
    if (variant == kNestedVariant) return RTMI_ABLATIONS != 0;
#define RT_HAS_COUNT(V, SCALAR, CULL, EXT, SPH) \
    if (variant == V) return true;
    RT_COUNT_TABLE(RT_HAS_COUNT)
#undef RT_HAS_COUNT
    return false;
}

bool variant_exists(unsigned variant) { return variant == 0 || variant_cull_mode(variant) >= 0; }

__global__ void item_params_kernel(unsigned int *queue, ItemParams ip) {
    int *dst = reinterpret_cast<int *>(queue) + RT_ITEM_PARAMS_AT;
    // quad 0: tiles_x, bands, num_items, sample_first; quad 1: sample_count, spp_chunk, n_big, n_med;
    // quad 2: q_med, q_small, tile_rotate, n_list; quad 3: tile_rows, tile_first, tile_stride, local_rows
    const int v[16] = {ip.tiles_x, ip.bands, ip.num_items, ip.sample_first, ip.sample_count, ip.spp_chunk, ip.n_big,
                       ip.n_med, ip.q_med, ip.q_small, ip.tile_rotate, ip.n_list, ip.tile_rows, ip.tile_first, ip.tile_stride, ip.local_rows};
    for (int k = 0; k < 16; ++k) dst[k] = v[k];
}

void launch_item_params(unsigned int *queue, const ItemParams &ip, hipStream_t stream) {
    hipLaunchKernelGGL(item_params_kernel, dim3(1), dim3(1), 0, stream, queue, ip);
}

void launch_finalize(const unsigned long long *acc, float *out, size_t n, hipStream_t stream) {
    unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(finalize_kernel, dim3(grid), dim3(256), 0, stream, acc, out, n);
}

int set_max_dynamic_lds_env(size_t bytes);    // render_env.hip
int set_max_dynamic_lds_media(size_t bytes);  // render_media.hip
int set_max_dynamic_lds_motion(size_t bytes); // render_motion.hip

int set_max_dynamic_lds(size_t bytes) {
#define RT_ATTR1(K)                                                                                                  \
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return 1;
#define RT_ATTR(V, POOL, SCALAR, CULL, SPH) RT_ATTR1((render_kernel<false, POOL, SCALAR, CULL, false, SPH>))
    RT_VARIANT_TABLE(RT_ATTR)
#undef RT_ATTR
#define RT_ATTR_EXT(V, POOL, SCALAR, CULL, SPH) RT_ATTR1((render_kernel<false, POOL, SCALAR, CULL, true, false>))
    RT_EXT_TABLE(RT_ATTR_EXT)
#undef RT_ATTR_EXT
#define RT_ATTR_COUNT(V, SCALAR, CULL, EXT, SPH) RT_ATTR1((render_kernel<true, true, SCALAR, CULL, EXT, SPH>))
    RT_COUNT_TABLE(RT_ATTR_COUNT)
#undef RT_ATTR_COUNT
#define RT_ATTR_NEE(V, SCALAR, CULL) RT_ATTR1((render_nee_kernel<SCALAR, CULL>))
    RT_NEE_TABLE(RT_ATTR_NEE)
#undef RT_ATTR_NEE
#define RT_ATTR_AOV(V, SCALAR, CULL) RT_ATTR1((render_feature_kernel<SCALAR, CULL>))
    RT_FEATURE_TABLE(RT_ATTR_AOV)
#undef RT_ATTR_AOV
#undef RT_ATTR1
    return set_max_dynamic_lds_env(bytes) || set_max_dynamic_lds_media(bytes) || set_max_dynamic_lds_motion(bytes);
}
#endif  // RT_ENV_TU, RT_MEDIA_TU, RT_MOTION_TU, RT_ISA_ONLY, RT_ISA_ONLY_NEE, RT_ISA_ONLY_NESTED, RT_ISA_ONLY_AOV

}  // namespace rtmi
