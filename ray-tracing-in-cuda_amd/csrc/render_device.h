// Device helpers shared by the render kernels (render_kernel.hip, render_env.hip, render_media.hip, render_motion.hip): the
// build-time knobs of the kernels (waves per SIMD, wave priorities), the per-lane generator, the IEEE square root, the small
// vector and texture helpers, the fixed-point conversion of a radiance sample and the light-sampling densities -- what
// render_body.h, the text of the kernels' body, calls.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "device_scene.h"
#include "philox.h"
#include "rt_env.h"
#include "rt_media.h"
#include "rt_motion.h"
#include "rt_trace.h"
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

// ---------------------------------------------------------------- ray queries (trace.hip)
// what trace_kernel gets beside the scene: n rays of two 16-byte records each {origin, t_max} {dir, reserved}; out: three
// 16-byte records per ray (mode 0, rt_hit) or one byte per ray (mode 1).  The render kernels carry a null one (render_body.h
// names its members in text that is compiled, and discarded, there).
struct TraceArgs {
    const float4 *rays;
    float4 *out;
    uint32_t n;
    int32_t mode;
};

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

// IEEE-correct fp32 square root, bit for bit what sqrtf() returns, for arguments that are ordinary numbers -- the kernel's
// discriminants and squared lengths: ~10 per iteration of its main loop.  hipcc expands sqrtf() to v_sqrt_f32 (1 ulp) plus a
// one-step correction, wrapped in a scaling for arguments below 2^-96 (v_sqrt_f32 flushes denormals) and a fix-up for 0 and
// inf: 17 instructions.  Here that wrapping only runs -- through sqrtf() itself -- when an argument really needs it.
// VOTE (the grid walks' kernels, render_body.h's ROOT_VOTE): the guard is a vote of the wave -- sqrtf() is exact everywhere, so
// ordinary lanes that go through it with an odd one lose nothing -- i.e. one compare and one scalar branch (not taken) behind
// the root, no exec-mask bookkeeping around it; and the root is the compiler's own correctly rounded sequence for flushed-denormal mode, one
// v_rsq_f32 and seven plain instructions without a compare or a select (inside the guarded range every intermediate value is a
// normal number).  Held to sqrtf() on all 2^32 bit patterns on the device (csrc/sqrt_sweep.hip).
// !VOTE (the nested walk, whose spilled registers rise with the vote, and the glossy materials): the guard per lane, then
// v_sqrt_f32 and the +-1 ulp correction.
template <bool VOTE = false>
__device__ __forceinline__ float rt_sqrtf(float x) {
    // [2^-96, inf): one unsigned compare on the bit pattern (negative numbers and NaN fall outside as well)
    const bool odd = (uint32_t)(__float_as_uint(x) - 0x0f800000u) >= (0x7f800000u - 0x0f800000u);
    if (VOTE) {
        // the root first, the vote after it: returning sqrtf(x) from inside the voted branch made the compiler rejoin the two
        // paths through a mask and a second branch in front of every fast root.  A wave with an odd lane has run the
        // sequence on arguments outside its range; it has no side effects, and sqrtf() replaces the result in every lane.
        const float r = __builtin_amdgcn_rsqf(x);
        float s = x * r, h = 0.5f * r;
        const float e = fmaf(-h, s, 0.5f);
        h = fmaf(h, e, h), s = fmaf(s, e, s);
        const float d = fmaf(-s, s, x);
        float res = fmaf(d, h, s);
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(odd) != 0ull, 0)) res = sqrtf(x);
        return res;
    }
    if (__builtin_expect(odd, 0)) return sqrtf(x);
    const float s = __builtin_amdgcn_sqrtf(x);
    const float s_dn = __uint_as_float(__float_as_uint(s) - 1u), s_up = __uint_as_float(__float_as_uint(s) + 1u);
    const float r_dn = fmaf(-s_dn, s, x), r_up = fmaf(-s_up, s, x);
    float r = r_dn <= 0.0f ? s_dn : s;
    r = r_up > 0.0f ? s_up : r;
    return r;
}

// number of set bits of a lane mask as a 32-bit SCALAR (popcll's result is compared as a 64-bit value, for which the
// scalar unit has no ordered compare: the comparison then runs on the vector ALU, once per pass of the walk's loops).
// One 64-bit scalar popcount: the builtin on two halves compiled to two 32-bit counts and an add, and the compare behind
// it to a mask (s_cselect, s_and with exec, a branch on vcc) where four of the six sites now branch on scc.  Plain asm, not
// volatile: a pure function of its operand.
__device__ __forceinline__ int mask_count(unsigned long long m) {
    int r;
    asm("s_bcnt1_i32_b64 %0, %1" : "=s"(r) : "s"(m) : "scc");
    return r;
}

// fminf for operands that are results of fp32 arithmetic or +-inf, never a signalling NaN: the bare v_min_f32 / v_min3_f32,
// which in the kernel's IEEE mode return the other operand for a quiet NaN, as fminf does.  fminf() itself quiets every
// operand whose origin the compiler cannot see (a value carried round a loop) with a v_max_f32 x, x, x of its own first.
// As inline assembly they take vector registers only and are opaque to the compiler -- no constant, scalar operand or source
// modifier folds in, no min3 / med3 forms across them -- so they are for the walk's step pass alone, whose operands are
// lane values in registers anyway; everywhere else fminf stays.
__device__ __forceinline__ float min_arith(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float min3_arith(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// The record `bytes` behind a wave-uniform table address, the offset a 32-bit lane value: the load takes its base from
// scalar registers and its offset from one vector register, and no 64-bit address is put together on the vector ALU.
// The callers' bounds, each refused with RT_ERR_LIMIT where the host would break it: a sphere's cold record, 16 x its slot
// with fewer than RT_MAX_SPHERE_SLOTS = 2^28 slots (pack.hip, lay_out_image); a material's record, 48 x its index with fewer
// than 2^24 materials (scene.cpp, scene_validate).
static_assert(RT_MAX_SPHERE_SLOTS * 16 <= (1LL << 32), "a cold record's byte offset in 32 bits");
__device__ __forceinline__ const float4 *rec_at(const float4 *table, uint32_t bytes) {
    return reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(table) + bytes);
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

// the glossy materials: behind rt_sqrtf, which they use
}  // namespace rtmi
#include "rt_glossy.h"
#include "rt_glass.h"
#include "rt_phase.h"
#include "rt_pbr.h"
#include "rt_noise.h"
#include "rt_quad.h"
#include "rt_lights.h"
#include "rt_tangent.h"
#include "rt_alpha.h"
#include "rt_camera.h"
namespace rtmi {

// a noise texture's colour at the point p: q1 = {c0, offset of the noise record (bits)}, q2 = {c1, _} of the
// material, the record {scale, distortion, seed, style | axis << 2 | octaves << 4} behind the texels (device_scene.h).
// Called from two places (the winner section; a plastic vertex's light sample) and inlined into both; RT_NOISE_INLINE=0 builds
// it as one __noinline__ function returning by value instead.  DESIGN 7o has both forms' rows: the call form is the slower one.
#ifndef RT_NOISE_INLINE
#define RT_NOISE_INLINE 1
#endif
#if RT_NOISE_INLINE
__device__ __forceinline__
#else
__device__ __noinline__
#endif
float4 noise_texel(const float4 *__restrict__ image, const float4 q1, const float4 q2, float px, float py, float pz) {
    const float4 nr = image[__float_as_int(q1.w)];
    float4 c = {0.0f, 0.0f, 0.0f, 0.0f};  // (by value: in registers, where three references would go through scratch)
    noise_color(__float_as_uint(nr.w), nr.x, nr.y, __float_as_uint(nr.z), q1.x, q1.y, q1.z, q2.x, q2.y, q2.z, px, py, pz, c.x, c.y, c.z);
    return c;
}

// the bumped shading normal (the rule: rt_noise.h, noise_bump).  boff: the material's bump record {offset of the noise
// record (bits), strength}; n: the face-turned shading normal, g: the face-turned geometric one, d: the ray's direction, p: the
// hit point.  -> n' where the rule accepts it, else n.  Called from one place, the winner section, and inlined into it;
// RT_BUMP_INLINE=0 builds it as one __noinline__ function returning by value instead.  DESIGN 7p has both forms' rows: the call
// form's save area costs the scenes WITHOUT a bump more (fog_room +22 %, motion_balls +25 %) than the inlined code does.
#ifndef RT_BUMP_INLINE
#define RT_BUMP_INLINE 1
#endif
#if RT_BUMP_INLINE
__device__ __forceinline__
#else
__device__ __noinline__
#endif
float4 bump_normal(const float4 *__restrict__ image, int boff, bool front, float nx, float ny, float nz, float gnx, float gny, float gnz,
                   float dx, float dy, float dz, float px, float py, float pz) {
    const float4 br = image[boff];
    const float4 nr = image[__float_as_int(br.x)];
    const uint32_t packed = __float_as_uint(nr.w);
    float Gx, Gy, Gz;
    noise_gradient((int)(packed & 3u), nr.x, (int)(packed >> 4) & 15, __float_as_uint(nr.z), (int)(packed >> 2) & 3, nr.y, px, py, pz, Gx, Gy, Gz);
    noise_bump(nx, ny, nz, gnx, gny, gnz, dx, dy, dz, front ? br.y : -br.y, Gx, Gy, Gz, [](float x) { return rt_sqrtf(x); });  // (the per-lane root, as the glossy materials')
    const float4 n = {nx, ny, nz, 0.0f};  // (by value: in registers, where three references would go through scratch)
    return n;
}

// a normal map's texel word: image_texel's nearest-texel lookup, with its row and column convention, of the record
// mr = {texel word offset (bits), rows (bits), cols (bits), scale} -> r8 | g8 << 8 | b8 << 16
__device__ __forceinline__ uint32_t image_texel_word(const float4 *__restrict__ image, const float4 mr, float u, float v) {
    const int rows = __float_as_int(mr.y), cols = __float_as_int(mr.z);
    const int x = min((int)((u - floorf(u)) * (float)rows), rows - 1);
    const int y = min((int)((v - floorf(v)) * (float)cols), cols - 1);
    return reinterpret_cast<const uint32_t *>(image)[__float_as_int(mr.x) + x * cols + y];
}

// the mapped shading normal (the rule: rt_tangent.h, tangent_normal) from the raw tangents (T, B) and the decoded
// texel (x, y, z); arguments as bump_normal's.  -> n' where the rule accepts it, else n.  Inlined into the winner section, its
// one caller, as bump_normal is
__device__ __forceinline__ float4 mapped_normal(bool front, float s, float nx, float ny, float nz, float gnx, float gny, float gnz, float dx,
                                                float dy, float dz, float tx, float ty, float tz, float bx, float by, float bz, float x, float y,
                                                float z) {
    tangent_normal(nx, ny, nz, gnx, gny, gnz, dx, dy, dz, front, s, tx, ty, tz, bx, by, bz, x, y, z, [](float v) { return rt_sqrtf(v); });
    const float4 n = {nx, ny, nz, 0.0f};
    return n;
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

}  // namespace rtmi
