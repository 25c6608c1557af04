// Procedural noise textures: gradient noise on the integer lattice (Perlin's improved noise over a hashed
// lattice in place of a permutation table), summed over octaves as fBm, turbulence and marble.  A SOLID texture: evaluated at
// the world-space hit point the checker reads, no (u, v), no memory traffic.  fp32 with a FIXED operation sequence, every
// fused multiply-add explicit, in the manner of rt_glossy.h: the kernels (render_body.h) and a host program
// (tests/noise_host_driver.cpp) compile this text, and tests/ref64_noise.py restates the model in numpy.
//
// The model.  Parameters: style, scale f, octaves K (1..8), seed (uint32), and for marble an axis a and a distortion D.
//   hash(i, j, k; s), all arithmetic mod 2^32 on the lattice coordinates taken as uint32 (two's complement):
//     h = s ^ (i * 0x8DA6B343) ^ (j * 0xD8163841) ^ (k * 0xCB1AB31F)
//     h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16
//   grad(h, x, y, z): the 16-case table of Perlin's improved noise from the TOP four bits, g = h >> 28:
//     u = g < 8 ? x : y;  v = g < 4 ? y : ((g == 12 || g == 14) ? x : z);  grad = ((g & 1) ? -u : u) + ((g & 2) ? -v : v)
//   n(q, s): q clamped to [-2^30, 2^30] per component (a NaN becomes 0), c = floor(q) as int32, t = q - floor(q); the eight
//     corners (dx, dy, dz) in {0, 1}^3 give grad(hash(c + (dx, dy, dz), s), t - (dx, dy, dz)); the fade is
//     w(t) = t^3 (t (6 t - 15) + 10) per axis; interpolated along x, then y, then z with a + w (b - a).
//     n is 0 at every lattice point and lies within (-1, 1).
//   octave o = 0 .. K - 1: n_o = n(2^o f p, seed + o) (the doubling is exact, the seed sum wraps);
//     S = sum 2^-o n_o,  A = sum 2^-o |n_o|
//   fbm (0): s = clamp(0.5 + 0.5 S, 0, 1);  turbulence (1): s = min(1, A);  marble (2): s = 0.5 + 0.5 sin(f p[a] + D A)
//   colour: c0 + s (c1 - c0) per channel.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef RTMI_HD
#ifdef __HIPCC__
#define RTMI_HD __host__ __device__ inline
#else
#define RTMI_HD inline
#endif
#endif

namespace rtmi {

#define RT_NOISE_FBM 0
#define RT_NOISE_TURBULENCE 1
#define RT_NOISE_MARBLE 2
#define RT_NOISE_MAX_OCTAVES 8

#define RT_NOISE_KX 0x8DA6B343u
#define RT_NOISE_KY 0xD8163841u
#define RT_NOISE_KZ 0xCB1AB31Fu

// the finaliser over the xor of the seed and the three per-axis products
RTMI_HD uint32_t noise_mix(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

RTMI_HD uint32_t noise_hash(int32_t i, int32_t j, int32_t k, uint32_t s) {
    return noise_mix(s ^ ((uint32_t)i * RT_NOISE_KX) ^ ((uint32_t)j * RT_NOISE_KY) ^ ((uint32_t)k * RT_NOISE_KZ));
}

RTMI_HD float noise_grad(uint32_t h, float x, float y, float z) {
    const uint32_t g = h >> 28;
    const float u = g < 8u ? x : y;
    const float v = g < 4u ? y : ((g == 12u || g == 14u) ? x : z);
    return ((g & 1u) ? -u : u) + ((g & 2u) ? -v : v);
}

RTMI_HD float noise_fade(float t) { return ((t * t) * t) * fmaf(t, fmaf(6.0f, t, -15.0f), 10.0f); }

// floor(q) of the clamped coordinate as a float (what t is taken from) and as int32: |q| <= 2^30 converts exactly, and the
// comparison chain sends a NaN to 0 without a conversion of one
RTMI_HD float noise_cell(float q, int32_t &c) {
    float x = q >= -1073741824.0f ? q : -1073741824.0f;  // (a NaN fails the comparison: -2^30 ...
    x = x <= 1073741824.0f ? x : 1073741824.0f;
    if (!(q == q)) x = 0.0f;                             // ... and becomes 0 here)
    const float fl = floorf(x);
    c = (int32_t)fl;
    return x - fl;
}

// n(q, s): one evaluation of the lattice noise.  The per-axis products of the hash differ by a constant between the two
// corners of an axis ((i + 1) K = i K + K): three multiplies for the cell, then two per corner in the finaliser.
RTMI_HD float noise3(float qx, float qy, float qz, uint32_t s) {
    int32_t ci, cj, ck;
    const float tx = noise_cell(qx, ci), ty = noise_cell(qy, cj), tz = noise_cell(qz, ck);
    const uint32_t x0 = s ^ ((uint32_t)ci * RT_NOISE_KX), x1 = s ^ ((uint32_t)ci * RT_NOISE_KX + RT_NOISE_KX);
    const uint32_t y0 = (uint32_t)cj * RT_NOISE_KY, y1 = y0 + RT_NOISE_KY;
    const uint32_t z0 = (uint32_t)ck * RT_NOISE_KZ, z1 = z0 + RT_NOISE_KZ;
    const float ux = tx - 1.0f, uy = ty - 1.0f, uz = tz - 1.0f;
    const float wx = noise_fade(tx), wy = noise_fade(ty), wz = noise_fade(tz);
    const float g000 = noise_grad(noise_mix(x0 ^ y0 ^ z0), tx, ty, tz), g100 = noise_grad(noise_mix(x1 ^ y0 ^ z0), ux, ty, tz);
    const float g010 = noise_grad(noise_mix(x0 ^ y1 ^ z0), tx, uy, tz), g110 = noise_grad(noise_mix(x1 ^ y1 ^ z0), ux, uy, tz);
    const float g001 = noise_grad(noise_mix(x0 ^ y0 ^ z1), tx, ty, uz), g101 = noise_grad(noise_mix(x1 ^ y0 ^ z1), ux, ty, uz);
    const float g011 = noise_grad(noise_mix(x0 ^ y1 ^ z1), tx, uy, uz), g111 = noise_grad(noise_mix(x1 ^ y1 ^ z1), ux, uy, uz);
    const float a00 = fmaf(wx, g100 - g000, g000), a10 = fmaf(wx, g110 - g010, g010);
    const float a01 = fmaf(wx, g101 - g001, g001), a11 = fmaf(wx, g111 - g011, g011);
    const float b0 = fmaf(wy, a10 - a00, a00), b1 = fmaf(wy, a11 - a01, a01);
    return fmaf(wz, b1 - b0, b0);
}

// sin of marble's phase: rt_trig.h's in the kernels' manner is not needed -- the phase is a few radians and the result
// is compared at 1e-4 -- but host and device must agree on WHICH sine: sinf on both (device: the ocml routine, correct to
// 1-2 ulp; a colour differs by parts in 1e-7 between the two, far inside the per-sample tolerance)
RTMI_HD float noise_sinf(float x) { return sinf(x); }

// the texture's scalar s in [0, 1] at the point p
RTMI_HD float noise_value(int style, float scale, int octaves, uint32_t seed, int axis, float distortion, float px, float py, float pz) {
    float qx = scale * px, qy = scale * py, qz = scale * pz;
    float sum = 0.0f, amp = 1.0f;
    for (int o = 0; o < octaves; ++o) {
        const float n = noise3(qx, qy, qz, seed + (uint32_t)o);
        sum = fmaf(amp, style == RT_NOISE_FBM ? n : fabsf(n), sum);
        amp *= 0.5f;
        qx *= 2.0f, qy *= 2.0f, qz *= 2.0f;
    }
    float v;
    if (style == RT_NOISE_FBM) {
        v = fminf(1.0f, fmaxf(0.0f, fmaf(0.5f, sum, 0.5f)));
    } else if (style == RT_NOISE_TURBULENCE) {
        v = fminf(1.0f, sum);
    } else {
        const float pa = axis == 0 ? px : (axis == 1 ? py : pz);
        v = fmaf(0.5f, noise_sinf(fmaf(distortion, sum, scale * pa)), 0.5f);
    }
    // (a NaN or an infinite coordinate reaches here as a finite sum, except through marble's phase: sin of a non-finite
    // number is a NaN, which the comparison sends to 0)
    return v >= 0.0f ? fminf(v, 1.0f) : 0.0f;
}

// the packed word of a noise record (device_scene.h): style | axis << 2 | octaves << 4
RTMI_HD uint32_t noise_pack(int style, int axis, int octaves) { return (uint32_t)style | (uint32_t)axis << 2 | (uint32_t)octaves << 4; }

// the texture's colour: c0 + s (c1 - c0) per channel
RTMI_HD void noise_color(uint32_t packed, float scale, float distortion, uint32_t seed, float c0r, float c0g, float c0b, float c1r,
                         float c1g, float c1b, float px, float py, float pz, float &r, float &g, float &b) {
    const float s = noise_value((int)(packed & 3u), scale, (int)(packed >> 4) & 15, seed, (int)(packed >> 2) & 3, distortion, px, py, pz);
    r = fmaf(s, c1r - c0r, c0r), g = fmaf(s, c1g - c0g, c0g), b = fmaf(s, c1b - c0b, c0b);
}

}  // namespace rtmi
