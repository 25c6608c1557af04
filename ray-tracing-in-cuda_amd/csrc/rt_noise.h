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

// ---------------------------------------------------------------- the gradient, for bump mapping
// The lattice noise is a quintic-faded trilinear interpolation of LINEAR corner functions g_abc(t) = G_abc . (t - (a, b, c)),
// so its gradient is analytic and comes from the same eight hashes in the same pass:
//   dn/dx = sum_abc Wa(tx) Wb(ty) Wc(tz) G_abc.x + w'(tx) sum_bc Wb(ty) Wc(tz) (g_1bc - g_0bc),  w'(t) = 30 t^2 (t - 1)^2
// and likewise for y and z, with W0 = 1 - w, W1 = w.  A coordinate outside (-2^30, 2^30), or a NaN, has a zero component.
//   grad S = f sum_o grad_q n(2^o f p, seed + o)  (the chain rule's 2^o cancels the amplitude 2^-o),
//   grad A = f sum_o sgn(n_o) grad_q n_o, sgn(0) = 0
//   fbm: grad s = 0.5 grad S where 0 < 0.5 + 0.5 S < 1, else 0;  turbulence: grad s = grad A where A < 1, else 0
//   marble: grad s = 0.5 cos(f p[a] + D A) (f e_a + D grad A)

// noise_grad's value and the constant corner gradient G it selects: (+-1, +-1, 0) and its kin, components in {-1, 0, 1}
RTMI_HD float noise_grad_vec(uint32_t h, float x, float y, float z, float &Gx, float &Gy, float &Gz) {
    const uint32_t g = h >> 28;
    const bool vx = g == 12u || g == 14u;
    const float su = (g & 1u) ? -1.0f : 1.0f, sv = (g & 2u) ? -1.0f : 1.0f;
    Gx = g < 8u ? su : (vx ? sv : 0.0f);
    Gy = g < 4u ? sv : (g < 8u ? 0.0f : su);
    Gz = (g < 4u || vx) ? 0.0f : sv;
    const float u = g < 8u ? x : y;
    const float v = g < 4u ? y : (vx ? x : z);
    return ((g & 1u) ? -u : u) + ((g & 2u) ? -v : v);
}

RTMI_HD float noise_fade_deriv(float t) {
    const float a = t * (t - 1.0f);
    return 30.0f * (a * a);
}

// is the coordinate one that noise_cell leaves alone (inside the clamp, not a NaN)?
RTMI_HD bool noise_free(float q) { return q > -1073741824.0f && q < 1073741824.0f; }

// one x edge of the cell: its two corners' values (d = g1 - g0) and the components of G, interpolated along x
struct NoiseEdge {
    float a, d, Gx, Gy, Gz;
};
RTMI_HD void noise_edge(uint32_t x0, uint32_t x1, uint32_t yz, float tx, float ux, float vy, float vz, float wx, NoiseEdge &e) {
    float G0x, G0y, G0z, G1x, G1y, G1z;
    const float g0 = noise_grad_vec(noise_mix(x0 ^ yz), tx, vy, vz, G0x, G0y, G0z);
    const float g1 = noise_grad_vec(noise_mix(x1 ^ yz), ux, vy, vz, G1x, G1y, G1z);
    e.d = g1 - g0;
    e.a = fmaf(wx, e.d, g0);
    e.Gx = fmaf(wx, G1x - G0x, G0x), e.Gy = fmaf(wx, G1y - G0y, G0y), e.Gz = fmaf(wx, G1z - G0z, G0z);
}

// n(q, s) as noise3 gives it, and its gradient with respect to q
RTMI_HD float noise3_grad(float qx, float qy, float qz, uint32_t s, float &dnx, float &dny, float &dnz) {
    int32_t ci, cj, ck;
    const float tx = noise_cell(qx, ci), ty = noise_cell(qy, cj), tz = noise_cell(qz, ck);
    const uint32_t x0 = s ^ ((uint32_t)ci * RT_NOISE_KX), x1 = s ^ ((uint32_t)ci * RT_NOISE_KX + RT_NOISE_KX);
    const uint32_t y0 = (uint32_t)cj * RT_NOISE_KY, y1 = y0 + RT_NOISE_KY;
    const uint32_t z0 = (uint32_t)ck * RT_NOISE_KZ, z1 = z0 + RT_NOISE_KZ;
    const float ux = tx - 1.0f, uy = ty - 1.0f, uz = tz - 1.0f;
    const float wx = noise_fade(tx), wy = noise_fade(ty), wz = noise_fade(tz);
    // the four x edges (y0 z0, y1 z0, y0 z1, y1 z1), then along y, then z
    NoiseEdge e0, e1, e2, e3;
    noise_edge(x0, x1, y0 ^ z0, tx, ux, ty, tz, wx, e0);
    noise_edge(x0, x1, y1 ^ z0, tx, ux, uy, tz, wx, e1);
    noise_edge(x0, x1, y0 ^ z1, tx, ux, ty, uz, wx, e2);
    noise_edge(x0, x1, y1 ^ z1, tx, ux, uy, uz, wx, e3);
    const float dY0 = e1.a - e0.a, dY1 = e3.a - e2.a;
    const float b0 = fmaf(wy, dY0, e0.a), b1 = fmaf(wy, dY1, e2.a);
    const float dZ = b1 - b0;
    const float n = fmaf(wz, dZ, b0);
    const float bx0 = fmaf(wy, e1.Gx - e0.Gx, e0.Gx), bx1 = fmaf(wy, e3.Gx - e2.Gx, e2.Gx);
    const float by0 = fmaf(wy, e1.Gy - e0.Gy, e0.Gy), by1 = fmaf(wy, e3.Gy - e2.Gy, e2.Gy);
    const float bz0 = fmaf(wy, e1.Gz - e0.Gz, e0.Gz), bz1 = fmaf(wy, e3.Gz - e2.Gz, e2.Gz);
    const float ex0 = fmaf(wy, e1.d - e0.d, e0.d), ex1 = fmaf(wy, e3.d - e2.d, e2.d);
    dnx = fmaf(noise_fade_deriv(tx), fmaf(wz, ex1 - ex0, ex0), fmaf(wz, bx1 - bx0, bx0));
    dny = fmaf(noise_fade_deriv(ty), fmaf(wz, dY1 - dY0, dY0), fmaf(wz, by1 - by0, by0));
    dnz = fmaf(noise_fade_deriv(tz), dZ, fmaf(wz, bz1 - bz0, bz0));
    if (!noise_free(qx)) dnx = 0.0f;
    if (!noise_free(qy)) dny = 0.0f;
    if (!noise_free(qz)) dnz = 0.0f;
    return n;
}

RTMI_HD float noise_cosf(float x) { return cosf(x); }  // (as noise_sinf: the same cosine on host and device)

// grad s of the texture's scalar with respect to the world point p
RTMI_HD void noise_gradient(int style, float scale, int octaves, uint32_t seed, int axis, float distortion, float px, float py, float pz,
                            float &gx, float &gy, float &gz) {
    float qx = scale * px, qy = scale * py, qz = scale * pz;
    float sum = 0.0f, amp = 1.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int o = 0; o < octaves; ++o) {
        float dx, dy, dz;
        const float n = noise3_grad(qx, qy, qz, seed + (uint32_t)o, dx, dy, dz);
        sum = fmaf(amp, style == RT_NOISE_FBM ? n : fabsf(n), sum);
        const float sg = style == RT_NOISE_FBM ? 1.0f : (n > 0.0f ? 1.0f : (n < 0.0f ? -1.0f : 0.0f));
        sx = fmaf(sg, dx, sx), sy = fmaf(sg, dy, sy), sz = fmaf(sg, dz, sz);
        amp *= 0.5f;
        qx *= 2.0f, qy *= 2.0f, qz *= 2.0f;
    }
    sx *= scale, sy *= scale, sz *= scale;
    if (style == RT_NOISE_FBM) {
        const float v = fmaf(0.5f, sum, 0.5f);
        const float m = (v > 0.0f && v < 1.0f) ? 0.5f : 0.0f;
        gx = m * sx, gy = m * sy, gz = m * sz;
    } else if (style == RT_NOISE_TURBULENCE) {
        const float m = sum < 1.0f ? 1.0f : 0.0f;
        gx = m * sx, gy = m * sy, gz = m * sz;
    } else {
        const float pa = axis == 0 ? px : (axis == 1 ? py : pz);
        const float c = 0.5f * noise_cosf(fmaf(distortion, sum, scale * pa));
        gx = c * fmaf(distortion, sx, axis == 0 ? scale : 0.0f);
        gy = c * fmaf(distortion, sy, axis == 1 ? scale : 0.0f);
        gz = c * fmaf(distortion, sz, axis == 2 ? scale : 0.0f);
    }
}

// The bump.  n: the face-turned shading normal, g: the face-turned geometric one, d: the ray's direction (any
// length), sk = sigma k (sigma = +1 on a front hit, -1 on a back hit: height is measured along the OUTWARD normal), G = grad s:
//   Gt = G - (G . n) n,  b = n - sigma k Gt,  n' = b / |b|
// n' replaces n iff it is finite, n' . g > 0 and n' . d < 0; else n stays.  root: the caller's square root (the kernels':
// rt_sqrtf).  -> was n replaced
template <class Root>
RTMI_HD bool noise_bump(float &nx, float &ny, float &nz, float gnx, float gny, float gnz, float dx, float dy, float dz, float sk, float Gx,
                        float Gy, float Gz, Root root) {
    const float gn = fmaf(Gx, nx, fmaf(Gy, ny, Gz * nz));
    const float tx = fmaf(-gn, nx, Gx), ty = fmaf(-gn, ny, Gy), tz = fmaf(-gn, nz, Gz);
    const float bx = fmaf(-sk, tx, nx), by = fmaf(-sk, ty, ny), bz = fmaf(-sk, tz, nz);
    const float l2 = fmaf(bx, bx, fmaf(by, by, bz * bz));
    if (!(l2 > 0.0f && l2 < INFINITY)) return false;  // (a NaN fails the comparison)
    const float inv = 1.0f / root(l2);
    const float ux = inv * bx, uy = inv * by, uz = inv * bz;
    if (!(fmaf(ux, gnx, fmaf(uy, gny, uz * gnz)) > 0.0f && fmaf(ux, dx, fmaf(uy, dy, uz * dz)) < 0.0f)) return false;
    nx = ux, ny = uy, nz = uz;
    return true;
}

}  // namespace rtmi
