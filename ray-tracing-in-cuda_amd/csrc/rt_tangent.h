// Tangent-space normal maps: the texel of an image texture at the hit record's (u, v), read as a direction in the
// surface's tangent frame, replaces the shading normal.  What is new here is the frame: per primitive type the directions in
// which u and v grow at the hit, T = dp/du and B = dp/dv, each up to a positive factor.  fp32 with a FIXED operation sequence,
// every fused multiply-add explicit, in the manner of rt_quad.h and rt_pbr.h: the kernels (render_body.h) and a host program
// (tests/normal_map_host_driver.cpp) compile this text.
//
//   decoding   x = max((r8 - 128) / 127, -1), y from g8, z from b8: byte 128 is exactly 0, byte 255 exactly 1.  A texel with
//              r8 == 128 && g8 == 128, or with z <= 0, leaves the normal as it was (tangent_decode -> false).
//              R runs along +dp/du, G along +dp/dv, B along the outward normal.
//   frame      n: the face-turned shading normal, sigma = +1 on a front hit, -1 on a back hit
//              T' = unit(T - (T.n) n),  B' = unit(B - (B.n) n - (B.T') T');  B' zero or not finite: B' = cross(sigma n, T');
//              T' zero or not finite: n stays
//   normal     b = sigma s (x T' + y B') + z n,  n' = b / |b|;  n' replaces n iff it is finite, n'.g > 0 and n'.d < 0
//              (g: the face-turned geometric normal, d: the ray's direction, any length) -- the two guards of the bump, 7p
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

RTMI_HD float tangent_dot(float ax, float ay, float az, float bx, float by, float bz) { return fmaf(ax, bx, fmaf(ay, by, az * bz)); }

// one channel: (c8 - 128) / 127, not below -1 (byte 0 alone would give -128 / 127)
RTMI_HD float tangent_channel(uint32_t c8) { return fmaxf((float)((int)c8 - 128) / 127.0f, -1.0f); }

// the texel word (r8 | g8 << 8 | b8 << 16) -> (x, y, z); false: the texel leaves the normal alone
RTMI_HD bool tangent_decode(uint32_t word, float &x, float &y, float &z) {
    const uint32_t r8 = word & 255u, g8 = (word >> 8) & 255u, b8 = (word >> 16) & 255u;
    x = tangent_channel(r8), y = tangent_channel(g8), z = tangent_channel(b8);
    return !(r8 == 128u && g8 == 128u) && z > 0.0f;
}

// ---------------------------------------------------------------- the raw tangents, per primitive type
// sphere, outward unit normal o: u is the azimuth atan2(-z, x), v the polar angle from -y
RTMI_HD void tangent_sphere(float ox, float oy, float oz, float &tx, float &ty, float &tz, float &bx, float &by, float &bz) {
    tx = oz, ty = 0.0f, tz = -ox;
    bx = -(oy * ox), by = fmaf(oz, oz, ox * ox), bz = -(oy * oz);  // o x T
}

// axis-aligned rectangle: `axis` as the rect record keeps it (0: xy, 1: xz, 2: yz), u along its first axis over the extent
// [a0, a1], v along its second over [b0, b1]: the axes' unit vectors, signed by the extents
RTMI_HD void tangent_rect(int axis, float a0, float a1, float b0, float b1, float &tx, float &ty, float &tz, float &bx, float &by,
                          float &bz) {
    const float su = a1 - a0 < 0.0f ? -1.0f : 1.0f, sv = b1 - b0 < 0.0f ? -1.0f : 1.0f;
    tx = axis == 2 ? 0.0f : su, ty = axis == 2 ? su : 0.0f, tz = 0.0f;
    bx = 0.0f, by = axis == 0 ? sv : 0.0f, bz = axis == 0 ? 0.0f : sv;
}

// cylinder: o is the outward unit normal in world space, (ax, ay, az) the third row of the world-to-object matrix's linear
// part, v runs from zmin to zmax.  The linear part is a proper rotation (scene.cpp builds it from an axis and an angle alone),
// so its inverse is its transpose: that row is the image of e_z, and the image of (-y_o, x_o, 0) = radius x (e_z x o_object) is
// radius x (image of e_z) x o, since a rotation keeps cross products
RTMI_HD void tangent_cylinder(float ax, float ay, float az, float ox, float oy, float oz, float zmin, float zmax, float &tx, float &ty,
                              float &tz, float &bx, float &by, float &bz) {
    tx = fmaf(ay, oz, -(az * oy)), ty = fmaf(az, ox, -(ax * oz)), tz = fmaf(ax, oy, -(ay * ox));
    const bool down = zmax - zmin < 0.0f;
    bx = down ? -ax : ax, by = down ? -ay : ay, bz = down ? -az : az;
}

// triangle: (u, v) is affine in the plane point.  Under the kernel's pairing the weight w1 that multiplies (u1, v1) is 1 at
// corner 3, w2 (u2, v2) at corner 2 and w3 (u3, v3) at corner 1; with E1 = V2 - V3, E2 = V1 - V3, du1 = u2 - u1, du2 = u3 - u1
// (dv alike) and det = du1 dv2 - du2 dv1:  T = (dv2 E1 - dv1 E2) / det,  B = (du1 E2 - du2 E1) / det.
// det == 0 (no usable vt): not finite, and the frame keeps n
RTMI_HD void tangent_triangle(float v1x, float v1y, float v1z, float v2x, float v2y, float v2z, float v3x, float v3y, float v3z,
                              float u1, float t1, float u2, float t2, float u3, float t3, float &tx, float &ty, float &tz, float &bx,
                              float &by, float &bz) {  // ((u1, t1): the pair (u1, v1) of the record, and so on)
    const float e1x = v2x - v3x, e1y = v2y - v3y, e1z = v2z - v3z;
    const float e2x = v1x - v3x, e2y = v1y - v3y, e2z = v1z - v3z;
    const float du1 = u2 - u1, du2 = u3 - u1, dv1 = t2 - t1, dv2 = t3 - t1;
    const float det = fmaf(du1, dv2, -(du2 * dv1));
    tx = fmaf(dv2, e1x, -(dv1 * e2x)) / det, ty = fmaf(dv2, e1y, -(dv1 * e2y)) / det, tz = fmaf(dv2, e1z, -(dv1 * e2z)) / det;
    bx = fmaf(du1, e2x, -(du2 * e1x)) / det, by = fmaf(du1, e2y, -(du2 * e1y)) / det, bz = fmaf(du1, e2z, -(du2 * e1z)) / det;
}

// quad: the record holds the outward unit normal n and the dual vectors A = v x w, B = w x u (w = c / c.c, c = u x v), of which
// B x n and n x A are the edges u and v, each over |c|: up to a positive factor
RTMI_HD void tangent_quad(float nx, float ny, float nz, float ax, float ay, float az, float bx_, float by_, float bz_, float &tx,
                          float &ty, float &tz, float &bx, float &by, float &bz) {
    tx = fmaf(by_, nz, -(bz_ * ny)), ty = fmaf(bz_, nx, -(bx_ * nz)), tz = fmaf(bx_, ny, -(by_ * nx));  // B x n
    bx = fmaf(ny, az, -(nz * ay)), by = fmaf(nz, ax, -(nx * az)), bz = fmaf(nx, ay, -(ny * ax));        // n x A
}

// ---------------------------------------------------------------- the frame and the normal
// n: the face-turned shading normal (replaced where the rule accepts n'), g: the face-turned geometric one, d: the ray's
// direction, front: the side, s: the map's scale, (T, B): the raw tangents, (x, y, z): the decoded texel.  root: the caller's
// square root (the kernels': rt_sqrtf).  -> was n replaced
template <class Root>
RTMI_HD bool tangent_normal(float &nx, float &ny, float &nz, float gnx, float gny, float gnz, float dx, float dy, float dz, bool front,
                            float s, float tx, float ty, float tz, float bx, float by, float bz, float x, float y, float z, Root root) {
    const float tn = tangent_dot(tx, ty, tz, nx, ny, nz);
    float px = fmaf(-tn, nx, tx), py = fmaf(-tn, ny, ty), pz = fmaf(-tn, nz, tz);
    const float tl = tangent_dot(px, py, pz, px, py, pz);
    if (!(tl > 0.0f && tl < INFINITY)) return false;  // (a NaN fails the comparison)
    const float ti = 1.0f / root(tl);
    px *= ti, py *= ti, pz *= ti;  // T'
    const float bn = tangent_dot(bx, by, bz, nx, ny, nz);
    float qx = fmaf(-bn, nx, bx), qy = fmaf(-bn, ny, by), qz = fmaf(-bn, nz, bz);
    const float bt = tangent_dot(qx, qy, qz, px, py, pz);
    qx = fmaf(-bt, px, qx), qy = fmaf(-bt, py, qy), qz = fmaf(-bt, pz, qz);
    const float bl = tangent_dot(qx, qy, qz, qx, qy, qz);
    const float bi = 1.0f / root(bl);
    qx *= bi, qy *= bi, qz *= bi;  // B'
    const float sg = front ? 1.0f : -1.0f;
    if (!(bl > 0.0f && bl < INFINITY)) {
        // cross(o, T') with o = sigma n
        const float cx = fmaf(ny, pz, -(nz * py)), cy = fmaf(nz, px, -(nx * pz)), cz = fmaf(nx, py, -(ny * px));
        qx = sg * cx, qy = sg * cy, qz = sg * cz;
    }
    const float k = sg * s;
    const float hx = k * fmaf(x, px, y * qx), hy = k * fmaf(x, py, y * qy), hz = k * fmaf(x, pz, y * qz);
    const float ex = fmaf(z, nx, hx), ey = fmaf(z, ny, hy), ez = fmaf(z, nz, hz);
    const float l2 = tangent_dot(ex, ey, ez, ex, ey, ez);
    if (!(l2 > 0.0f && l2 < INFINITY)) return false;
    const float inv = 1.0f / root(l2);
    const float ux = inv * ex, uy = inv * ey, uz = inv * ez;
    if (!(tangent_dot(ux, uy, uz, gnx, gny, gnz) > 0.0f && tangent_dot(ux, uy, uz, dx, dy, dz) < 0.0f)) return false;  // (a NaN fails both)
    nx = ux, ny = uy, nz = uz;
    return true;
}

}  // namespace rtmi
