// Quads: a parallelogram with corner Q and edges u, v -- the corners Q, Q + u, Q + u + v, Q + v.  A box is six of
// them, and a rotated or translated quad is a quad: the host applies the transform to Q, u, v (scene.cpp, add_quad) and the
// device sees nothing else.  fp32 with a FIXED operation sequence, every fused multiply-add explicit, in the manner of
// rt_glossy.h: the kernels (render_body.h) and a host program (tests/quad_host_driver.cpp) compile this text.
//
// What the host derives in fp64 from the fp32 Q, u, v and rounds once (rt_prim, include/rtmi.h):
//   c = u x v,  n = c / |c| (the outward unit normal),  w = c / (c.c),  A = v x w,  B = w x u
// so that a point p = Q + a u + b v of the plane has a = A.(p - Q), b = B.(p - Q).
#pragma once
#include <math.h>

#ifndef RTMI_HD
#ifdef __HIPCC__
#define RTMI_HD __host__ __device__ inline
#else
#define RTMI_HD inline
#endif
#endif

namespace rtmi {

RTMI_HD float quad_dot(float ax, float ay, float az, float bx, float by, float bz) { return fmaf(ax, bx, fmaf(ay, by, az * bz)); }

// the parallelogram's coordinates of the point p: a = A.(p - Q), b = B.(p - Q) -- the hit record's (u, v)
RTMI_HD void quad_uv(float qx, float qy, float qz, float ax, float ay, float az, float bx, float by, float bz, float px, float py,
                     float pz, float &a, float &b) {
    const float rx = px - qx, ry = py - qy, rz = pz - qz;
    a = quad_dot(ax, ay, az, rx, ry, rz);
    b = quad_dot(bx, by, bz, rx, ry, rz);
}

// The hit test.  den = n.d (zero or not finite: a miss), t = n.(Q - o) / den accepted within [t_min, t_max], p = o + t d,
// (a, b) of p; a hit iff both lie in [0, 1].  `front` is den < 0, and the record's normal n turned against the ray: the caller
// has both from n and d.
RTMI_HD bool quad_hit(float qx, float qy, float qz, float nx, float ny, float nz, float ax, float ay, float az, float bx, float by,
                      float bz, float ox, float oy, float oz, float dx, float dy, float dz, float t_min, float t_max, float &t,
                      float &a, float &b) {
    const float den = quad_dot(dx, dy, dz, nx, ny, nz);
    if (!(fabsf(den) > 0.0f && fabsf(den) < INFINITY)) return false;
    t = quad_dot(nx, ny, nz, qx - ox, qy - oy, qz - oz) / den;
    if (t < t_min || t > t_max || t != t) return false;
    quad_uv(qx, qy, qz, ax, ay, az, bx, by, bz, fmaf(t, dx, ox), fmaf(t, dy, oy), fmaf(t, dz, oz), a, b);
    return a >= 0.0f && a <= 1.0f && b >= 0.0f && b <= 1.0f;
}

// The light sample: the point y = Q + u1 u + u2 v, uniform by area ...
RTMI_HD void quad_light_point(float qx, float qy, float qz, float ux, float uy, float uz, float vx, float vy, float vz, float u1,
                              float u2, float &yx, float &yy, float &yz) {
    yx = fmaf(u2, vx, fmaf(u1, ux, qx));
    yy = fmaf(u2, vy, fmaf(u1, uy, qy));
    yz = fmaf(u2, vz, fmaf(u1, uz, qz));
}

// ... and the solid-angle density of the direction ld = y - p as seen from p: selection / |c| x |ld|^2 / |n.ld / |ld||, the
// by-area rule every flat light of the kernels shares (sel_over_area = selection probability x 1 / |c|)
RTMI_HD float quad_light_pdf(float sel_over_area, float nx, float ny, float nz, float ldx, float ldy, float ldz) {
    const float d2 = quad_dot(ldx, ldy, ldz, ldx, ldy, ldz);
    return (sel_over_area * (d2 * sqrtf(d2))) / fabsf(quad_dot(nx, ny, nz, ldx, ldy, ldz));
}

}  // namespace rtmi
