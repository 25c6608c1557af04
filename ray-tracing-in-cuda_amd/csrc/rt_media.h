// Homogeneous participating media: the record of a medium in the scene image and the interval of a ray inside its
// boundary, shared by the media kernels (render_media.hip, through render_body.h) and the host evaluation
// (rt_medium_interval), like rt_env.h.  Every step is one fp32 operation in a fixed order.
//
// MEDIA part of the scene image (only with at least one medium; global memory, behind everything else): per medium
//   3 x float4   {f0, f1, f2, f3} {albedo.rgb, density} {f4, f5, shape(bits), g}      sphere f = {c.xyz, r}; box f = {min.xyz, max.xyz}
// (record 1 has the place of a material's {c0.xyz, p3}: the scatter step reads the albedo as it reads a lambertian's.)
// Where the part lies is said by two words of the camera block, which are zero in a scene without media:
//   record off_cam + 1, .w   number of media (bits)          record off_cam + 2, .w   float4 offset of the MEDIA part (bits)
#pragma once
#include <math.h>
#include <stdint.h>

#include "rt_trig.h"  // RTMI_HD

#define RT_MEDIUM_STRIDE 3
// the asymmetry g of a medium's phase function (rt_phase.h), .w of record 2: |g| <= MAX, and |g| < SNAP is stored as 0
#define RT_PHASE_G_MAX 0.99f
#define RT_PHASE_G_SNAP 1e-3f
// the isotropic phase function's density per steradian, 1 / (4 pi): pdf_b of a medium vertex with the stored g = 0
#define RT_PHASE_ISOTROPIC 0.0795774715459476678844f

namespace rtmi {

// [a, b]: the stay of the ray o + t d inside the boundary, clipped to [0.001, t_max]; false: empty (a < b does not hold).
//   sphere: the two roots of |o + t d - c|^2 = r^2 -- oc = o - c, A = d.d, hb = oc.d, cc = oc.oc - r r, disc = hb hb - A cc;
//           no interval unless disc > 0; a = (-hb - sqrt(disc)) / A, b = (-hb + sqrt(disc)) / A
//   box:    the slab test of aabb.hpp:15-29 -- per axis inv = 1 / d, t0 = (min - o) inv, t1 = (max - o) inv, swapped if inv < 0,
//           a = t0 > a ? t0 : a, b = t1 < b ? t1 : b, starting from [0.001, t_max]
RTMI_HD bool medium_interval(int shape, float f0, float f1, float f2, float f3, float f4, float f5, float ox, float oy, float oz,
                             float dx, float dy, float dz, float t_max, float &a, float &b) {
    a = 0.001f, b = t_max;
    if (shape == 0) {
        const float ocx = ox - f0, ocy = oy - f1, ocz = oz - f2;
        const float A = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
        const float hb = fmaf(ocx, dx, fmaf(ocy, dy, ocz * dz));
        const float cc = fmaf(ocx, ocx, fmaf(ocy, ocy, fmaf(ocz, ocz, -(f3 * f3))));
        const float disc = fmaf(hb, hb, -(A * cc));
        if (!(disc > 0.0f)) return false;
        const float sq = sqrtf(disc);
        const float t0 = (-hb - sq) / A, t1 = (-hb + sq) / A;
        a = t0 > a ? t0 : a;
        b = t1 < b ? t1 : b;
    } else {
        const float o[3] = {ox, oy, oz}, d[3] = {dx, dy, dz}, mn[3] = {f0, f1, f2}, mx[3] = {f3, f4, f5};
        for (int k = 0; k < 3; ++k) {
            const float inv = 1.0f / d[k];
            float t0 = (mn[k] - o[k]) * inv, t1 = (mx[k] - o[k]) * inv;
            if (inv < 0.0f) {
                const float tmp = t0;
                t0 = t1;
                t1 = tmp;
            }
            a = t0 > a ? t0 : a;
            b = t1 < b ? t1 : b;
        }
    }
    return a < b;
}

// A shadow ray through the media: the optical depth tau of the segment o + t d, t in [0.001, t_max], is summed
// over the media in list order -- a non-empty stay [a, b] in a medium of density sigma adds sigma (b - a) |d| as
//   s = b - a;  x = sigma * s;  tau = fma(x, len, tau)       (len = |d|: the caller's root of d.d)
// and an unoccluded light sample is multiplied by T = exp(-tau): expf of either side's math library, as the azimuth's
// sincosf is.  tau = 0 (no stay) gives exactly 1 without a call.
RTMI_HD float medium_tau_add(float sigma, float a, float b, float len, float tau) {
    const float s = b - a;
    const float x = sigma * s;
    return fmaf(x, len, tau);
}

RTMI_HD float media_transmittance(float tau) { return tau > 0.0f ? expf(-tau) : 1.0f; }

}  // namespace rtmi
