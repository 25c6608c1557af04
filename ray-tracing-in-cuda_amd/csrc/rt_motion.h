// Moving spheres: the record of a mover in the scene image, the shutter time of a sample and the intersection of a
// ray with a mover at that time, shared by the motion kernels (render_motion.hip, through render_body.h) and the host
// evaluation (rt_moving_sphere_hit, rt_shutter_time), like rt_media.h.  Every step is one fp32 operation in a fixed order.
//
// MOTION part of the scene image (only with at least one mover; global memory, behind everything else): per mover
//   3 x float4   {center0.xyz, radius} {v.xyz, 1 / radius} {material(bits), kind(bits), 0, 0}      v = center1 - center0 (fp32, host)
// Where the part lies is said by two words of the camera block, which are zero in a scene without movers:
//   record off_cam + 3, .w   number of movers (bits)         record off_cam + 4, .w   float4 offset of the MOTION part (bits)
#pragma once
#include <math.h>
#include <stdint.h>

#include "philox.h"  // RTMI_HD

#define RT_MOTION_STRIDE 3

namespace rtmi {

// the shutter time of sample (pixel, sample): NOT a draw of the sample's stream but the top 24 bits of word 0 of the Philox
// block beside the one that seeds the stream (counter word 2 = 1 instead of 0), so every draw of the sample stays where it is
RTMI_HD float shutter_time(uint32_t pixel, uint32_t sample, uint32_t k0, uint32_t k1) {
    const Philox4 p = philox4x32_10(pixel, sample, 1u, 0u, k0, k1);
    return (float)(p.v[0] >> 8) * (1.0f / 16777216.0f);
}

// sphere::hit (object.cuh:47-75) against the sphere (c(s), r), c(s) = c0 + s v per component as one fma, for the ray o + t d
// with A = d.d and inv_a = 1 / A: oc, half_b, c, discriminant, the near root and, if that lies outside [0.001, t_max], the far
// one.  true: a root inside [0.001, t_max], returned in t (a root EQUAL to t_max is a hit: the later entry wins a tie).
RTMI_HD bool moving_sphere_hit(float c0x, float c0y, float c0z, float r, float vx, float vy, float vz, float s, float ox, float oy,
                               float oz, float dx, float dy, float dz, float A, float inv_a, float t_max, float &t) {
    const float cx = fmaf(s, vx, c0x), cy = fmaf(s, vy, c0y), cz = fmaf(s, vz, c0z);
    const float ocx = ox - cx, ocy = oy - cy, ocz = oz - cz;
    const float hb = fmaf(ocx, dx, fmaf(ocy, dy, ocz * dz));
    const float cc = fmaf(ocx, ocx, fmaf(ocy, ocy, fmaf(ocz, ocz, -(r * r))));
    const float disc = fmaf(hb, hb, -(A * cc));
    // no real root, or both roots behind the origin (hb >= 0 and c >= 0: then sqrt(disc) <= hb and -hb + sqrt(disc) <= 0)
    if (disc < 0.0f || (hb >= 0.0f && cc >= 0.0f)) return false;
    const float sq = sqrtf(disc);
    float root = (-hb - sq) * inv_a;
    if (root < 0.001f || t_max < root) root = (-hb + sq) * inv_a;
    if (root < 0.001f || t_max < root) return false;
    t = root;
    return true;
}

}  // namespace rtmi
