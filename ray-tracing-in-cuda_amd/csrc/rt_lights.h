// Analytic lights: point, spot and distant lights -- emitters without geometry, which act through the light sample
// of a vertex alone.  fp32 with a FIXED operation sequence, every fused multiply-add explicit, in the manner of rt_quad.h: the
// kernels (render_body.h, section 7) and a host program (tests/analytic_light_host_driver.cpp) compile this text.
//
// Each sample is stated as the vector ld from the vertex p towards the light and a "density" pl, so that the sample's weight
// is f cos x colour / pl with no MIS factor (the BSDF strategy can never produce the direction of a delta light, and a distant
// light's cone is sampled by this strategy alone):
//   point    ld = x - p,  pl = psel |ld|^2
//   spot     the point light's, pl divided by falloff = s^2 (3 - 2 s), s = clamp((a.(-ld/|ld|) - cos_o) inv, 0, 1); falloff 0: pl = 0
//   distant  ld = D w, w uniform in the cone of 1 - cos(half-angle) = omc about the unit direction t, pl = psel (the host has
//            folded radiance x solid angle into the colour: E x 2 / (1 + cos alpha))
// What the host derives in fp64 and rounds once (scene.cpp, analytic_record): the unit axes, cos_o, inv = min(1 / (cos_i -
// cos_o), FLT_MAX), omc = 1 - cos alpha, D = 4 x the scene's bounding radius, the folded colour.
#pragma once
#include <math.h>

#include "rt_glossy.h"  // duff_frame

namespace rtmi {

RTMI_HD float light_dot(float ax, float ay, float az, float bx, float by, float bz) { return fmaf(ax, bx, fmaf(ay, by, az * bz)); }

// A direction uniform in the cone of 1 - cos(half-angle) = omc about the unit axis a: 1 - cos(theta) = u1 omc, azimuth 2 pi u2 in
// the frame of Duff et al. 2017.  The sphere light's own expressions, shared with it: also returned are cos and sin
// of theta, which the sphere's nearer intersection needs.  omc = 0 gives e = a exactly (sin(theta) = 0, cos(theta) = 1).
RTMI_HD void light_cone_direction(float ax, float ay, float az, float omc, float u1, float u2, float &ex, float &ey, float &ez, float &cth,
                                  float &sth) {
    const float om = u1 * omc;
    cth = 1.0f - om;
    sth = sqrtf(fmaxf(0.0f, om * (2.0f - om)));
    float sp, cp;
    sincosf((2.0f * 3.14159265358979323846f) * u2, &sp, &cp);
    float t1x, t1y, t1z, t2x, t2y, t2z;
    duff_frame(ax, ay, az, t1x, t1y, t1z, t2x, t2y, t2z);
    const float s1 = sth * cp, s2 = sth * sp;
    ex = fmaf(s1, t1x, fmaf(s2, t2x, cth * ax));
    ey = fmaf(s1, t1y, fmaf(s2, t2y, cth * ay));
    ez = fmaf(s1, t1z, fmaf(s2, t2z, cth * az));
}

// the point light's density of ld (d2 = ld.ld): psel d2
RTMI_HD float point_light_density(float psel, float d2) { return psel * d2; }

// the spot's falloff towards the vertex at -ld from it: smoothstep of the cosine to its unit axis a between cos_o and cos_i
RTMI_HD float spot_falloff(float ax, float ay, float az, float ldx, float ldy, float ldz, float d2, float cos_o, float inv) {
    const float c = -(light_dot(ax, ay, az, ldx, ldy, ldz) / sqrtf(d2));
    const float s = fminf(fmaxf((c - cos_o) * inv, 0.0f), 1.0f);
    return (s * s) * fmaf(-2.0f, s, 3.0f);
}

// the spot's density: the point light's over the falloff; 0 (no sample) where the falloff is 0
RTMI_HD float spot_light_density(float psel, float d2, float falloff) { return falloff > 0.0f ? (psel * d2) / falloff : 0.0f; }

}  // namespace rtmi
