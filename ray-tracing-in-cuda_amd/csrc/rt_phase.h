// Anisotropic media: the Henyey-Greenstein phase function of a medium with asymmetry g,
//   p(cos t) = (1 - g^2) / (4 pi (1 + g^2 - 2 g cos t)^(3/2)),   t between the arriving and the leaving direction of travel,
// its sample from two uniforms and its density, shared by the media kernels (render_body.h) and the host evaluations
// (rt_phase_hg_sample, rt_phase_hg_eval), like rt_media.h.  Every step is one fp32 operation in a fixed order, every fused
// multiply-add explicit; the sine and cosine of the azimuth are sincosf of either side's math library, as the glossy lobe's.
//
// A medium's g rides in .w of its record 2 (rt_media.h), which is 0 for the isotropic medium: |g| < RT_PHASE_G_SNAP is stored
// as exactly 0, and such a medium never gets here.
#pragma once
#include <math.h>

#include "rt_glossy.h"  // RTMI_HD, duff_frame, glossy_sqrtf
#include "rt_media.h"   // RT_PHASE_G_MAX, RT_PHASE_G_SNAP

namespace rtmi {

// cos t of the sample, the inverse of the distribution function of cos t (g != 0):
//   s = (1 - g^2) / (1 - g + 2 g u1), cos t = (1 + g^2 - s^2) / (2 g), clamped to [-1, 1].  u1 = 0: cos t = -1; u1 -> 1: cos t -> 1
RTMI_HD float phase_hg_cos(float g, float u1) {
    const float s = fmaf(-g, g, 1.0f) / fmaf(2.0f * g, u1, 1.0f - g);
    const float c = fmaf(-s, s, fmaf(g, g, 1.0f)) / (2.0f * g);
    return fminf(1.0f, fmaxf(-1.0f, c));
}

// The scattered direction of a medium vertex with g != 0 from two uniforms: (wx, wy, wz) the UNIT direction of travel that
// arrived; cos t from u1, sin t = sqrt(max(0, 1 - cos^2 t)), (sin p, cos p) of p = 2 pi u2, in the frame (t1, t2) = duff_frame(w):
//   out = sin t cos p t1 + sin t sin p t2 + cos t w.   The sample's density is the phase function: the vertex weighs the albedo.
RTMI_HD void phase_hg_sample(float g, float wx, float wy, float wz, float u1, float u2, float &ox, float &oy, float &oz) {
    const float ct = phase_hg_cos(g, u1);
    const float st = glossy_sqrtf(fmaxf(0.0f, fmaf(-ct, ct, 1.0f)));
    float sp, cp;
    sincosf(6.283185307179586476925f * u2, &sp, &cp);
    float t1x, t1y, t1z, t2x, t2y, t2z;
    duff_frame(wx, wy, wz, t1x, t1y, t1z, t2x, t2y, t2z);
    const float a = st * cp, b = st * sp;
    ox = fmaf(a, t1x, fmaf(b, t2x, ct * wx));
    oy = fmaf(a, t1y, fmaf(b, t2y, ct * wy));
    oz = fmaf(a, t1z, fmaf(b, t2z, ct * wz));
}

// p(cos t), per steradian.  1 + g^2 - 2 g c is formed without its cancellation near the peak:
//   g >= 0: (1 - g)^2 + 2 g (1 - c);   g < 0: (1 + g)^2 - 2 g (1 + c)   -- two non-negative terms either way
RTMI_HD float phase_hg_eval(float g, float c) {
    const float e = g < 0.0f ? 1.0f + g : 1.0f - g;
    const float f = g < 0.0f ? 1.0f + c : 1.0f - c;
    const float b = fmaf(2.0f * fabsf(g), f, e * e);
    return fmaf(-g, g, 1.0f) / (12.566370614359172953850f * (b * sqrtf(b)));
}

}  // namespace rtmi
