// Glossy materials: a GGX microfacet lobe with height-correlated Smith masking, sampled through its visible
// normals (Heitz 2018), as a rough metal (Schlick Fresnel about F0) and as a coated plastic (the same lobe with the coat's r0
// over a diffuse body).  fp32 with a FIXED operation sequence, every fused multiply-add explicit, in the manner of rt_trig.h:
// the kernels (render_body.h) and a host program (tests/glossy_host_driver.cpp) compile this text, and tests/ref64_glossy.py
// restates it in numpy.
//
// All vectors of the lobe are LOCAL: components along the orthonormal frame (t1, t2, n) of Duff et al. 2017 about the shading
// normal n, z along n.  wo = -unit(d) points back along the arriving ray, wi along the scattered one, h is their half vector.
// alpha = max(r^2, 1e-3) comes from the packer.
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

// a vertex of either material takes a light sample iff its roughness r is at least this (the role of metal's fuzz >= 0.05)
#define RT_GLOSSY_MIN_ROUGHNESS 0.05f

// the square root of the kernels (render_device.h: IEEE-correct, bit for bit sqrtf) where they compile this, sqrtf elsewhere
RTMI_HD float glossy_sqrtf(float x) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
    return rt_sqrtf(x);
#else
    return sqrtf(x);
#endif
}

// orthonormal frame about the unit vector a (Duff et al. 2017): t1, t2 with (t1, t2, a) right-handed
RTMI_HD void duff_frame(float ax, float ay, float az, float &t1x, float &t1y, float &t1z, float &t2x, float &t2y, float &t2z) {
    const float sg = copysignf(1.0f, az), fa = -1.0f / (sg + az), fb = ax * ay * fa;
    t1x = fmaf(sg * ax * ax, fa, 1.0f), t1y = sg * fb, t1z = -sg * ax;
    t2x = fb, t2y = fmaf(ay * ay, fa, sg), t2z = -ay;
}

RTMI_HD float glossy_dot(float ax, float ay, float az, float bx, float by, float bz) { return fmaf(ax, bx, fmaf(ay, by, az * bz)); }

// schlick(f0, c) = f0 + (1 - f0)(1 - c)^5
RTMI_HD float glossy_schlick(float f0, float c) {
    const float x = 1.0f - c, x2 = x * x;
    return fmaf(1.0f - f0, (x2 * x2) * x, f0);
}

// D(h) = alpha^2 / (pi (alpha^2 h.z^2 + h.x^2 + h.y^2)^2): no cancellation at small alpha
RTMI_HD float ggx_d(float alpha, float hx, float hy, float hz) {
    const float a2 = alpha * alpha;
    const float q = fmaf(a2, hz * hz, fmaf(hx, hx, hy * hy));
    return a2 / (3.14159265358979323846f * (q * q));
}

// Lambda(w) = (sqrt(1 + alpha^2 (w.x^2 + w.y^2) / w.z^2) - 1) / 2
RTMI_HD float ggx_lambda(float alpha, float wx, float wy, float wz) {
    const float a2 = alpha * alpha;
    const float t = (a2 * fmaf(wx, wx, wy * wy)) / (wz * wz);
    return 0.5f * (glossy_sqrtf(1.0f + t) - 1.0f);
}

// a visible normal of the lobe seen from wo (wo.z > 0), from two uniforms: rr = sqrt(u1), (sp, cp) = sin, cos of 2 pi u2
RTMI_HD void ggx_sample_h(float alpha, float wox, float woy, float woz, float rr, float sp, float cp, float &hx, float &hy, float &hz) {
    float vx = alpha * wox, vy = alpha * woy, vz = woz;
    const float il = 1.0f / glossy_sqrtf(glossy_dot(vx, vy, vz, vx, vy, vz));
    vx *= il, vy *= il, vz *= il;
    const float l2 = fmaf(vx, vx, vy * vy);
    float t1x = 1.0f, t1y = 0.0f;
    if (l2 > 0.0f) {
        const float i1 = 1.0f / glossy_sqrtf(l2);
        t1x = -vy * i1, t1y = vx * i1;
    }
    // T2 = Vh x T1, T1.z = 0
    const float t2x = -(vz * t1y), t2y = vz * t1x, t2z = fmaf(vx, t1y, -(vy * t1x));
    const float a = rr * cp;
    float b = rr * sp;
    const float s = 0.5f * (1.0f + vz);
    b = fmaf(1.0f - s, glossy_sqrtf(fmaxf(0.0f, fmaf(-a, a, 1.0f))), s * b);
    const float c = glossy_sqrtf(fmaxf(0.0f, 1.0f - fmaf(a, a, b * b)));
    const float nhx = fmaf(a, t1x, fmaf(b, t2x, c * vx));
    const float nhy = fmaf(a, t1y, fmaf(b, t2y, c * vy));
    const float nhz = fmaf(b, t2z, c * vz);
    hx = alpha * nhx, hy = alpha * nhy, hz = fmaxf(0.0f, nhz);
    const float ih = 1.0f / glossy_sqrtf(glossy_dot(hx, hy, hz, hx, hy, hz));
    hx *= ih, hy *= ih, hz *= ih;
}

// What the lobe gives for a pair of directions with wo.z > 0 and wi.z > 0 and their half vector h:
// spec = D(h) G2(wo, wi) / (4 wo.z) (f cos of the lobe without its Fresnel factor), pdf_s = G1(wo) D(h) / (4 wo.z), and
// ratio = G2 / G1(wo) = spec / pdf_s
RTMI_HD void ggx_terms(float alpha, float wox, float woy, float woz, float wix, float wiy, float wiz, float hx, float hy, float hz,
                       float &spec, float &pdf_s, float &ratio) {
    const float lo = ggx_lambda(alpha, wox, woy, woz), li = ggx_lambda(alpha, wix, wiy, wiz);
    const float dq = ggx_d(alpha, hx, hy, hz) / (4.0f * woz);
    const float g1 = 1.0f / (1.0f + lo), g2 = 1.0f / ((1.0f + lo) + li);
    spec = dq * g2, pdf_s = dq * g1;
    ratio = g2 / g1;
}

// ---- the two materials, in WORLD vectors: n the unit shading normal, (ux, uy, uz) = unit(d) of the arriving ray.
// A sample returns false for an absorbed vertex (wo.z <= 0 or wi.z <= 0: *absorbed_wo tells which); otherwise the unit
// scattered direction, the attenuation and pdf_b of that direction.
struct GlossyLocal {
    float t1x, t1y, t1z, t2x, t2y, t2z;  // the frame
    float wox, woy, woz;                 // wo in it
};
RTMI_HD GlossyLocal glossy_local(float nx, float ny, float nz, float ux, float uy, float uz) {
    GlossyLocal g;
    duff_frame(nx, ny, nz, g.t1x, g.t1y, g.t1z, g.t2x, g.t2y, g.t2z);
    g.wox = -glossy_dot(ux, uy, uz, g.t1x, g.t1y, g.t1z);
    g.woy = -glossy_dot(ux, uy, uz, g.t2x, g.t2y, g.t2z);
    g.woz = -glossy_dot(ux, uy, uz, nx, ny, nz);
    return g;
}
RTMI_HD void glossy_to_world(const GlossyLocal &g, float nx, float ny, float nz, float lx, float ly, float lz, float &wx, float &wy,
                             float &wz) {
    wx = fmaf(lx, g.t1x, fmaf(ly, g.t2x, lz * nx));
    wy = fmaf(lx, g.t1y, fmaf(ly, g.t2y, lz * ny));
    wz = fmaf(lx, g.t1z, fmaf(ly, g.t2z, lz * nz));
}

// the lobe's sample: wi (local) = 2 (wo.h) h - wo and wo.h
RTMI_HD void ggx_sample_wi(float alpha, const GlossyLocal &g, float rr, float sp, float cp, float &hx, float &hy, float &hz, float &woh,
                           float &wix, float &wiy, float &wiz) {
    ggx_sample_h(alpha, g.wox, g.woy, g.woz, rr, sp, cp, hx, hy, hz);
    woh = glossy_dot(g.wox, g.woy, g.woz, hx, hy, hz);
    const float k2 = 2.0f * woh;
    wix = fmaf(k2, hx, -g.wox), wiy = fmaf(k2, hy, -g.woy), wiz = fmaf(k2, hz, -g.woz);
}

// half vector of two local directions and wo.h
RTMI_HD void glossy_half(const GlossyLocal &g, float wix, float wiy, float wiz, float &hx, float &hy, float &hz, float &woh) {
    hx = g.wox + wix, hy = g.woy + wiy, hz = g.woz + wiz;
    const float ih = 1.0f / glossy_sqrtf(glossy_dot(hx, hy, hz, hx, hy, hz));
    hx *= ih, hy *= ih, hz *= ih;
    woh = glossy_dot(g.wox, g.woy, g.woz, hx, hy, hz);
}

// ---- the two materials through one body (plastic: false for a rough metal).
// rough metal: f cos = schlick(F0, wo.h) D G2 / (4 wo.z), pdf_b = pdf_s, attenuation = schlick(F0, wo.h) G2 / G1(wo).
// plastic: f cos = schlick(r0, wo.h) D G2 / (4 wo.z) + (1 - Fo)(1 - Fi) rho wi.z / pi, the lobe drawn with probability
// ps = 1/4 + 3/4 Fo and the cosine hemisphere otherwise, pdf_b = ps pdf_s + (1 - ps) wi.z / pi, attenuation = f cos / pdf_b.
// f0: F0 of the metal, or the coat's r0 in every channel; rho: the body's colour (not read for a metal).
RTMI_HD void glossy_terms(bool plastic, float alpha, float f0r, float f0g, float f0b, float rho_r, float rho_g, float rho_b,
                          const GlossyLocal &g, float wix, float wiy, float wiz, float hx, float hy, float hz, float woh, float &fc_r,
                          float &fc_g, float &fc_b, float &pdf, float &ratio) {
    float spec, pdf_s;
    ggx_terms(alpha, g.wox, g.woy, g.woz, wix, wiy, wiz, hx, hy, hz, spec, pdf_s, ratio);
    fc_r = glossy_schlick(f0r, woh) * spec, fc_g = glossy_schlick(f0g, woh) * spec, fc_b = glossy_schlick(f0b, woh) * spec;
    pdf = pdf_s;
    if (plastic) {
        const float fo = glossy_schlick(f0r, g.woz), fi = glossy_schlick(f0r, wiz);
        const float ps = fmaf(0.75f, fo, 0.25f);
        const float cpi = wiz * 0.318309886183790671538f;
        const float body = ((1.0f - fo) * (1.0f - fi)) * cpi;
        fc_r = fmaf(body, rho_r, fc_r), fc_g = fmaf(body, rho_g, fc_g), fc_b = fmaf(body, rho_b, fc_b);
        pdf = fmaf(ps, pdf_s, (1.0f - ps) * cpi);
    }
}
// ---- rough glass (rt_glass.h has its entry points and the tint), the third material of the same body: a rough metal
// with F0 = 1 whose microfacet reflects with the exact unpolarised Fresnel term F(c; eta) of c = wo.h and refracts otherwise.
// s2 = eta^2 (1 - c^2); F = 1 (and ct = 0) where s2 >= 1, else ct = sqrt(1 - s2), rs = (eta c - ct) / (eta c + ct),
// rp = (c - eta ct) / (c + eta ct), F = (rs^2 + rp^2) / 2
RTMI_HD float glass_fresnel(float eta, float c, float &ct) {
    const float s2 = (eta * eta) * fmaf(-c, c, 1.0f);
    ct = 0.0f;
    if (s2 >= 1.0f) return 1.0f;
    ct = glossy_sqrtf(1.0f - s2);
    const float ec = eta * c, et = eta * ct;
    const float rs = (ec - ct) / (ec + ct), rp = (c - et) / (c + et);
    return 0.5f * fmaf(rs, rs, rp * rp);
}
// The same term behind a call, for the kernels in which the inlined text costs the scenes WITHOUT the material more than a call's
// save area does (DESIGN 7r has both forms' rows: the light-sampling kernels without an environment).  A body called with
// fresnel_call takes this one on the device; the values are the same bits either way.
struct GlassFresnel {
    float F, ct;  // (by value: in registers, where two references would go through scratch)
};
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
__device__ inline __attribute__((noinline)) GlassFresnel glass_fresnel_call(float eta, float c) {
    GlassFresnel r;
    r.F = glass_fresnel(eta, c, r.ct);
    return r;
}
#endif
RTMI_HD float glass_fresnel_of(bool call, float eta, float c, float &ct) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
    if (call) {
        const GlassFresnel r = glass_fresnel_call(eta, c);
        ct = r.ct;
        return r.F;
    }
#endif
    return glass_fresnel(eta, c, ct);
}
enum GlossyMode : int { GLOSSY_METAL = 0, GLOSSY_PLASTIC = 1, GLOSSY_GLASS = 2 };

// The scatter step.  Draws: u1, u2, and in front of them ul for plastic (the choice between coat and body) and for glass (reflect
// iff ul < F).  false: an absorbed vertex (absorbed_wo: wo.z <= 0, else the direction came out on the wrong side: wi.z <= 0, for a
// refracted one wi.z >= 0); true: the unit scattered direction (world), the attenuation and pdf_b of that direction.
// Glass (f0 = 1, eta = front ? 1 / ir : ir): reflected, wi = 2 c h - wo and pdf_b = F pdf_s; refracted (lobe comes back false),
// wi = (eta c - ct) h - eta wo and pdf_b = -1 (the light strategy never produces it); the attenuation is G2 / G1(wo) either way,
// Lambda of wi as it stands (it is even in z), and the caller multiplies it by the tint.
RTMI_HD bool glossy_sample_body(int mode, float nx, float ny, float nz, float ux, float uy, float uz, float alpha, float f0r, float f0g,
                                float f0b, float rho_r, float rho_g, float rho_b, float eta, float ul, float u1, float u2, float &wx,
                                float &wy, float &wz, float &at_r, float &at_g, float &at_b, float &pdf, bool &absorbed_wo, bool &lobe,
                                bool fresnel_call = false) {
    const bool plastic = mode == GLOSSY_PLASTIC, glass = mode == GLOSSY_GLASS;
    const GlossyLocal g = glossy_local(nx, ny, nz, ux, uy, uz);
    absorbed_wo = !(g.woz > 0.0f);
    lobe = false;
    if (absorbed_wo) return false;
    lobe = !plastic || ul < fmaf(0.75f, glossy_schlick(f0r, g.woz), 0.25f);
    float hx, hy, hz, woh, wix, wiy, wiz;
    // (both lobes turn u1, u2 into a point of the unit disk: one square root, one sine and cosine)
    const float rr = glossy_sqrtf(u1);
    float sp, cp;
    sincosf(6.283185307179586476925f * u2, &sp, &cp);
    if (lobe) {
        ggx_sample_wi(alpha, g, rr, sp, cp, hx, hy, hz, woh, wix, wiy, wiz);
    } else {
        wix = rr * cp, wiy = rr * sp, wiz = glossy_sqrtf(1.0f - u1);
        glossy_half(g, wix, wiy, wiz, hx, hy, hz, woh);
    }
    float F = 1.0f;
    if (glass) {
        float ct;
        F = glass_fresnel_of(fresnel_call, eta, woh, ct);
        lobe = ul < F;
        if (!lobe) {
            const float k = fmaf(eta, woh, -ct);
            wix = fmaf(k, hx, -(eta * g.wox)), wiy = fmaf(k, hy, -(eta * g.woy)), wiz = fmaf(k, hz, -(eta * g.woz));
        }
    }
    if ((glass && !lobe) ? !(wiz < 0.0f) : !(wiz > 0.0f)) return false;
    float fr, fg, fb, ratio;
    glossy_terms(plastic, alpha, f0r, f0g, f0b, rho_r, rho_g, rho_b, g, wix, wiy, wiz, hx, hy, hz, woh, fr, fg, fb, pdf, ratio);
    if (plastic) {
        at_r = fr / pdf, at_g = fg / pdf, at_b = fb / pdf;
    } else {
        at_r = glossy_schlick(f0r, woh) * ratio, at_g = glossy_schlick(f0g, woh) * ratio, at_b = glossy_schlick(f0b, woh) * ratio;
    }
    if (glass) pdf = lobe ? F * pdf : -1.0f;
    glossy_to_world(g, nx, ny, nz, wix, wiy, wiz, wx, wy, wz);
    return true;
}
RTMI_HD bool glossy_sample(bool plastic, float nx, float ny, float nz, float ux, float uy, float uz, float alpha, float f0r, float f0g,
                           float f0b, float rho_r, float rho_g, float rho_b, float ul, float u1, float u2, float &wx, float &wy,
                           float &wz, float &at_r, float &at_g, float &at_b, float &pdf, bool &absorbed_wo, bool &lobe) {
    return glossy_sample_body(plastic ? GLOSSY_PLASTIC : GLOSSY_METAL, nx, ny, nz, ux, uy, uz, alpha, f0r, f0g, f0b, rho_r, rho_g, rho_b, 1.0f,
                              ul, u1, u2, wx, wy, wz, at_r, at_g, at_b, pdf, absorbed_wo, lobe);
}
// f cos and pdf_b of the unit world direction (lx, ly, lz); zeros where the vertex or the direction is below the surface
// (glass, f0 = 1: the reflection hemisphere alone -- f cos = F(wo.h) D G2 / (4 wo.z) without the tint, pdf_b = F(wo.h) pdf_s)
RTMI_HD void glossy_eval_body(int mode, float nx, float ny, float nz, float ux, float uy, float uz, float alpha, float f0r, float f0g,
                              float f0b, float rho_r, float rho_g, float rho_b, float eta, float lx, float ly, float lz, float &fc_r,
                              float &fc_g, float &fc_b, float &pdf, bool fresnel_call = false) {
    const bool plastic = mode == GLOSSY_PLASTIC;
    const GlossyLocal g = glossy_local(nx, ny, nz, ux, uy, uz);
    const float wix = glossy_dot(lx, ly, lz, g.t1x, g.t1y, g.t1z), wiy = glossy_dot(lx, ly, lz, g.t2x, g.t2y, g.t2z),
                wiz = glossy_dot(lx, ly, lz, nx, ny, nz);
    fc_r = fc_g = fc_b = pdf = 0.0f;
    if (!(g.woz > 0.0f) || !(wiz > 0.0f)) return;
    float hx, hy, hz, woh, ratio;
    glossy_half(g, wix, wiy, wiz, hx, hy, hz, woh);
    glossy_terms(plastic, alpha, f0r, f0g, f0b, rho_r, rho_g, rho_b, g, wix, wiy, wiz, hx, hy, hz, woh, fc_r, fc_g, fc_b, pdf, ratio);
    if (mode == GLOSSY_GLASS) {
        float ct;
        const float F = glass_fresnel_of(fresnel_call, eta, woh, ct);
        fc_r *= F, fc_g *= F, fc_b *= F, pdf *= F;
    }
}
RTMI_HD void glossy_eval(bool plastic, float nx, float ny, float nz, float ux, float uy, float uz, float alpha, float f0r, float f0g,
                         float f0b, float rho_r, float rho_g, float rho_b, float lx, float ly, float lz, float &fc_r, float &fc_g,
                         float &fc_b, float &pdf) {
    glossy_eval_body(plastic ? GLOSSY_PLASTIC : GLOSSY_METAL, nx, ny, nz, ux, uy, uz, alpha, f0r, f0g, f0b, rho_r, rho_g, rho_b, 1.0f, lx, ly,
                     lz, fc_r, fc_g, fc_b, pdf);
}

}  // namespace rtmi
