// Rough glass: the third member of the glossy family.  Reflection or refraction about a visible normal of the GGX
// lobe, chosen by the exact unpolarised Fresnel term of that normal, with a Beer-Lambert tint for the distance travelled inside
// the object.  The material runs through the one body of rt_glossy.h (glossy_sample_body / glossy_eval_body with GLOSSY_GLASS:
// a rough metal with F0 = 1, glass_fresnel and the refracted direction); this file holds the tint and the material's entry
// points as the kernels use the body.  fp32 with a FIXED operation sequence, every fused multiply-add explicit: the kernels
// (render_body.h) and a host program (tests/glass_host_driver.cpp) compile this text, and tests/ref64_glass.py restates the
// model in numpy from its definition (include/rtmi.h).
//
// Vectors are LOCAL to duff_frame about the face-turned shading normal n, wo = -unit(d); alpha = max(r^2, 1e-3) comes from the
// packer; eta = front ? 1/ir : ir (the dielectric's ratio), both words from the packer.
#pragma once
#include "rt_glossy.h"

namespace rtmi {

// Tr of one channel: exp(-sigma dist), dist the length of the segment that arrived at a back hit
RTMI_HD float glass_tint(float sigma, float dist) { return expf(-(sigma * dist)); }

// The scatter step, in WORLD vectors as glossy_sample: n the unit shading normal, (ux, uy, uz) = unit(d) of the arriving ray.
// Draws: uf (reflect iff uf < F), then u1, u2 for the visible normal.  false: an absorbed vertex (absorbed_wo: wo.z <= 0; else
// the direction came out on the wrong side: wi.z <= 0 reflected, wi.z >= 0 refracted).  true: the unit direction (world),
// ratio = G2 / G1(wo) (the attenuation without the tint), and pdf_b = F G1(wo) D(h) / (4 wo.z) of a reflected direction, -1 of
// a refracted one (the light strategy never produces it: an emitter behind it counts at full weight).
RTMI_HD bool glass_sample(float nx, float ny, float nz, float ux, float uy, float uz, float alpha, float eta, float uf, float u1,
                          float u2, float &wx, float &wy, float &wz, float &ratio, float &pdf, bool &absorbed_wo, bool &reflected) {
    float at_g, at_b;
    return glossy_sample_body(GLOSSY_GLASS, nx, ny, nz, ux, uy, uz, alpha, 1.0f, 1.0f, 1.0f, 0.0f, 0.0f, 0.0f, eta, uf, u1, u2, wx, wy, wz,
                              ratio, at_g, at_b, pdf, absorbed_wo, reflected);
}

// The light sample's evaluation: f cos (without the tint) and pdf_b of the unit world direction (lx, ly, lz).  The light
// strategy covers the reflection hemisphere alone: zeros where the vertex or the direction is below the surface.
RTMI_HD void glass_eval(float nx, float ny, float nz, float ux, float uy, float uz, float alpha, float eta, float lx, float ly,
                        float lz, float &fc, float &pdf) {
    float fc_g, fc_b;
    glossy_eval_body(GLOSSY_GLASS, nx, ny, nz, ux, uy, uz, alpha, 1.0f, 1.0f, 1.0f, 0.0f, 0.0f, 0.0f, eta, lx, ly, lz, fc, fc_g, fc_b, pdf);
}

}  // namespace rtmi
