// The metallic-roughness material: a base colour, a metalness and a roughness, the last two optionally scaled by
// the G and B channels of one map (glTF 2.0's metallicRoughnessTexture).  This file holds what is new about it -- how a hit's
// parameters are formed and how a vertex chooses its lobe.  Everything after the choice is rt_glossy.h: the vertex IS a rough
// metal (F0 = base colour) or a plastic (body = base colour, coat r0 from the index) of roughness r.  fp32 with a FIXED operation
// sequence, every fused multiply-add explicit, in the manner of rt_quad.h: the kernels (render_body.h) and a host program
// (tests/pbr_host_driver.cpp) compile this text, and tests/ref64_pbr.py restates the model in numpy from its definition
// (include/rtmi.h).
//
// Per-hit parameters are 8-bit BY DEFINITION: the base colour c8[3], the roughness r8 and the metalness m8 are integers in
// 0..255, x8 = (uint)fma(clamp(x, 0, 1), 255, 0.5), and the float of a byte is x8 / 255 (one division, as image_texel's).
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

// x in [0, 1] (clamped; a NaN goes to 0) -> its byte
RTMI_HD uint32_t pbr_byte(float x) { return (uint32_t)fmaf(fminf(fmaxf(x, 0.0f), 1.0f), 255.0f, 0.5f); }
// a byte -> its float
RTMI_HD float pbr_unit(uint32_t b) { return (float)b / 255.0f; }
// the lobe's alpha of a per-hit roughness (the packer's expression for the other glossy materials)
RTMI_HD float pbr_alpha(float r) { return fmaxf(r * r, 1e-3f); }

// A hit's parameters: base colour (cr, cg, cb), the map's channels G and B (1 without a map), the factors rf and mf ->
// c8 = r | g << 8 | b << 16 | r8 << 24 (the 32 bits a glossy vertex keeps for its light sample), and m8
RTMI_HD uint32_t pbr_params(float cr, float cg, float cb, float G, float B, float rf, float mf, uint32_t &m8) {
    m8 = pbr_byte(mf * B);
    return pbr_byte(cr) | pbr_byte(cg) << 8 | pbr_byte(cb) << 16 | pbr_byte(rf * G) << 24;
}

// The lobe choice from the first of the vertex's three draws: rough metal iff ul < m (m8 = 255: always, ul < 1; m8 = 0: never).
// Otherwise plastic, whose own lobe draw is the rest of the unit interval rescaled: ul' = (ul - m) / (1 - m); at m = 0 that is
// ul bit for bit.  -> metal; ulp = ul' (ul itself for a metal vertex, which does not use it)
RTMI_HD bool pbr_choose(uint32_t m8, float ul, float &ulp) {
    const float m = pbr_unit(m8);
    const bool metal = ul < m;
    ulp = metal ? ul : (ul - m) / (1.0f - m);
    return metal;
}

}  // namespace rtmi
