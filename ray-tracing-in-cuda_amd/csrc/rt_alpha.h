// Alpha cutouts: the alpha byte of an image texture at the hit record's (u, v) against the material's cutoff byte
// decides whether the hit is a surface or a hole.  The rule itself, on integers, shared by the kernels (render_body.h), the
// packer (pack.hip) and a host program (tests/alpha_host_driver.cpp), as rt_tangent.h is.
//
//   texel    image_texel's nearest texel (render_device.h, image_texel_word): row from u, column from v, clamped
//   word     r8 | g8 << 8 | b8 << 16 | (255 - a8) << 24: an image without alpha keeps a zero top byte, the word it always had
//   cutoff   c8 = clamp(ceil(255 cutoff), 1, 255), once on the host in fp64 (0.5 -> 128)
//   verdict  transparent iff a8 < c8
//   cap      a query passes through at most RT_ALPHA_MAX_PASSES holes (device_scene.h); the next masked hit is opaque
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

// the cutoff byte of a cutoff in (0, 1] (host: fp64)
inline uint32_t alpha_cutoff_byte(double cutoff) {
    const double c = ceil(255.0 * cutoff);
    return c < 1.0 ? 1u : (c > 255.0 ? 255u : (uint32_t)c);
}

// the texel word's top byte <-> the alpha byte
RTMI_HD uint32_t alpha_word_bits(uint32_t a8) { return (255u - (a8 & 255u)) << 24; }
RTMI_HD uint32_t alpha_of_word(uint32_t word) { return 255u - (word >> 24); }

// the verdict: is a hit whose mask texel is `word` a hole for the cutoff byte c8?
RTMI_HD bool alpha_transparent(uint32_t word, uint32_t c8) { return alpha_of_word(word) < c8; }

}  // namespace rtmi
