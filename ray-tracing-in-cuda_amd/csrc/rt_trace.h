// Ray queries: the guard a caller-supplied ray passes before it may enter the walk, shared by the kernel
// (trace.hip, through render_body.h) and the host evaluation (rt_ray_valid), like rt_motion.h.  The guard is bit tests and
// one fp32 expression in a fixed order: the host and the device give the same verdict.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "philox.h"  // RTMI_HD

// (Rays per work item of trace_kernel, RT_TRACE_ITEM of include/rtmi.h = 64: a run of consecutive rays that one wave pulls
// from the global counter.  One wave-width: a wave that starts, or has gone idle as a whole, fills every lane from one item,
// neighbours of a coherent batch share a wave, an item costs one atomic for 64 queries, and what a wave holds when the counter
// runs dry -- the launch's tail -- is at most 64 rays.  It decides who traces a ray, never what the ray's record is.)

namespace rtmi {

RTMI_HD uint32_t trace_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

// finite: the exponent field is not all ones
RTMI_HD bool trace_finite(float x) { return (trace_bits(x) & 0x7f800000u) != 0x7f800000u; }

// May this ray enter the walk?  Every component of origin and dir finite, t_max not NaN (+-inf and negative values are
// fine: a negative t_max misses), and dir.dir -- the fp32 value the kernels keep as the ray's A -- a normal number: not zero,
// denormal, infinite or NaN (1 / A and the reciprocals of the DDA have to be finite).
RTMI_HD bool ray_valid(float ox, float oy, float oz, float t_max, float dx, float dy, float dz) {
    const bool fin = trace_finite(ox) && trace_finite(oy) && trace_finite(oz) && trace_finite(dx) && trace_finite(dy) && trace_finite(dz);
    const float dd = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
    const uint32_t e = trace_bits(dd) & 0x7f800000u;
    return fin && !(t_max != t_max) && e != 0u && e != 0x7f800000u;
}

}  // namespace rtmi
