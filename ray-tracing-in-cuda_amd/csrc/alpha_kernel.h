// The kernels of a scene with alpha masks: the render loop of render_body.h with ALPHA on, once per family that
// takes masks.  A kernel template and two translation units of their own (alpha_kernel.hip, alpha_nee_kernel.hip): every
// other instance is compiled with ALPHA off and keeps the code it had, whatever the masks' code costs in registers -- with
// the masks' code behind a run-time flag in the families' own instances, the layout-16 light-sampling kernel spilled 156
// vector registers instead of 123 and scenes without a mask rendered up to 10 % slower.  The host picks a row of these
// files iff the scene has a mask (render_host.hip).
#pragma once
#include "kernels.h"
#include "render_device.h"

#ifndef RT_MOTION_WAVES_PER_SIMD
#define RT_MOTION_WAVES_PER_SIMD RT_WAVES_PER_SIMD
#endif

namespace rtmi {

// FAMILY: what the instance carries beside the masks -- light sampling, a feature pass, an environment map, moving spheres;
// 0: the plain general kernel (render_kernel with EXT; CULL 8: render_nested_kernel).  SCALAR, CULL: the layouts 16, 36, 44, 52
enum AlphaFamily : int { AF_NEE = 1, AF_AOV = 2, AF_ENV = 4, AF_MOTION = 8 };
constexpr int alpha_waves(int family) {
    return (family & AF_NEE) ? RT_NEE_WAVES_PER_SIMD : (family & AF_MOTION) ? RT_MOTION_WAVES_PER_SIMD : RT_WAVES_PER_SIMD;
}

template <int FAMILY, bool SCALAR, int CULL>
__global__ __launch_bounds__(256, alpha_waves(FAMILY)) void alpha_kernel(const RenderParams P, const float4 *__restrict__ image,
                                                                         unsigned long long *__restrict__ acc, unsigned int *__restrict__ queue,
                                                                         DevCounters *__restrict__ counters) {
    static_assert(!((FAMILY & AF_NEE) && (FAMILY & AF_AOV)) && (!(FAMILY & AF_MOTION) || FAMILY == AF_MOTION), "no such family");
    constexpr bool COUNT = false, POOL = true, EXT = true, SPH = false, NEE = (FAMILY & AF_NEE) != 0, AOV = (FAMILY & AF_AOV) != 0,
                   ENV = (FAMILY & AF_ENV) != 0, MEDIA = false, MOTION = (FAMILY & AF_MOTION) != 0, QUERY = false, ALPHA = true, CAMERA = false;
    constexpr TraceArgs TQ{nullptr, nullptr, 0u, 0};
#include "render_body.h"
}

#ifdef RT_ISA_ONLY
// tools/isa_stats.py: one instance alone (RT_ISA_ONLY = its template-id, e.g. alpha_kernel<1,false,0>)
template __global__ void RT_ISA_ONLY(const RenderParams, const float4 *__restrict__, unsigned long long *__restrict__,
                                     unsigned int *__restrict__, DevCounters *__restrict__);
#endif

}  // namespace rtmi
