// The kernels of a scene whose camera is not the perspective one: the render loop of render_body.h with CAMERA on,
// once per family and general layout.  A kernel template and three translation units of their own (camera_kernel.hip,
// camera_nee_kernel.hip, camera_media_kernel.hip), after the pattern of alpha_kernel.h: every other instance is compiled with
// CAMERA off and keeps the instructions it had.  The host picks a row of these files iff the scene's projection is
// orthographic, panoramic or fisheye (render_host.hip); the model number is a kernel argument (RT_PFLAG_PROJ_*), so one
// instance serves the three.  Not combined with alpha masks: a third copy of every family is not worth its build time now,
// and the host refuses such a scene.
#pragma once
#include "kernels.h"
#include "render_device.h"

#ifndef RT_MOTION_WAVES_PER_SIMD
#define RT_MOTION_WAVES_PER_SIMD RT_WAVES_PER_SIMD
#endif
#ifndef RT_MEDIA_WAVES_PER_SIMD
#define RT_MEDIA_WAVES_PER_SIMD RT_WAVES_PER_SIMD
#endif

namespace rtmi {

// FAMILY: what the instance carries beside the projections -- light sampling, a feature pass, an environment map, moving
// spheres, media; 0: the plain general kernel (render_kernel with EXT; CULL 8: render_nested_kernel).  SCALAR, CULL: the
// layouts 16, 36, 44, 52
enum CameraFamily : int { CF_NEE = 1, CF_AOV = 2, CF_ENV = 4, CF_MOTION = 8, CF_MEDIA = 16 };
constexpr int camera_waves(int family) {
    return (family & CF_NEE)      ? RT_NEE_WAVES_PER_SIMD
           : (family & CF_MOTION) ? RT_MOTION_WAVES_PER_SIMD
           : (family & CF_MEDIA)  ? RT_MEDIA_WAVES_PER_SIMD
                                  : RT_WAVES_PER_SIMD;
}

template <int FAMILY, bool SCALAR, int CULL>
__global__ __launch_bounds__(256, camera_waves(FAMILY)) void camera_kernel(const RenderParams P, const float4 *__restrict__ image,
                                                                           unsigned long long *__restrict__ acc, unsigned int *__restrict__ queue,
                                                                           DevCounters *__restrict__ counters) {
    static_assert(!((FAMILY & CF_NEE) && (FAMILY & CF_AOV)) && (!(FAMILY & CF_MOTION) || FAMILY == CF_MOTION) &&
                      (!(FAMILY & CF_MEDIA) || FAMILY == CF_MEDIA),
                  "no such family");
    constexpr bool COUNT = false, POOL = true, EXT = true, SPH = false, NEE = (FAMILY & CF_NEE) != 0, AOV = (FAMILY & CF_AOV) != 0,
                   ENV = (FAMILY & CF_ENV) != 0, MEDIA = (FAMILY & CF_MEDIA) != 0, MOTION = (FAMILY & CF_MOTION) != 0, QUERY = false,
                   ALPHA = false, CAMERA = true;
    constexpr TraceArgs TQ{nullptr, nullptr, 0u, 0};
#include "render_body.h"
}

#ifdef RT_ISA_ONLY
// tools/isa_stats.py: one instance alone (RT_ISA_ONLY = its template-id, e.g. camera_kernel<1,false,0>)
template __global__ void RT_ISA_ONLY(const RenderParams, const float4 *__restrict__, unsigned long long *__restrict__,
                                     unsigned int *__restrict__, DevCounters *__restrict__);
#endif

}  // namespace rtmi
