// Light sampling in participating media: the render loop of render_body.h with MEDIA and NEE both on -- a medium
// vertex takes a light sample weighed by its phase function (rt_phase.h), and a shadow ray sums the optical depth of its stays
// in the media (rt_media.h) without a draw; an unoccluded sample is multiplied by exp(-tau).  Opt-in per scene
// (rt_scene_set_media_light_sampling).  A kernel name and a translation unit of its own, like camera_kernel.hip: the instances
// of render_media.hip and render_kernel.hip keep their code.  The host finds the instances through this file's rows (kernels.h).
#include "kernels.h"
#include "render_device.h"

// minimum resident waves per SIMD: one fewer than the light-sampling kernels' 6 -- at 96 registers the instances spill 88 to 92
// vector registers into 208 bytes of scratch, at 80 they spill 131 to 178 into 272 to 288 (ISA rows and timings of both
// candidate shapes in DESIGN 7z)
#ifndef RT_MEDIA_NEE_WAVES_PER_SIMD
#define RT_MEDIA_NEE_WAVES_PER_SIMD 5
#endif

namespace rtmi {

// SCALAR, CULL: the layouts of variant 0's general scenes (16, 36, 44), always with triangles and image textures (EXT)
template <bool SCALAR, int CULL>
__global__ __launch_bounds__(256, RT_MEDIA_NEE_WAVES_PER_SIMD) void media_nee_kernel(
    const RenderParams P, const float4 *__restrict__ image, unsigned long long *__restrict__ acc, unsigned int *__restrict__ queue,
    DevCounters *__restrict__ counters) {
    constexpr bool COUNT = false, POOL = true, EXT = true, SPH = false, NEE = true, AOV = false, ENV = false, MEDIA = true, MOTION = false, QUERY = false;
    constexpr TraceArgs TQ{nullptr, nullptr, 0u, 0};
    constexpr bool ALPHA = false;  // (alpha cutouts, DESIGN 7v: the instances of alpha_kernel.h alone)
    constexpr bool CAMERA = false;  // (camera projections, DESIGN 7w: the instances of camera_kernel.h alone)
#include "render_body.h"
}

#ifdef RT_ISA_ONLY
// tools/isa_stats.py: one instance alone (RT_ISA_ONLY = its template-id, e.g. media_nee_kernel<false,7>)
template __global__ void RT_ISA_ONLY(const RenderParams, const float4 *__restrict__, unsigned long long *__restrict__,
                                     unsigned int *__restrict__, DevCounters *__restrict__);
#else
static const KernelRow kRows[] = {
    // {{family, layout, ext, count, nee}, CULL, instance}
    {{K_MEDIA, 36, true, false, true}, 7, (const void *)&media_nee_kernel<false, 7>},
    {{K_MEDIA, 44, true, false, true}, 7, (const void *)&media_nee_kernel<true, 7>},
    {{K_MEDIA, 16, true, false, true}, 0, (const void *)&media_nee_kernel<false, 0>},
};

const KernelRow *media_nee_kernel_rows(size_t *n) {
    *n = sizeof kRows / sizeof kRows[0];
    return kRows;
}
#endif  // RT_ISA_ONLY

}  // namespace rtmi
