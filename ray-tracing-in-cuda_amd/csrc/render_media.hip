// The media kernels: the render loop of render_body.h with MEDIA on -- after every closest-hit query the scene's
// homogeneous media (rt_media.h) are walked, and a free-flight event nearer than the surface hit becomes a scattering
// vertex: isotropic, or by the medium's Henyey-Greenstein phase function (rt_phase.h).  A kernel family and a translation unit of its own, like render_env.hip: the instances of
// render_kernel.hip keep their code.  The helpers are render_device.h's; the host finds the instances through this file's
// rows (kernels.h).
#include "kernels.h"
#include "render_device.h"

// minimum resident waves per SIMD of the media kernels: the plain kernels' (the walk keeps two values per lane; ISA row in DESIGN 7f)
#ifndef RT_MEDIA_WAVES_PER_SIMD
#define RT_MEDIA_WAVES_PER_SIMD RT_WAVES_PER_SIMD
#endif

namespace rtmi {

// SCALAR, CULL: the layouts of variant 0's general scenes (16, 36, 44), always with triangles and image textures (EXT)
template <bool SCALAR, int CULL>
__global__ __launch_bounds__(256, RT_MEDIA_WAVES_PER_SIMD) void render_media_kernel(
    const RenderParams P, const float4 *__restrict__ image, unsigned long long *__restrict__ acc, unsigned int *__restrict__ queue,
    DevCounters *__restrict__ counters) {
    constexpr bool COUNT = false, POOL = true, EXT = true, SPH = false, NEE = false, AOV = false, ENV = false, MEDIA = true, MOTION = false, QUERY = false;
    constexpr TraceArgs TQ{nullptr, nullptr, 0u, 0};
    constexpr bool ALPHA = false;  // (alpha cutouts, DESIGN 7v: the instances of alpha_kernel.h alone)
    constexpr bool CAMERA = false;  // (camera projections, DESIGN 7w: the instances of camera_kernel.h alone)
#include "render_body.h"
}

#ifdef RT_ISA_ONLY
// tools/isa_stats.py: one instance alone (RT_ISA_ONLY = its template-id, e.g. render_media_kernel<false,7>)
template __global__ void RT_ISA_ONLY(const RenderParams, const float4 *__restrict__, unsigned long long *__restrict__,
                                     unsigned int *__restrict__, DevCounters *__restrict__);
#else
static const KernelRow kRows[] = {
    // {{family, layout, ext}, CULL, instance}
    {{K_MEDIA, 36, true}, 7, (const void *)&render_media_kernel<false, 7>},
    {{K_MEDIA, 44, true}, 7, (const void *)&render_media_kernel<true, 7>},
    {{K_MEDIA, 16, true}, 0, (const void *)&render_media_kernel<false, 0>},
};

const KernelRow *media_kernel_rows(size_t *n) {
    *n = sizeof kRows / sizeof kRows[0];
    return kRows;
}
#endif  // RT_ISA_ONLY

}  // namespace rtmi
