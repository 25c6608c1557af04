// The motion kernels: the render loop of render_body.h with MOTION on -- every sample carries a shutter time, and
// every closest-hit query tests the scene's moving spheres (rt_motion.h) at that time behind the static primitives.  A kernel
// family and a translation unit of its own, like render_media.hip: the instances of render_kernel.hip keep their code.  The
// helpers are render_kernel.hip's: included here without its kernels' instances.
#define RT_MOTION_TU 1
#include "render_kernel.hip"

// minimum resident waves per SIMD of the motion kernels: the plain kernels' (a path keeps one more value per lane, its shutter time; ISA rows in DESIGN 7g)
#ifndef RT_MOTION_WAVES_PER_SIMD
#define RT_MOTION_WAVES_PER_SIMD RT_WAVES_PER_SIMD
#endif

namespace rtmi {

// SCALAR, CULL: the layouts of variant 0's general scenes (16, 36, 44), always with triangles and image textures (EXT)
template <bool SCALAR, int CULL>
__global__ __launch_bounds__(256, RT_MOTION_WAVES_PER_SIMD) void render_motion_kernel(
    const RenderParams P, const float4 *__restrict__ image, unsigned long long *__restrict__ acc, unsigned int *__restrict__ queue,
    DevCounters *__restrict__ counters) {
    constexpr bool COUNT = false, POOL = true, EXT = true, SPH = false, NEE = false, AOV = false, ENV = false, MEDIA = false, MOTION = true;
#include "render_body.h"
}

#if defined(RT_ISA_ONLY_MOTION)
// tools/isa_stats.py --motion: one instance alone (RT_ISA_ONLY_MOTION = SCALAR, CULL)
template __global__ void render_motion_kernel<RT_ISA_ONLY_MOTION>(const RenderParams, const float4 *__restrict__, unsigned long long *__restrict__,
                                                                unsigned int *__restrict__, DevCounters *__restrict__);
#else
// X(layout, SCALAR, CULL)
#define RT_MOTION_TABLE(X) \
    X(36, false, 7)       \
    X(44, true, 7)        \
    X(16, false, 0)

// launches the motion kernel of a layout (16, 36 or 44); false: no such build
bool launch_render_motion(const RenderParams &P, const void *image, unsigned long long *acc, unsigned int *queue, size_t lds_bytes,
                         unsigned grid, hipStream_t stream, unsigned layout) {
    const float4 *img = (const float4 *)image;
    DevCounters *none = nullptr;
#define RT_LAUNCH_MOTION(V, SCALAR, CULL)                                                                                          \
    if (layout == V) {                                                                                                             \
        hipLaunchKernelGGL((render_motion_kernel<SCALAR, CULL>), dim3(grid), dim3(256), lds_bytes, stream, P, img, acc, queue, none); \
        return true;                                                                                                               \
    }
    RT_MOTION_TABLE(RT_LAUNCH_MOTION)
#undef RT_LAUNCH_MOTION
    return false;
}

bool layout_has_motion(unsigned layout) {
#define RT_HAS_MOTION(V, SCALAR, CULL) \
    if (layout == V) return true;
    RT_MOTION_TABLE(RT_HAS_MOTION)
#undef RT_HAS_MOTION
    return false;
}

int blocks_per_cu_motion(unsigned layout, size_t lds_bytes) {
    int n = 0;
    hipError_t e = hipErrorInvalidValue;
#define RT_OCC_MOTION(V, SCALAR, CULL) \
    if (layout == V) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_motion_kernel<SCALAR, CULL>, 256, lds_bytes);
    RT_MOTION_TABLE(RT_OCC_MOTION)
#undef RT_OCC_MOTION
    return (e == hipSuccess && n > 0) ? n : 4;
}

int set_max_dynamic_lds_motion(size_t bytes) {
#define RT_ATTR_MOTION(V, SCALAR, CULL)                                                                                              \
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&render_motion_kernel<SCALAR, CULL>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                            (int)bytes) != hipSuccess)                                                                              \
        return 1;
    RT_MOTION_TABLE(RT_ATTR_MOTION)
#undef RT_ATTR_MOTION
    return 0;
}
#endif  // RT_ISA_ONLY_MOTION

}  // namespace rtmi
