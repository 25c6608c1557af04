// The environment-map kernels: the render loop of render_body.h with ENV on -- a miss looks the direction up in the
// scene's environment map (rt_env.h), and with light sampling the map is one more sampled emitter.  A kernel family and a
// translation unit of its own: the instances of render_kernel.hip keep their code, and the two files compile side by side.
// The helpers (generator, square root, fixed point, ...) are render_kernel.hip's: included here without its kernels' instances.
#define RT_ENV_TU 1
#include "render_kernel.hip"

namespace rtmi {

// SCALAR, CULL: the layouts of variant 0's general scenes (16, 36, 44), always with triangles and image textures (EXT).
// NEE_: light sampling (the shadow phase; 6 waves per SIMD like render_nee_kernel).  AOV_: a first-hit feature pass.
template <bool SCALAR, int CULL, bool NEE_, bool AOV_>
__global__ __launch_bounds__(256, NEE_ ? RT_NEE_WAVES_PER_SIMD : RT_WAVES_PER_SIMD) void render_env_kernel(
    const RenderParams P, const float4 *__restrict__ image, unsigned long long *__restrict__ acc, unsigned int *__restrict__ queue,
    DevCounters *__restrict__ counters) {
    static_assert(!(NEE_ && AOV_), "a feature sample ends at its first query");
    constexpr bool COUNT = false, POOL = true, EXT = true, SPH = false, NEE = NEE_, AOV = AOV_, ENV = true, MEDIA = false, MOTION = false;
#include "render_body.h"
}

#if defined(RT_ISA_ONLY_ENV)
// tools/isa_stats.py --env: one instance alone (RT_ISA_ONLY_ENV = SCALAR, CULL, NEE, AOV)
template __global__ void render_env_kernel<RT_ISA_ONLY_ENV>(const RenderParams, const float4 *__restrict__, unsigned long long *__restrict__,
                                                            unsigned int *__restrict__, DevCounters *__restrict__);
#else
// X(layout, SCALAR, CULL)
#define RT_ENV_TABLE(X) \
    X(36, false, 7)     \
    X(44, true, 7)      \
    X(16, false, 0)

// launches the environment kernel of a layout (16, 36 or 44): plain, with light sampling, or a feature pass; false: no such build
bool launch_render_env(const RenderParams &P, const void *image, unsigned long long *acc, unsigned int *queue, size_t lds_bytes,
                       unsigned grid, hipStream_t stream, unsigned layout, bool nee, bool feature) {
    const float4 *img = (const float4 *)image;
    DevCounters *none = nullptr;
    const dim3 g(grid), t(256);
#define RT_LAUNCH_ENV(V, SCALAR, CULL)                                                                                               \
    if (layout == V) {                                                                                                                \
        if (feature) hipLaunchKernelGGL((render_env_kernel<SCALAR, CULL, false, true>), g, t, lds_bytes, stream, P, img, acc, queue, none); \
        else if (nee) hipLaunchKernelGGL((render_env_kernel<SCALAR, CULL, true, false>), g, t, lds_bytes, stream, P, img, acc, queue, none); \
        else hipLaunchKernelGGL((render_env_kernel<SCALAR, CULL, false, false>), g, t, lds_bytes, stream, P, img, acc, queue, none); \
        return true;                                                                                                                  \
    }
    RT_ENV_TABLE(RT_LAUNCH_ENV)
#undef RT_LAUNCH_ENV
    return false;
}

bool layout_has_env(unsigned layout) {
#define RT_HAS_ENV(V, SCALAR, CULL) \
    if (layout == V) return true;
    RT_ENV_TABLE(RT_HAS_ENV)
#undef RT_HAS_ENV
    return false;
}

int blocks_per_cu_env(unsigned layout, size_t lds_bytes, bool nee, bool feature) {
    int n = 0;
    hipError_t e = hipErrorInvalidValue;
#define RT_OCC_ENV(V, SCALAR, CULL)                                                                                                   \
    if (layout == V) {                                                                                                                \
        if (feature) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_env_kernel<SCALAR, CULL, false, true>, 256, lds_bytes); \
        else if (nee) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_env_kernel<SCALAR, CULL, true, false>, 256, lds_bytes); \
        else e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_env_kernel<SCALAR, CULL, false, false>, 256, lds_bytes);   \
    }
    RT_ENV_TABLE(RT_OCC_ENV)
#undef RT_OCC_ENV
    return (e == hipSuccess && n > 0) ? n : 4;
}

int set_max_dynamic_lds_env(size_t bytes) {
#define RT_ATTR1(K)                                                                                                  \
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return 1;
#define RT_ATTR_ENV(V, SCALAR, CULL)                          \
    RT_ATTR1((render_env_kernel<SCALAR, CULL, false, false>)) \
    RT_ATTR1((render_env_kernel<SCALAR, CULL, true, false>))  \
    RT_ATTR1((render_env_kernel<SCALAR, CULL, false, true>))
    RT_ENV_TABLE(RT_ATTR_ENV)
#undef RT_ATTR_ENV
#undef RT_ATTR1
    return 0;
}
#endif  // RT_ISA_ONLY_ENV

}  // namespace rtmi
