// The environment-map kernels: the render loop of render_body.h with ENV on -- a miss looks the direction up in the
// scene's environment map (rt_env.h), and with light sampling the map is one more sampled emitter.  A kernel family and a
// translation unit of its own: the instances of render_kernel.hip keep their code, and the two files compile side by side.
// The helpers (generator, square root, fixed point, ...) are render_device.h's; the host finds the instances through this
// file's rows (kernels.h).
#include "kernels.h"
#include "render_device.h"

namespace rtmi {

// SCALAR, CULL: the layouts of variant 0's general scenes (16, 36, 44), always with triangles and image textures (EXT).
// NEE_: light sampling (the shadow phase; 6 waves per SIMD like render_nee_kernel).  AOV_: a first-hit feature pass.
template <bool SCALAR, int CULL, bool NEE_, bool AOV_>
__global__ __launch_bounds__(256, NEE_ ? RT_NEE_WAVES_PER_SIMD : RT_WAVES_PER_SIMD) void render_env_kernel(
    const RenderParams P, const float4 *__restrict__ image, unsigned long long *__restrict__ acc, unsigned int *__restrict__ queue,
    DevCounters *__restrict__ counters) {
    static_assert(!(NEE_ && AOV_), "a feature sample ends at its first query");
    constexpr bool COUNT = false, POOL = true, EXT = true, SPH = false, NEE = NEE_, AOV = AOV_, ENV = true, MEDIA = false, MOTION = false, QUERY = false;
    constexpr TraceArgs TQ{nullptr, nullptr, 0u, 0};
    constexpr bool ALPHA = false;  // (alpha cutouts, DESIGN 7v: the instances of alpha_kernel.h alone)
    constexpr bool CAMERA = false;  // (camera projections, DESIGN 7w: the instances of camera_kernel.h alone)
#include "render_body.h"
}

#ifdef RT_ISA_ONLY
// tools/isa_stats.py: one instance alone (RT_ISA_ONLY = its template-id, e.g. render_env_kernel<false,7,true,false>)
template __global__ void RT_ISA_ONLY(const RenderParams, const float4 *__restrict__, unsigned long long *__restrict__,
                                     unsigned int *__restrict__, DevCounters *__restrict__);
#else
static const KernelRow kRows[] = {
    // {{family, layout, ext, count, nee, feature}, CULL, instance}: plain, with light sampling, a feature pass
    {{K_ENV, 36, true, false, false, false}, 7, (const void *)&render_env_kernel<false, 7, false, false>},
    {{K_ENV, 36, true, false, true, false}, 7, (const void *)&render_env_kernel<false, 7, true, false>},
    {{K_ENV, 36, true, false, false, true}, 7, (const void *)&render_env_kernel<false, 7, false, true>},
    {{K_ENV, 44, true, false, false, false}, 7, (const void *)&render_env_kernel<true, 7, false, false>},
    {{K_ENV, 44, true, false, true, false}, 7, (const void *)&render_env_kernel<true, 7, true, false>},
    {{K_ENV, 44, true, false, false, true}, 7, (const void *)&render_env_kernel<true, 7, false, true>},
    {{K_ENV, 16, true, false, false, false}, 0, (const void *)&render_env_kernel<false, 0, false, false>},
    {{K_ENV, 16, true, false, true, false}, 0, (const void *)&render_env_kernel<false, 0, true, false>},
    {{K_ENV, 16, true, false, false, true}, 0, (const void *)&render_env_kernel<false, 0, false, true>},
};

const KernelRow *env_kernel_rows(size_t *n) {
    *n = sizeof kRows / sizeof kRows[0];
    return kRows;
}
#endif  // RT_ISA_ONLY

}  // namespace rtmi
