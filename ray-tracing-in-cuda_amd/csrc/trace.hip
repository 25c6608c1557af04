// The ray-query kernels: closest hit and occlusion for rays the caller supplies (rt_trace_hip).  The body is
// render_body.h with QUERY on -- its candidate search and its winner section, nothing else: the refill hands out rays in
// place of (pixel, sample) pairs, behind the guard of rt_trace.h, and the winner writes the ray's record to memory in
// place of a scatter step.  There is one traversal in this project; this file adds a way in, not a second walk.  A kernel
// family and a translation unit of its own, like render_motion.hip: the render kernels keep their code.  Not a render
// kernel and not named like one (tests/golden/trace_kernel_instances.json lists its instances).
#include "kernels.h"
#include "render_device.h"

// minimum resident waves per SIMD of the query kernels: the plain kernels' (ISA rows in DESIGN 7k)
#ifndef RT_TRACE_WAVES_PER_SIMD
#define RT_TRACE_WAVES_PER_SIMD RT_WAVES_PER_SIMD
#endif

namespace rtmi {

// SCALAR, CULL: the general layouts render_feature_kernel has -- the linear scan (CULL 0), the wide grid walk (7) and the nested
// walk (8), tables in LDS or in global memory (SCALAR) -- always with triangles and image textures (EXT).  mode (RT_TRACE_*)
// is a launch value: it decides what a finished ray stores, once per ray.
template <bool SCALAR, int CULL>
__global__ __launch_bounds__(256, RT_TRACE_WAVES_PER_SIMD) void trace_kernel(const RenderParams P, const float4 *__restrict__ image,
                                                                             const float4 *__restrict__ rays, float4 *__restrict__ out,
                                                                             unsigned int *__restrict__ queue, unsigned int n, int mode) {
    constexpr bool COUNT = false, POOL = true, EXT = true, SPH = false, NEE = false, AOV = false, ENV = false, MEDIA = false, MOTION = false, QUERY = true;
    const TraceArgs TQ{rays, out, n, mode};
    // what the body's text names of the render kernels' parameters: never touched under QUERY
    unsigned long long *const acc = nullptr;
    DevCounters *const counters = nullptr;
    constexpr bool ALPHA = false;  // (alpha cutouts, DESIGN 7v: the instances of alpha_kernel.h alone)
    constexpr bool CAMERA = false;  // (camera projections, DESIGN 7w: the instances of camera_kernel.h alone)
#include "render_body.h"
}

#ifdef RT_ISA_ONLY
// tools/isa_stats.py: one instance alone (RT_ISA_ONLY = its template-id, e.g. trace_kernel<false,7>)
template __global__ void RT_ISA_ONLY(const RenderParams, const float4 *__restrict__, const float4 *__restrict__, float4 *__restrict__,
                                     unsigned int *__restrict__, unsigned int, int);
#else
static const KernelRow kRows[] = {
    // {{family, layout, ext}, CULL, instance}
    {{K_TRACE, 36, true}, 7, (const void *)&trace_kernel<false, 7>},
    {{K_TRACE, 44, true}, 7, (const void *)&trace_kernel<true, 7>},
    {{K_TRACE, 16, true}, 0, (const void *)&trace_kernel<false, 0>},
    {{K_TRACE, 24, true}, 0, (const void *)&trace_kernel<true, 0>},
    {{K_TRACE, 52, true}, 8, (const void *)&trace_kernel<true, 8>},
};

const KernelRow *trace_kernel_rows(size_t *n) {
    *n = sizeof kRows / sizeof kRows[0];
    return kRows;
}

// one persistent launch of `grid` workgroups of 256 over the n rays at `rays` (an error surfaces in the caller's hipGetLastError)
void launch_trace(const KernelRow &row, const RenderParams &P, const void *image, const void *rays, void *out, unsigned int *queue,
                  unsigned int n, int mode, size_t lds_bytes, unsigned grid, hipStream_t stream) {
    void *args[] = {const_cast<RenderParams *>(&P), &image, &rays, &out, &queue, &n, &mode};
    (void)hipLaunchKernel(row.fn, dim3(grid), dim3(256), args, lds_bytes, stream);
}
#endif  // RT_ISA_ONLY

}  // namespace rtmi
