// The hot path: per-pixel path tracing on gfx950 (MI355X).
//
// Replaces   render<<<(W/8+1,H/8+1),(8,8)>>>   gpu-version/main.cu:72-105
//            ray_color                         gpu-version/main.cu:17-70  (semantics:
//                                              cmake-cpu-version/main.cpp:13-43)
//            hittable_list::hit + sphere/rect/cylinder::hit   gpu-version/object.cuh
//            material::scatter / emitted       gpu-version/material.cuh
//            camera::get_ray                   cmake-cpu-version/camera.h:32-39
//            curand XORWOW per-pixel state     -> Philox-seeded xorshift128 per (pixel, sample) (philox.h)
//
// Shape of the kernel
//   * 256-thread workgroup = 4 wave64 (variants 2 and 6: 15 wave64, kernels.h); the grid only fills the chip (persistent waves) and
//     every wave pulls work items -- an 8x8 pixel tile x 64 sample indices -- from one
//     global counter.  A work-item (lane) owns ONE PATH at a time and runs its whole
//     bounce loop (get_color), exactly as the reference's thread does for its pixel.
//   * lanes stay converged across bounces: every iteration of the main loop is one
//     closest-hit query for all live lanes over a wave-uniform primitive loop.  A lane
//     whose path ended adds the radiance to its pixel and immediately takes the next
//     (pixel, sample) item of the tile's pool -- __ballot of the idle lanes, mbcnt for
//     the rank, a wave-uniform cursor -- so no lane waits for the slowest pixel of the
//     tile; the loop leaves on !__any(active) with the pool empty.
//     (variant bit 0 restores strict ownership: a lane only takes samples of its own
//     pixel.  Results are identical; it is kept to measure what the pool buys.)
//   * that hand-off is legal because the per-pixel sum is exact: each fp32 sample is
//     added as 64-bit fixed point (2^-24), in LDS per tile, then one 64-bit global
//     atomic per pixel and channel; a second kernel converts to the fp32 framebuffer
//     with fully coalesced stores.
//   * the primitive tables the inner loop reads ("hot" part of the scene image,
//     device_scene.h) are copied into LDS once per workgroup; all lanes read the same
//     record (broadcast ds_read_b128), four spheres are fetched one batch ahead of use.
//     No virtual calls, no pointer chasing; cold data (1/r, material records) stays in
//     global memory / L2 and is read once per bounce.
//   * the list is not scanned blindly: after the few big spheres, clusters of 8 spheres are
//     tested only when some lane's ray reaches the cluster's bounding box (aabb.hpp slab test
//     per lane + one __ballot), with a per-lane margin that covers the fp32 error of the
//     sphere test so that the closest hit -- and the framebuffer -- stay bit-identical to the
//     full scan (variant bit 4 is the full scan).
//   * arithmetic: fp32, every fused multiply-add explicit (-ffp-contract=off), IEEE
//     sqrt and divide, so results are bit-identical to the scalar restatement the
//     tests check against.
#include "kernels.h"
#include "render_device.h"

namespace rtmi {

// ---------------------------------------------------------------- kernel
// POOL:     idle lanes take the next (pixel, sample) item of the wave's tile (default)
//           / false: a lane only renders samples of its own pixel (ablation: the north_star's literal lane-per-pixel shape)
// SCALAR:   nothing is staged in LDS: every table is read from global memory -- wave-uniform reads through
//           the scalar cache (SGPR operands), per-lane reads through the vector L1/L2.  The mode for scenes
//           whose tables would crowd out occupancy or not fit the 160 KB at all.
// CULL:     the candidate search of the closest-hit query.  Every search is conservative with respect to the fp32 error of
//           the primitive tests, so the closest hit -- and the framebuffer -- equal the reference's linear scan bit for bit.
//           5  uniform grid over the clustered spheres, COMPACT tables (16-bit list entries, one word per cell): sphere-only
//              scenes whose tables fit LDS beside full occupancy.  Every lane walks the cells its ray crosses front to back.
//           6  the same for a grid one cell high (a sheet of spheres on the ground: RTIOW): the walk has no y axis
//           7  the same walk over the WIDE tables (32-bit list entries, two words per cell, up to 1023 cells per axis): every
//              other scene.  Its cells also list the rectangles, cylinders and triangles (taichi-version/bvh.py:109-199
//              indexes every hittable): a lane tests what its cells list; only the oversized primitives (the RTIOW ground,
//              a room's walls) are tested for every query
//           8  the walk of 7 over wide tables with NESTED cells (rt_scene_set_nested_grid): a cell that clustered geometry
//              overfills carries a sub-grid, which the lane walks while its ray is inside the cell.  Tables in global memory only
//           ablations (RTMI_ABLATIONS builds): 3 range tables, 2 two-level box hierarchy per lane (round 1's default), 1 wave
//           votes per cluster box (aabb.hpp:15-29 + __any), 0 no culling: the reference's linear hittable_list scan
// EXT:      the Taichi renderer's extras -- triangles (taichi-version/hittable.py:38-71) and image textures read at the
//           hit record's (u, v) (material.py:137-144).  Only the builds for scenes that use them carry the code: it
//           costs the kernel its register budget (86 spilled VGPRs instead of 23) whether a scene uses it or not.
// SPH:      the scene holds spheres only (RTIOW, the 3-sphere scene): no rectangle / cylinder / triangle code, no dispatch
//           on the winner's type -- and, what pays, a dozen fewer launch values and loop-invariant masks competing for scalar
//           registers (the surplus of those lives in the lanes of a spill VGPR: one v_readlane per use).  The compact-table
//           kernels (CULL 5, 6) are built this way only.
// NEE:      light sampling (rt_scene_set_light_sampling): one light sample per eligible vertex, combined with the BSDF sample
//           by multiple importance sampling (power heuristic).  The sample's visibility is a SHADOW PHASE of the lane: the
//           lane's next query is the shadow ray (same origin, best_t starting below 1, any hit occludes); then the lane
//           adds the sample's contribution and restores its continuation.  Only render_nee_kernel carries it.
// The sphere-only compact-table instances (variants 2 and 6) run workgroups of kBigGroupWaves waves that share one staged
// copy of the tables, two per CU at a register budget of their own (kernels.h); every other instance runs four waves.
template <bool COUNT, bool POOL, bool SCALAR, int CULL, bool EXT, bool SPH>
__global__ __launch_bounds__(64 * (big_group(COUNT, POOL, SCALAR, CULL, SPH) ? kBigGroupWaves : kGroupWaves),
                             big_group(COUNT, POOL, SCALAR, CULL, SPH) ? RT_BIG_WAVES_PER_SIMD : RT_WAVES_PER_SIMD) void render_kernel(const RenderParams P, const float4 *__restrict__ image,
                                                     unsigned long long *__restrict__ acc,
                                                     unsigned int *__restrict__ queue,
                                                     DevCounters *__restrict__ counters) {
    constexpr bool NEE = false, AOV = false, ENV = false, MEDIA = false, MOTION = false, QUERY = false;
    constexpr TraceArgs TQ{nullptr, nullptr, 0u, 0};
    constexpr bool ALPHA = false;  // (alpha cutouts, DESIGN 7v: the instances of alpha_kernel.h alone)
    constexpr bool CAMERA = false;  // (camera projections, DESIGN 7w: the instances of camera_kernel.h alone)
#include "render_body.h"
}

// light sampling (NEE): the general layouts with triangles and image textures -- the linear scan (CULL 0) and the wide grid
// walk (CULL 7) with its tables in LDS or in global memory (SCALAR)
template <bool SCALAR, int CULL>
__global__ __launch_bounds__(256, RT_NEE_WAVES_PER_SIMD) void render_nee_kernel(const RenderParams P, const float4 *__restrict__ image,
                                                         unsigned long long *__restrict__ acc,
                                                         unsigned int *__restrict__ queue,
                                                         DevCounters *__restrict__ counters) {
    constexpr bool COUNT = false, POOL = true, EXT = true, SPH = false, NEE = true, AOV = false, ENV = false, MEDIA = false, MOTION = false, QUERY = false;
    constexpr TraceArgs TQ{nullptr, nullptr, 0u, 0};
    constexpr bool ALPHA = false;  // (alpha cutouts, DESIGN 7v: the instances of alpha_kernel.h alone)
    constexpr bool CAMERA = false;  // (camera projections, DESIGN 7w: the instances of camera_kernel.h alone)
#include "render_body.h"
}

// nested grid (rt_scene_set_nested_grid): the global-memory walk over wide tables with nested cells (CULL 8), plain and with
// triangles / image textures, and its counting build.  A kernel of its own, like the light-sampling one: the render_kernel
// instances of a product build stay the eight they were.
template <bool COUNT, bool EXT>
__global__ __launch_bounds__(256, RT_WAVES_PER_SIMD) void render_nested_kernel(const RenderParams P, const float4 *__restrict__ image,
                                                            unsigned long long *__restrict__ acc,
                                                            unsigned int *__restrict__ queue,
                                                            DevCounters *__restrict__ counters) {
    constexpr bool POOL = true, SCALAR = true, SPH = false, NEE = false, AOV = false, ENV = false, MEDIA = false, MOTION = false, QUERY = false;
    constexpr TraceArgs TQ{nullptr, nullptr, 0u, 0};
    constexpr int CULL = 8;
    constexpr bool ALPHA = false;  // (alpha cutouts, DESIGN 7v: the instances of alpha_kernel.h alone)
    constexpr bool CAMERA = false;  // (camera projections, DESIGN 7w: the instances of camera_kernel.h alone)
#include "render_body.h"
}

// first-hit feature passes (rt_render_hip_feature): a sample runs as in render_kernel up to its first closest-hit query -- same
// stream, jitter, lens draw, camera ray and walk -- and there adds the feature P.feature selects (a launch value) in place of
// radiance.  One query per sample, so the general builds (triangles, image textures) serve every scene: the linear scan (CULL 0),
// the wide grid walk (7) and the nested walk (8), tables in LDS or in global memory (SCALAR).
template <bool SCALAR, int CULL>
__global__ __launch_bounds__(256, RT_WAVES_PER_SIMD) void render_feature_kernel(const RenderParams P, const float4 *__restrict__ image,
                                                             unsigned long long *__restrict__ acc,
                                                             unsigned int *__restrict__ queue,
                                                             DevCounters *__restrict__ counters) {
    constexpr bool COUNT = false, POOL = true, EXT = true, SPH = false, NEE = false, AOV = true, ENV = false, MEDIA = false, MOTION = false, QUERY = false;
    constexpr TraceArgs TQ{nullptr, nullptr, 0u, 0};
    constexpr bool ALPHA = false;  // (alpha cutouts, DESIGN 7v: the instances of alpha_kernel.h alone)
    constexpr bool CAMERA = false;  // (camera projections, DESIGN 7w: the instances of camera_kernel.h alone)
#include "render_body.h"
}


// fixed-point pixel sums -> fp32 framebuffer (rgb_sum[(row*W + x)*3 + c]); every store
// instruction writes 256 contiguous bytes
__global__ __launch_bounds__(256) void finalize_kernel(const unsigned long long *__restrict__ acc,
                                                       float *__restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)((double)(long long)acc[i] * (1.0 / 16777216.0));
}

#ifdef RT_ISA_ONLY
// tools/isa_stats.py: one instance alone (RT_ISA_ONLY = its template-id, e.g. render_nee_kernel<false,7>) in place of the
// table, compiled to assembly in seconds
template __global__ void RT_ISA_ONLY(const RenderParams, const float4 *__restrict__, unsigned long long *__restrict__,
                                     unsigned int *__restrict__, DevCounters *__restrict__);
#else
// ---------------------------------------------------------------- the instances (kernels.h), and how render_host.hip runs one
// render_kernel<COUNT, POOL, SCALAR, CULL, EXT, SPH>.  The host resolves variant 0 to one of the five PRODUCT instances:
//    2  compact grid one cell high, tables in LDS (RTIOW)         6  compact grid, 3-D walk, tables in LDS (sphere-only scenes)
//   36  wide grid tables in LDS (scenes with other primitives)   44  wide grid tables in global memory (large scenes)
//   16  no culling -- the reference's linear hittable_list scan: what a scene of a handful of primitives of several types runs
//       (nothing is listed in a grid there; sample_scene.json 54 ms against 79 ms for 36 with its empty grid), and the
//       definition every other kernel's image is held to
// and 36, 44 and 16 also exist with EXT (triangles, image textures): eight render_kernel instances in a product build
// (make ABLATIONS=0), beside the light-sampling kernels, the feature kernels and variant 52, the nested-grid walk
// (render_nested_kernel: scenes with the nested grid on and a cell to nest; plain and EXT in every build, its counting build with
// RTMI_ABLATIONS).  The default build (RTMI_ABLATIONS=1: tests, bench.py) adds the measurement variants -- same image, bit for
// bit -- and the counting kernels:
//    1  variant 6 with strict one-lane-per-pixel ownership       40  variant 6 with its tables in global memory
//   17  variant 16 with strict ownership                         24  variant 16 with its tables in global memory
//   32  wave-level cluster votes      64  per-lane cluster lists through the two-level box hierarchy (round 1's default)
//  128  per-lane cluster lists through the range tables (first half of round 2)
// (the workgroup of variants 2 and 6: kernels.h)
constexpr int headline_waves(int cull) { return big_group(false, true, false, cull, true) ? kBigGroupWaves : kGroupWaves; }
constexpr int headline_wave_lds(int cull) { return kWaveAccBytes + (burst_starts(false, true, false, cull, true) ? kWaveSlabBytes : 0); }
constexpr int headline_groups(int cull) { return big_group(false, true, false, cull, true) ? kBigGroupsPerCu : 0; }
static const KernelRow kRows[] = {
    // {{family, variant, ext, count}, CULL, instance}
    {{K_PLAIN, 2, false}, 6, (const void *)&render_kernel<false, true, false, 6, false, true>, headline_waves(6), headline_wave_lds(6), headline_groups(6)},
    {{K_PLAIN, 6, false}, 5, (const void *)&render_kernel<false, true, false, 5, false, true>, headline_waves(5), headline_wave_lds(5), headline_groups(5)},
    {{K_PLAIN, 36, false}, 7, (const void *)&render_kernel<false, true, false, 7, false, false>},
    {{K_PLAIN, 44, false}, 7, (const void *)&render_kernel<false, true, true, 7, false, false>},
    {{K_PLAIN, 16, false}, 0, (const void *)&render_kernel<false, true, false, 0, false, false>},
    {{K_PLAIN, 36, true}, 7, (const void *)&render_kernel<false, true, false, 7, true, false>},
    {{K_PLAIN, 44, true}, 7, (const void *)&render_kernel<false, true, true, 7, true, false>},
    {{K_PLAIN, 16, true}, 0, (const void *)&render_kernel<false, true, false, 0, true, false>},
#if RTMI_ABLATIONS
    {{K_PLAIN, 1, false}, 5, (const void *)&render_kernel<false, false, false, 5, false, true>},
    {{K_PLAIN, 40, false}, 5, (const void *)&render_kernel<false, true, true, 5, false, true>},
    {{K_PLAIN, 17, false}, 0, (const void *)&render_kernel<false, false, false, 0, false, false>},
    {{K_PLAIN, 24, false}, 0, (const void *)&render_kernel<false, true, true, 0, false, false>},
    {{K_PLAIN, 32, false}, 1, (const void *)&render_kernel<false, true, false, 1, false, false>},
    {{K_PLAIN, 64, false}, 2, (const void *)&render_kernel<false, true, false, 2, false, false>},
    {{K_PLAIN, 128, false}, 3, (const void *)&render_kernel<false, true, false, 3, false, false>},
    {{K_PLAIN, 24, true}, 0, (const void *)&render_kernel<false, true, true, 0, true, false>},
    // counting kernels (rt_render_hip_count), one per variant: with EXT where the variant has such a build
    {{K_PLAIN, 6, false, true}, 5, (const void *)&render_kernel<true, true, false, 5, false, true>},
    {{K_PLAIN, 36, true, true}, 7, (const void *)&render_kernel<true, true, false, 7, true, false>},
    {{K_PLAIN, 44, true, true}, 7, (const void *)&render_kernel<true, true, true, 7, true, false>},
    {{K_PLAIN, 64, false, true}, 2, (const void *)&render_kernel<true, true, false, 2, false, false>},
    {{K_PLAIN, 128, false, true}, 3, (const void *)&render_kernel<true, true, false, 3, false, false>},
    {{K_NESTED, 52, true, true}, 8, (const void *)&render_nested_kernel<true, true>},
#endif
    // render_nested_kernel<COUNT, EXT>
    {{K_NESTED, 52, false}, 8, (const void *)&render_nested_kernel<false, false>},
    {{K_NESTED, 52, true}, 8, (const void *)&render_nested_kernel<false, true>},
    // render_nee_kernel<SCALAR, CULL>: the layouts of variant 0's general scenes
    {{K_NEE, 36, true}, 7, (const void *)&render_nee_kernel<false, 7>},
    {{K_NEE, 44, true}, 7, (const void *)&render_nee_kernel<true, 7>},
    {{K_NEE, 16, true}, 0, (const void *)&render_nee_kernel<false, 0>},
    // render_feature_kernel<SCALAR, CULL>: the layouts of variant 0's general scenes, the nested walk, and the linear scan over
    // global memory (24) for compact-table scenes whose scan tables do not fit LDS
    {{K_FEATURE, 36, true}, 7, (const void *)&render_feature_kernel<false, 7>},
    {{K_FEATURE, 44, true}, 7, (const void *)&render_feature_kernel<true, 7>},
    {{K_FEATURE, 16, true}, 0, (const void *)&render_feature_kernel<false, 0>},
    {{K_FEATURE, 24, true}, 0, (const void *)&render_feature_kernel<true, 0>},
    {{K_FEATURE, 52, true}, 8, (const void *)&render_feature_kernel<true, 8>},
};

const KernelRow *render_kernel_rows(size_t *n) {
    *n = sizeof kRows / sizeof kRows[0];
    return kRows;
}

bool has_ablations() { return RTMI_ABLATIONS != 0; }

const KernelRow *find_kernel(const KernelKey &key) {
    const KernelRow *(*const tables[])(size_t *) = {render_kernel_rows, env_kernel_rows, media_kernel_rows, motion_kernel_rows, trace_kernel_rows,
                                                       alpha_kernel_rows, alpha_nee_kernel_rows,
                                                       camera_kernel_rows, camera_nee_kernel_rows, camera_media_kernel_rows, media_nee_kernel_rows};
    for (auto rows_of : tables) {
        size_t n = 0;
        const KernelRow *rows = rows_of(&n);
        for (size_t i = 0; i < n; ++i) {
            const KernelKey &r = rows[i].key;
            if (r.family == key.family && r.variant == key.variant && r.count == key.count && (key.count || r.ext == key.ext) &&
                r.nee == key.nee && r.feature == key.feature && r.alpha == key.alpha && r.camera == key.camera)
                return &rows[i];
        }
    }
    return nullptr;
}

// one persistent launch of `grid` workgroups of the row's size (an error surfaces in the caller's hipGetLastError)
void launch_kernel(const KernelRow &row, const RenderParams &P, const void *image, unsigned long long *acc, unsigned int *queue,
                   DevCounters *counters, size_t lds_bytes, unsigned grid, hipStream_t stream) {
    void *args[] = {const_cast<RenderParams *>(&P), &image, &acc, &queue, &counters};
    (void)hipLaunchKernel(row.fn, dim3(grid), dim3(group_threads(row)), args, lds_bytes, stream);
}

// resident workgroups per CU of an instance at this dynamic-LDS size (advisory; an over-estimate only
// leaves late workgroups that find the queue empty)
int blocks_per_cu(const KernelRow &row, size_t lds_bytes) {
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, row.fn, (int)group_threads(row), lds_bytes);
    return (e == hipSuccess && n > 0) ? n : (row.groups_per_cu > 0 ? row.groups_per_cu : 4);
}

// lets the instance be launched with more than 64 KB of dynamic LDS; nonzero: refused
int set_max_dynamic_lds(const KernelRow &row, size_t bytes) {
    return hipFuncSetAttribute(row.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess;
}

__global__ void item_params_kernel(unsigned int *queue, ItemParams ip) {
    int *dst = reinterpret_cast<int *>(queue) + RT_ITEM_PARAMS_AT;
    // quad 0: tiles_x, bands, num_items, sample_first; quad 1: sample_count, spp_chunk, n_big, n_med;
    // quad 2: q_med, q_small, tile_rotate, n_list; quad 3: tile_rows, tile_first, tile_stride, local_rows
    const int v[16] = {ip.tiles_x, ip.bands, ip.num_items, ip.sample_first, ip.sample_count, ip.spp_chunk, ip.n_big,
                       ip.n_med, ip.q_med, ip.q_small, ip.tile_rotate, ip.n_list, ip.tile_rows, ip.tile_first, ip.tile_stride, ip.local_rows};
    for (int k = 0; k < 16; ++k) dst[k] = v[k];
}

void launch_item_params(unsigned int *queue, const ItemParams &ip, hipStream_t stream) {
    hipLaunchKernelGGL(item_params_kernel, dim3(1), dim3(1), 0, stream, queue, ip);
}

void launch_finalize(const unsigned long long *acc, float *out, size_t n, hipStream_t stream) {
    unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(finalize_kernel, dim3(grid), dim3(256), 0, stream, acc, out, n);
}
#endif  // RT_ISA_ONLY

}  // namespace rtmi
