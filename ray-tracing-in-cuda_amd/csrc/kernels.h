// The render kernels as the host sees them: one row per built instance, named by what render_host.hip knows when it has
// to pick one.  Each of the kernel translation units (render_kernel.hip, render_env.hip, render_media.hip,
// render_motion.hip, and trace.hip for the ray queries) lists its instances in a static array of rows -- taking a kernel's address in a row is what
// instantiates it -- and the host resolves a launch ONCE, to a row, and launches, sizes the grid and raises the LDS limit
// through the row's function pointer.  A new family is a kernel definition and its rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "device_scene.h"
#include "rt_beam.h"

namespace rtmi {

enum KernelFamily {
    K_PLAIN,    // render_kernel
    K_NEE,      // render_nee_kernel: light sampling
    K_NESTED,   // render_nested_kernel: the nested-grid walk (variant 52)
    K_FEATURE,  // render_feature_kernel: first-hit feature passes
    K_ENV,      // render_env_kernel: an environment map (plain, with light sampling, or a feature pass)
    K_MEDIA,    // render_media_kernel; with light sampling (key.nee): media_nee_kernel
    K_MOTION,   // render_motion_kernel
    K_TRACE,    // trace_kernel: ray queries (rt_trace_hip); not a render kernel, launched through launch_trace
};

struct KernelKey {
    KernelFamily family;
    unsigned variant;      // the variant (K_PLAIN, K_NESTED) or layout (every other family) number of rt_opts.variant, never 0
    bool ext;              // built with triangles and image textures (every family but K_PLAIN and K_NESTED: always)
    bool count = false;    // a counting build (rt_render_hip_count).  It serves scenes with and without triangles / textures:
                           // find_kernel() does not compare `ext` for it
    bool nee = false;      // K_ENV, K_MEDIA: with light sampling
    bool feature = false;  // K_ENV: a feature pass
    bool alpha = false;    // an instance of alpha_kernel.h: the family's kernel with the alpha cutouts' code, for a scene
                           // with masks; every other scene runs the rows without it, whose code knows nothing of masks
    bool camera = false;   // an instance of camera_kernel.h: the family's kernel with the projections' path start, for a
                           // scene whose camera is orthographic, panoramic or fisheye; a perspective scene runs the rows without it
};

// The workgroup of an instance.  Every family runs 4 waves with one 1.5 KB tile accumulator each; the sphere-only
// compact-table instances (variants 2 and 6) run kBigGroupWaves, which share ONE staged copy of the scene tables, and each
// wave of theirs has a slab of 64 prepared camera rays behind its accumulator (render_body.h, the burst).  Two such
// workgroups are resident on a CU; with the largest LDS-resident tables (pack.h, kLdsTableBytes) they take
// 2 x (17.3 + 15 x (1.5 + 2.5)) = 154.6 of its 160 KB.
// The shape is the measured one (profiles/headline_bursts_mi355x.txt).  A workgroup's waves are dealt to the four
// SIMDs from the first one on, so two groups of n waves put 2 ceil(n / 4) waves on SIMD 0: at the 72-register budget of
// 7 waves per SIMD two groups of 14 never share a CU (one ran alone: 148 ms against 105).  What fits is 24 waves at 80
// registers (3 x 8 or 2 x 12) or up to 32 at 64 registers; 2 x 15 at 64 is the fastest shape that also holds the largest tables.
// (measurement knobs of render_kernel.hip, tools/build_ab.sh: -DRT_BIG_GROUPS=0 builds variants 2 and 6 in the 4-wave shape,
//  -DRT_BURSTS=0 the big groups without the slabs, -DRT_BIG_WAVES=n -DRT_BIG_WAVES_PER_SIMD=m other shapes)
#ifndef RT_BIG_GROUPS
#define RT_BIG_GROUPS 1
#endif
#ifndef RT_BURSTS
#define RT_BURSTS 1
#endif
// The burst also TRACES its 64 camera rays (render_body.h): the first closest-hit query of every path runs there, dense and
// coherent, a ray that leaves the scene or ends on an emitter is settled there, and the slot of a scattering hit holds
// {hit point, direction, generator state} -- the winner's id rides in the upper half of the lane's home-row register.
// -DRT_BURST_TRACE=0: the burst hands out camera rays and the main loop runs every query (the control of the A/B);
// -DRT_BURST_REPOP=0: a lane that pops a settled slot waits for the next iteration instead of taking a following slot.
#ifndef RT_BURST_TRACE
#define RT_BURST_TRACE 1
#endif
#ifndef RT_BURST_REPOP
#define RT_BURST_REPOP 1
#endif
// The traced burst tests its tile's LIST (rt_beam.h, render_burst.h): the 64 rays of a burst are one sample of every pixel of
// one 8x8 tile, a thin beam that the camera, the frame size and the tile fix; which staged spheres it can touch is a table
// the host builds once per camera (tile_beams.hip, render_host.hip) and the burst reads with uniform loads.  Behind a record
// the first query of a path is a wave-uniform loop over its ids: no prefix, no grid clip, no walk.
// -DRT_BURST_LISTS=0: the burst runs the full query for every tile (the control of the A/B); no table is built.
#ifndef RT_BURST_LISTS
#define RT_BURST_LISTS 1
#endif
// (The traced burst sits at the top of the main loop's iteration.  Inside the refill, where the untraced one sits, it was
//  measured 5 ms slower than the parent: DESIGN 5, profiles/headline_first_hit_mi355x.txt.)
// The id's bits above the row (bits 16 .. 16 + kBurstIdBits - 1 of c_hy): enough for every record index of a table that is
// staged in LDS at all, whatever bound the packer sets for it (pack.h, kLdsTableBytes; render_host.hip asserts that one too)
constexpr size_t kCuLdsBytes = 160 * 1024;  // LDS of a CU
constexpr int kBurstIdBits = 15;
#ifndef RT_BIG_WAVES
#define RT_BIG_WAVES 15
#endif
#ifndef RT_BIG_WAVES_PER_SIMD
#define RT_BIG_WAVES_PER_SIMD 8
#endif
constexpr int kGroupWaves = 4, kBigGroupWaves = RT_BIG_WAVES;
// workgroups of kBigGroupWaves that a CU holds: waves dealt from SIMD 0 on, RT_BIG_WAVES_PER_SIMD on each
constexpr int kBigGroupsPerCu = RT_BIG_WAVES_PER_SIMD / ((RT_BIG_WAVES + 3) / 4);
// is render_kernel<COUNT, POOL, SCALAR, CULL, EXT, SPH> built in the big shape / with bursts?
constexpr bool big_group(bool count, bool pool, bool scalar, int cull, bool sph) {
    return RT_BIG_GROUPS != 0 && sph && pool && !scalar && !count && (cull == 5 || cull == 6);
}
constexpr bool burst_starts(bool count, bool pool, bool scalar, int cull, bool sph) {
    return RT_BURSTS != 0 && big_group(count, pool, scalar, cull, sph);
}
constexpr int kWaveAccBytes = 192 * 8;          // 64 pixels x rgb, 64-bit fixed point
// alpha cutouts: five words per lane of a 4-wave workgroup behind the accumulators -- what a query keeps while it
// passes through holes (render_body.h).  Added to the LDS of a launch of an alpha_kernel.h instance
constexpr int kAlphaLdsBytes = 5 * 4 * 64 * 4;
constexpr int kWaveSlabBytes = 64 * 10 * 4;     // 64 x {hit point (RT_BURST_TRACE=0: origin), direction, generator state}

struct KernelRow {
    KernelKey key;
    int cull;        // the instance's CULL template argument: decides how much of the hot tables is staged
    const void *fn;  // the kernel instance
    int waves = kGroupWaves;         // waves per workgroup
    int wave_lds = kWaveAccBytes;    // LDS per wave behind the staged tables
    int groups_per_cu = 0;           // workgroups a CU holds by registers and wave slots (0: one per wave of a SIMD's budget)
};

// block size and dynamic LDS of a launch of `row` with `table_bytes` of staged tables
inline unsigned group_threads(const KernelRow &row) { return 64u * (unsigned)row.waves; }
inline size_t group_lds(const KernelRow &row, size_t table_bytes) { return table_bytes + (size_t)row.waves * (size_t)row.wave_lds; }

// the rows of a translation unit; *n: how many
const KernelRow *render_kernel_rows(size_t *n);  // render_kernel.hip: K_PLAIN, K_NEE, K_NESTED, K_FEATURE
const KernelRow *env_kernel_rows(size_t *n);     // render_env.hip
const KernelRow *alpha_kernel_rows(size_t *n);      // alpha_kernel.hip: K_PLAIN, K_NESTED, K_FEATURE, K_MOTION with alpha
const KernelRow *alpha_nee_kernel_rows(size_t *n);  // alpha_nee_kernel.hip: K_NEE, K_ENV with alpha
const KernelRow *camera_kernel_rows(size_t *n);        // camera_kernel.hip: K_PLAIN, K_NESTED, K_FEATURE, K_MOTION with a projection
const KernelRow *camera_nee_kernel_rows(size_t *n);    // camera_nee_kernel.hip: K_NEE, K_ENV with a projection
const KernelRow *camera_media_kernel_rows(size_t *n);  // camera_media_kernel.hip: K_MEDIA with a projection
const KernelRow *media_kernel_rows(size_t *n);   // render_media.hip
const KernelRow *media_nee_kernel_rows(size_t *n);  // media_nee_kernel.hip: K_MEDIA with light sampling
const KernelRow *motion_kernel_rows(size_t *n);  // render_motion.hip
const KernelRow *trace_kernel_rows(size_t *n);   // trace.hip

// render_kernel.hip
const KernelRow *find_kernel(const KernelKey &key);  // null: no such build
void launch_kernel(const KernelRow &row, const RenderParams &P, const void *image, unsigned long long *acc, unsigned int *queue,
                   DevCounters *counters, size_t lds_bytes, unsigned grid, hipStream_t stream);
int blocks_per_cu(const KernelRow &row, size_t lds_bytes);
int set_max_dynamic_lds(const KernelRow &row, size_t bytes);
bool has_ablations();
void launch_finalize(const unsigned long long *acc, float *out, size_t n, hipStream_t stream);
void launch_item_params(unsigned int *queue, const ItemParams &ip, hipStream_t stream);

// tile_beams.hip: the beam table of a frame (rt_beam.h) -- one record per 8x8 tile of the whole frame, row-major -- built from
// the device's packed image, and the table's address written behind the item parameters (queue[RT_BEAMS_AT], 64 bits)
void launch_tile_beams(const float *image, const BeamFrame &f, int tiles_x, int tiles_y, uint16_t *table, hipStream_t stream);
void launch_beam_address(unsigned int *queue, const uint16_t *table, hipStream_t stream);

// trace.hip: n rays (two 16-byte records each) -> out (three 16-byte records per ray, or one byte per ray in occlusion mode)
void launch_trace(const KernelRow &row, const RenderParams &P, const void *image, const void *rays, void *out, unsigned int *queue,
                  unsigned int n, int mode, size_t lds_bytes, unsigned grid, hipStream_t stream);

}  // namespace rtmi
