// The render kernels as the host sees them: one row per built instance, named by what render_host.hip knows when it has
// to pick one.  Each of the kernel translation units (render_kernel.hip, render_env.hip, render_media.hip,
// render_motion.hip, and trace.hip for the ray queries) lists its instances in a static array of rows -- taking a kernel's address in a row is what
// instantiates it -- and the host resolves a launch ONCE, to a row, and launches, sizes the grid and raises the LDS limit
// through the row's function pointer.  A new family is a kernel definition and its rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "device_scene.h"

namespace rtmi {

enum KernelFamily {
    K_PLAIN,    // render_kernel
    K_NEE,      // render_nee_kernel: light sampling
    K_NESTED,   // render_nested_kernel: the nested-grid walk (variant 52)
    K_FEATURE,  // render_feature_kernel: first-hit feature passes
    K_ENV,      // render_env_kernel: an environment map (plain, with light sampling, or a feature pass)
    K_MEDIA,    // render_media_kernel
    K_MOTION,   // render_motion_kernel
    K_TRACE,    // trace_kernel: ray queries (rt_trace_hip); not a render kernel, launched through launch_trace
};

struct KernelKey {
    KernelFamily family;
    unsigned variant;      // the variant (K_PLAIN, K_NESTED) or layout (every other family) number of rt_opts.variant, never 0
    bool ext;              // built with triangles and image textures (every family but K_PLAIN and K_NESTED: always)
    bool count = false;    // a counting build (rt_render_hip_count).  It serves scenes with and without triangles / textures:
                           // find_kernel() does not compare `ext` for it
    bool nee = false;      // K_ENV: with light sampling
    bool feature = false;  // K_ENV: a feature pass
};

struct KernelRow {
    KernelKey key;
    int cull;        // the instance's CULL template argument: decides how much of the hot tables is staged
    const void *fn;  // the kernel instance
};

// the rows of a translation unit; *n: how many
const KernelRow *render_kernel_rows(size_t *n);  // render_kernel.hip: K_PLAIN, K_NEE, K_NESTED, K_FEATURE
const KernelRow *env_kernel_rows(size_t *n);     // render_env.hip
const KernelRow *media_kernel_rows(size_t *n);   // render_media.hip
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

// trace.hip: n rays (two 16-byte records each) -> out (three 16-byte records per ray, or one byte per ray in occlusion mode)
void launch_trace(const KernelRow &row, const RenderParams &P, const void *image, const void *rays, void *out, unsigned int *queue,
                  unsigned int n, int mode, size_t lds_bytes, unsigned grid, hipStream_t stream);

}  // namespace rtmi
