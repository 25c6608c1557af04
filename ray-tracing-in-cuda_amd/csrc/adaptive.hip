// Device side of adaptive sampling (rt_render_hip_adaptive, render_host.hip): the noise estimate that decides which tiles
// keep sampling, and the merge of the two accumulator planes into the framebuffer and the per-pixel sample counts.
// The render passes themselves are render_kernel / render_nee_kernel launches over a tile list (device_scene.h, n_list).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_scene.h"

namespace rtmi {

// One wave64 per listed tile, one lane per pixel of the 8x8 tile.  A and B hold the tile's exact sums of nA and nB samples
// (2^-24 fixed point, [row][x][rgb] planes); the metric is include/rtmi.h's, in fp64 without fused operations (the build has
// -ffp-contract=off), so that a host restatement decides bit for bit alike.  A tile converges when every on-image pixel
// does (__ballot); it retires with its count n written to tile_n, or stays active and is appended to next_list (the order of
// the list changes the schedule only, never a pixel's sum).  Reads 48 bytes per pixel: memory-bound.
__global__ __launch_bounds__(256) void adaptive_estimate_kernel(const long long *__restrict__ A, const long long *__restrict__ B,
                                                                const unsigned int *__restrict__ list, int n_list,
                                                                unsigned int *__restrict__ next_list, unsigned int *__restrict__ next_count,
                                                                int *__restrict__ tile_n, int width, int height, int tiles_x, int nA,
                                                                int nB, int n, int retire_all, int use_metric, double t4) {
    const int w = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (w >= n_list) return;  // wave-uniform
    const unsigned int entry = list[w];
    const int x0 = (int)(entry & 0xffffu), band = (int)(entry >> 16);
    const int x = x0 + (lane & 7), y = band * 8 + (lane >> 3);
    bool conv = true;
    if (x < width && y < height) {
        const size_t i = ((size_t)y * width + x) * 3;
        const double s = 1.0 / 16777216.0, dA = (double)nA, dB = (double)nB, dN = (double)n;
        double d = 0.0, m = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long sa = A[i + c], sb = B[i + c];
            const double a = ((double)sa * s) / dA, b = ((double)sb * s) / dB, mc = ((double)(sa + sb) * s) / dN;
            d = c ? d + fabs(a - b) : fabs(a - b);
            m = c ? m + mc : mc;
        }
        const double M = fmax(m, 1e-4);
        conv = use_metric && d * d <= t4 * M;
    }
    const bool retire = retire_all || __ballot(!conv) == 0ull;
    if (lane == 0) {
        if (retire) {
            tile_n[band * tiles_x + (x0 >> 3)] = n;
        } else {
            const unsigned int at = atomicAdd(next_count, 1u);
            next_list[at] = entry;
        }
    }
}

// rgb_sum = fp32 of A + B (exact 64-bit addition, then finalize_kernel's conversion), spp_map = the pixel's tile count
__global__ __launch_bounds__(256) void adaptive_merge_kernel(const long long *__restrict__ A, const long long *__restrict__ B,
                                                             const int *__restrict__ tile_n, float *__restrict__ out,
                                                             int *__restrict__ spp_map, int width, int height, int tiles_x) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)width * height) return;
    const int y = (int)(p / (size_t)width), x = (int)(p - (size_t)y * width);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[p * 3 + c] = (float)((double)(A[p * 3 + c] + B[p * 3 + c]) * (1.0 / 16777216.0));
    spp_map[p] = tile_n[(y >> 3) * tiles_x + (x >> 3)];
}

void launch_adaptive_estimate(const long long *A, const long long *B, const unsigned int *list, int n_list, unsigned int *next_list,
                              unsigned int *next_count, int *tile_n, int width, int height, int tiles_x, int nA, int nB, int n,
                              bool retire_all, bool use_metric, double t4, hipStream_t stream) {
    const unsigned grid = (unsigned)((n_list + 3) / 4);
    hipLaunchKernelGGL(adaptive_estimate_kernel, dim3(grid), dim3(256), 0, stream, A, B, list, n_list, next_list, next_count, tile_n,
                       width, height, tiles_x, nA, nB, n, retire_all ? 1 : 0, use_metric ? 1 : 0, t4);
}

void launch_adaptive_merge(const long long *A, const long long *B, const int *tile_n, float *out, int *spp_map, int width, int height,
                           int tiles_x, hipStream_t stream) {
    const size_t pixels = (size_t)width * height;
    hipLaunchKernelGGL(adaptive_merge_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, stream, A, B, tile_n, out, spp_map,
                       width, height, tiles_x);
}

}  // namespace rtmi
