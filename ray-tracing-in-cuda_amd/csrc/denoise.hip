// Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on the demodulated image, guided by the first-hit feature
// sums of rt_render_hip_feature (include/rtmi.h, rt_denoise_hip; definition: DESIGN.md section 7d).
//
// Three kernels, one lane per pixel, no atomics, every load and store of a record 16 bytes wide:
//   prepare   sums -> two float4 records per pixel: C = {demodulated r, g, b, mean t}, G = {mean normal.xyz, coverage}
//   filter    one pass of 5 x 5 taps `step` pixels apart: C -> C' (ping-pong); G is read-only
//   finish    C -> rgb_sum: re-modulate with the albedo, multiply by the pixel's sample count
// A workgroup covers 16 x 16 pixels, a wave 16 x 4: the 16 lanes of a row read consecutive records (256 contiguous bytes
// per tap row and wave row).
// Arithmetic: single fp32 + - x / min max only, in a fixed order, no fused operations (-ffp-contract=off), no exp / pow:
// tests/test_gpu_denoise.py restates it in numpy float32 and compares bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <memory>
#include <mutex>
#include <vector>

#include "hip_host.h"
#include "scene.hpp"

namespace rtmi {

static constexpr float kAlbedoEps = 1.0f / 1024.0f;  // demodulation floor
static constexpr float kDepthFloor = 1e-6f;          // relative depth differences are taken against max(t, this)
static constexpr float kLumFloor2 = 1.0f / 16.0f;    // colour differences are taken against lum^2 + this

struct DenoiseParams {
    int width, height;
    int spp, feature_spp;
    float inv_sn2, inv_sd2;  // 1 / sigma_normal^2, 1 / sigma_depth^2
};

__device__ __forceinline__ float pixel_count(const int *__restrict__ spp_map, int spp, size_t p) {
    return (float)(spp_map ? max(spp_map[p], 1) : spp);
}

__global__ __launch_bounds__(256) void denoise_prepare_kernel(const DenoiseParams D, const float *__restrict__ rgb,
                                                              const int *__restrict__ spp_map, const float *__restrict__ albedo,
                                                              const float *__restrict__ normal, const float *__restrict__ depth,
                                                              float4 *__restrict__ C, float4 *__restrict__ G) {
    const int x = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15), y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    if (x >= D.width || y >= D.height) return;
    const size_t p = (size_t)y * D.width + x;
    const float n = pixel_count(spp_map, D.spp, p), nf = (float)D.feature_spp;
    float4 c, g;
    c.x = (rgb[3 * p + 0] / n) / fmaxf(albedo[3 * p + 0] / nf, kAlbedoEps);
    c.y = (rgb[3 * p + 1] / n) / fmaxf(albedo[3 * p + 1] / nf, kAlbedoEps);
    c.z = (rgb[3 * p + 2] / n) / fmaxf(albedo[3 * p + 2] / nf, kAlbedoEps);
    c.w = depth[3 * p + 0] / nf;
    g.x = normal[3 * p + 0] / nf, g.y = normal[3 * p + 1] / nf, g.z = normal[3 * p + 2] / nf;
    g.w = depth[3 * p + 1] / nf;
    C[p] = c, G[p] = g;
}

// One pass.  Tap (i, j), i, j in -2 .. 2, row by row (j outer, i inner), lies at (x + i step, y + j step); taps outside the
// image, and taps whose coverage is zero where the centre's is not (or the other way round), are skipped.
//   w = (((h_i h_j) wn) wd) wc,   h = (1/16, 1/4, 3/8, 1/4, 1/16)
//   wn = kn kn, kn = 1 / (1 + |n_q - n_p|^2 inv_sn2)
//   wd = kd kd, kd = 1 / (1 + r r inv_sd2),  r = |t_q - t_p| / max(t_p, 1e-6)
//   wc = kc kc, kc = 1 / (1 + |e_q - e_p|^2 inv_c),  inv_c = inv_sc2 / (l l + 1/16),  l = (e_p.r + e_p.g) + e_p.b
// (sums of three terms are (a + b) + c).  out = (sum w e_q) / (sum w), channel by channel; t is carried along unchanged.
__global__ __launch_bounds__(256) void denoise_filter_kernel(const DenoiseParams D, int step, float inv_sc2,
                                                             const float4 *__restrict__ C, const float4 *__restrict__ G,
                                                             float4 *__restrict__ out) {
    const int x = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15), y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    if (x >= D.width || y >= D.height) return;
    const size_t p = (size_t)y * D.width + x;
    const float4 cp = C[p], gp = G[p];
    const float lum = (cp.x + cp.y) + cp.z;
    const float inv_c = inv_sc2 / (lum * lum + kLumFloor2);
    const float t_ref = fmaxf(cp.w, kDepthFloor);
    const bool hit_p = gp.w != 0.0f;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
        const int yy = y + j * step;
        if (yy < 0 || yy >= D.height) continue;
        const float hj = j == 0 ? 0.375f : ((j == 1 || j == -1) ? 0.25f : 0.0625f);
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int xx = x + i * step;
            if (xx < 0 || xx >= D.width) continue;
            const float hi = i == 0 ? 0.375f : ((i == 1 || i == -1) ? 0.25f : 0.0625f);
            const size_t q = (size_t)yy * D.width + xx;
            const float4 cq = C[q], gq = G[q];
            if ((gq.w != 0.0f) != hit_p) continue;
            const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
            const float kn = 1.0f / (1.0f + ((nx * nx + ny * ny) + nz * nz) * D.inv_sn2);
            const float r = fabsf(cq.w - cp.w) / t_ref;
            const float kd = 1.0f / (1.0f + (r * r) * D.inv_sd2);
            const float ex = cq.x - cp.x, ey = cq.y - cp.y, ez = cq.z - cp.z;
            const float kc = 1.0f / (1.0f + ((ex * ex + ey * ey) + ez * ez) * inv_c);
            const float w = (((hi * hj) * (kn * kn)) * (kd * kd)) * (kc * kc);
            sw = sw + w;
            sr = sr + w * cq.x, sg = sg + w * cq.y, sb = sb + w * cq.z;
        }
    }
    float4 o;
    o.x = sr / sw, o.y = sg / sw, o.z = sb / sw, o.w = cp.w;
    out[p] = o;
}

__global__ __launch_bounds__(256) void denoise_finish_kernel(const DenoiseParams D, const float4 *__restrict__ C,
                                                             const int *__restrict__ spp_map, const float *__restrict__ albedo,
                                                             float *__restrict__ out) {
    const int x = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15), y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    if (x >= D.width || y >= D.height) return;
    const size_t p = (size_t)y * D.width + x;
    const float n = pixel_count(spp_map, D.spp, p), nf = (float)D.feature_spp;
    const float4 c = C[p];
    out[3 * p + 0] = (c.x * fmaxf(albedo[3 * p + 0] / nf, kAlbedoEps)) * n;
    out[3 * p + 1] = (c.y * fmaxf(albedo[3 * p + 1] / nf, kAlbedoEps)) * n;
    out[3 * p + 2] = (c.z * fmaxf(albedo[3 * p + 2] / nf, kAlbedoEps)) * n;
}

namespace {

constexpr int kDefaultIterations = 3, kMaxIterations = 10;  // defaults: the sweep of DESIGN.md section 7d
constexpr float kDefaultSigmaColor = 0.5f, kDefaultSigmaNormal = 0.125f, kDefaultSigmaDepth = 0.05f;

struct Resolved {
    int iterations;
    float sigma_color, sigma_normal, sigma_depth;
};

// the arguments both entry points share, checked before any device access
int check_args(int width, int height, const void *rgb, int spp, const void *spp_map, const void *albedo, const void *normal,
               const void *depth, int feature_spp, const rt_denoise *p, const void *out, Resolved &r) {
    if (!rgb || !albedo || !normal || !depth || !out) {
        set_error("rt_denoise_hip: null buffer");
        return RT_ERR_ARG;
    }
    if (width <= 0 || height <= 0 || width > 65536 || height > 65536) {
        set_error("rt_denoise_hip: frame of %d x %d", width, height);
        return RT_ERR_ARG;
    }
    if (!spp_map && spp <= 0) {
        set_error("rt_denoise_hip: spp %d must be positive (or pass an spp_map)", spp);
        return RT_ERR_ARG;
    }
    if (feature_spp <= 0) {
        set_error("rt_denoise_hip: feature_spp %d must be positive", feature_spp);
        return RT_ERR_ARG;
    }
    r.iterations = kDefaultIterations;
    r.sigma_color = kDefaultSigmaColor, r.sigma_normal = kDefaultSigmaNormal, r.sigma_depth = kDefaultSigmaDepth;
    if (p) {
        const float sg[3] = {p->sigma_color, p->sigma_normal, p->sigma_depth};
        for (float v : sg)
            if (!std::isfinite(v) || v < 0.0f) {
                set_error("rt_denoise_hip: sigmas must be finite and >= 0 (0: the default)");
                return RT_ERR_ARG;
            }
        if (p->iterations < RT_DENOISE_DEFAULT_ITERATIONS || p->iterations > kMaxIterations) {
            set_error("rt_denoise_hip: iterations %d outside 0 .. %d (%d: the default)", p->iterations, kMaxIterations,
                      RT_DENOISE_DEFAULT_ITERATIONS);
            return RT_ERR_ARG;
        }
        if (p->iterations != RT_DENOISE_DEFAULT_ITERATIONS) r.iterations = p->iterations;
        if (p->sigma_color > 0.0f) r.sigma_color = p->sigma_color;
        if (p->sigma_normal > 0.0f) r.sigma_normal = p->sigma_normal;
        if (p->sigma_depth > 0.0f) r.sigma_depth = p->sigma_depth;
    }
    return RT_OK;
}

// scratch records of a device (C, C', G), kept between calls
struct Scratch {
    int device = -1;
    DeviceBuffer<float4> buf;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};
std::mutex g_mu;
// never destroyed at process exit, as tiles.hip's g_groups: the records own device memory, and the HIP runtime may already be
// gone by then
std::vector<std::unique_ptr<Scratch>> &g_scratch = *new std::vector<std::unique_ptr<Scratch>>();

int denoise_device(int width, int height, const float *d_rgb, int spp, const int *d_spp_map, const float *d_albedo,
                   const float *d_normal, const float *d_depth, int feature_spp, const Resolved &r, int device, float *d_out,
                   hipStream_t stream, double *ms) {
    const size_t pixels = (size_t)width * height;
    if (r.iterations == 0) {  // no pass: the frame as it came
        HIP_TRY(hipMemcpyAsync(d_out, d_rgb, pixels * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream));
        if (ms) {
            HIP_TRY(hipStreamSynchronize(stream));
            *ms = 0.0;
        }
        return RT_OK;
    }
    std::lock_guard<std::mutex> lock(g_mu);
    Scratch *sc = device_record(g_scratch, device);
    if (int rc = sc->buf.reserve(pixels * 3)) return rc;
    if (ms && !sc->ev0) {
        HIP_TRY(hipEventCreate(&sc->ev0));
        HIP_TRY(hipEventCreate(&sc->ev1));
    }
    float4 *C0 = sc->buf.get(), *C1 = C0 + pixels, *G = C0 + 2 * pixels;
    DenoiseParams D;
    D.width = width, D.height = height, D.spp = spp, D.feature_spp = feature_spp;
    D.inv_sn2 = 1.0f / (r.sigma_normal * r.sigma_normal);
    D.inv_sd2 = 1.0f / (r.sigma_depth * r.sigma_depth);
    const dim3 grid((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16)), block(256);
    if (ms) HIP_TRY(hipEventRecord(sc->ev0, stream));
    hipLaunchKernelGGL(denoise_prepare_kernel, grid, block, 0, stream, D, d_rgb, d_spp_map, d_albedo, d_normal, d_depth, C0, G);
    // the colour term narrows from pass to pass (Dammertz et al.: sigma_rt halves), so inv_sc2 is multiplied by 4
    float inv_sc2 = 1.0f / (r.sigma_color * r.sigma_color);
    for (int i = 0; i < r.iterations; ++i) {
        hipLaunchKernelGGL(denoise_filter_kernel, grid, block, 0, stream, D, 1 << i, inv_sc2, C0, G, C1);
        std::swap(C0, C1);
        inv_sc2 = inv_sc2 * 4.0f;
    }
    hipLaunchKernelGGL(denoise_finish_kernel, grid, block, 0, stream, D, C0, d_spp_map, d_albedo, d_out);
    HIP_TRY(hipGetLastError());
    if (ms) {
        HIP_TRY(hipEventRecord(sc->ev1, stream));
        HIP_TRY(hipEventSynchronize(sc->ev1));
        float t = 0.0f;
        HIP_TRY(hipEventElapsedTime(&t, sc->ev0, sc->ev1));
        *ms = t;
    }
    return RT_OK;
}

}  // namespace
}  // namespace rtmi

using namespace rtmi;

extern "C" {

int rt_denoise_hip_device(int width, int height, const void *d_rgb_sum, int spp, const void *d_spp_map, const void *d_albedo_sum,
                          const void *d_normal_sum, const void *d_depth_sum, int feature_spp, const rt_denoise *p, int device,
                          void *d_out_rgb_sum, void *stream, double *ms) {
    Resolved r;
    int rc = check_args(width, height, d_rgb_sum, spp, d_spp_map, d_albedo_sum, d_normal_sum, d_depth_sum, feature_spp, p,
                        d_out_rgb_sum, r);
    if (rc) return rc;
    DeviceScope scope;
    rc = scope.enter(device, "the denoiser");
    if (rc) return rc;
    return denoise_device(width, height, (const float *)d_rgb_sum, spp, (const int *)d_spp_map, (const float *)d_albedo_sum,
                          (const float *)d_normal_sum, (const float *)d_depth_sum, feature_spp, r, device, (float *)d_out_rgb_sum,
                          (hipStream_t)stream, ms);
}

int rt_denoise_hip(int width, int height, const float *rgb_sum, int spp, const int32_t *spp_map, const float *albedo_sum,
                   const float *normal_sum, const float *depth_sum, int feature_spp, const rt_denoise *p, int device,
                   float *out_rgb_sum, double *ms) {
    Resolved r;
    int rc = check_args(width, height, rgb_sum, spp, spp_map, albedo_sum, normal_sum, depth_sum, feature_spp, p, out_rgb_sum, r);
    if (rc) return rc;
    DeviceScope scope;
    rc = scope.enter(device, "the denoiser");
    if (rc) return rc;
    const size_t pixels = (size_t)width * height, plane = pixels * 3 * sizeof(float);
    // one allocation: the four input planes, the output plane, the sample counts
    DeviceBuffer<char> staging;
    rc = staging.reserve(5 * plane + pixels * sizeof(int32_t));
    if (rc) return rc;
    char *const d = staging.get();
    float *d_rgb = (float *)d, *d_alb = (float *)(d + plane), *d_nrm = (float *)(d + 2 * plane), *d_dep = (float *)(d + 3 * plane);
    float *d_out = (float *)(d + 4 * plane);
    int *d_map = spp_map ? (int *)(d + 5 * plane) : nullptr;
    HIP_TRY(hipMemcpy(d_rgb, rgb_sum, plane, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_alb, albedo_sum, plane, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_nrm, normal_sum, plane, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_dep, depth_sum, plane, hipMemcpyHostToDevice));
    if (spp_map) HIP_TRY(hipMemcpy(d_map, spp_map, pixels * sizeof(int32_t), hipMemcpyHostToDevice));
    rc = denoise_device(width, height, d_rgb, spp, d_map, d_alb, d_nrm, d_dep, feature_spp, r, device, d_out, nullptr, ms);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_rgb_sum, d_out, plane, hipMemcpyDeviceToHost));
    return RT_OK;
}

}  // extern "C"
