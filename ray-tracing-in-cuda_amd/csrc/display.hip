// Display stage: exposure (fixed or chosen from the frame), bloom, tone curve and 8-bit quantisation of a finished frame of
// sums (include/rtmi.h, rt_display_hip; definition: DESIGN.md section 7i).
//
// Kernels, one lane per pixel, every record of a plane 16 bytes, loaded and stored by one instruction (the compiler loads the
// three used words of a record and stores all four):
//   reduce    (auto exposure only) sums -> one 64-bit integer: the sum of the luminances' bit patterns (a piecewise-linear log2)
//   prepare   sums -> X = {x_r, x_g, x_b, 0}, the mean scaled by the exposure, and -- with bloom -- B = max(X - threshold, 0)
//   blur      one direction of one a-trous level: five taps `step` pixels apart along x (B -> T) or along y (T -> B, and the
//             running sum S of the levels' smooth planes)
//   finish    X, S -> tone curve -> out_rgb and the quantised bytes, rows flipped
// A workgroup covers 64 x 4 pixels, a wave one row of 64: it reads 1 KiB of consecutive records per tap (768 consecutive bytes
// of the 12-byte framebuffer records).
// Arithmetic: single fp32 + - x / min max sqrt only, in a fixed order, no fused operations (-ffp-contract=off), no exp / log /
// pow: tests/test_gpu_display.py restates it in numpy float32 and compares bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <memory>
#include <mutex>
#include <vector>

#include "hip_host.h"
#include "scene.hpp"

namespace rtmi {

static constexpr int kTileW = 64, kTileH = 4;   // pixels of a workgroup (256 lanes)
static constexpr int kMaxLevels = 8;
static constexpr int kMaxKernels = 3 + 2 * kMaxLevels;  // reduce, prepare, two per level, finish

struct DisplayParams {
    int width, height, spp;
    int tonemap;
    int bloom;      // levels, 0: off
    int identity;   // clamp, exposure 1 given (no auto exposure), no bloom: the byte comes from the sum in the host writer's form
    float E;        // exposure multiplier
    float iw2;      // Reinhard: 1 / white^2
    float threshold, strength, inv_levels;
};

__device__ __forceinline__ float display_count(const int *__restrict__ spp_map, int spp, size_t p) {
    return (float)(spp_map ? max(spp_map[p], 1) : spp);
}

// step 2: I(p) - 0x3F800000 summed over the frame; integer addition, so the order of the lanes, waves and workgroups is free
__global__ __launch_bounds__(256) void display_reduce_kernel(const DisplayParams D, const float *__restrict__ rgb,
                                                             const int *__restrict__ spp_map, unsigned long long *__restrict__ sum) {
    const int x = (int)blockIdx.x * kTileW + (int)(threadIdx.x & 63), y = (int)blockIdx.y * kTileH + (int)(threadIdx.x >> 6);
    long long v = 0;
    if (x < D.width && y < D.height) {
        const size_t p = (size_t)y * D.width + x;
        const float n = display_count(spp_map, D.spp, p);
        const float r = fmaxf(rgb[3 * p + 0] / n, 0.0f), g = fmaxf(rgb[3 * p + 1] / n, 0.0f), b = fmaxf(rgb[3 * p + 2] / n, 0.0f);
        const float Y = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
        const float Yc = fminf(fmaxf(Y, 9.5367431640625e-07f), 1048576.0f);  // 2^-20 .. 2^20
        v = (long long)__float_as_int(Yc) - 0x3F800000LL;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __shared__ long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sum, (unsigned long long)(((part[0] + part[1]) + part[2]) + part[3]));
}

// steps 1, 3 and the bright pass
__global__ __launch_bounds__(256) void display_prepare_kernel(const DisplayParams D, const float *__restrict__ rgb,
                                                              const int *__restrict__ spp_map, float4 *__restrict__ X,
                                                              float4 *__restrict__ B) {
    const int x = (int)blockIdx.x * kTileW + (int)(threadIdx.x & 63), y = (int)blockIdx.y * kTileH + (int)(threadIdx.x >> 6);
    if (x >= D.width || y >= D.height) return;
    const size_t p = (size_t)y * D.width + x;
    const float n = display_count(spp_map, D.spp, p);
    float4 c;
    c.x = fmaxf(rgb[3 * p + 0] / n, 0.0f) * D.E;
    c.y = fmaxf(rgb[3 * p + 1] / n, 0.0f) * D.E;
    c.z = fmaxf(rgb[3 * p + 2] / n, 0.0f) * D.E;
    c.w = 0.0f;
    X[p] = c;
    if (D.bloom) {
        float4 b;
        b.x = fmaxf(c.x - D.threshold, 0.0f), b.y = fmaxf(c.y - D.threshold, 0.0f), b.z = fmaxf(c.z - D.threshold, 0.0f);
        b.w = 0.0f;
        B[p] = b;
    }
}

// One direction of one level: out(q) = sum over d = -2 .. 2 of h_d in(q + step d) along the axis, h = (1/16, 1/4, 3/8, 1/4, 1/16),
// coordinates clamped to the image, accumulated from 0 in tap order.  The vertical pass completes the level: it adds its plane
// to the running sum S (level 0 starts it) and writes it for the next level unless it is the last (out == nullptr).
template <bool VERTICAL>
__global__ __launch_bounds__(256) void display_blur_kernel(const DisplayParams D, int step, const float4 *__restrict__ in,
                                                           float4 *__restrict__ out, float4 *__restrict__ S, int first) {
    const int x = (int)blockIdx.x * kTileW + (int)(threadIdx.x & 63), y = (int)blockIdx.y * kTileH + (int)(threadIdx.x >> 6);
    if (x >= D.width || y >= D.height) return;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
#pragma unroll
    for (int d = -2; d <= 2; ++d) {
        const float h = d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
        // (step <= 128 and the frame <= 65536: no overflow)
        const int xx = VERTICAL ? x : min(max(x + step * d, 0), D.width - 1);
        const int yy = VERTICAL ? min(max(y + step * d, 0), D.height - 1) : y;
        const float4 v = in[(size_t)yy * D.width + xx];
        ar = ar + h * v.x, ag = ag + h * v.y, ab = ab + h * v.z;
    }
    const size_t p = (size_t)y * D.width + x;
    float4 o;
    o.x = ar, o.y = ag, o.z = ab, o.w = 0.0f;
    if (!VERTICAL) {
        out[p] = o;
        return;
    }
    if (out) out[p] = o;
    if (first) {
        S[p] = o;
    } else {
        float4 s = S[p];
        s.x = s.x + o.x, s.y = s.y + o.y, s.z = s.z + o.z;
        S[p] = s;
    }
}

__device__ __forceinline__ float display_tone(const DisplayParams &D, float x) {
    if (D.tonemap == RT_TONEMAP_REINHARD) return (x * (1.0f + x * D.iw2)) / (1.0f + x);
    if (D.tonemap == RT_TONEMAP_ACES) {  // Narkowicz's fit of the ACES filmic curve
        const float num = x * (2.51f * x + 0.03f);
        const float den = x * (2.43f * x + 0.59f) + 0.14f;
        return fminf(fmaxf(num / den, 0.0f), 1.0f);
    }
    return x;
}

// write_color's quantisation (capi.cpp quantize, gamma 2): NaN is written black
__device__ __forceinline__ uint8_t display_byte(float y) {
    float v = sqrtf(y);
    if (!(v == v)) return 0;
    if (v < 0.0f) v = 0.0f;
    if (v > 0.999f) v = 0.999f;
    return (uint8_t)(int)(256.0f * v);
}

// the bloom's sum and scale, the tone curve, both outputs
__global__ __launch_bounds__(256) void display_finish_kernel(const DisplayParams D, const float4 *__restrict__ X,
                                                             const float4 *__restrict__ S, const float *__restrict__ rgb,
                                                             const int *__restrict__ spp_map, float *__restrict__ out_rgb,
                                                             uint8_t *__restrict__ out_rgb8) {
    const int x = (int)blockIdx.x * kTileW + (int)(threadIdx.x & 63), y = (int)blockIdx.y * kTileH + (int)(threadIdx.x >> 6);
    if (x >= D.width || y >= D.height) return;
    const size_t p = (size_t)y * D.width + x;
    float4 c = X[p];
    if (D.bloom) {
        const float4 s = S[p];
        c.x = c.x + D.strength * (D.inv_levels * s.x);
        c.y = c.y + D.strength * (D.inv_levels * s.y);
        c.z = c.z + D.strength * (D.inv_levels * s.z);
    }
    const float yr = display_tone(D, c.x), yg = display_tone(D, c.y), yb = display_tone(D, c.z);
    if (out_rgb) out_rgb[3 * p + 0] = yr, out_rgb[3 * p + 1] = yg, out_rgb[3 * p + 2] = yb;
    if (out_rgb8) {
        const size_t q = ((size_t)(D.height - 1 - y) * D.width + x) * 3;
        if (D.identity) {  // the host writer's own expression: sqrt(sum x (1 / n))
            const float scale = 1.0f / display_count(spp_map, D.spp, p);
            out_rgb8[q + 0] = display_byte(rgb[3 * p + 0] * scale);
            out_rgb8[q + 1] = display_byte(rgb[3 * p + 1] * scale);
            out_rgb8[q + 2] = display_byte(rgb[3 * p + 2] * scale);
        } else {
            out_rgb8[q + 0] = display_byte(yr), out_rgb8[q + 1] = display_byte(yg), out_rgb8[q + 2] = display_byte(yb);
        }
    }
}

namespace {

constexpr float kDefaultWhite = 4.0f;
constexpr int kDefaultLevels = 5;

struct Resolved {
    int tonemap, levels;  // levels: 0 when bloom is off
    float exposure, auto_key, white, strength, threshold;
};

// the arguments both entry points share, checked before any device access
int check_args(int width, int height, const void *rgb, int spp, const void *spp_map, const rt_display *p, const void *out_rgb,
               const void *out_rgb8, Resolved &r) {
    if (!rgb) {
        set_error("rt_display_hip: null rgb_sum");
        return RT_ERR_ARG;
    }
    if (!out_rgb && !out_rgb8) {
        set_error("rt_display_hip: both outputs are null");
        return RT_ERR_ARG;
    }
    if (width <= 0 || height <= 0 || width > 65536 || height > 65536) {
        set_error("rt_display_hip: frame of %d x %d", width, height);
        return RT_ERR_ARG;
    }
    if (!spp_map && spp <= 0) {
        set_error("rt_display_hip: spp %d must be positive (or pass an spp_map)", spp);
        return RT_ERR_ARG;
    }
    r.tonemap = RT_TONEMAP_CLAMP, r.levels = 0;
    r.exposure = 1.0f, r.auto_key = 0.0f, r.white = kDefaultWhite, r.strength = 0.0f, r.threshold = 0.0f;
    if (p) {
        const float f[5] = {p->exposure, p->auto_key, p->white, p->bloom_strength, p->bloom_threshold};
        for (float v : f)
            if (!std::isfinite(v) || v < 0.0f) {
                set_error("rt_display_hip: exposure, auto_key, white, bloom_strength and bloom_threshold must be finite and >= 0");
                return RT_ERR_ARG;
            }
        if (p->tonemap < RT_TONEMAP_CLAMP || p->tonemap > RT_TONEMAP_ACES) {
            set_error("rt_display_hip: tonemap %d outside 0 .. 2", p->tonemap);
            return RT_ERR_ARG;
        }
        if (p->bloom_levels < 0 || p->bloom_levels > kMaxLevels) {
            set_error("rt_display_hip: bloom_levels %d outside 0 .. %d (0: the default, %d)", p->bloom_levels, kMaxLevels, kDefaultLevels);
            return RT_ERR_ARG;
        }
        r.tonemap = p->tonemap;
        if (p->exposure > 0.0f) r.exposure = p->exposure;
        r.auto_key = p->auto_key;
        if (p->white > 0.0f) r.white = p->white;
        r.strength = p->bloom_strength, r.threshold = p->bloom_threshold;
        if (r.strength > 0.0f) r.levels = p->bloom_levels ? p->bloom_levels : kDefaultLevels;
    }
    return RT_OK;
}

// what a device keeps between calls: the four planes (X, B, T, S) and the sum's word, the events, the host entry's staging
struct Scratch {
    int device = -1;
    DeviceBuffer<float4> planes;
    DeviceBuffer<unsigned long long> d_sum;
    long long *h_sum = nullptr;  // pinned
    hipEvent_t ev[kMaxKernels + 2] = {};
    bool have_events = false;
    DeviceBuffer<char> stage;    // rt_display_hip: sums, sample counts, both outputs
};
std::mutex g_mu;
// never destroyed at process exit, as tiles.hip's g_groups: the records own device memory, and the HIP runtime may already be
// gone by then
std::vector<std::unique_ptr<Scratch>> &g_scratch = *new std::vector<std::unique_ptr<Scratch>>();
thread_local double t_kernel_ms[kMaxKernels];
thread_local int t_kernels = 0;

// (g_mu held)
int display_device(int width, int height, const float *d_rgb, int spp, const int *d_spp_map, const Resolved &r, Scratch *sc,
                   float *d_out_rgb, uint8_t *d_out_rgb8, hipStream_t stream, rt_display_stats *st) {
    const size_t pixels = (size_t)width * height;
    const size_t planes = r.levels ? 4 : 1;
    if (int rc = sc->planes.reserve(pixels * planes)) return rc;
    if (r.auto_key > 0.0f) {
        if (int rc = sc->d_sum.reserve(1)) return rc;
        if (!sc->h_sum) HIP_TRY(hipHostMalloc((void **)&sc->h_sum, sizeof(long long), hipHostMallocDefault));
    }
    if (st && !sc->have_events) {
        for (hipEvent_t &e : sc->ev) HIP_TRY(hipEventCreate(&e));
        sc->have_events = true;
    }
    float4 *X = sc->planes.get(), *B = X + pixels, *T = X + 2 * pixels, *S = X + 3 * pixels;
    DisplayParams D;
    D.width = width, D.height = height, D.spp = spp;
    D.tonemap = r.tonemap, D.bloom = r.levels;
    D.iw2 = 1.0f / (r.white * r.white);
    D.threshold = r.threshold, D.strength = r.strength;
    D.inv_levels = r.levels ? 1.0f / (float)r.levels : 0.0f;
    const dim3 grid((unsigned)((width + kTileW - 1) / kTileW), (unsigned)((height + kTileH - 1) / kTileH)), block(256);
    int n_ev = 0;  // events recorded; kernel k ran between events k and k + 1, except across the read-back (gap)
    int gap = -1;
    auto mark = [&]() -> hipError_t { return st ? hipEventRecord(sc->ev[n_ev++], stream) : hipSuccess; };

    unsigned long long *const d_sum = sc->d_sum.get();
    long long log_sum = 0;
    double E = r.exposure;
    if (r.auto_key > 0.0f) {
        HIP_TRY(hipMemsetAsync(d_sum, 0, sizeof(unsigned long long), stream));
        HIP_TRY(mark());
        hipLaunchKernelGGL(display_reduce_kernel, grid, block, 0, stream, D, d_rgb, d_spp_map, d_sum);
        HIP_TRY(hipGetLastError());
        HIP_TRY(mark());
        gap = n_ev;
        HIP_TRY(hipMemcpyAsync(sc->h_sum, d_sum, sizeof(long long), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        log_sum = *sc->h_sum;
        // the mean of the piecewise-linear log2 of the luminance, then key / 2^mean: fp64 on the host, rounded once
        const double m = (double)log_sum / ((double)pixels * 8388608.0);
        E = (double)r.auto_key * (double)r.exposure / std::exp2(m);
    }
    D.E = (float)E;
    // asked for by the parameters, never the outcome of a computed exposure
    D.identity = (r.tonemap == RT_TONEMAP_CLAMP && r.auto_key == 0.0f && r.exposure == 1.0f && !r.levels) ? 1 : 0;

    HIP_TRY(mark());
    hipLaunchKernelGGL(display_prepare_kernel, grid, block, 0, stream, D, d_rgb, d_spp_map, X, B);
    for (int k = 0; k < r.levels; ++k) {
        const bool last = k + 1 == r.levels;
        HIP_TRY(mark());
        hipLaunchKernelGGL(display_blur_kernel<false>, grid, block, 0, stream, D, 1 << k, (const float4 *)B, T, S, 0);
        HIP_TRY(mark());
        hipLaunchKernelGGL(display_blur_kernel<true>, grid, block, 0, stream, D, 1 << k, (const float4 *)T, last ? nullptr : B, S,
                           k == 0 ? 1 : 0);
    }
    HIP_TRY(mark());
    hipLaunchKernelGGL(display_finish_kernel, grid, block, 0, stream, D, (const float4 *)X, (const float4 *)S, d_rgb, d_spp_map,
                       d_out_rgb, d_out_rgb8);
    HIP_TRY(hipGetLastError());
    if (st) {
        HIP_TRY(mark());
        HIP_TRY(hipEventSynchronize(sc->ev[n_ev - 1]));
        t_kernels = 0;
        double total = 0.0;
        for (int k = 0; k + 1 < n_ev; ++k) {
            if (k + 1 == gap) continue;  // (the read-back between the reduction and the rest)
            float t = 0.0f;
            HIP_TRY(hipEventElapsedTime(&t, sc->ev[k], sc->ev[k + 1]));
            t_kernel_ms[t_kernels++] = t;
            total += t;
        }
        st->log_sum = log_sum;
        st->exposure_used = D.E;
        st->ms = total;
    }
    return RT_OK;
}

}  // namespace
}  // namespace rtmi

using namespace rtmi;

extern "C" {

int rt_display_timing(double *ms, int cap) {
    for (int k = 0; ms && k < cap && k < t_kernels; ++k) ms[k] = t_kernel_ms[k];
    return t_kernels;
}

int rt_display_hip_device(int width, int height, const void *d_rgb_sum, int spp, const void *d_spp_map, const rt_display *p,
                          int device, void *d_out_rgb, void *d_out_rgb8, void *stream, rt_display_stats *st) {
    Resolved r;
    int rc = check_args(width, height, d_rgb_sum, spp, d_spp_map, p, d_out_rgb, d_out_rgb8, r);
    if (rc) return rc;
    DeviceScope scope;
    rc = scope.enter(device, "the display stage");
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(g_mu);
    Scratch *sc = device_record(g_scratch, device);
    return display_device(width, height, (const float *)d_rgb_sum, spp, (const int *)d_spp_map, r, sc, (float *)d_out_rgb,
                          (uint8_t *)d_out_rgb8, (hipStream_t)stream, st);
}

int rt_display_hip(int width, int height, const float *rgb_sum, int spp, const int32_t *spp_map, const rt_display *p, int device,
                   float *out_rgb, uint8_t *out_rgb8, rt_display_stats *st) {
    Resolved r;
    int rc = check_args(width, height, rgb_sum, spp, spp_map, p, out_rgb, out_rgb8, r);
    if (rc) return rc;
    DeviceScope scope;
    rc = scope.enter(device, "the display stage");
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(g_mu);
    Scratch *sc = device_record(g_scratch, device);
    const size_t pixels = (size_t)width * height, plane = pixels * 3 * sizeof(float);
    // staging, kept between calls: the sums, the float output, the sample counts, the bytes
    const size_t need = 2 * plane + pixels * sizeof(int32_t) + pixels * 3;
    rc = sc->stage.reserve(need);
    if (rc) return rc;
    char *const stage = sc->stage.get();
    float *d_rgb = (float *)stage, *d_out = (float *)(stage + plane);
    int *d_map = (int *)(stage + 2 * plane);
    uint8_t *d_out8 = (uint8_t *)(stage + 2 * plane + pixels * sizeof(int32_t));
    HIP_TRY(hipMemcpy(d_rgb, rgb_sum, plane, hipMemcpyHostToDevice));
    if (spp_map) HIP_TRY(hipMemcpy(d_map, spp_map, pixels * sizeof(int32_t), hipMemcpyHostToDevice));
    rc = display_device(width, height, d_rgb, spp, spp_map ? d_map : nullptr, r, sc, out_rgb ? d_out : nullptr,
                        out_rgb8 ? d_out8 : nullptr, nullptr, st);
    if (rc) return rc;
    if (out_rgb) HIP_TRY(hipMemcpy(out_rgb, d_out, plane, hipMemcpyDeviceToHost));
    if (out_rgb8) HIP_TRY(hipMemcpy(out_rgb8, d_out8, pixels * 3, hipMemcpyDeviceToHost));
    return RT_OK;
}

}  // extern "C"
