// Test scaffolding (RTMI_ABLATIONS builds only; not in include/rtmi.h, not in the product library): both forms of rt_sqrtf
// (render_device.h) against sqrtf on every one of the 2^32 fp32 bit patterns, on the device -- the fast path of rt_sqrtf rests on v_rsq_f32,
// for which no CPU stands in.  tests/test_gpu_headline_roots.py calls it.
#include "hip_host.h"
#include "render_device.h"

#if RTMI_ABLATIONS
namespace rtmi {

// the values of the odd lane of layout 1, by lane: 0, a denormal, inf, a NaN, -1
__device__ __forceinline__ uint32_t odd_pattern(int which) {
    return which == 0 ? 0u : which == 1 ? 0x00000123u : which == 2 ? 0x7f800000u : which == 3 ? 0x7fc00000u : 0xbf800000u;
}

// out[0]: mismatches, out[1]: the smallest mismatching pattern (2^32: none).  Equal: the same bits, or both NaN.
// layout 0: a wave holds 64 consecutive patterns starting at 64 w + 32 (mod 2^32), so waves straddle every boundary that is a
//           multiple of 64: 2^-96 (0x0f800000), inf (0x7f800000), the sign (0x80000000) and 0 (the wave 0xffffffe0 .. 0x1f).
// layout 1: wave w holds the 63 consecutive patterns from 63 w in its lanes other than w % 5, and odd_pattern(w % 5) in that
//           lane: the whole-wave fallback of rt_sqrtf runs with ordinary lanes in it.  (The last wave's patterns wrap round.)
__global__ __launch_bounds__(256) void sqrt_sweep_kernel(int layout, unsigned long long *__restrict__ out) {
    const unsigned long long n_waves = layout == 0 ? (1ull << 26) : ((1ull << 32) + 62) / 63;
    const unsigned long long wave0 = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) >> 6, stride = ((unsigned long long)gridDim.x * 256) >> 6;
    const int lane = threadIdx.x & 63;
    unsigned long long bad = 0, first = 1ull << 32;
    for (unsigned long long w = wave0; w < n_waves; w += stride) {
        uint32_t bits;
        if (layout == 0) {
            bits = (uint32_t)(w * 64 + 32 + lane);
        } else {
            const int j = (int)(w % 5);
            bits = lane == j ? odd_pattern(j) : (uint32_t)(w * 63 + (lane - (lane > j ? 1 : 0)));
        }
        const float x = __uint_as_float(bits);
        // both forms: the wave-voted guard in front of the v_rsq_f32 sequence (the grid walks' kernels), and the per-lane guard in
        // front of v_sqrt_f32 and its one-step correction (the nested walk, the glossy materials)
        const float voted = rt_sqrtf<true>(x), laned = rt_sqrtf<false>(x), want = sqrtf(x);
        const bool same = (__float_as_uint(voted) == __float_as_uint(want) || (voted != voted && want != want)) &&
                          (__float_as_uint(laned) == __float_as_uint(want) || (laned != laned && want != want));
        if (!same) {
            ++bad;
            if (bits < first) first = bits;
        }
    }
    if (bad != 0) {
        atomicAdd(&out[0], bad);
        atomicMin(&out[1], first);
    }
}

}  // namespace rtmi

// mismatches[0]: how many patterns differ, first[0]: the smallest of them (unset when there is none); layout 0 or 1 as above
extern "C" int rtmi_test_sqrt_sweep(int layout, unsigned long long *mismatches, uint32_t *first) {
    using namespace rtmi;
    if ((layout != 0 && layout != 1) || !mismatches || !first) {
        set_error("rtmi_test_sqrt_sweep: layout 0 or 1, and two result pointers");
        return RT_ERR_ARG;
    }
    DeviceScope scope;
    if (int rc = scope.enter(0, "the square-root sweep")) return rc;
    DeviceBuffer<unsigned long long> out;
    if (int rc = out.reserve(2)) return rc;
    const unsigned long long init[2] = {0ull, 1ull << 32};
    HIP_TRY(hipMemcpy(out.get(), init, sizeof init, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sqrt_sweep_kernel, dim3(8192), dim3(256), 0, nullptr, layout, out.get());
    HIP_TRY(hipGetLastError());
    unsigned long long res[2] = {0, 0};
    HIP_TRY(hipMemcpy(res, out.get(), sizeof res, hipMemcpyDeviceToHost));
    *mismatches = res[0];
    if (res[0] != 0) *first = (uint32_t)res[1];
    return RT_OK;
}
#endif  // RTMI_ABLATIONS
