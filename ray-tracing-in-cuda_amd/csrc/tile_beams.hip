// The beam table of a frame (rt_beam.h): one wave per 8x8 tile of the whole frame evaluates the bound of rt_beam.h
// against the slots of the hot sphere table, 64 at a time -- lane l the slot base + l -- and packs the reachable ones in
// ascending order by a vote: the record the host writes slot by slot (beam_tile_record), word for word.  Run when the camera,
// the frame size or the sphere tables change (render_host.hip keeps the table beside the device's image), on the launch stream.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace rtmi {

__global__ void __launch_bounds__(64) tile_beams_kernel(const float *image, BeamFrame f, int tiles_x, uint16_t *table) {
    __shared__ uint16_t rec[kBeamRecordWords];
    const int t = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const Beam b = beam_of_tile(image, f, tx, ty);
    if (lane < kBeamRecordWords) rec[lane] = 0;
    __syncthreads();
    int n = 0;
    for (int base = 0; base < f.nslots; base += 64) {
        const int i = base + lane;
        bool reached = false;
        if (i < f.nslots) {
            const float4 s = reinterpret_cast<const float4 *>(image)[i];
            reached = s.w >= 0.0f && beam_reaches(b, (double)s.x, (double)s.y, (double)s.z, (double)s.w);  // (a never-hit slot: r^2 = -inf)
        }
        const unsigned long long m = __ballot(reached);
        const int at = n + __popcll(m & ((1ull << lane) - 1ull));
        if (reached && at < kBeamCapacity) rec[1 + at] = (uint16_t)i;
        n += __popcll(m);
    }
    __syncthreads();
    if (lane < kBeamRecordWords) {
        const uint16_t w = lane == 0 ? (n > kBeamCapacity ? kBeamOverflow : (uint16_t)n) : (n > kBeamCapacity ? (uint16_t)0 : rec[lane]);
        table[(size_t)t * kBeamRecordWords + lane] = w;
    }
}

__global__ void beam_address_kernel(unsigned int *queue, unsigned long long address) {
    queue[RT_BEAMS_AT] = (unsigned int)address;
    queue[RT_BEAMS_AT + 1] = (unsigned int)(address >> 32);
}

void launch_tile_beams(const float *image, const BeamFrame &f, int tiles_x, int tiles_y, uint16_t *table, hipStream_t stream) {
    // (a frame has at most 8192 x 8192 tiles -- 65 536 columns, render_host.hip -- so the tile count is a grid size)
    hipLaunchKernelGGL(tile_beams_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(64), 0, stream, image, f, tiles_x, table);
}

void launch_beam_address(unsigned int *queue, const uint16_t *table, hipStream_t stream) {
    hipLaunchKernelGGL(beam_address_kernel, dim3(1), dim3(1), 0, stream, queue, (unsigned long long)(uintptr_t)table);
}

}  // namespace rtmi
