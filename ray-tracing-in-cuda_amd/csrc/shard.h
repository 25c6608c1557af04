// How the row tiles of a frame are dealt out to shards (rt_opts.tile_rotate: 0 plain interleave, 1 rotated, 2 there and
// back; include/rtmi.h is the contract), stated once for the host, the render kernel and the placement of gathered shards.
// In every deal a shard's tiles increase with its local tile k and the shards partition the tiles: a shard's tiles are its
// local tiles k = 0, 1, ... while shard_tile() < the frame's tile count, and only the last of them can be ragged.
#pragma once
#include <hip/hip_runtime.h>

namespace rtmi {

// global tile of local tile k of shard tile_first of N = tile_stride; I: the type of k * N and of the result
template <typename I>
__host__ __device__ __forceinline__ I shard_tile(int tile_first, int tile_stride, int tile_rotate, int k) {
    I tile = tile_first + (I)k * tile_stride;
    if (tile_rotate == 2) {  // groups of 2 N tiles go to shards 0 .. N-1, then N-1 .. 0
        tile = (I)(k >> 1) * 2 * tile_stride + ((k & 1) ? 2 * tile_stride - 1 - tile_first : tile_first);
    } else if (tile_rotate) {  // tile t belongs to shard (t + t / N) mod N
        int j = (tile_first - k) % tile_stride;
        if (j < 0) j += tile_stride;
        tile = (I)k * tile_stride + j;
    }
    return tile;
}

}  // namespace rtmi
