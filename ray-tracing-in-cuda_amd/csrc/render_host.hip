// Host side of the render path: keeps the scene image (device_scene.h, packed by
// pack.hip) resident per device, computes the shard geometry and launches
// render_kernel.  Replaces jsonmain()'s device set-up, gpu-version/main.cu:
// 462-513 (move_to_device<<<1,1>>>, cudaMallocManaged framebuffer, curand state
// allocation + init_random_library<<<W*H,1>>>, render<<<>>>, cudaDeviceSynchronize):
// one hipMemcpy of a few KB replaces the object-graph rebuild, and there is no RNG
// state to allocate or initialise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "device_scene.h"
#include "hip_host.h"
#include "kernels.h"
#include "pack.h"
#include "scene.hpp"
#include "shard.h"

namespace rtmi {

void launch_adaptive_estimate(const long long *A, const long long *B, const unsigned int *list, int n_list, unsigned int *next_list,
                              unsigned int *next_count, int *tile_n, int width, int height, int tiles_x, int nA, int nB, int n,
                              bool retire_all, bool use_metric, double t4, hipStream_t stream);
void launch_adaptive_merge(const long long *A, const long long *B, const int *tile_n, float *out, int *spp_map, int width, int height,
                           int tiles_x, hipStream_t stream);
// the row of a render variant (rt_opts.variant, never 0) -- render_kernel, or render_nested_kernel for 52; null: no such build.
// Its cull is the variant's candidate search.  ext: the build with triangles and image textures; count: the counting build
static const KernelRow *variant_row(unsigned variant, bool ext = false, bool count = false, bool alpha = false, bool camera = false) {
    const KernelRow *row = find_kernel({K_PLAIN, variant, ext, count, false, false, alpha, camera});
    return row ? row : find_kernel({K_NESTED, variant, ext, count, false, false, alpha, camera});
}

static bool variant_exists(unsigned variant) { return variant == 0 || variant_row(variant); }

// Everything a beam table depends on (rt_beam.h): the camera records as packed, the frame size and the defocus flag (`frame`),
// and the identity of the sphere tables -- the scene version that was packed and the device image it was uploaded to.  The
// growth of the bound is a function of these (the camera's distance and the sphere's), so it needs no word of its own.
struct BeamKey {
    bool valid = false;
    uint64_t version = 0;
    const void *image = nullptr;
    BeamFrame frame{};
    float camera[16] = {};
    bool same(const BeamKey &o) const {
        return valid && o.valid && version == o.version && image == o.image && !memcmp(&frame, &o.frame, sizeof frame) &&
               !memcmp(camera, o.camera, sizeof camera);
    }
};

struct DeviceEntry {
    int device = -1;
    uint64_t version = 0;
    DeviceBuffer<float> d_image;
    DeviceBuffer<unsigned long long> d_acc;  // fixed-point pixel accumulators of the last launch
    DeviceBuffer<DevCounters> d_counters;
    DeviceBuffer<float> d_out;  // framebuffer of the host-buffer entry points (rt_render_hip), kept between calls
    DeviceBuffer<char> d_adapt;  // adaptive sampling: accumulator plane B, next tile list, tile counts, list counter
    DeviceBuffer<int> d_spp;     // spp_map of rt_render_hip_adaptive (host-buffer entry point)
    DeviceBuffer<unsigned int> d_trace_queue;  // ray queries: the work counter of a launch (64 words)
    DeviceBuffer<char> d_trace_io;             // rays and records of rt_trace_hip (host-buffer entry point), kept between calls
    // the beam table of variants 2 and 6 (rt_beam.h): one record per 8x8 tile of the whole frame, and what it was built from
    DeviceBuffer<uint16_t> d_beams;
    BeamKey beams_key;
    int num_cus = 0;
};

struct DeviceSceneCache {
    std::mutex mu;  // guards the packed image and the entry list -- not the launches of an entry
    std::vector<std::unique_ptr<DeviceEntry>> entries;  // stable addresses: one entry per device
    // host-side packed image (rebuilt when the scene version changes)
    uint64_t packed_version = 0;
    std::vector<float> image;  // float4 records
    RenderParams layout;       // ns/nr/nc/nm + offsets filled by pack
    NestedInfo nested;         // the nested cells of that packing (all zero: flat tables)
};

// the scene's packed tables and device entries (created by the first call that needs them)
static DeviceSceneCache &cache_of(const Scene &s) {
    Scene &ms = const_cast<Scene &>(s);
    if (!ms.dev) ms.dev = std::make_shared<DeviceSceneCache>();
    return *ms.dev;
}

// packs the scene's tables unless the cache holds them for its version; under cache.mu.  The image, the layout and the
// version are installed together: a failed pack leaves the cache as it was.
static int ensure_packed(const Scene &s, DeviceSceneCache &cache) {
    if (cache.packed_version == s.version) return RT_OK;
    std::vector<float> image;
    RenderParams layout;
    NestedInfo nested;
    int rc = pack_scene(s, image, layout, &nested);
    if (rc) return rc;
    cache.image = std::move(image);
    cache.layout = layout;
    cache.nested = nested;
    cache.packed_version = s.version;
    return RT_OK;
}

// ---- the beam table (rt_beam.h) -------------------------------------------------------
// what the lists of scene s's frame are computed from, with the packed layout L
static BeamFrame beam_frame_of(const Scene &s, const RenderParams &L) {
    BeamFrame f;
    memset(&f, 0, sizeof f);  // (the key compares bytes)
    f.off_cam = L.off_cam, f.nslots = L.np + (RT_CLUSTER + 1) * L.ncl;
    f.width = s.width, f.height = s.height;
    f.inv_wm1 = 1.0f / (float)(s.width - 1), f.inv_hm1 = 1.0f / (float)(s.height - 1);  // (as the launch parameters)
    f.defocus = (s.flags & RT_FLAG_DEFOCUS_BLUR) ? 1u : 0u;
    return f;
}

// do a scene's bursts read lists at all?  Compact sphere tables (what variants 2 and 6 walk), the perspective camera, and a
// frame whose jitter scale is finite
static bool beams_apply(const Scene &s, const RenderParams &L) {
    return !L.grid_wide && s.cam.projection == RT_PROJ_PERSPECTIVE && s.width > 1 && s.height > 1 &&
           L.np + (RT_CLUSTER + 1) * L.ncl <= 65535;
}

// the device's table for the packed scene, built on `stream` unless the entry holds it for this key; under cache.mu
static int ensure_beams(const Scene &s, const DeviceSceneCache &cache, DeviceEntry *ent, hipStream_t stream) {
    BeamKey key;
    key.valid = true, key.version = ent->version, key.image = ent->d_image.get();
    key.frame = beam_frame_of(s, cache.layout);
    memcpy(key.camera, cache.image.data() + 4 * (size_t)cache.layout.off_cam, sizeof key.camera);
    const int tiles_x = (s.width + 7) / 8, tiles_y = (s.height + 7) / 8;
    if (ent->beams_key.same(key) && ent->d_beams.get()) return RT_OK;
    ent->beams_key.valid = false;
    int rc = ent->d_beams.reserve((size_t)tiles_x * tiles_y * kBeamRecordWords);
    if (rc) return rc;
    launch_tile_beams(ent->d_image.get(), key.frame, tiles_x, tiles_y, ent->d_beams.get(), stream);
    HIP_TRY(hipGetLastError());
    ent->beams_key = key;
    return RT_OK;
}

// ---- shard geometry ----------------------------------------------------------------
struct Shard {
    int tile_rows, tile_first, tile_stride, tile_rotate, num_tiles, local_tiles, local_rows;
};

static int shard_of(const Scene &s, const rt_opts *o, Shard &sh) {
    sh.tile_rows = (o && o->tile_rows > 0) ? o->tile_rows : 8;
    sh.tile_first = o ? o->tile_first : 0;
    sh.tile_stride = (o && o->tile_stride > 1) ? o->tile_stride : 1;
    sh.tile_rotate = (o && sh.tile_stride > 1) ? o->tile_rotate : 0;
    if (sh.tile_rotate < 0 || sh.tile_rotate > 2) {
        set_error("tile_rotate %d: 0 (plain interleave), 1 (rotated) or 2 (there and back)", sh.tile_rotate);
        return RT_ERR_ARG;
    }
    sh.num_tiles = (s.height + sh.tile_rows - 1) / sh.tile_rows;
    if (sh.tile_first < 0 || (sh.tile_stride > 1 && sh.tile_first >= sh.tile_stride)) {
        set_error("tile_first %d out of range for tile_stride %d", sh.tile_first, sh.tile_stride);
        return RT_ERR_ARG;
    }
    sh.local_tiles = 0;
    sh.local_rows = 0;
    // (shard.h: the shard's tiles are its local tiles 0 .. local_tiles - 1)
    for (int k = 0;; ++k) {
        const long long t64 = shard_tile<long long>(sh.tile_first, sh.tile_stride, sh.tile_rotate, k);
        if (t64 >= sh.num_tiles) break;
        const int t = (int)t64;
        int rows = s.height - t * sh.tile_rows;
        if (rows > sh.tile_rows) rows = sh.tile_rows;
        sh.local_rows += rows;
        sh.local_tiles++;
    }
    return RT_OK;
}

static int shard_global_row(const Shard &sh, int local_row) {
    const int tl = local_row / sh.tile_rows;
    const int t = (int)shard_tile<long long>(sh.tile_first, sh.tile_stride, sh.tile_rotate, tl);
    return t * sh.tile_rows + (local_row - tl * sh.tile_rows);
}

}  // namespace rtmi

using namespace rtmi;

extern "C" {

int rt_shard_rows(const rt_scene *s, const rt_opts *o) {
    if (!s) return -RT_ERR_ARG;
    Shard sh;
    int rc = shard_of(s->s, o, sh);
    return rc ? -rc : sh.local_rows;
}

int rt_shard_deal(const rt_scene *s, const rt_opts *o, int n_ranks) {
    if (!s || n_ranks < 1) return -RT_ERR_ARG;
    if (n_ranks == 1) return 0;
    const int tile_rows = (o && o->tile_rows > 0) ? o->tile_rows : 8;
    const long long tiles = (s->s.height + tile_rows - 1) / tile_rows;
    // The rotated interleave evens the ranks out once its phase has gone round a few times (a revolution is n_ranks groups of
    // n_ranks tiles); a frame too short for that is dealt there and back, which cancels the cost's trend inside every 2 n_ranks
    // tiles.  Measured on per-tile query counts of RTIOW 1080p, 135 tiles (tools/gpu_tilecost.py, tile_deal.py), busiest rank
    // above the mean: 4 ranks 0.36 % rotated / 0.86 % there and back, 8 ranks 2.17 % / 0.92 % (plain interleave: 1.16 %, 1.84 %).
    return tiles >= 4LL * n_ranks * n_ranks ? 1 : 2;
}

int rt_shard_global_row(const rt_scene *s, const rt_opts *o, int local_row) {
    if (!s) return -RT_ERR_ARG;
    Shard sh;
    int rc = shard_of(s->s, o, sh);
    if (rc) return -rc;
    if (local_row < 0 || local_row >= sh.local_rows) return -RT_ERR_ARG;
    return shard_global_row(sh, local_row);
}

int rt_shard_scatter_rows(const rt_scene *s, const rt_opts *o, const float *local_rgb, float *full_rgb) {
    if (!s || !local_rgb || !full_rgb) {
        set_error("rt_shard_scatter_rows: null argument");
        return RT_ERR_ARG;
    }
    Shard sh;
    int rc = shard_of(s->s, o, sh);
    if (rc) return rc;
    const size_t row_floats = (size_t)s->s.width * 3;
    for (int lr = 0; lr < sh.local_rows; ++lr)
        memcpy(full_rgb + (size_t)shard_global_row(sh, lr) * row_floats, local_rgb + (size_t)lr * row_floats,
               row_floats * sizeof(float));
    return RT_OK;
}

int rt_has_ablations(void) { return has_ablations() ? 1 : 0; }

int rt_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        set_error("hipGetDeviceCount failed: %s", hipGetErrorString(e));
        return -RT_ERR_HIP;
    }
    return n;
}

// what rt_opts.variant = 0 stands for in a scene with these tables
static unsigned pick_variant(const RenderParams &P, bool counting, size_t lds_table_bytes) {
    if (!P.grid_wide) return P.grid_sheet ? 2u : 6u;
    if (P.grid_wide == 2) return 52u;  // nested cells: the walk over global memory (such scenes are large)
    const size_t grid_bytes = (size_t)P.hot_vec4_grid * 16, scan_bytes = (size_t)(P.hot_vec4 - (P.off_box - P.off_grid)) * 16;
    // a handful of primitives of several types, none of them listed in a grid: the plain scan is the same search without
    // the per-query set-up (sample_scene.json: 54 against 79 ms)
    if (P.grid_cells == 0 && P.ncl == 0 && !counting && scan_bytes <= lds_table_bytes) return 16u;
    return grid_bytes <= lds_table_bytes ? 36u : 44u;
}

// the scene's tables (packed if needed) under one lock: fills *out, copies at most cap_floats floats of the image to dst
static int read_tables(const rt_scene *sc, rt_table_info *out, float *dst, int cap_floats) {
    if (!sc || !out) {
        set_error("rt_scene_table_info: null argument");
        return RT_ERR_ARG;
    }
    int rc = scene_validate(sc->s);
    if (rc) return rc;
    DeviceSceneCache &cache = cache_of(sc->s);
    std::lock_guard<std::mutex> lock(cache.mu);
    rc = ensure_packed(sc->s, cache);
    if (rc) return rc;
    if (cache.image.size() > (size_t)INT32_MAX) {
        set_error("scene image of %zu floats exceeds the int32 count of rt_table_info", cache.image.size());
        return RT_ERR_LIMIT;
    }
    const RenderParams &L = cache.layout;
    memset(out, 0, sizeof *out);
    out->image_floats = (int32_t)cache.image.size();
    out->grid_wide = L.grid_wide, out->grid_sheet = L.grid_sheet, out->grid_cells = L.grid_cells;
    const float *g = cache.image.data() + (size_t)L.off_grid * 4;
    for (int a = 0; a < 3; ++a) {
        out->grid_min[a] = g[a], out->grid_size[a] = g[8 + a];
        memcpy(&out->grid_n[a], g + 12 + a, 4);
    }
    out->ob_near2 = g[3], out->ob_far2 = g[7];
    out->ns = L.ns, out->np = L.np, out->ncl = L.ncl;
    out->nr = L.nr, out->nc = L.nc, out->nt = L.nt, out->nr_a = L.nr_a, out->nc_a = L.nc_a, out->nt_a = L.nt_a;
    out->off_grid_cells = L.off_grid_cells, out->off_grid_items = L.off_grid_items;
    out->off_sph_cold = L.off_sph_cold, out->off_rect_cold = L.off_rect_cold, out->off_cyl_cold = L.off_cyl_cold, out->off_tri_cold = L.off_tri_cold;
    out->off_rect_hot = L.off_rect_hot, out->off_cyl_hot = L.off_cyl_hot, out->off_tri_hot = L.off_tri_hot;
    out->hot_bytes_grid = L.hot_vec4_grid * 16;
    out->kernel_variant = (int32_t)pick_variant(L, false, (size_t)knob("RTMI_GLOBAL_TABLE_BYTES", (double)kLdsTableBytes));
    if (L.nl > 0) out->kernel_variant |= 256;  // light sampling: the layout's light-sampling kernel
    if (L.env_rows > 0) out->kernel_variant |= 1024;  // an environment map: the layout's environment kernel
    if (!sc->s.media.empty()) out->kernel_variant |= 2048;  // media: the layout's media kernel
    if (!sc->s.movers.empty()) out->kernel_variant |= 4096;  // moving spheres: the layout's motion kernel
    if (dst && cap_floats > 0) memcpy(dst, cache.image.data(), sizeof(float) * std::min((size_t)cap_floats, cache.image.size()));
    return RT_OK;
}

int rt_scene_table_info(const rt_scene *sc, rt_table_info *out) { return read_tables(sc, out, nullptr, 0); }

// a traced burst (render_burst.h) carries the id of a staged sphere in kBurstIdBits bits of a lane's home-row register: the
// packer's bound for LDS-resident tables, and the CU's LDS that bounds any raised one (RTMI_GLOBAL_TABLE_BYTES), fit them
static_assert(kLdsTableBytes <= kCuLdsBytes && kLdsTableBytes / 16 <= (size_t(1) << kBurstIdBits), "a staged record's index fits the burst's id bits");

int rt_variant_workgroup(unsigned variant, int32_t out[5]) {
    const KernelRow *row = out && variant != 0 ? variant_row(variant) : nullptr;
    if (!row) {
        set_error("rt_variant_workgroup: %s", out ? "no such render variant in this library" : "null argument");
        return RT_ERR_ARG;
    }
    out[0] = (int32_t)group_threads(*row), out[1] = row->wave_lds, out[2] = (int32_t)kLdsTableBytes;
    out[3] = (int32_t)group_lds(*row, kLdsTableBytes);
    out[4] = row->groups_per_cu > 0 ? row->groups_per_cu : 4 * RT_WAVES_PER_SIMD / row->waves;
    return RT_OK;
}

int rt_scene_nested_info(const rt_scene *sc, rt_nested_info *out) {
    if (!sc || !out) {
        set_error("rt_scene_nested_info: null argument");
        return RT_ERR_ARG;
    }
    int rc = scene_validate(sc->s);
    if (rc) return rc;
    DeviceSceneCache &cache = cache_of(sc->s);
    std::lock_guard<std::mutex> lock(cache.mu);
    rc = ensure_packed(sc->s, cache);
    if (rc) return rc;
    const NestedInfo &n = cache.nested;
    memset(out, 0, sizeof *out);
    out->cells = n.cells, out->sub_cells = n.sub_cells, out->sub_items = n.sub_items;
    out->off_sub_grids = n.off_sub_grids, out->off_sub_cells = n.off_sub_cells, out->first_sub_cell = n.first_sub_cell;
    out->threshold = n.threshold, out->axis_cap = n.axis_cap, out->longest = n.longest;
    return RT_OK;
}

int rt_scene_quad_counts(const rt_scene *sc, int32_t *nq, int32_t *nq_a) {
    if (!sc || !nq || !nq_a) {
        set_error("rt_scene_quad_counts: null argument");
        return RT_ERR_ARG;
    }
    int rc = scene_validate(sc->s);
    if (rc) return rc;
    DeviceSceneCache &cache = cache_of(sc->s);
    std::lock_guard<std::mutex> lock(cache.mu);
    rc = ensure_packed(sc->s, cache);
    if (rc) return rc;
    *nq = cache.layout.nq, *nq_a = cache.layout.nq_a;
    return RT_OK;
}

int rt_scene_tile_beams(const rt_scene *sc, uint16_t *out, int cap_tiles) {
    if (!sc) {
        set_error("rt_scene_tile_beams: null scene");
        return -RT_ERR_ARG;
    }
    int rc = scene_validate(sc->s);
    if (rc) return -rc;
    const Scene &s = sc->s;
    DeviceSceneCache &cache = cache_of(s);
    std::lock_guard<std::mutex> lock(cache.mu);
    rc = ensure_packed(s, cache);
    if (rc) return -rc;
    if (!beams_apply(s, cache.layout)) {
        set_error("rt_scene_tile_beams: the bursts of this scene read no lists (compact sphere tables, the perspective camera and a frame of at least 2 x 2 pixels have them)");
        return -RT_ERR_LIMIT;
    }
    const int tiles_x = (s.width + 7) / 8, tiles_y = (s.height + 7) / 8;
    const BeamFrame f = beam_frame_of(s, cache.layout);
    for (int t = 0; out && t < tiles_x * tiles_y && t < cap_tiles; ++t)
        beam_tile_record(cache.image.data(), f, t % tiles_x, t / tiles_x, out + (size_t)t * kBeamRecordWords);
    return tiles_x * tiles_y;
}

int rt_scene_tile_beams_device(const rt_scene *sc, const rt_opts *o, uint16_t *out, int cap_tiles) {
    if (!sc) {
        set_error("rt_scene_tile_beams_device: null scene");
        return -RT_ERR_ARG;
    }
    int rc = scene_validate(sc->s);
    if (rc) return -rc;
    const Scene &s = sc->s;
    const int device = o ? o->device : 0;
    DeviceScope scope;
    rc = scope.enter(device, "the beam table");
    if (rc) return -rc;
    DeviceSceneCache &cache = cache_of(s);
    std::lock_guard<std::mutex> lock(cache.mu);
    rc = ensure_packed(s, cache);
    if (rc) return -rc;
    if (!beams_apply(s, cache.layout)) {
        set_error("rt_scene_tile_beams_device: the bursts of this scene read no lists (compact sphere tables, the perspective camera and a frame of at least 2 x 2 pixels have them)");
        return -RT_ERR_LIMIT;
    }
    DeviceEntry *ent = device_record(cache.entries, device);
    if (ent->version != s.version || !ent->d_image.get()) {
        rc = ent->d_image.reserve(cache.image.size());
        if (rc) return -rc;
        if (hipMemcpy(ent->d_image.get(), cache.image.data(), cache.image.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            set_error("rt_scene_tile_beams_device: the upload of the scene image failed");
            return -RT_ERR_HIP;
        }
        ent->version = s.version;
    }
    rc = ensure_beams(s, cache, ent, nullptr);
    if (rc) return -rc;
    const int tiles = ((s.width + 7) / 8) * ((s.height + 7) / 8);
    const int n = std::min(tiles, cap_tiles);
    if (hipStreamSynchronize(nullptr) != hipSuccess ||
        (out && n > 0 && hipMemcpy(out, ent->d_beams.get(), (size_t)n * kBeamRecordWords * sizeof(uint16_t), hipMemcpyDeviceToHost) != hipSuccess)) {
        set_error("rt_scene_tile_beams_device: reading the table back failed");
        return -RT_ERR_HIP;
    }
    return tiles;
}

int rt_scene_tile_beams_capacity(void) { return kBeamCapacity; }

int rt_scene_table_image(const rt_scene *sc, float *dst, int cap_floats) {
    rt_table_info info;
    int rc = read_tables(sc, &info, dst, cap_floats);
    return rc ? -rc : info.image_floats;
}

// How a launch cuts samples [first, first + sample_count) of `tiles` tiles into work items (ItemParams); spp_chunk_opt: rt_opts.spp_chunk
struct ChunkPlan {
    int spp_chunk, num_chunks, n_big, n_med, q_med, q_small, orphan_max;
};

static ChunkPlan plan_chunks(long long tiles, int sample_count, int spp_chunk_opt) {
    // samples per work item: scheduling only (the pixel sum is exact).  64 and 128 measure the same on MI355X for
    // frames that fill the chip (199.8 / 200.2 ms; 256: 204.3) and 128 halves the accumulator traffic -- one 1.5 KB
    // tile flush and a handful of orphaned paths per item; small frames get smaller chunks so that there are a few items per
    // resident wave (a 400x225 frame has 1450 tiles for ~6000 resident waves)
    int spp_chunk = spp_chunk_opt > 0 ? spp_chunk_opt : 0;
    if (spp_chunk == 0) {
        // 8 items per resident wave, down to 4 samples each: the cost of a tile varies by two orders of magnitude (sky against a
        // triangle mesh), and a wave's share evens out only over several items (20 000 triangles at 1280 x 720 x 16: 31.2 ms
        // with 4 items of 8 samples per wave, 24.6 with 8 of 4; 20 000 spheres 10.1 either way)
        const long long want_items = 8LL * 256 * RT_WAVES_PER_SIMD * 4;
        // (256 for launches that have the items: with the graded tail below the whole 1080p x 1024 spp frame takes the same 119.3 -
        //  119.7 ms with 128- or 256-sample items (512: 120.0); the tail's medium and small items keep the item count -- 16 per tile
        //  against 14 -- and with it the accumulator flushes where they were: 1.28 GB of HBM writes per frame, PMC)
        spp_chunk = 256;
        while (spp_chunk > 4 && tiles * ((sample_count + spp_chunk - 1) / spp_chunk) < want_items) spp_chunk /= 2;
    }
    if (spp_chunk > sample_count) spp_chunk = sample_count;
    // Guided self-scheduling of the chunk-major queue: big chunks first, then chunks a quarter as long, then
    // a sixteenth.  A launch ends when the last wave finishes its last item; a 64-sample item takes ~3 ms of
    // wall time (seven waves share a SIMD) and an item over glass and dense spheres several times the average,
    // so the runs of shorter items have to last long enough for the other waves to have something to do
    // meanwhile.  How many big chunks are given up follows from r = resident waves / tiles: a whole 1080p
    // frame (r = 0.22) gives up one of four 256-sample chunks, a 1/8 row shard (r = 1.8) twelve of sixteen 64-sample ones; of
    // the medium chunks that many again are cut into small ones.  Short items cost little since stragglers no longer
    // block a wave's next item (chunk sizes 16..128 measure within 1.5 % on the whole frame).
    // (knob(): measurement knobs of the default build, constants in a product build)
    static const int tail_mode = (int)knob("RTMI_TAIL_MODE", 1);  // 0 = one run of equal chunks
    // (round 2: 4 / 6 / 8 / 12 -> a 1/4 shard 66.0 / 63.8 / 63.2 / 61.8 ms.  Round 3, four times as many items, RTIOW 1080p x 1024 spp
    //  (tools/gpu_tail_sweep.py): 5 / 6 / 7 / 8 / 12 -> rank 0's 1/8 shard 16.70 / 16.32 / 16.34 / 16.41 / 16.53 ms, a 1/4 shard 31.62 /
    //  31.21 / 31.42 / 31.49 / 31.63, the whole frame within 0.2 %; at 4 and below the last big items outlast the short ones: 17.7 ms)
    //  Round 3's last session (tools/gpu_tail_sweep.py; whole frame / a 1/2 / a 1/4 / rank 0's and rank 3's 1/8 shard, ms): with a run of
    //  small items for the big launches too (below) 120.35 / 61.60 / 31.06 / 16.13 / 15.49 -> 119.52 / 60.45 / 31.05 / 16.15 / 15.51.
    //  The number of big chunks given up rounded DOWN as well (one for a whole 1080p frame instead of two; 3 / 6 / 12 for the shards): 119.72 /
    //  60.98 / 31.09 / 16.15 / 15.54 -> 119.42 / 60.72 / 30.97 / 16.15 / 15.48, the DNA frame 6.61 -> 6.52, 20 000 triangles 26.8 -> 25.5 ms;
    //  the cliff (factor 5 rounded down: four chunks for a 1/4 shard, 32.06 ms) is two chunks away.)
    static const double tail_factor = knob("RTMI_TAIL_FACTOR", 7.0);
    static const int tail_div = std::max(2, (int)knob("RTMI_TAIL_DIV", 4));  // big : medium item length
    static const int orphan_env = (int)knob("RTMI_ORPHAN_MAX", -1);
    int n_big = sample_count / spp_chunk, n_med = 0, q_med = spp_chunk, q_small = spp_chunk;
    int num_chunks, orphan_max = 12;
    {
        const double r = 256.0 * 4 * RT_WAVES_PER_SIMD / (double)std::max(1LL, tiles);
        const int rem = sample_count - n_big * spp_chunk;
        int rest = rem;  // samples after the big chunks
        if (tail_mode > 0 && spp_chunk >= 16 && n_big >= 1) {
            static const int tail_floor = (int)knob("RTMI_TAIL_FLOOR", 1);  // (0: round up, as until the end of round 3)
            const int n_split = std::min(n_big, std::max(1, tail_floor ? (int)std::floor(tail_factor * r) : (int)std::ceil(tail_factor * r)));  // big chunks given up
            n_big -= n_split;
            rest += n_split * spp_chunk;
            q_med = std::max(4, spp_chunk / tail_div);
            q_small = std::max(4, q_med / 4);
            int small_samples = 0;
            // a run of small items behind the medium ones: for launches of few tiles per wave, and (round 3's end) for every launch whose
            // small items are still 16 samples long (the whole 1080p x 1024 spp frame 120.35 -> 119.5 ms, a 1/2 shard 61.6 -> 60.5; with
            // 4-sample items at r = 0.5 the DNA frame goes from 6.6 to 7.7 ms: 400 000 items for 6 ms of work)
            static const double small_r = knob("RTMI_SMALL_R", 0.5);
            if ((r >= small_r || q_small >= 16) && q_small < q_med)
                small_samples = std::min(rest - q_med, std::max(1, (int)std::ceil(tail_factor * r)) * q_med);
            if (small_samples < 0) small_samples = 0;
            n_med = (rest - small_samples) / q_med;  // whole medium chunks; the small run takes what is left
        } else {
            q_med = q_small = spp_chunk;  // one run of equal chunks (the remainder is the last, shorter one)
        }
        const int after_med = rest - n_med * q_med;
        num_chunks = n_big + n_med + (after_med + q_small - 1) / q_small;
        // orphans: waiting for an item's last paths costs short items more (render_kernel.hip, step 4)
        orphan_max = orphan_env >= 0 ? std::min(63, orphan_env) : (r >= 0.5 ? 63 : 12);
    }
    return ChunkPlan{spp_chunk, num_chunks, n_big, n_med, q_med, q_small, orphan_max};
}

// adaptive sampling (rt_render_hip_adaptive_device): the schedule that replaces render_impl's single launch
struct AdaptiveRun {
    const rt_adaptive *a;
    int max_spp;          // resolved (0 -> the scene's spp)
    int *d_spp_map;
    rt_adaptive_stats *st;
};

// What the render launches of one call share.  enqueue(): one launch, samples [first, first + n) of every tile of the shard
// (n_list = 0), or of the n_list tiles listed at queue[RT_TILE_LIST_AT] (the kernel's item decode then reads tiles_x as n_list
// and bands as 1)
struct Launcher {
    const RenderParams &P;
    const Shard &sh;
    DeviceEntry *ent;
    DevCounters *d_cnt;
    hipStream_t stream;
    size_t lds_bytes;
    unsigned long long resident;  // workgroups that fill the chip
    const KernelRow &kernel;      // the instance every launch of the call runs (kernels.h)
    int feature;                  // >= 0: a feature pass
    const uint16_t *beams;        // the beam table the launches' bursts read (variants 2 and 6), or null

    int enqueue(unsigned long long *acc, unsigned int *d_queue, int first, int n, int n_list, const ChunkPlan &pl) const {
        RenderParams Q = P;
        Q.sample_first = first, Q.sample_count = n;
        Q.spp_chunk = pl.spp_chunk, Q.num_chunks = pl.num_chunks;
        Q.n_big = pl.n_big, Q.n_med = pl.n_med, Q.q_med = pl.q_med, Q.q_small = pl.q_small;
        Q.orphan_max = pl.orphan_max;
        const unsigned long long items = (unsigned long long)(n_list ? n_list : (long long)P.tiles_x * P.bands) * pl.num_chunks;
        if (items > 0x7fffffffull) {
            set_error("%llu work items exceed the queue counter", items);
            return RT_ERR_LIMIT;
        }
        Q.num_items = (int)items;
        {  // what a wave reads when it fetches or flushes an item (kept out of the kernel's SGPRs)
            ItemParams ip;
            ip.tiles_x = n_list ? n_list : Q.tiles_x, ip.bands = n_list ? 1 : Q.bands, ip.num_items = Q.num_items;
            ip.sample_first = Q.sample_first, ip.sample_count = Q.sample_count, ip.spp_chunk = Q.spp_chunk;
            ip.n_big = Q.n_big, ip.n_med = Q.n_med, ip.q_med = Q.q_med, ip.q_small = Q.q_small;
            ip.tile_rows = Q.tile_rows, ip.tile_first = Q.tile_first, ip.tile_stride = Q.tile_stride;
            ip.tile_rotate = sh.tile_rotate;
            ip.local_rows = Q.local_rows;
            ip.n_list = n_list;
            launch_item_params(d_queue, ip, stream);
            if (beams) launch_beam_address(d_queue, beams, stream);
        }
        // persistent launch: enough workgroups to fill the chip, never more than the work needs
        const unsigned long long need_blocks = (items + kernel.waves - 1) / kernel.waves;
        const unsigned long long grid = need_blocks < resident ? (need_blocks ? need_blocks : 1) : resident;
        if (feature >= 0) Q.feature = feature;
        launch_kernel(kernel, Q, ent->d_image.get(), acc, d_queue, d_cnt, lds_bytes, (unsigned)grid, stream);
        return RT_OK;
    }
};

// ---- adaptive sampling (replaces the single launch).  Pass k renders samples [n_{k-1}, n_k) of the active tiles, the first
// half into plane A (ent->d_acc), the rest into plane B; the estimate kernel then retires the tiles that meet the noise target
// (or max_spp) and lists the others for the next pass.  The host reads the list's length back once per pass, to size the next
// launches: a stream synchronisation, i.e. the launch gap of a pass (~tens of us, <= 23 passes).
static int run_adaptive(const Launcher &launch, const AdaptiveRun &ad, const Scene &s, size_t queue_off, size_t need, float *d_out,
                        int spp_chunk_opt, int &launches) {
    const RenderParams &P = launch.P;
    DeviceEntry *ent = launch.ent;
    const hipStream_t stream = launch.stream;
    const long long frame_tiles = (long long)P.tiles_x * P.bands;
    int rc = ent->d_acc.reserve(need / sizeof(unsigned long long));  // (need: a multiple of 256 bytes)
    if (rc) return rc;
    unsigned long long *const d_acc = ent->d_acc.get();
    const size_t b_off = 0, list_off = queue_off, tn_off = list_off + (size_t)frame_tiles * 4;
    const size_t cnt_off = tn_off + (size_t)frame_tiles * 4;
    rc = ent->d_adapt.reserve(cnt_off + 256);
    if (rc) return rc;
    char *const d_adapt = ent->d_adapt.get();
    HIP_TRY(hipMemsetAsync(d_acc, 0, need, stream));
    HIP_TRY(hipMemsetAsync(d_adapt, 0, cnt_off + 256, stream));
    long long *dA = reinterpret_cast<long long *>(d_acc);
    long long *dB = reinterpret_cast<long long *>(d_adapt + b_off);
    unsigned int *d_queue = reinterpret_cast<unsigned int *>(reinterpret_cast<char *>(d_acc) + queue_off);
    unsigned int *d_list = d_queue + RT_TILE_LIST_AT;
    unsigned int *d_next = reinterpret_cast<unsigned int *>(d_adapt + list_off);
    int *d_tn = reinterpret_cast<int *>(d_adapt + tn_off);
    unsigned int *d_next_count = reinterpret_cast<unsigned int *>(d_adapt + cnt_off);
    std::vector<unsigned int> all((size_t)frame_tiles);  // every tile: band << 16 | x0
    for (long long t = 0; t < frame_tiles; ++t) all[(size_t)t] = (unsigned)((t / P.tiles_x) << 16 | (t % P.tiles_x) * 8);
    HIP_TRY(hipMemcpyAsync(d_list, all.data(), all.size() * 4, hipMemcpyHostToDevice, stream));
    const double T = (double)ad.a->threshold;
    const double t4 = (4.0 * T) * T;
    rt_adaptive_stats &st = *ad.st;
    int n_active = (int)frame_tiles, prev = 0, nA = 0, nB = 0;
    for (int k = 0; n_active > 0; ++k) {
        const int n = k == 0 ? ad.a->min_spp : (int)std::min(2LL * prev, (long long)ad.max_spp);
        const int delta = n - prev, half = delta / 2;
        for (int h = 0; h < 2 && s.max_depth > 0; ++h) {  // (max_depth <= 0: every sample is black, main.cpp:20,42)
            const int first = h ? prev + half : prev, len = h ? delta - half : half;
            if (len == 0) continue;
            HIP_TRY(hipMemsetAsync(d_queue, 0, 4, stream));
            rc = launch.enqueue(h ? reinterpret_cast<unsigned long long *>(dB) : reinterpret_cast<unsigned long long *>(dA), d_queue,
                                first, len, n_active, plan_chunks(n_active, len, spp_chunk_opt));
            if (rc) return rc;
            ++launches;
        }
        nA += half, nB += delta - half;
        HIP_TRY(hipMemsetAsync(d_next_count, 0, 4, stream));
        launch_adaptive_estimate(dA, dB, d_list, n_active, d_next, d_next_count, d_tn, s.width, s.height, P.tiles_x, nA, nB, n,
                                 n == ad.max_spp, T > 0.0, t4, stream);
        ++launches;
        unsigned int next = 0;
        HIP_TRY(hipMemcpyAsync(&next, d_next_count, 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        st.spp_after[k] = n, st.active[k] = n_active, st.passes = k + 1;
        n_active = (int)next;
        if (n_active > 0) HIP_TRY(hipMemcpyAsync(d_list, d_next, (size_t)n_active * 4, hipMemcpyDeviceToDevice, stream));
        prev = n;
    }
    launch_adaptive_merge(dA, dB, d_tn, d_out, ad.d_spp_map, s.width, s.height, P.tiles_x, stream);
    ++launches;
    std::vector<int> tn((size_t)frame_tiles);
    HIP_TRY(hipMemcpyAsync(tn.data(), d_tn, tn.size() * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    st.tiles = (int32_t)frame_tiles;
    st.samples = 0;
    for (long long t = 0; t < frame_tiles; ++t) {
        const int x0 = (int)(t % P.tiles_x) * 8, y0 = (int)(t / P.tiles_x) * 8;
        st.samples += (uint64_t)tn[(size_t)t] * (uint64_t)(std::min(8, s.width - x0) * std::min(8, s.height - y0));
    }
    return RT_OK;
}

// the counting kernels' counters -> stats (rt_render_hip_count)
static int read_counters(const DevCounters *d_cnt, const RenderParams &P, int cull_mode, size_t n_prims, rt_stats *stats) {
    DevCounters h;
    HIP_TRY(hipMemcpy(&h, d_cnt, sizeof h, hipMemcpyDeviceToHost));
    stats->samples = h.samples;
    stats->queries = h.queries;
    stats->prim_tests = h.queries * (unsigned long long)n_prims;
    stats->hits = h.hits;
    stats->misses = h.misses;
    for (int i = 0; i < 4; ++i) stats->scatter[i] = h.scatter[i];
    stats->rng_draws = h.rng_draws;
    stats->cand_lanes = h.cand_lanes;
    stats->cand_waves = h.cand_waves;
    stats->clusters_visited = h.clusters_visited;
    stats->groups_visited = h.groups_visited;
    stats->lane_clusters = h.lane_clusters;
    stats->lane_groups = h.lane_groups;
    stats->lane_cands = h.lane_cands;
    stats->group_maxpop = h.group_maxpop;
    stats->query_maxpop = h.query_maxpop;
    stats->walk_resumed = (int32_t)std::min<unsigned long long>(h.walk_resumed, (unsigned long long)INT32_MAX);
    for (int i = 0; i < 6; ++i) stats->cycles[i] = h.cycles[i];
    stats->wave_start_spread_us = (double)(h.t_start_max - h.t_start_min) * 0.01;
    stats->wave_end_spread_us = (double)(h.t_end_max - h.t_end_min) * 0.01;
    stats->wave_span_us = (double)(h.t_end_max - h.t_start_min) * 0.01;
    if (knob_set("RTMI_DEBUG_DRAIN")) {
        fprintf(stderr, "shader clock over the waves' lifetimes: %.0f MHz\n", h.life_ticks ? 100.0 * (double)h.life_cycles / (double)h.life_ticks : 0.0);
        fprintf(stderr, "queue-empty seen over %.1f us; first exit %.1f us after the first queue-empty; drain histogram (50 us bins):",
                (double)(h.t_qe_max - h.t_qe_min) * 0.01, (double)(h.t_end_min - h.t_qe_min) * 0.01);
        for (int i = 0; i < 32; ++i) fprintf(stderr, " %u", h.drain_hist[i]);
        for (int e = 0; e < 2; ++e) {
            fprintf(stderr, "\nwave-queries by live lanes (bins of 4 lanes, last = all 64), %s:", e ? "after the wave found the queue empty" : "while the queue had items");
            for (int i = 0; i < 17; ++i) fprintf(stderr, " %llu", h.occ_hist[e][i]);
        }
        fprintf(stderr, "\nwaves by time from start to queue-empty (64 us bins, first nonzero bin on):");
        int first = 0;
        while (first < 1023 && !h.qe_hist[first]) ++first;
        fprintf(stderr, " [bin %d]", first);
        for (int i = first; i < 1024 && i < first + 60; ++i) fprintf(stderr, " %u", h.qe_hist[i]);
        fprintf(stderr, "\nwaves by time from start to exit (same bins):");
        for (int i = first; i < 1024 && i < first + 60; ++i) fprintf(stderr, " %u", h.exit_hist[i]);
        fprintf(stderr, "\n");
    }
    stats->wave_queries = h.wave_queries;
    stats->cull_prefix = P.np, stats->cull_clusters = P.ncl, stats->cull_groups = P.ngr;
    stats->cull_cluster_size = P.cluster;
    stats->cull_mode = cull_mode, stats->cull_windows = P.nwin;  // (of the kernel that ran)
    stats->grid_sheet = P.grid_sheet;
    return RT_OK;
}

// timing events: three per (host thread, device), created at the thread's first timed call there and kept
static int timing_events(int device, std::array<hipEvent_t, 3> *&out) {
    struct Events {
        std::vector<std::array<hipEvent_t, 3>> per_device;
        ~Events() {
            for (auto &t : per_device)
                for (hipEvent_t ev : t)
                    if (ev) (void)hipEventDestroy(ev);
        }
    };
    static thread_local Events events;
    if ((int)events.per_device.size() <= device) events.per_device.resize((size_t)device + 1, {nullptr, nullptr, nullptr});
    auto &t = events.per_device[(size_t)device];
    for (hipEvent_t &ev : t)
        if (!ev) HIP_TRY(hipEventCreate(&ev));
    out = &t;
    return RT_OK;
}

static int render_impl(const rt_scene *sc, const rt_opts *o, void *d_rgb_sum, void *stream_v, rt_stats *stats,
                       long long *h_acc, bool count, const AdaptiveRun *ad = nullptr, int feature = -1) {
    if (!sc || (!d_rgb_sum && !h_acc)) {
        set_error("rt_render_hip_device: null scene or output pointer");
        return RT_ERR_ARG;
    }
    const Scene &s = sc->s;
    int rc = scene_validate(s);
    if (rc) return rc;
    Shard sh;
    rc = shard_of(s, o, sh);
    if (rc) return rc;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->local_rows = sh.local_rows;
    }
    if (sh.local_rows == 0) return RT_OK;

    int sample_first = o ? o->sample_first : 0;
    int sample_count = (o && o->sample_count > 0) ? o->sample_count : s.spp;
    const ChunkPlan plan = plan_chunks((long long)((s.width + 7) / 8) * ((sh.local_rows + 7) / 8), sample_count,
                                       o ? o->spp_chunk : 0);
    if (sample_first < 0) {
        set_error("sample_first must be >= 0");
        return RT_ERR_ARG;
    }
    // a sample contributes at most 2^16 (radiance_to_fixed clamps) in units of 2^-24: 2^23 samples keep the 64-bit
    // pixel sums exact (the reference's float sum saturates gracefully instead; a silent wrap here would not)
    if ((long long)sample_first + sample_count > RT_MAX_SAMPLES_PER_PIXEL) {
        set_error("samples [%d, %lld) exceed %d samples per pixel, the range over which the fixed-point pixel sums are exact",
                  sample_first, (long long)sample_first + sample_count, RT_MAX_SAMPLES_PER_PIXEL);
        return RT_ERR_LIMIT;
    }

    unsigned variant = o ? o->variant : 0;
    if (feature >= 0) {
        // a feature pass names a LAYOUT: the scene's own (0, or 2 / 6 for compact tables), or one a feature kernel is built for
        const unsigned ok[] = {0u, 2u, 6u, 16u, 24u, 36u, 44u, 52u};
        if (std::find(std::begin(ok), std::end(ok), variant) == std::end(ok)) {
            set_error("rt_render_hip_feature: layout %u (0, 16, 24, 36, 44 or 52; 2 and 6 run the linear scan)", variant);
            return RT_ERR_ARG;
        }
    } else if (!variant_exists(variant)) {
        set_error("unknown kernel variant %u%s", variant, has_ablations() ? "" : " (this library was built without the measurement variants: make ABLATIONS=1)");
        return RT_ERR_ARG;
    }
    // homogeneous media: kernels of their own; a feature pass ignores them (the first SURFACE hit)
    const bool media = !s.media.empty() && feature < 0;
    if (media && count) {
        set_error("rt_render_hip_count: this scene has participating media, which the counting kernels do not carry");
        return RT_ERR_ARG;
    }
    // moving spheres: kernels of their own
    const bool motion = !s.movers.empty();
    if (motion && count) {
        set_error("rt_render_hip_count: this scene has moving spheres, which the counting kernels do not carry");
        return RT_ERR_ARG;
    }
    if (motion && feature >= 0) {
        set_error("a feature pass of a scene with moving spheres: the guides would show the scene at no particular time (clear the moving spheres for the pass)");
        return RT_ERR_ARG;
    }
    if (motion && media) {
        set_error("this scene has moving spheres and participating media, which no kernel combines: remove one of them");
        return RT_ERR_ARG;
    }
    if (count && !has_ablations()) {
        set_error("rt_render_hip_count: this library was built without the counting kernels (make ABLATIONS=1)");
        return RT_ERR_LIMIT;
    }
    // triangles and image textures live in separate builds of the kernels (template argument EXT)
    bool ext = !s.images.empty();
    for (const rt_prim &p : s.prims) ext = ext || p.type == RT_PRIM_TRIANGLE || p.type == RT_PRIM_QUAD;  // (quads: DESIGN 7q)
    ext = ext || scene_has_glossy(s);  // (the glossy materials' code sits in those builds alone)
    ext = ext || scene_has_noise(s);   // (and the noise textures')
    ext = ext || scene_has_bump(s);    // (and the bumps')
    ext = ext || scene_has_normal_map(s);  // (and the normal maps', DESIGN 7u -- an image texture, so it is set already)
    const bool alpha = scene_has_alpha(s);  // (alpha masks, DESIGN 7v: an image texture's plane, so ext is set already)
    ext = ext || alpha;
    // a projection other than the perspective one: the instances of camera_kernel.h, which are general builds
    const int projection = s.cam.projection;
    const bool camera = projection != RT_PROJ_PERSPECTIVE;
    ext = ext || camera;
    const bool force_ext = knob_set("RTMI_FORCE_EXT");  // measurement: the EXT builds on scenes that do not need them
    const int device = o ? o->device : 0;
    DeviceScope scope;
    rc = scope.enter(device, "the render path");
    if (rc) return rc;

    hipStream_t stream = (hipStream_t)stream_v;

    // ---- resident scene image
    DeviceSceneCache &cache = cache_of(s);
    // The lock covers packing, the entry list and the enqueueing of this call's work; it is released before the
    // call waits for the device (stats), so that threads which render one scene on DIFFERENT devices overlap.
    std::unique_lock<std::mutex> lock(cache.mu);
    rc = ensure_packed(s, cache);
    if (rc) return rc;
    DeviceEntry *ent = device_record(cache.entries, device);
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    if (stats) {
        std::array<hipEvent_t, 3> *t = nullptr;
        rc = timing_events(device, t);
        if (rc) return rc;
        ev0 = (*t)[0], ev1 = (*t)[1], ev2 = (*t)[2];
        HIP_TRY(hipEventRecord(ev0, stream));
    }
    size_t image_bytes = cache.image.size() * sizeof(float);
    if (ent->version != s.version || !ent->d_image.get()) {
        rc = ent->d_image.reserve(cache.image.size());
        if (rc) return rc;
        // stream-ordered: the launches below follow on the same stream (renders of one scene object on one device share
        // a stream: include/rtmi.h).  The source is pageable, so the call returns once the bytes are staged.
        HIP_TRY(hipMemcpyAsync(ent->d_image.get(), cache.image.data(), image_bytes, hipMemcpyHostToDevice, stream));
        ent->version = s.version;
    }

    // ---- kernel parameters
    RenderParams P = cache.layout;
    for (int i = 0; i < 3; ++i) P.background[i] = s.background[i];
    P.flags = s.flags | (scene_has_normal_map(s) ? RT_PFLAG_NORMAL_MAPS : 0u);
    if (camera) P.flags |= (uint32_t)projection << RT_PFLAG_PROJ_SHIFT;  // (the model number, DESIGN 7w: read by the camera instances alone)
    P.rr_p = feature >= 0 ? 0.0f : s.rr_p;  // (a feature sample ends at its first query: no roulette, any max_depth)
    P.width = s.width, P.height = s.height, P.max_depth = feature >= 0 ? 1 : s.max_depth;
    P.inv_wm1 = 1.0f / (float)(s.width - 1), P.inv_hm1 = 1.0f / (float)(s.height - 1);  // IEEE fp32 divisions, as the checker's
    P.tile_rows = sh.tile_rows, P.tile_first = sh.tile_first, P.tile_stride = sh.tile_stride;
    P.num_tiles = sh.num_tiles, P.local_rows = sh.local_rows;
    P.sample_first = sample_first, P.sample_count = sample_count;
    P.spp_chunk = plan.spp_chunk, P.num_chunks = plan.num_chunks;
    P.n_big = plan.n_big, P.n_med = plan.n_med, P.q_med = plan.q_med, P.q_small = plan.q_small;
    P.orphan_max = plan.orphan_max;
    uint64_t seed = o ? o->seed : 0;
    P.seed_lo = (uint32_t)seed, P.seed_hi = (uint32_t)(seed >> 32);
    P.tiles_x = (s.width + 7) / 8;
    P.bands = (sh.local_rows + 7) / 8;

    // ---- which kernel.  LDS per workgroup: the hot tables (unless the variant reads them from global memory: bit 3, and variant 52) + one
    // tile accumulator per wave.  The tables live in LDS while that leaves room for the kernel's full occupancy
    // (RT_WAVES_PER_SIMD workgroups per CU); larger scenes run the same walk over global memory (4000 spheres 6.7 vs 19 ms),
    // which has no size limit.  The packer has chosen the table format (device_scene.h): COMPACT for sphere-only scenes whose
    // tables fit that LDS budget, WIDE for every other scene.
    // (variants 2 and 6: workgroups of 14 waves, each with a slab of prepared rays behind its accumulator -- kernels.h)
    auto hot_bytes_of = [&](int mode) {  // (each candidate search stages the part of the hot tables it reads)
        if (mode == 5 || mode == 6 || mode == 7 || mode == 8) return (size_t)P.hot_vec4_grid * 16;
        return (size_t)((mode == 3 ? P.hot_vec4_tables : P.hot_vec4) - (P.off_box - P.off_grid)) * 16;  // (without the grid tables)
    };
    static const size_t global_threshold = (size_t)knob("RTMI_GLOBAL_TABLE_BYTES", (double)kLdsTableBytes);
    const bool sphere_only = P.nr + P.nc + P.nt == 0 && !ext;
    auto pick = [&](bool counting) -> unsigned { return pick_variant(P, counting, global_threshold); };
    if (variant == 0) variant = pick(count);
    // light sampling on and something to sample: the layout's light-sampling kernel (built with triangles and textures)
    const bool nee = P.nl > 0 && feature < 0;
    if (feature >= 0 && (variant == 2 || variant == 6)) {
        // compact tables list spheres for the sphere-only kernels; a feature pass is one query per sample and scans the list
        // instead -- staged in LDS while that fits the table budget, from global memory beyond (no size limit)
        if (P.grid_wide) {
            set_error("layout %u reads the compact grid tables, which this scene does not have: use 0", variant);
            return RT_ERR_LIMIT;
        }
        variant = (size_t)(P.hot_vec4 - (P.off_box - P.off_grid)) * 16 <= global_threshold ? 16u : 24u;
    }
    // an environment map: kernels of their own, for the general layouts
    const bool env = P.env_rows > 0;
    // alpha masks: what no kernel renders
    if (alpha) {
        if (count) {
            set_error("rt_render_hip_count: this scene has a material with an alpha mask, which the counting kernels do not carry");
            return RT_ERR_ARG;
        }
        if (variant == 2 || variant == 6) {
            set_error("kernel variant %u is a compact sphere-only layout, which knows no alpha mask: use variant 0, 16, 36 or 44", variant);
            return RT_ERR_ARG;
        }
        if (media) {
            set_error("this scene has participating media and a material with an alpha mask, which no kernel combines (the media "
                      "kernels draw one free-flight distance per query): remove the media or the masks");
            return RT_ERR_ARG;
        }
        for (const rt_moving_sphere &m : s.movers)
            if (scene_alpha(s, m.material)) {
                set_error("this scene has a moving sphere whose material carries an alpha mask, which no kernel renders (the holes "
                          "would swim through the ball): remove the mask or give the mover another material");
                return RT_ERR_ARG;
            }
    }
    // camera projections: what no kernel renders
    if (camera) {
        if (count) {
            set_error("rt_render_hip_count: this scene's camera is not the perspective one, which the counting kernels do not carry: "
                      "count with rt_scene_set_projection(RT_PROJ_PERSPECTIVE)");
            return RT_ERR_ARG;
        }
        if (variant == 2 || variant == 6) {
            set_error("kernel variant %u is a compact sphere-only layout, whose path start is the perspective camera's: use variant 0, 16, 36 or 44", variant);
            return RT_ERR_ARG;
        }
        if (alpha) {
            set_error("this scene has a material with an alpha mask and a camera projection other than the perspective one, which no "
                      "kernel combines: remove the masks or render with the perspective projection");
            return RT_ERR_ARG;
        }
    }
    // light sampling in media (rt_scene_set_media_light_sampling): acts only with media and something to sample
    const bool media_nee = media && nee && s.media_light_sampling;
    if (media) {
        if (nee && !media_nee) {
            set_error("this scene has participating media and light sampling with emitters to sample, which no kernel combines: switch one of them off "
                      "(or switch light sampling in media on: rt_scene_set_media_light_sampling, \"media_light_sampling\": true, --nee-media)");
            return RT_ERR_ARG;
        }
        if (media_nee && camera) {
            set_error("this scene has light sampling in participating media and a camera projection other than the perspective one, which no "
                      "kernel combines: render with the perspective projection or switch rt_scene_set_media_light_sampling off");
            return RT_ERR_ARG;
        }
        if (env) {
            set_error("this scene has participating media and an environment map, which no kernel combines: remove one of them");
            return RT_ERR_ARG;
        }
        if (P.grid_wide == 2) {
            set_error("this scene has participating media and the nested grid, which no kernel combines: switch the nested grid off");
            return RT_ERR_ARG;
        }
        if (!find_kernel({K_MEDIA, variant, true, false, media_nee})) {
            set_error("kernel variant %u does not carry participating media (the media kernels are variants 0, 16, 36 and 44)", variant);
            return RT_ERR_ARG;
        }
    }
    if (motion) {
        if (nee) {
            set_error("this scene has moving spheres and light sampling with emitters to sample, which no kernel combines: switch light sampling off");
            return RT_ERR_ARG;
        }
        if (env) {
            set_error("this scene has moving spheres and an environment map, which no kernel combines: remove one of them");
            return RT_ERR_ARG;
        }
        if (P.grid_wide == 2) {
            set_error("this scene has moving spheres and the nested grid, which no kernel combines: switch the nested grid off");
            return RT_ERR_ARG;
        }
        for (const rt_moving_sphere &m : s.movers)
            if (scene_bump(s, m.material)) {
                set_error("this scene has a moving sphere whose material carries a bump, which no kernel renders (the relief would swim "
                          "through the ball): remove the bump or give the mover another material");
                return RT_ERR_ARG;
            }
        for (const rt_moving_sphere &m : s.movers)
            if (scene_normal_map(s, m.material)) {
                set_error("this scene has a moving sphere whose material carries a normal map, which no kernel renders (as a bump's, "
                          "the relief would swim through the ball): remove the map or give the mover another material");
                return RT_ERR_ARG;
            }
        if (!find_kernel({K_MOTION, variant, true})) {
            set_error("kernel variant %u does not carry moving spheres (the motion kernels are variants 0, 16, 36 and 44)", variant);
            return RT_ERR_ARG;
        }
    }
    if (env && P.grid_wide == 2) {
        set_error("this scene has the nested grid and an environment map, which no kernel combines: switch one of them off");
        return RT_ERR_ARG;
    }
    if (env && (count || !find_kernel({K_ENV, variant, true}))) {
        set_error("%s: this scene has an environment map, which the %s (the environment kernels are variants 0, 16, 36 and 44)",
                  count ? "rt_render_hip_count" : "kernel variant", count ? "counting kernels do not carry" : "requested variant does not carry");
        return RT_ERR_ARG;
    }
    if (nee && P.grid_wide == 2) {
        set_error("this scene has the nested grid and light sampling on, which no kernel combines: switch one of them off");
        return RT_ERR_ARG;
    }
    if (nee && (count || !find_kernel({K_NEE, variant, true}))) {
        set_error("%s: this scene has light sampling on, which the %s (the light-sampling kernels are variants 0, 16, 36 and 44)",
                  count ? "rt_render_hip_count" : "kernel variant", count ? "counting kernels do not carry" : "requested variant does not carry");
        return RT_ERR_ARG;
    }
    // the counting kernels exist for the grid walks (3-D) and two ablation searches: anything else is counted by the kernel
    // variant 0 would run (reported in stats->kernel_variant / cull_mode)
    if (count && !variant_row(variant, false, true)) variant = (variant == 2) ? 6u : pick(true);
    if (count && variant == 2) variant = 6;
    // (the feature layouts exist in every build; variant 24 as a render variant only with RTMI_ABLATIONS)
    const KernelRow *plain = variant_row(variant);
    const int mode = feature >= 0 ? (variant == 52 ? 8 : (variant == 36 || variant == 44) ? 7 : 0) : plain ? plain->cull : -1;
    // nested cells are walked by variant 52 alone, and variant 52 walks nothing else; the linear scans read no grid
    if (mode == 8 && P.grid_wide != 2) {
        set_error("kernel variant %u walks tables with nested cells, which this scene does not have (rt_scene_set_nested_grid, and a "
                  "cell to nest): use variant 0", variant);
        return RT_ERR_ARG;
    }
    if (P.grid_wide == 2 && mode >= 5 && mode != 8) {
        set_error("kernel variant %u does not walk the nested cells of this scene's tables: use variant 0, 52 or the linear scans 16 / 24", variant);
        return RT_ERR_ARG;
    }
    if ((mode == 5 || mode == 6) && P.grid_wide) {
        set_error("kernel variant %u reads the compact grid tables of a sphere-only scene that fits LDS; this scene has the wide ones "
                  "(other primitives, textures, 65536 sphere slots or more, or tables beyond %zu bytes): use variant 0, 36 or 44",
                  variant, global_threshold);
        return RT_ERR_LIMIT;
    }
    if (mode == 7 && !P.grid_wide) {
        set_error("kernel variant %u walks the wide grid tables; this scene (spheres only, small enough for LDS) has the compact ones: "
                  "use variant 0, 2 or 6", variant);
        return RT_ERR_LIMIT;
    }
    if (variant == 2 && !P.grid_sheet) {
        set_error("kernel variant 2 walks a grid that is one cell high, which this scene does not have");
        return RT_ERR_LIMIT;
    }
    if (feature >= 0) ext = true;  // (the feature kernels are general builds)
    if (feature < 0 && ext && !variant_row(variant, true)) {
        set_error("kernel variant %u has no build with triangles / image textures (variants 0, 36, 44 and the linear scans 16 / 24 have)", variant);
        return RT_ERR_LIMIT;
    }
    if (!sphere_only && (mode == 5 || mode == 6)) {  // (cannot happen: such scenes get wide tables)
        set_error("kernel variant %u is built for sphere-only scenes", variant);
        return RT_ERR_LIMIT;
    }
    if (force_ext && variant_row(variant, true) && P.grid_wide) ext = true;
    if (nee || env || media || motion) ext = true;
    const size_t hot_bytes = hot_bytes_of(mode);
    const bool tables_global = (variant & 8u) != 0 || mode == 8;
    // ---- the instance: resolved once; the block size, the per-wave LDS, the launches, the grid size and the LDS limit go
    // through its row
    const char *family = env ? "environment" : media ? "media" : motion ? "motion" : feature >= 0 ? "feature" : nullptr;
    // (a scene with alpha masks, DESIGN 7v: the family's instance of alpha_kernel.h; every other scene: the rows it always ran)
    // (a projection, DESIGN 7w: the family's instance of camera_kernel.h, likewise)
    const KernelRow *kernel = env            ? find_kernel({K_ENV, variant, true, false, nee, feature >= 0, alpha, camera})
                              : media        ? find_kernel({K_MEDIA, variant, true, false, media_nee, false, false, camera})
                              : motion       ? find_kernel({K_MOTION, variant, true, false, false, false, alpha, camera})
                              : feature >= 0 ? find_kernel({K_FEATURE, variant, true, false, false, false, alpha, camera})
                              : nee          ? find_kernel({K_NEE, variant, true, false, false, false, alpha, camera})
                                             : variant_row(variant, ext, count, alpha, camera);
    if (!kernel) {
        if (family) set_error("layout %u has no %s kernel", variant, family);
        else set_error("kernel variant %u has no %s build", variant, count ? "counting" : (ext ? "triangle / texture" : "such"));
        return env || media || motion ? RT_ERR_ARG : RT_ERR_LIMIT;
    }
    // (alpha masks, DESIGN 7v: the passing queries' state, behind the accumulators of the 4-wave workgroups that render such a scene)
    const size_t lds_bytes = group_lds(*kernel, tables_global ? 0 : hot_bytes) + (kernel->key.alpha ? (size_t)kAlphaLdsBytes : 0);
    if (knob_set("RTMI_DEBUG_LAYOUT")) {
        const float *g = cache.image.data() + (size_t)P.off_grid * 4;
        int gn[3];
        memcpy(gn, g + 12, sizeof gn);
        fprintf(stderr, "variant %u: LDS %zu bytes per workgroup (tables %zu); %d prefix slots, %d clusters of %d; always-tested others %d + %d + %d "
                "of %d + %d + %d; %s grid %d x %d x %d = %d cells, cell %.3f x %.3f x %.3f (vec4 records: cells %d, lists %d)\n",
                variant, lds_bytes, tables_global ? (size_t)0 : hot_bytes, P.np, P.ncl, P.cluster, P.nr_a, P.nc_a, P.nt_a, P.nr, P.nc, P.nt,
                P.grid_wide ? "wide" : "compact", gn[0], gn[1], gn[2], P.grid_cells,
                g[8], g[9], g[10], P.off_grid_items - P.off_grid_cells, P.hot_vec4_grid - P.off_grid_items);
    }
    if (lds_bytes > 160 * 1024) {
        set_error("kernel variant %u keeps the scene tables in LDS and this scene needs %zu bytes per workgroup "
                  "(limit 163840); use the default variant",
                  variant, lds_bytes);
        return RT_ERR_LIMIT;
    }
    if (s.width > 65536 || P.bands > 32767) {  // the kernel packs (tile x0, band) of a wave's older item into one register
        set_error("frame of %d x %d rows per shard exceeds the tile index range (65536 columns, 262136 rows)", s.width,
                  sh.local_rows);
        return RT_ERR_LIMIT;
    }
    const size_t plane = (size_t)sh.local_rows * s.width * 3;
    const unsigned long long items64 = (unsigned long long)P.tiles_x * P.bands * plan.num_chunks;
    if (items64 > 0x7fffffffull) {
        set_error("%llu work items exceed the queue counter", items64);
        return RT_ERR_LIMIT;
    }
    P.num_items = (int)items64;
    // persistent launches: enough workgroups to fill the chip, never more than the work needs
    if (ent->num_cus == 0) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        ent->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    if (lds_bytes > 64 * 1024 && set_max_dynamic_lds(*kernel, lds_bytes)) {
        set_error("cannot raise the dynamic LDS limit to %zu bytes", lds_bytes);
        return RT_ERR_HIP;
    }
    const unsigned long long resident = (unsigned long long)ent->num_cus * blocks_per_cu(*kernel, lds_bytes);
    if (knob_set("RTMI_DEBUG_LAYOUT"))
        fprintf(stderr, "variant %u: workgroups of %u threads, %llu resident on %d CUs\n", variant, group_threads(*kernel), resident, ent->num_cus);

    float *d_out = (float *)d_rgb_sum;
    DevCounters *d_cnt = nullptr;
    if (count) {
        rc = ent->d_counters.reserve(1);
        if (rc) return rc;
        d_cnt = ent->d_counters.get();
        HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(DevCounters), stream));
        // the two minima start at all-ones
        HIP_TRY(hipMemsetAsync(&d_cnt->t_start_min, 0xff, sizeof(unsigned long long), stream));
        HIP_TRY(hipMemsetAsync(&d_cnt->t_end_min, 0xff, sizeof(unsigned long long), stream));
        HIP_TRY(hipMemsetAsync(&d_cnt->t_qe_min, 0xff, sizeof(unsigned long long), stream));
    }
    if (stats) HIP_TRY(hipEventRecord(ev1, stream));

    // accumulators, then (256-byte aligned: the kernel reads the ItemParams with 16-byte loads) the queue counter and the
    // ItemParams, and for adaptive sampling the tile list.  They belong to this (scene, device): concurrent renders of ONE
    // scene object on one device must share a stream (different scene objects, or clones, are independent)
    const size_t queue_off = (plane * sizeof(unsigned long long) + 255) & ~(size_t)255;
    const long long frame_tiles = (long long)P.tiles_x * P.bands;
    const size_t need = queue_off + (ad ? (((size_t)(RT_TILE_LIST_AT + frame_tiles) * 4 + 255) & ~(size_t)255) : 256);
    // the beam table (rt_beam.h): for the instances whose bursts read it, when a band of the shard is a band of the frame (a
    // record is indexed by whole-frame tile coordinates, whatever the shard and its deal)
    const uint16_t *beams = nullptr;
    if (RT_BURST_LISTS != 0 && kernel->key.family == K_PLAIN && !kernel->key.count && (kernel->cull == 5 || kernel->cull == 6) &&
        sh.tile_rows % 8 == 0 && beams_apply(s, cache.layout)) {
        rc = ensure_beams(s, cache, ent, stream);
        if (rc) return rc;
        beams = ent->d_beams.get();
    }
    const Launcher launch{P, sh, ent, d_cnt, stream, lds_bytes, resident, *kernel, feature, beams};

    int launches = 0;
    if (ad) {
        rc = run_adaptive(launch, *ad, s, queue_off, need, d_out, o ? o->spp_chunk : 0, launches);
        if (rc) return rc;
    } else if (s.max_depth <= 0 && !h_acc && feature < 0) {
        // while (depth > 0) never runs: every sample is black (main.cpp:20,42)
        HIP_TRY(hipMemsetAsync(d_out, 0, plane * sizeof(float), stream));
    } else {
        rc = ent->d_acc.reserve(need / sizeof(unsigned long long));  // (need: a multiple of 256 bytes)
        if (rc) return rc;
        unsigned long long *const d_acc = ent->d_acc.get();
        HIP_TRY(hipMemsetAsync(d_acc, 0, need, stream));
        // progressive rendering: continue from the caller's exact sums
        if (h_acc) HIP_TRY(hipMemcpyAsync(d_acc, h_acc, plane * sizeof(long long), hipMemcpyHostToDevice, stream));
        unsigned int *d_queue = reinterpret_cast<unsigned int *>(reinterpret_cast<char *>(d_acc) + queue_off);
        if (s.max_depth > 0 || feature >= 0) {
            rc = launch.enqueue(d_acc, d_queue, sample_first, sample_count, 0, plan);
            if (rc) return rc;
            ++launches;
        }
        if (d_out) {
            launch_finalize(d_acc, d_out, plane, stream);
            ++launches;
        }
        if (h_acc) {
            HIP_TRY(hipMemcpyAsync(h_acc, d_acc, plane * sizeof(long long), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
    }
    HIP_TRY(hipGetLastError());

    if (stats) {
        // what variant 0 (or a counting call) resolved to (| 256: light sampling, | 512: a feature pass, | 1024: an environment map, | 2048: media, | 4096: moving spheres)
        stats->kernel_variant = (int32_t)(variant | (nee ? 256u : 0u) | (feature >= 0 ? 512u : 0u) | (env ? 1024u : 0u) | (media ? 2048u : 0u) |
                                          (motion ? 4096u : 0u));
        HIP_TRY(hipEventRecord(ev2, stream));
        lock.unlock();
        HIP_TRY(hipEventSynchronize(ev2));
        float up = 0, k = 0;
        HIP_TRY(hipEventElapsedTime(&up, ev0, ev1));
        HIP_TRY(hipEventElapsedTime(&k, ev1, ev2));
        stats->upload_ms = up;
        stats->kernel_ms = k;
        stats->launches = launches;
        if (count) return read_counters(d_cnt, P, kernel->cull, s.prims.size(), stats);
    }
    return RT_OK;
}

int rt_render_hip_device(const rt_scene *s, const rt_opts *o, void *d_rgb_sum, void *stream, rt_stats *stats) {
    return render_impl(s, o, d_rgb_sum, stream, stats, nullptr, false);
}

static int render_host_buffer(const rt_scene *sc, const rt_opts *o, float *rgb_sum, rt_stats *stats, bool count,
                              long long *h_acc = nullptr, AdaptiveRun *ad = nullptr, int32_t *spp_map = nullptr, int feature = -1) {
    if (!sc) {
        set_error("null scene");
        return RT_ERR_ARG;
    }
    if (count && !stats) {
        set_error("rt_render_hip_count needs a stats pointer");
        return RT_ERR_ARG;
    }
    if (!count && !rgb_sum && !h_acc) {
        set_error("null output buffer");
        return RT_ERR_ARG;
    }
    Shard sh;
    int rc = shard_of(sc->s, o, sh);
    if (rc) return rc;
    const int device = o ? o->device : 0;
    DeviceScope scope;
    rc = scope.enter(device, "the render path");
    if (rc) return rc;
    const size_t bytes = (size_t)sh.local_rows * sc->s.width * 3 * sizeof(float);
    // the device framebuffer of this (scene, device) is kept between calls (no hipMalloc / hipFree per frame)
    float *d_out = nullptr;
    rt_stats local;
    if (bytes && (rgb_sum || !h_acc)) {
        DeviceSceneCache &cache = cache_of(sc->s);
        std::lock_guard<std::mutex> lock(cache.mu);
        DeviceEntry *ent = device_record(cache.entries, device);
        rc = ent->d_out.reserve(bytes / sizeof(float));
        if (rc) return rc;
        d_out = ent->d_out.get();
        if (ad) {  // ... and so is the sample-count map of the adaptive entry point
            rc = ent->d_spp.reserve(bytes / 3 / sizeof(float));
            if (rc) return rc;
            ad->d_spp_map = ent->d_spp.get();
        }
    }
    rc = bytes ? render_impl(sc, o, d_out, nullptr, stats ? stats : &local, h_acc, count, ad, feature) : RT_OK;
    if (rc == RT_OK && rgb_sum && bytes) {
        hipError_t e = hipMemcpy(rgb_sum, d_out, bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess && ad) e = hipMemcpy(spp_map, ad->d_spp_map, bytes / 3 / sizeof(float) * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            set_error("hipMemcpy D2H failed: %s", hipGetErrorString(e));
            rc = RT_ERR_HIP;
        }
    }
    return rc;
}

int rt_render_hip(const rt_scene *s, const rt_opts *o, float *rgb_sum, rt_stats *stats) {
    return render_host_buffer(s, o, rgb_sum, stats, false);
}

int rt_render_hip_count(const rt_scene *s, const rt_opts *o, float *rgb_sum, rt_stats *stats) {
    return render_host_buffer(s, o, rgb_sum, stats, true);
}

// the arguments of the adaptive entry points, checked before any device access; fills the options of the run (samples [0, max_spp))
static int adaptive_args(const rt_scene *sc, const rt_opts *o, const rt_adaptive *a, const void *rgb_sum, const void *spp_map,
                         rt_opts &run, int &max_spp) {
    if (!sc || !a || !rgb_sum || !spp_map) {
        set_error("rt_render_hip_adaptive: null scene, schedule or output pointer");
        return RT_ERR_ARG;
    }
    max_spp = a->max_spp ? a->max_spp : sc->s.spp;
    if (a->min_spp < 2 || max_spp < a->min_spp) {
        set_error("rt_render_hip_adaptive: min_spp %d must be >= 2 and max_spp %d >= min_spp", a->min_spp, max_spp);
        return RT_ERR_ARG;
    }
    if (!(a->threshold >= 0.0f) || !std::isfinite(a->threshold)) {
        set_error("rt_render_hip_adaptive: threshold must be finite and >= 0");
        return RT_ERR_ARG;
    }
    if (max_spp > RT_MAX_SAMPLES_PER_PIXEL) {  // (render_impl's cap on the samples of a pixel)
        set_error("max_spp %d exceeds %d samples per pixel, the range over which the fixed-point pixel sums are exact", max_spp,
                  RT_MAX_SAMPLES_PER_PIXEL);
        return RT_ERR_LIMIT;
    }
    if (o) {
        run = *o;
    } else {
        rt_opts_default(&run);
    }
    if (run.tile_stride > 1) {
        set_error("rt_render_hip_adaptive renders whole frames: tile_stride must be <= 1");
        return RT_ERR_ARG;
    }
    if (run.sample_first != 0 || run.sample_count != 0) {
        set_error("rt_render_hip_adaptive: the schedule owns the samples (sample_first and sample_count must be 0)");
        return RT_ERR_ARG;
    }
    if (!variant_exists(run.variant)) {
        set_error("unknown kernel variant %u", run.variant);
        return RT_ERR_ARG;
    }
    run.tile_first = 0, run.tile_stride = 1;
    run.sample_count = max_spp;
    return RT_OK;
}

int rt_render_hip_adaptive_device(const rt_scene *s, const rt_opts *o, const rt_adaptive *a, void *d_rgb_sum, void *d_spp_map,
                                  void *stream, rt_adaptive_stats *st) {
    rt_opts run;
    int max_spp = 0;
    int rc = adaptive_args(s, o, a, d_rgb_sum, d_spp_map, run, max_spp);
    if (rc) return rc;
    rt_adaptive_stats local_st;
    if (!st) st = &local_st;
    memset(st, 0, sizeof *st);
    AdaptiveRun ad{a, max_spp, static_cast<int *>(d_spp_map), st};
    rt_stats stats;
    rc = render_impl(s, &run, d_rgb_sum, stream, &stats, nullptr, false, &ad);
    st->kernel_ms = stats.kernel_ms;
    return rc;
}

int rt_render_hip_adaptive(const rt_scene *s, const rt_opts *o, const rt_adaptive *a, float *rgb_sum, int32_t *spp_map,
                           rt_adaptive_stats *st) {
    rt_opts run;
    int max_spp = 0;
    int rc = adaptive_args(s, o, a, rgb_sum, spp_map, run, max_spp);
    if (rc) return rc;
    rt_adaptive_stats local_st;
    if (!st) st = &local_st;
    memset(st, 0, sizeof *st);
    AdaptiveRun ad{a, max_spp, nullptr, st};
    rt_stats stats;
    rc = render_host_buffer(s, &run, rgb_sum, &stats, false, nullptr, &ad, spp_map);
    st->kernel_ms = stats.kernel_ms;
    return rc;
}

// the arguments of the feature entry points, checked before any device access
static int feature_args(const rt_scene *sc, int feature, const void *sum) {
    if (!sc || !sum) {
        set_error("rt_render_hip_feature: null scene or output pointer");
        return RT_ERR_ARG;
    }
    if (feature < RT_FEATURE_ALBEDO || feature > RT_FEATURE_DEPTH) {
        set_error("rt_render_hip_feature: feature %d (0 albedo, 1 normal, 2 depth)", feature);
        return RT_ERR_ARG;
    }
    return RT_OK;
}

int rt_render_hip_feature(const rt_scene *s, const rt_opts *o, int feature, float *sum, rt_stats *stats) {
    int rc = feature_args(s, feature, sum);
    if (rc) return rc;
    return render_host_buffer(s, o, sum, stats, false, nullptr, nullptr, nullptr, feature);
}

int rt_render_hip_feature_device(const rt_scene *s, const rt_opts *o, int feature, void *d_sum, void *stream, rt_stats *stats) {
    int rc = feature_args(s, feature, d_sum);
    if (rc) return rc;
    return render_impl(s, o, d_sum, stream, stats, nullptr, false, nullptr, feature);
}

// ---- ray queries.  The arguments, checked before any device access; *layout: the variant as given
static int trace_args(const rt_scene *sc, const rt_opts *o, int mode, const void *rays, size_t n, const void *out, unsigned *layout) {
    if (!sc) {
        set_error("rt_trace_hip: null scene");
        return RT_ERR_ARG;
    }
    if (mode != RT_TRACE_CLOSEST && mode != RT_TRACE_OCCLUDED) {
        set_error("rt_trace_hip: mode %d (0 closest hit, 1 occlusion)", mode);
        return RT_ERR_ARG;
    }
    if (n >= ((size_t)1 << 31)) {
        set_error("rt_trace_hip: %zu rays in one batch (fewer than 2^31: split the batch)", n);
        return RT_ERR_LIMIT;
    }
    if (!sc->s.movers.empty()) {
        set_error("rt_trace_hip: this scene has moving spheres and a ray query has no shutter time: clear the moving spheres for the query (rt_scene_clear_moving_spheres)");
        return RT_ERR_ARG;
    }
    const unsigned variant = o ? o->variant : 0;
    const unsigned ok[] = {0u, 16u, 24u, 36u, 44u, 52u};
    if (std::find(std::begin(ok), std::end(ok), variant) == std::end(ok)) {
        set_error("rt_trace_hip: layout %u (0, 16, 24, 36, 44 or 52)", variant);
        return RT_ERR_ARG;
    }
    *layout = variant;
    if (n > 0 && (!rays || !out)) {
        set_error("rt_trace_hip: null rays or output pointer");
        return RT_ERR_ARG;
    }
    return RT_OK;
}

// n > 0 rays at d_rays -> d_out, both on o->device (the arguments have been checked)
static int trace_impl(const rt_scene *sc, const rt_opts *o, unsigned variant, int mode, const void *d_rays, size_t n, void *d_out,
                      void *stream_v, rt_stats *stats) {
    const Scene &s = sc->s;
    int rc = scene_validate(s);
    if (rc) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    const int device = o ? o->device : 0;
    DeviceScope scope;
    rc = scope.enter(device, "the ray-query path");
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_v;
    DeviceSceneCache &cache = cache_of(s);
    std::unique_lock<std::mutex> lock(cache.mu);  // (as render_impl: packing, the entry list and the enqueueing)
    rc = ensure_packed(s, cache);
    if (rc) return rc;
    DeviceEntry *ent = device_record(cache.entries, device);
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    if (stats) {
        std::array<hipEvent_t, 3> *t = nullptr;
        rc = timing_events(device, t);
        if (rc) return rc;
        ev0 = (*t)[0], ev1 = (*t)[1], ev2 = (*t)[2];
        HIP_TRY(hipEventRecord(ev0, stream));
    }
    if (ent->version != s.version || !ent->d_image.get()) {
        rc = ent->d_image.reserve(cache.image.size());
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(ent->d_image.get(), cache.image.data(), cache.image.size() * sizeof(float), hipMemcpyHostToDevice, stream));
        ent->version = s.version;
    }
    // the layout: the scene's own, or the one named; compact tables list spheres for the sphere-only kernels, a query scans
    // the list instead (as a feature pass does)
    const RenderParams &P = cache.layout;
    static const size_t global_threshold = (size_t)knob("RTMI_GLOBAL_TABLE_BYTES", (double)kLdsTableBytes);
    if (variant == 0) variant = pick_variant(P, false, global_threshold);
    const size_t scan_bytes = (size_t)(P.hot_vec4 - (P.off_box - P.off_grid)) * 16;
    if (variant == 2 || variant == 6) variant = scan_bytes <= global_threshold ? 16u : 24u;
    const int mode_cull = variant == 52 ? 8 : (variant == 36 || variant == 44) ? 7 : 0;
    if (mode_cull == 8 && P.grid_wide != 2) {
        set_error("layout 52 walks tables with nested cells, which this scene does not have (rt_scene_set_nested_grid, and a cell to nest): use 0");
        return RT_ERR_ARG;
    }
    if (mode_cull == 7 && P.grid_wide == 2) {
        set_error("layout %u does not walk the nested cells of this scene's tables: use 0, 52 or the linear scans 16 / 24", variant);
        return RT_ERR_ARG;
    }
    if (mode_cull == 7 && !P.grid_wide) {
        set_error("layout %u walks the wide grid tables; this scene (spheres only, small enough for LDS) has the compact ones: use 0, 16 or 24", variant);
        return RT_ERR_LIMIT;
    }
    const KernelRow *kernel = find_kernel({K_TRACE, variant, true});
    if (!kernel) {
        set_error("layout %u has no ray-query kernel", variant);
        return RT_ERR_ARG;
    }
    // LDS per workgroup: the hot tables the search reads, unless it reads them from global memory -- and nothing else
    const bool tables_global = (variant & 8u) != 0 || mode_cull == 8;
    const size_t lds_bytes = tables_global ? 0 : (mode_cull == 7 ? (size_t)P.hot_vec4_grid * 16 : scan_bytes);
    if (lds_bytes > 160 * 1024) {
        set_error("layout %u keeps the scene tables in LDS and this scene needs %zu bytes per workgroup (limit 163840); use layout 0", variant, lds_bytes);
        return RT_ERR_LIMIT;
    }
    if (ent->num_cus == 0) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        ent->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    if (lds_bytes > 64 * 1024 && set_max_dynamic_lds(*kernel, lds_bytes)) {
        set_error("cannot raise the dynamic LDS limit to %zu bytes", lds_bytes);
        return RT_ERR_HIP;
    }
    const unsigned long long resident = (unsigned long long)ent->num_cus * blocks_per_cu(*kernel, lds_bytes);
    rc = ent->d_trace_queue.reserve(64);
    if (rc) return rc;
    if (stats) HIP_TRY(hipEventRecord(ev1, stream));
    HIP_TRY(hipMemsetAsync(ent->d_trace_queue.get(), 0, 4, stream));
    // persistent launch: enough workgroups to fill the chip, never more than the work needs (an item per wave)
    const unsigned long long items = (n + RT_TRACE_ITEM - 1) / RT_TRACE_ITEM, need_blocks = (items + 3) / 4;
    const unsigned long long grid = need_blocks < resident ? need_blocks : resident;
    RenderParams Q = P;
    Q.rr_p = 0.0f, Q.flags = 0u, Q.max_depth = 1;
    launch_trace(*kernel, Q, ent->d_image.get(), d_rays, d_out, ent->d_trace_queue.get(), (unsigned int)n, mode, lds_bytes, (unsigned)grid, stream);
    HIP_TRY(hipGetLastError());
    if (stats) {
        stats->kernel_variant = (int32_t)(variant | 8192u);
        HIP_TRY(hipEventRecord(ev2, stream));
        lock.unlock();
        HIP_TRY(hipEventSynchronize(ev2));
        float up = 0, k = 0;
        HIP_TRY(hipEventElapsedTime(&up, ev0, ev1));
        HIP_TRY(hipEventElapsedTime(&k, ev1, ev2));
        stats->upload_ms = up, stats->kernel_ms = k, stats->launches = 1;
    }
    return RT_OK;
}

int rt_trace_hip_device(const rt_scene *s, const rt_opts *o, int mode, const void *d_rays, size_t n, void *d_out, void *stream, rt_stats *stats) {
    unsigned layout = 0;
    int rc = trace_args(s, o, mode, d_rays, n, d_out, &layout);
    if (rc) return rc;
    if (n == 0) {
        if (stats) memset(stats, 0, sizeof *stats);
        return RT_OK;
    }
    return trace_impl(s, o, layout, mode, d_rays, n, d_out, stream, stats);
}

int rt_trace_hip(const rt_scene *s, const rt_opts *o, int mode, const rt_ray *rays, size_t n, void *out, rt_stats *stats) {
    unsigned layout = 0;
    int rc = trace_args(s, o, mode, rays, n, out, &layout);
    if (rc) return rc;
    if (n == 0) {
        if (stats) memset(stats, 0, sizeof *stats);
        return RT_OK;
    }
    const int device = o ? o->device : 0;
    DeviceScope scope;
    rc = scope.enter(device, "the ray-query path");
    if (rc) return rc;
    // the device copies of this (scene, device) are kept between calls: rays, then (256-byte aligned) the records
    const size_t ray_bytes = n * sizeof(rt_ray), out_bytes = mode == RT_TRACE_OCCLUDED ? n : n * sizeof(rt_hit);
    const size_t out_off = (ray_bytes + 255) & ~(size_t)255;
    char *d_io = nullptr;
    {
        DeviceSceneCache &cache = cache_of(s->s);
        std::lock_guard<std::mutex> lock(cache.mu);
        DeviceEntry *ent = device_record(cache.entries, device);
        rc = ent->d_trace_io.reserve(out_off + out_bytes);
        if (rc) return rc;
        d_io = ent->d_trace_io.get();
    }
    HIP_TRY(hipMemcpy(d_io, rays, ray_bytes, hipMemcpyHostToDevice));
    rt_stats local;
    rc = trace_impl(s, o, layout, mode, d_io, n, d_io + out_off, nullptr, stats ? stats : &local);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out, d_io + out_off, out_bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_render_hip_accumulate(const rt_scene *s, const rt_opts *o, int64_t *acc, float *rgb_sum, rt_stats *stats) {
    if (!acc) {
        set_error("rt_render_hip_accumulate: null accumulator");
        return RT_ERR_ARG;
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "accumulator width");
    return render_host_buffer(s, o, rgb_sum, stats, false, reinterpret_cast<long long *>(acc));
}

}  // extern "C"
