// Device-side scene image shared between the host packer (pack.hip) and the
// kernel.  One contiguous buffer, 16-byte records:
//
//   HOT part (copied into LDS by every workgroup; everything the primitive loop reads)
//     sphere  [ns + 4]  1 x float4   {cx, cy, cz, r*r}   big spheres first, then Morton-ordered
//                                clusters of 8; padded with never-hit records (r*r = -inf)
//     box     [ncl] 2 x float4   inflated bounding box of each cluster (culling variant)
//     rect    [nr]  2 x float4   {a0, a1, b0, b1} {k, axis(bits), 0, 0}
//     cyl     [nc]  6 x float4   m_inv rows 0..2, {radius^2, zmin, zmax, 0}, then the world-space bounding box of the open tube
//                                {min.xyz, _} {max.xyz, _}: one run of records, so that a lane that finds the cylinder in a cell's
//                                list has its box and its matrix in flight together
//     tri     [nt]  5 x float4   {v1.xyz, n.x} {v2.xyz, n.y} {v3.xyz, n.z}   (n = unit normal, hittable.py:104), then its box
//     quad    [nq]  5 x float4   {Q.xyz, n.x} {A.xyz, n.y} {B.xyz, n.z}   (rt_quad.h: the corner, the unit normal, and the
//                                two vectors that turn p - Q into the parallelogram's coordinates), then its box.  Straight behind
//                                the triangles, with their stride: a cell's entry finds its box at one address for both
//   COLD part (stays in global memory / L2; read once per bounce by the winning lane)
//     sphere  [ns]  1 x float4   {1/r, material(bits), list index(bits), material kind(bits)}
//     rect    [nr]  1 x float4   {material(bits), list index(bits), material kind(bits), 0}
//     cyl     [nc]  4 x float4   m rows 0..2, {material(bits), list index(bits), material kind(bits), 0}
//     tri     [nt]  2 x float4   {material(bits), list index(bits), u1.x, u1.y} {u2.x, u2.y, u3.x, u3.y}
//     quad    [nq]  2 x float4   {material(bits), list index(bits), 0, 0} {0, 0, 0, 0}: straight behind the triangles' and as wide
//                                as theirs, so that the tie rule's list_index_of reads both through one address
//     mat     [nm]  3 x float4   {kind(bits), p0, p1, p2} {c0.xyz, p3} {c1.xyz, 0}
//     alpha   [nm]  1 x float4   (only when a material carries an alpha mask; straight behind the material table, at
//                                off_mat + 3 nm: found without a word of its own in the parameter block, which stays as it was
//                                for every kernel) one per material: {word offset of the mask's texels (bits), rows (bits), cols
//                                (bits), c8 (bits)}; rows = 0: the material has no mask.  Read by the instances of alpha_kernel.h
//                                alone.  (With alpha, a texel word's top byte holds 255 - a8: zero for an opaque texel and for
//                                every image without alpha)
//     image   texels of the image textures, one 32-bit word each (r | g << 8 | b << 16), row-major
//     noise   [nn]  1 x float4   (only with noise textures; behind the texels) per noise texture, in texture order:
//                                {scale, distortion, seed(bits), style | axis << 2 | octaves << 4 (bits)}.  A material with such a
//                                texture keeps the two colours in c0.xyz / c1.xyz and the record's offset (in float4 records
//                                from the image's start, bits) in c0.w -- the one word plastic's p0..p2 leave free
//     bump    [nb]  1 x float4   (only with bumped materials; behind the noise records) per bumped material, in
//                                material order: {offset of the height texture's noise record (bits), strength, 0, 0}.  Such a
//                                material holds its bump record's offset (bits) in c1.w, the word no kind uses; 0: no bump
//     nmap    [nn]  1 x float4   (only with normal-mapped materials; behind the bump records) per mapped material, in
//                                material order: {word offset of the map's texels (bits), rows (bits), cols (bits), scale}.  Such a
//                                material holds MINUS its record's offset (bits) in c1.w: a bump or a map, never both
//   LIGHT part (only with light sampling on and at least one sampled emitter; global memory, read by the light-sampling kernels)
//     light   [nl]  7 x float4   {shape(bits): 0 sphere, 1 rect, 2 cylinder, 4 triangle, 5 quad, grouped id(bits), selection probability, 1/area}
//                                {emission even.rgb, checker(bits)} {emission odd.rgb, 0}, then the geometry:
//                                sphere {c.xyz, |r|}; rect {a0, a1, b0, b1} {k, axis(bits), 0, 0}; cylinder o2w rows 0..2,
//                                {|radius|, zmin, zmax, 0}; triangle (mesh lights) {v1, 0} {e1 = v2 - v1, 0}
//                                {e2 = v3 - v1, 0} {the geometric unit normal, 0}; quad {Q, 0} {u, 0} {v, 0} {n, 0}
//     alias   [nl]  1 x float4   {threshold, alias light(bits), 0, 0}: one draw u picks i = floor(u nl), then i or its alias
//     slot    [ns + nr + nc + nt + nq] one 32-bit word per grouped primitive id: its light, -1 = not a sampled light
//     (an environment that is sampled is the last light: {3, -1, selection probability, 1 / 4 pi}, no geometry)
//     (analytic lights, DESIGN 7s, behind the area emitters: {shape(bits) 6 point / 7 spot / 8 distant, -1, selection
//      probability, 1 / measure} {colour, 0} {colour, 0}, then point {x, 0}; spot {x, 0} {unit axis a, 0} {cos_o, inv, 0, 0};
//      distant {unit direction t towards it, 1 - cos alpha} {D = 4 x bounding radius, 0, 0, 0}.  No slot points at them.)
//   ENVIRONMENT part (only with an environment map; global memory, read by the environment kernels): rt_env.h
//   MEDIA part (only with at least one medium; global memory, read by the media kernels): rt_media.h.  Two words of the camera
//     block say where it lies ({count, offset} in the .w of records off_cam + 1 and + 2; zero without media)
//   NORMALS part (smooth shading; only when at least one triangle has vertex normals; global memory, read by the
//     winner section of the general kernels): per triangle of the triangle tables 3 x float4 {n1.xyz, has normals(bits)}
//     {n2.xyz, 0} {n3.xyz, 0}; a flat triangle's records are zeros.  The .w of record off_cam + 5 is the part's first record
//     (zero: the scene has no vertex normals and no such part)
//
// Primitives are grouped by type (spheres, rects, cylinders), each group in list
// order; the original list index is kept for the reference's tie rule (a later
// object replaces an earlier one at equal t: hittable_list::hit accepts
// root <= closest_so_far, gpu-version/object.cuh:23-37 with :61).
#pragma once
#include <stdint.h>

// measurement variants, counting kernels and RTMI_* environment knobs (the default build); 0: the product kernels alone
#ifndef RTMI_ABLATIONS
#define RTMI_ABLATIONS 1
#endif

// spheres per cluster of the sphere table (a cluster occupies RT_CLUSTER + 1 slots, the last one never hit)
#define RT_CLUSTER 8
// sphere slots of a scene: fewer than this, so that 16 x a slot -- the byte offset of its cold record -- fits 32 bits
// (the packer's lay_out_image refuses with RT_ERR_LIMIT; the kernels' rec_at relies on it)
#define RT_MAX_SPHERE_SLOTS (1LL << 28)

// records per light of the light table (light sampling)
#define RT_LIGHT_STRIDE 7

// records per cylinder / triangle of the hot tables: the primitive, then its bounding box (2 records)
#define RT_CYL_STRIDE 6
#define RT_TRI_STRIDE 5
// ... and per quad.  The quads' hot records follow the triangles' as one table (the cells' lists and the box tests
// address both by RT_TRI_STRIDE x (id - ns - nr - nc)), so the two strides are one number
#define RT_QUAD_STRIDE 5
static_assert(RT_QUAD_STRIDE == RT_TRI_STRIDE, "quads and triangles share one hot table");

// consecutive clusters under one outer box
#ifndef RT_GROUP
#define RT_GROUP 4
#endif

// slabs per axis of a window box in the range tables (candidate clusters of a ray segment): R[i0 * RT_SLABS + i1]
#ifndef RT_SLABS
#define RT_SLABS 16
#endif

// Pixel sums: signed 64-bit fixed point with RT_FIX_BITS fractional bits (include/rtmi.h, rt_render_hip_accumulate)
#define RT_FIX_BITS 24  /* = RT_ACC_FIX_BITS of include/rtmi.h (static_assert in render_kernel.hip) */
#define RT_FIX_CLAMP 65536.0f
#define RT_MAX_SAMPLES_PER_PIXEL (1 << 23)

namespace rtmi {

enum MatKind : int32_t {
    MK_LAMBERT_SOLID = 0,    // c0 = albedo
    MK_LAMBERT_CHECKER = 1,  // c0 = even, c1 = odd
    MK_LAMBERT_IMAGE = 2,    // c0 = {texel word offset (bits), rows (bits), cols (bits)}: image texture
    MK_METAL = 3,            // c0 = albedo, p0 = fuzz
    MK_DIELECTRIC = 4,       // p0 = ir, p1 = 1/ir, p2 = r0(1/ir), p3 = r0(ir)
    MK_LIGHT_SOLID = 5,      // c0 = emission
    MK_LIGHT_CHECKER = 6,    // c0 = even, c1 = odd
    MK_LIGHT_IMAGE = 7,      // as MK_LAMBERT_IMAGE
    MK_MEDIUM = 8,           // a medium event of the media kernels (rt_media.h): no material record, `mat` is the medium's index
    // glossy materials (rt_glossy.h), in the general (EXT) builds alone.  p0 = alpha = max(r^2, 1e-3), p2 = the
    // roughness r itself (what the light-sample threshold is asked of)
    MK_ROUGH_METAL = 9,      // c0 = F0
    MK_PLASTIC_SOLID = 10,   // p1 = r0 of the coat, c0 = body colour
    MK_PLASTIC_CHECKER = 11, // p1 = r0, c0 = even, c1 = odd
    MK_PLASTIC_IMAGE = 12,   // p1 = r0, c0 as MK_LAMBERT_IMAGE
    // noise textures (rt_noise.h), in the general (EXT) builds alone: c0 = colour at s = 0, c1 = colour at s = 1,
    // p3 (c0.w) = the offset of the texture's noise record (bits).  The winner section evaluates the texture and hands the
    // vertex on as the matching *_IMAGE kind, except plastic (whose light sample needs the colour again at full precision)
    MK_LAMBERT_NOISE = 13,
    MK_LIGHT_NOISE = 14,
    MK_PLASTIC_NOISE = 15,   // p1 = r0 (the kind rides in 6 bits of a glossy vertex's packed word: kinds stay below 64)
    // rough glass (rt_glass.h), the third glossy material: {kind, alpha, 1/ir, r}{sigma.rgb, ir}{., ., ., bump} --
    // p0 and p2 as the other two, p1 = 1/ir (eta of a front hit), c0 = the absorption coefficient per unit length,
    // p3 (c0.w) = ir (eta of a back hit).  In a glossy vertex's packed word a back hit rides as kind 17 (bit 0 set)
    MK_ROUGH_GLASS = 16,
    // the metallic-roughness material (rt_pbr.h): {kind, offset of its side record (bits), r0 of the coat,
    // base type | map type << 4 (bits; 0 solid, 1 checker, 2 image, 3 noise)}, then c0 / c1 of the BASE texture as the
    // textured kinds above keep them (c0.w: a noise base's record), c1.w the bump.  The side record is three rows shaped as a
    // material's: {metallic factor, roughness factor, 0, 0}, then c0 / c1 of the MAP (none: solid white).  The winner section
    // resolves both textures to bytes; in a glossy vertex's packed word the vertex rides as the lobe it chose: 18 plastic, 19 metal
    MK_PBR = 18
};

// Per-launch values the kernel needs only when a wave fetches or flushes a work item.  They live in global
// memory behind the queue counter (16 ints at queue[RT_ITEM_PARAMS_AT], written by a one-thread kernel before the
// render launch; layout in item_params_kernel) and are read there, instead of occupying 14 SGPRs for the whole launch.
#define RT_ITEM_PARAMS_AT 16
// Adaptive sampling (rt_render_hip_adaptive): a launch with n_list != 0 renders only the tiles listed at queue[RT_TILE_LIST_AT ..
// + n_list), one word per tile: band << 16 | x0 (x0 = 8 x tile column); item i is chunk i / n_list of tile list[i % n_list].
// Such a launch carries tiles_x = n_list and bands = 1, which makes the plain decode compute i % n_list and i / n_list.
#define RT_TILE_LIST_AT 64
// The beam table's address (rt_beam.h; variants 2 and 6): 64 bits at queue[RT_BEAMS_AT], between the item parameters and the
// tile list; zero: the launch has no table and every burst runs the full query.  Read by the bursts with a uniform load.
#define RT_BEAMS_AT 32
struct ItemParams {
    int32_t tiles_x, bands, num_items, sample_first, sample_count, spp_chunk, n_big, n_med, q_med, q_small;
    int32_t tile_rows, tile_first, tile_stride, local_rows;
    int32_t tile_rotate;  // how the tiles are dealt out to the shards (rt_opts.tile_rotate; shard.h)
    int32_t n_list = 0;   // 0: every tile of the shard; else the length of the tile list
};

// RenderParams::flags carries the scene's RT_FLAG_* bits (include/rtmi.h) and, above them, what the launch path adds:
// "this scene has a normal map" (DESIGN 7u).  A kernel argument, so the test is a scalar branch around the whole step
#define RT_PFLAG_NORMAL_MAPS (1u << 16)
// ... and the camera's projection (rt_camera.h): the model number in two bits, 0 = perspective.  Read by the
// instances of camera_kernel.h alone, which a non-perspective scene runs
#define RT_PFLAG_PROJ_SHIFT 17
// alpha cutouts: the holes one query passes through at most; the next masked hit counts as opaque whatever its texel says
#define RT_ALPHA_MAX_PASSES 64

// kernel parameter block (passed by value: lands in SGPRs / the kernarg segment)
struct RenderParams {
    int32_t off_cam;         // 6 records of the hot table: {origin, lens_radius}, lower_left, horizontal, vertical, u, v (a projection
                             // other than the perspective one: what rt_camera.h says)
    float background[3];
    uint32_t flags;
    float rr_p;              // Russian-roulette survival probability per bounce, 0 = off
    int32_t width, height, max_depth;
    float inv_wm1, inv_hm1;  // 1 / (W - 1), 1 / (H - 1) in fp32 (the jitter's scale, main.cu:96-97): computed by the host, because a
                             // value the kernel derives before its main loop is a VGPR that gets spilled to scratch
    // shard geometry (see rt_opts)
    int32_t tile_rows, tile_first, tile_stride, num_tiles, local_rows;
    // samples
    // samples [sample_first, +sample_count) are cut into three runs of chunks, handed out in this order by the
    // chunk-major queue: n_big chunks of spp_chunk, n_med chunks of q_med, then chunks of q_small to the end
    // (guided self-scheduling: the later an item is handed out, the shorter it is); num_chunks = total
    int32_t sample_first, sample_count, spp_chunk, num_chunks, n_big, n_med, q_med, q_small;
    int32_t orphan_max;      // an item is retired once at most this many of its paths are alive (render_kernel.hip)
    uint32_t seed_lo, seed_hi;
    // scene image
    int32_t ns, nr, nc, nm;
    int32_t nt;              // triangles (grouped ids ns + nr + nc ...)
    // the leading rectangles / cylinders / triangles of their tables that are tested for every query (the oversized ones: a
    // room's walls); the rest is listed in the cells of the wide grid tables.  The searches without a grid test all of them.
    int32_t nr_a, nc_a, nt_a;
    int32_t off_tri_hot, off_tri_cold;
    int32_t feature;         // render_feature_kernel: the first-hit feature of this launch (RT_FEATURE_*, include/rtmi.h); no other
                             // kernel reads it (the word was a copy of ns that nothing read)
    int32_t np;              // leading slots that are always tested (big spheres), padded to a multiple of 4
    int32_t ncl;             // clusters of 8 slots after the prefix, each with a bounding box
    int32_t cluster;         // spheres per culling cluster (RT_CLUSTER)
    int32_t off_box;         // 2 float4 per cluster: {min.xyz,_}, {max.xyz,_}
    int32_t ngr, off_gbox;   // outer boxes over RT_GROUP consecutive clusters
    int32_t nwin, off_wbox;  // window boxes over 64 consecutive clusters (64 / RT_GROUP outer boxes)
    // range tables: per window {box min.xyz}, {1 / slab width .xyz}, then per enabled axis RT_SLABS^2 64-bit masks
    int32_t off_rtab, rt_stride, rt_axes;  // float4 offset, float4 records per window, enabled axes (bit a)
    // uniform grid over the clustered spheres and the listed other primitives (the grid walks, CULL == 5, 6, 7): 4 header
    // records, then the cells and their lists in the format of grid_wide; grid_cells == 0: the scene has no grid (nothing listed)
    int32_t off_grid, off_grid_cells, off_grid_items, grid_cells;
    int32_t grid_wide;       // 0: compact tables: 16-bit list entries, one 32-bit word per cell (first << 12 | n_near << 6 | n_all), up to 255
                             // cells per axis and 63 entries per cell (CULL == 5, 6; sphere-only scenes whose tables fit LDS).
                             // 1: wide tables: 32-bit list entries, two 32-bit words per cell {first entry, n_near | n_all << 10 |
                             // n_other << 20}, up to 1023 cells per axis, 1023 sphere entries per tier and 4095 other entries per cell
                             // (CULL == 7; scenes with other primitives or image textures, 65536 sphere slots or more, light
                             // sampling, or compact tables beyond the LDS budget)
    int32_t grid_sheet;      // 1: the grid is one cell high (ny == 1): the walk steps along x and z only (CULL == 6)
    int32_t hot_vec4_grid;   // float4 count of the hot part through the grid tables (what the grid-walk kernel stages)
    int32_t hot_vec4_tables; // float4 count of the hot part including the range tables (what the range-table kernel stages)
    float cull_extent1;      // 1 + max |coordinate| of the clustered spheres (per-lane box margin, see packer)
    int32_t hot_vec4;        // float4 count of the hot part without the range tables (LDS bytes / 16 of the other variants)
    int32_t off_rect_hot;    // float4 offsets inside the image
    int32_t off_cyl_hot;
    int32_t off_sph_cold;
    int32_t off_rect_cold;
    int32_t off_cyl_cold;
    int32_t off_mat;
    int32_t tiles_x;         // 8-pixel tile columns
    int32_t bands;           // 8-row bands in the shard
    int32_t num_items;       // work items = tiles_x * bands * num_chunks (one wave each)
    // light sampling (render_nee_kernel only; nl == 0: the scene has no LIGHT part)
    int32_t nl, off_light, off_alias, off_lslot;
    // environment map (the environment kernels only; env_rows == 0: none).  Offsets in fp32 WORDS of the image (rt_env.h: texels,
    // marginal CDF, conditional CDFs, texel solid angle per row, cos(theta) at the row borders)
    int32_t env_rows, env_cols;
    float env_scale, env_uoff;
    int32_t off_env_tex, off_env_marg, off_env_cond, off_env_band, off_env_ct;
    float env_sel;           // selection probability of the environment's entry in the light table (the last one); 0: not sampled
    // quads (grouped ids ns + nr + nc + nt ...) and the leading ones that are tested for every query.  Their hot and
    // cold records follow the triangles' (off_tri_hot + RT_TRI_STRIDE nt, off_tri_cold + 2 nt).  Last in the block: the
    // sphere-only kernels never read them, and every word in front of them stays where it was
    int32_t nq, nq_a;
};

struct DevCounters {
    unsigned long long samples, queries, prim_tests, hits, misses;
    unsigned long long scatter[4];
    unsigned long long rng_draws;
    unsigned long long cand_lanes, cand_waves;  // sphere candidates resolved: per lane / per wave entry
    unsigned long long clusters_visited;         // culling: clusters whose spheres were tested (per wave)
    unsigned long long groups_visited;           // culling: outer boxes that passed (per wave)
    unsigned long long lane_clusters, lane_groups;  // culling: boxes that passed, per lane
    unsigned long long t_start_min, t_start_max, t_end_min, t_end_max;  // s_memrealtime (100 MHz) of wave starts / exits
    unsigned long long life_cycles, life_ticks;  // per-wave lifetime in shader cycles (s_memtime) and 100 MHz ticks, summed
    unsigned long long t_qe_min, t_qe_max;  // when a wave first found the queue empty
    unsigned int drain_hist[32];            // waves by time from queue-empty to exit, 50 us bins
    unsigned long long occ_hist[2][17];     // wave-queries by live lanes (bins of 4; 16 = all 64), [0] while the queue has items, [1] after
    unsigned int qe_hist[1024];             // waves by time from their start to queue-empty, 64 us bins
    unsigned int exit_hist[1024];           // waves by time from their start to exit, 64 us bins
    unsigned long long cycles[6];  // shader-clock time per main-loop section, summed over waves
    unsigned long long group_maxpop, query_maxpop;  // culling: max over lanes of needed clusters, per visited group / per wave-query
    unsigned long long wave_queries;             // closest-hit queries executed per wave (loop iterations)
    unsigned long long lane_cands;               // range tables: candidate clusters per lane (before the box test)
    unsigned long long walk_resumed;             // grid: lanes that took up a walk cut short in the previous iteration
};

}  // namespace rtmi
