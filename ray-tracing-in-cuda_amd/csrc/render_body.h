// The body of the render kernels: included INSIDE render_kernel, render_nee_kernel, render_nested_kernel and render_feature_kernel
// (render_kernel.hip), render_env_kernel (render_env.hip), render_media_kernel (render_media.hip), media_nee_kernel
// (media_nee_kernel.hip: MEDIA and NEE together) and render_motion_kernel (render_motion.hip), after their template arguments and a constexpr NEE, AOV, ENV, MEDIA, MOTION and QUERY (with the TraceArgs
// TQ of render_device.h: null there), and inside trace_kernel (trace.hip), where QUERY is set.  The device functions it
// calls are render_device.h's, which each of those files includes.  As text rather than a force-inlined device function, so that the render_kernel
// instances compile to the very instructions they did before light sampling came (a device function that takes the
// kernel's parameters by reference changes the order of the kernel-argument loads and with it the register allocation).
// Not a header of its own: it needs the kernel's scope (P, image, acc, queue, counters and the template arguments).
    extern __shared__ float4 lds[];
    constexpr bool GRID = CULL == 5 || CULL == 6 || CULL == 7 || CULL == 8, SHEET = CULL == 6, WIDE = CULL == 7 || CULL == 8;
    constexpr bool NEST = CULL == 8;  // wide tables with nested cells (rt_scene_set_nested_grid)
    static_assert(!NEST || (SCALAR && !SPH), "the nested walk reads its tables from global memory, in the general builds");
    constexpr int CSIZE = RT_CLUSTER;
    static_assert(!(CULL == 5 || CULL == 6) || SPH, "the compact grid tables list spheres only");
    static_assert(!(SPH && EXT), "image textures and triangles come with the general builds");
    static_assert(!QUERY || (EXT && POOL && !COUNT && !NEE && !AOV && !ENV && !MEDIA && !MOTION), "a ray query is the general build's walk and winner, nothing else");
    // stage the hot tables (hittable_list contents) into LDS: each candidate search stages the part it reads
    // (the cluster searches leave the grid tables, which lie in front of their boxes, out: `gap` records)
    const int gap = (SCALAR || GRID) ? 0 : P.off_box - P.off_grid;
    const int staged = SCALAR ? 0 : (GRID ? P.hot_vec4_grid : (CULL == 3 ? P.hot_vec4_tables : P.hot_vec4) - gap);
    // (BIG, kernels.h: the sphere-only compact-table instances run kBigGroupWaves waves on one staged copy, two workgroups per
    //  CU; BURST: their paths start from a per-wave slab of 64 prepared camera rays -- the refill, below)
    constexpr bool BIG = big_group(COUNT, POOL, SCALAR, CULL, SPH) && !QUERY && !NEE && !AOV && !ENV && !MEDIA && !MOTION;
    constexpr bool BURST = BIG && burst_starts(COUNT, POOL, SCALAR, CULL, SPH);
    // (TRACE: the burst also runs the first closest-hit query of its 64 camera rays and settles the paths that end there;
    //  REPOP: a lane that pops a settled slot takes a following one in the same refill)
    constexpr bool TRACE = BURST && RT_BURST_TRACE != 0, REPOP = TRACE && RT_BURST_REPOP != 0;
    // (LISTS: the traced burst tests its tile's list of the beam table instead of running the prefix and the walk -- rt_beam.h,
    //  render_burst.h; the host hands the table's address over behind the item parameters, RT_BEAMS_AT)
    constexpr bool LISTS = TRACE && RT_BURST_LISTS != 0;
    // (the winner's id of a traced slot rides in the upper half of the home-row register, above a row of at most 65 535 and
    //  below the sign, in kBurstIdBits bits: a record of an LDS-resident table has an index below the CU's LDS / 16 --
    //  kernels.h; render_host.hip asserts the same of the packer's table bound)
    static_assert(kCuLdsBytes / 16 <= (size_t(1) << kBurstIdBits) && 16 + kBurstIdBits <= 31, "a staged sphere's id fits the bits above the row");
    constexpr int GW = BIG ? kBigGroupWaves : kGroupWaves;
    for (int i = threadIdx.x; i < staged; i += 64 * GW) lds[i] = image[i < P.off_grid ? i : i + gap];
    // per-wave tile accumulator of the current work item: 64 pixels x rgb, 64-bit fixed point
    unsigned long long *tile_acc = reinterpret_cast<unsigned long long *>(lds + staged);
    // (QUERY: a ray's record goes straight to memory: no accumulators, and no LDS reserved for them)
    if constexpr (!QUERY)
        for (int i = threadIdx.x; i < GW * 64 * 3; i += 64 * GW) tile_acc[i] = 0ull;
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;  // (wave: in a scalar register)
    unsigned long long *my_acc = tile_acc + wave * 192;
    // BURST: the wave's slab behind the accumulators, three arrays of 64 so that every read and write is one aligned
    // instruction over consecutive addresses: {p.xyz, d.x} {d.yz, g.xy} {g.zw} -- p the point where the camera ray hits a
    // surface that scatters (TRACE; without it o, the ray's origin).  A slot nobody continues from has a NaN in d.x: an
    // off-image pixel's, and with TRACE that of a path that ended in the burst (the sky, an emitter, the roulette).
    float4 *slab_a = lds + staged + GW * (kWaveAccBytes / 16) + (BURST ? wave * (kWaveSlabBytes / 16) : 0);
    float4 *slab_b = slab_a + 64;
    float2 *slab_c = reinterpret_cast<float2 *>(slab_a + 128);
    const uint32_t k0 = P.seed_lo, k1 = P.seed_hi;
    const float4 *hot = SCALAR ? image : lds;
    const float4 *sph = hot;
    const float4 *rect = hot + P.off_rect_hot;
    const float4 *cyl = hot + P.off_cyl_hot;
    const int ns = P.ns, nr = SPH ? 0 : P.nr, nc = SPH ? 0 : P.nc, nt = SPH ? 0 : P.nt;
    const float4 *tri = hot + P.off_tri_hot;
    // quads: the general builds alone.  Their records follow the triangles', hot and cold
    const int nq = EXT ? P.nq : 0;
    // original list index of a grouped primitive id (the tie rule)
    // (the sphere's cold record at a 32-bit byte offset, as the winner's is read: fewer than 2^28 slots, lay_out_image)
    auto lidx = [&](int id) { return SPH ? __float_as_int(rec_at(image + P.off_sph_cold, (uint32_t)id << 4)->z) : list_index_of(P, image, id); };
    // The wave's votes on a lane flag that was merged across branches -- any(active), ballot(enters), ballot(far_scan),
    // any(active || started) -- compile to v_cndmask 0 / 1 from the flag's lane mask and a v_cmp_ne back into one.  With
    // VOTE_MASKS the questions are asked of lane masks in scalar registers instead: a ballot straight from the compare that
    // decides the flag, combined with scalar and / and-not, and `inverse_ballot` where a lane-level `if` needs the flag.
    // (Not in the moving-sphere kernels: their spilled vector registers rose from 109 to 114 with it.  The refill's start
    // mask below is the same idea and holds for every family.)
    constexpr bool VOTE_MASKS = !MOTION;
    // rt_sqrtf's guard as a vote of the wave and its root from v_rsq_f32 (render_device.h).  (Not in the nested walk: with
    // triangles and textures its spilled vector registers rose from 86 to 97 with the vote.)
    constexpr bool ROOT_VOTE = !NEST;
    // u = (x + xi) / (W - 1), main.cu:96-97, evaluated as a multiply by the fp32 reciprocal (as the checker does)
    // (the two reciprocals come with the launch parameters: computed here they were vector registers, spilled to scratch and
    //  fetched back with two dependent scratch loads in every refill)

    uint32_t c_samples = 0, c_queries = 0, c_hits = 0, c_misses = 0;
    uint32_t c_scatter0 = 0, c_scatter1 = 0, c_scatter2 = 0, c_scatter3 = 0;
    uint32_t c_cand = 0, c_cand_wave = 0, c_clusters = 0, c_groups = 0, c_wave_queries = 0, c_lane_clusters = 0, c_lane_groups = 0, c_lane_cands = 0, c_group_maxpop = 0, c_query_maxpop = 0, c_walk_resumed = 0;
    // COUNT: shader-clock time of the main loop's sections, per wave (refill, prefix spheres, culled spheres +
    // rects + cylinders, shading, pixel accumulation, loop control)
    unsigned long long cyc[6] = {0, 0, 0, 0, 0, 0}, tmark = 0, t_qe = 0;
    auto tick = [&](int section) {
        if (COUNT) {
            const unsigned long long now = __builtin_amdgcn_s_memtime();
            cyc[section] += now - tmark;
            tmark = now;
        }
    };
    if (COUNT) tmark = __builtin_amdgcn_s_memtime();
    unsigned long long t_begin = 0, c_begin = 0;
    if (COUNT) t_begin = __builtin_amdgcn_s_memrealtime(), c_begin = __builtin_amdgcn_s_memtime();
    if (COUNT && lane == 0) {
        const unsigned long long t = t_begin;
        atomicMin(&counters->t_start_min, t);
        atomicMax(&counters->t_start_max, t);
    }

    // ---- persistent waves, streaming work items.  The grid only fills the chip; every wave pulls
    // (8x8 tile, sample chunk) work items from one global counter until it runs dry.  A wave does not
    // drain an item before taking the next: when the pool of the current item is handed out and a lane
    // is idle, the item's tile accumulator (LDS) is flushed and the paths still alive finish as ORPHANS
    // that add their sample straight to the global accumulators (integer sums: any split of an item's
    // additions gives the same total).  So lanes only idle at the very end of the launch, and items can
    // be short.  From here on the four waves of the workgroup never synchronise again.
    unsigned long long *c_acc = my_acc;  // accumulator of the current item (wave-uniform pointer)
    int c_x0 = 0, c_band = 0, c_sbegin = 0, c_pool = 0, cursor = 0;  // c_pool = 64 x samples of the item
    bool c_valid = false, queue_empty = false;
    [[maybe_unused]] int slab_for = -1;  // TRACE: the batch of the current item that the slab holds (-1: none)
    int c_hy = 0, c_hvalid = 0;  // this lane's home pixel in the current item (row, on-image; POOL: the row is -1 off-image)
    int mine = 0;                // !POOL: samples of the home pixel started so far (current item)

    // home pixel of this lane in the tile (x0, band): column, dense local row, image row, on-image
    // item-level launch values, read where they are needed (device_scene.h, ItemParams): wave-uniform
    // 16-byte loads behind a compiler barrier, so that they are neither hoisted out of the main loop (and
    // then spilled) nor kept in registers between items
    auto ipar4 = [&](int quad) {
        asm volatile("" ::: "memory");
        return reinterpret_cast<const int4 *>(queue + RT_ITEM_PARAMS_AT)[quad];
    };
    auto home_pixel = [&](int x0, int band, int &hx, int &hlr, int &hy, int &hvalid) {
        const int4 g = ipar4(3);  // {tile_rows, tile_first, tile_stride, local_rows}
        const int tile_rows = g.x, tile_first = g.y, tile_stride = g.z, local_rows = g.w;
        const int tile_rotate = ipar4(2).z;
        hx = x0 + (lane & 7);
        hlr = band * 8 + (lane >> 3);
        const int htl = hlr / tile_rows;
        const int tile = shard_tile<int>(tile_first, tile_stride, tile_rotate, htl);
        hy = tile * tile_rows + (hlr - htl * tile_rows);
        hvalid = (hx < P.width && hlr < local_rows && hy < P.height) ? 1 : 0;
    };
    // tile accumulator -> global accumulators (image[y*W + x] += res, main.cu:104; other sample chunks of the same
    // pixels are other work items, hence atomics), then clear it for reuse.  The tile's 192 sums lie in LDS as
    // [row][column][channel], which is also the order of a tile row in the global plane (24 consecutive 64-bit
    // words): lane l adds the words l, 64 + l and 128 + l, so one instruction covers 512 contiguous bytes of LDS and
    // 2 2/3 tile rows of 192 contiguous bytes in memory (the atomics execute memory-side in 64-byte requests: with
    // one pixel per lane -- 24 bytes apart -- every request carried 8 useful bytes).  Words that are zero are
    // skipped: black samples, and the pixels of a ragged tile outside the image or the shard, which never receive a
    // sample -- so no bounds logic is needed here.
    auto flush_tile = [&](unsigned long long *tile, int x0, int band) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int k = j * 64 + lane;
            const unsigned long long v = tile[k];
            if (v != 0ull) {
                const int row = k / 24, rem = k - row * 24;
                atomicAdd(acc + ((size_t)(band * 8 + row) * P.width + x0) * 3 + rem, v);
                tile[k] = 0ull;
            }
        }
        __builtin_amdgcn_wave_barrier();
    };

    LaneRng rng;
    rng.g.x = rng.g.y = rng.g.z = 0u, rng.g.w = 1u, rng.draws = 0;

    float ox = 0, oy = 0, oz = 0, dx = 0, dy = 0, dz = 1, ra = 1, rinv_a = 1;
    // (no radiance accumulator: in this integrator a path collects radiance exactly once, in the event that ends it -- the sky
    //  or the background on a miss, main.cpp:36-38 / main.cu:63, or an emitter, which never scatters, main.cu:48-58 -- so
    //  ray_color's accumulated colour is throughput x that event's radiance, and a path that is absorbed, runs out of depth
    //  or loses the roulette contributes exactly zero: nothing to add)
    float beta_r = 1, beta_g = 1, beta_b = 1;
    int depth = 0;
    // NEE: pdf of the BSDF sample that made the current ray (< 0: its vertex took no light sample, an emitter it hits keeps
    // weight 1); the shadow phase (0: none, 1: a shadow query, then the continuation, 2: a shadow query, then the path ends);
    // the continuation's direction while the shadow ray is out, and the light sample's contribution if nothing occludes it
    float mis_pdf = -1.0f;
    int shadow = 0;
    float cdx = 0, cdy = 0, cdz = 0, pend_r = 0, pend_g = 0, pend_b = 0;
    // MOTION: the shutter time of the lane's sample (rt_motion.h), set where the sample starts and kept for the life of its path
    float mot_s = 0.0f;
    // ALPHA (alpha cutouts, DESIGN 7v, rt_alpha.h; a constant of the including kernel, true in the instances of alpha_kernel.h
    // alone, which the host picks for a scene with masks): a winner whose material carries a mask and whose texel is transparent
    // is no vertex -- the lane's query starts again from the hit point.  What a query keeps while it passes through holes: how
    // many (at most RT_ALPHA_MAX_PASSES), the ray parameter covered so far, and the origin it set out from, which comes back
    // with the query's verdict (a shadow ray's continuation, an emitter's pdf, a glass segment and the depth feature all
    // measure from there).  All zero between queries.  The five words live in LDS, behind the accumulators, in five arrays of
    // one word per lane (kAlphaLdsBytes, kernels.h: the launch of such an instance adds them).
    static_assert(!ALPHA || (EXT && !QUERY && !MEDIA), "masks come with the general builds, and not with media");
    constexpr bool has_alpha = ALPHA;
    static_assert(!ALPHA || 5 * 4 * 64 * GW == kAlphaLdsBytes, "the alpha state is five words per lane of the workgroup");
    constexpr int AL_T = 64 * GW, AL_OX = 2 * AL_T, AL_OY = 3 * AL_T, AL_OZ = 4 * AL_T;  // (the pass count: word 0)
    float *al_state = reinterpret_cast<float *>(lds + staged + GW * (kWaveAccBytes / 16)) + threadIdx.x;
    if constexpr (ALPHA) {
        if (has_alpha) al_state[0] = __int_as_float(0), al_state[AL_T] = 0.0f;
    }
    // CAMERA (camera projections): the path start of section 6b alone; such an instance starts paths lane by lane
    static_assert(!CAMERA || (EXT && POOL && !QUERY && !COUNT && !BURST && !ALPHA), "projections come with the general builds, and not with masks");
    const int *lslot = reinterpret_cast<const int *>(image + P.off_lslot);
    // ENV: the environment's tables (rt_env.h), built where they are used from launch values (wave-uniform)
    auto env_view = [&]() -> EnvView {
        const float *w = reinterpret_cast<const float *>(image);
        return EnvView{w + P.off_env_tex, w + P.off_env_marg, w + P.off_env_cond, w + P.off_env_band, w + P.off_env_ct,
                       P.env_rows, P.env_cols, P.env_scale, P.env_uoff};
    };
    // where this lane's live path adds its sample: >= 0 the tile-local pixel (0 .. 63) in the current item's accumulator; < 0 the
    // path outlived its item (an orphan): ~cur_p is its dense local pixel index for a direct global add
    int cur_p = lane;
    bool active = false;

    // One iteration of the main loop:
    //   (1) closest-hit query of every live lane              hittable_list::hit
    //   (2) hit record + material of the winner; a miss or an emitter ends the path here
    //   (3) pixel accumulation of the paths that ended
    //   (4) refill: idle lanes take the next (pixel, sample) of the tile's pool, seed their stream, draw the jitter
    //   (5) ONE rejection loop for both kinds of lanes: random_in_unit_sphere for the scatter step of a lambertian /
    //       metal hit (three draws per attempt) and random_in_unit_disk for the lens sample of a new path (two)
    //   (6) the scatter step (lambertian / metal / dielectric) | the camera ray, then what both share: |d|^2, 1 / |d|^2
    // The loops of (5) cost max-over-lanes attempts each; as two loops (one inside the refill, one inside the shading)
    // they took 13 % of the frame (measured by cutting them out).
    // CULL == 5: ray parameter at which this lane's grid walk was cut short in the previous iteration (0: it was not);
    // the walk goes on from there in this one
    float t_res = 0.0f;
    // QUERY: the ray this lane traces, and its t_max: the best_t its query starts from -- and starts from again when its walk was
    // cut short.  A record is three 16-byte stores (rt_hit), or one byte in occlusion mode.
    uint32_t q_ray = 0u;
    float q_tmax = INFINITY;
    auto put_record = [&](uint32_t ray, float t, int prim, int material, int is_front, float rnx, float rny, float rnz, float ru,
                          float rpx, float rpy, float rpz, float rv) {
        if (TQ.mode != 0) {
            reinterpret_cast<uint8_t *>(TQ.out)[ray] = prim >= 0 ? (uint8_t)1 : (uint8_t)0;
        } else {
            float4 *rec = TQ.out + (size_t)ray * 3;
            rec[0] = make_float4(t, __int_as_float(prim), __int_as_float(material), __int_as_float(is_front));
            rec[1] = make_float4(rnx, rny, rnz, ru);
            rec[2] = make_float4(rpx, rpy, rpz, rv);
        }
    };
    for (;;) {
        if constexpr (TRACE) {
            // the traced burst sits at the top of the iteration, when the slab does not hold the batch the cursor stands in and the pool
            // is not handed out: here a path's state is its ray, throughput, depth, pixel and generator -- no hit record of
            // a lane that awaits its scatter step is live across the burst's query
            if (c_valid && cursor < c_pool && (cursor >> 6) != slab_for) {
                __builtin_amdgcn_wave_barrier();
#include "render_burst.h"
                __builtin_amdgcn_wave_barrier();
                slab_for = cursor >> 6;
            }
        }
        tick(5);
        bool path_done = false;
        bool nee_add = false;  // NEE: a light sample that reached its light adds L (the path goes on)
        float L_r = 0, L_g = 0, L_b = 0;  // the sample of a path that ends in this iteration
        asm volatile("" : "=v"(L_r), "=v"(L_g), "=v"(L_b));  // (read by the lanes with path_done, which set them)
        // the winner's hit record, kept for the scatter step
        float px = 0, py = 0, pz = 0, nx = 0, ny = 0, nz = 0, inv_len = 0;
        int mat = 0, kind = -1;  // kind >= 0: a scatter step is due in (6)
        // (only lanes with kind >= 0 read the record, and they have written it; an "undefined" value from an empty asm
        //  spares the eight v_mov ..., 0 per iteration that the zero initialisers above cost)
        asm volatile("" : "=v"(px), "=v"(py), "=v"(pz), "=v"(nx), "=v"(ny), "=v"(nz), "=v"(inv_len), "=v"(mat));
        bool front = false;
        float tex_r = 0, tex_g = 0, tex_b = 0;  // the texel of an image texture at the hit's (u, v)
        // (VOTE_MASKS: no vote here.  Everything below sits behind `if (active)`, whose own branch on an empty exec mask skips
        //  it when no lane is live; the vote in front of it was two vector instructions per iteration for the same answer.)
        if (VOTE_MASKS || __any(active)) {
        {
#define RT_QUERY_CUT true
#define RT_QUERY_SKIP false
#include "render_query.h"
#undef RT_QUERY_SKIP
#undef RT_QUERY_CUT
            if (active) {
#undef RT_SPHERE_TEST

            // ---- rectangles, cylinders and triangles that are tested for every query: all of them in the searches without a grid
            // (the reference's loop), the oversized ones in the grid kernels -- plus, for a lane whose origin lies beyond the reach
            // of the cells' lists (far_scan), the listed ones as well
            if (!SPH) {
                const bool any_far = GRID && (VOTE_MASKS ? far_m != 0ull : __builtin_amdgcn_ballot_w64(far_scan) != 0ull);
                const int nr_loop = (GRID && !any_far) ? P.nr_a : nr, nc_loop = (GRID && !any_far) ? P.nc_a : nc;
                const int nt_loop = EXT ? ((GRID && !any_far) ? P.nt_a : nt) : 0;
                for (int j = 0; j < nr_loop; ++j)
                    if (!GRID || j < P.nr_a || far_scan) test_rect(j);
                // the boxes of cylinders and triangles: the box-test values once more (see box_params)
                BoxP bq = {};
                const int nq_loop = EXT ? ((GRID && !any_far) ? P.nq_a : nq) : 0;
                if (CULL && (nc_loop > 0 || nt_loop > 0 || nq_loop > 0)) bq = box_params();
                for (int k = 0; k < nc_loop; ++k) {
                    const bool mine = !GRID || k < P.nc_a || far_scan;
                    if (CULL) {
                        blim = best_t * 1.0001f;  // the cylinder's world-space box, same margin (the object-space quadratic has the
                                 // same error structure as the sphere test: ~1e-3 |o| in space)
                        const float4 *cb = cyl + RT_CYL_STRIDE * k + 4;
                        if (__builtin_amdgcn_ballot_w64(mine && slab_live(bq, cb[0], cb[1])) == 0ull) continue;
                    }
                    if (mine) test_cyl(k);
                }
                for (int k = 0; k < nt_loop; ++k) {
                    const bool mine = !GRID || k < P.nt_a || far_scan;
                    if (CULL) {
                        blim = best_t * 1.0001f;
                        const float4 *tb = tri + RT_TRI_STRIDE * k + 3;
                        if (__builtin_amdgcn_ballot_w64(mine && slab_live(bq, tb[0], tb[1])) == 0ull) continue;
                    }
                    if (mine) test_tri(k);
                }
                if constexpr (EXT) {
                    for (int k = 0; k < nq_loop; ++k) {
                        const bool mine = !GRID || k < P.nq_a || far_scan;
                        if (CULL) {
                            blim = best_t * 1.0001f;
                            const float4 *tb = tri + RT_TRI_STRIDE * nt + RT_QUAD_STRIDE * k + 3;
                            if (__builtin_amdgcn_ballot_w64(mine && slab_live(bq, tb[0], tb[1])) == 0ull) continue;
                        }
                        if (mine) test_quad(k);
                    }
                }
            }
            // (a lane whose grid walk was cut short has no result yet: its query goes on in the next iteration)
            const bool unfinished = GRID && t_res != 0.0f;
            if (COUNT) {
                if (!unfinished) c_queries++;
                const unsigned long long alive = __builtin_amdgcn_ballot_w64(true);
                if ((int)__builtin_ctzll(alive) == lane) {
                    c_wave_queries++;
                    atomicAdd(&counters->occ_hist[queue_empty ? 1 : 0][__popcll(alive) >> 2], 1ull);
                }
            }

            tick(2);
            // ---- (2) the winner (ray_color body, main.cu:45-65 / main.cpp:22-38)
            // 1/|d| once per query (metal, dielectric and the sky all normalise the direction)
            inv_len = 1.0f / rt_sqrtf<ROOT_VOTE>(ra);
            // MEDIA: the media walk of a finished query.  The media -- records behind a count and an offset in the camera
            // block, all wave-uniform reads from global memory -- in list order: the ray's stay [a, b] inside the boundary up to
            // the surface winner; a non-empty stay in a medium of positive density takes ONE draw, the free-flight distance.
            // The smallest event wins over the surface hit.  What outlives the walk: med_t, med_i and the winner's asymmetry med_g
            // (.w of its record 2, which the walk reads anyway; 0: the isotropic medium).
            // MEDIA && NEE: a lane in its shadow phase draws nothing and proposes no event -- each non-empty stay adds its
            // optical depth sigma (b - a) |d| to tau, which lives where med_t lives (0 before the walk); lanes of both kinds share
            // the trip through the loop and its wave-uniform record loads
            float med_t = INFINITY;
            int med_i = -1;
            float med_g = 0.0f;
            bool med_sh = false;
            if constexpr (MEDIA && NEE) {
                med_sh = shadow != 0;
                if (med_sh) med_t = 0.0f;
            }
            if constexpr (MEDIA) {
                if (!unfinished) {
                    const int n_med = __builtin_amdgcn_readfirstlane(__float_as_int(image[P.off_cam + 1].w));
                    const float4 *med = image + __builtin_amdgcn_readfirstlane(__float_as_int(image[P.off_cam + 2].w));
                    const float len = rt_sqrtf<ROOT_VOTE>(ra);
                    for (int m = 0; m < n_med; ++m) {
                        const float4 g0 = med[RT_MEDIUM_STRIDE * m], g1 = med[RT_MEDIUM_STRIDE * m + 1], g2 = med[RT_MEDIUM_STRIDE * m + 2];
                        float ta, tb;
                        if (g1.w > 0.0f &&
                            medium_interval(__float_as_int(g2.z), g0.x, g0.y, g0.z, g0.w, g2.x, g2.y, ox, oy, oz, dx, dy, dz, best_t, ta, tb)) {
                            if (MEDIA && NEE && med_sh) {
                                med_t = medium_tau_add(g1.w, ta, tb, len, med_t);
                                continue;
                            }
                            const float u = rng_next<COUNT>(rng);
                            const float t = ta + (-logf(1.0f - u) / g1.w) / len;
                            if (t < tb && t < med_t) med_t = t, med_i = m, med_g = g2.w;
                        }
                    }
                }
            }
            // MOTION: the moving spheres of a finished query.  The movers -- records behind a count and an offset in the
            // camera block, all wave-uniform reads from global memory -- in list order, each at the lane's shutter time, against
            // what the query has found so far: a mover behaves as a sphere listed behind every static primitive (a root equal
            // to the winner's takes over, the later mover wins a tie among movers).  What outlives the loop: best_t and mot_i.
            int mot_i = -1;
            if constexpr (MOTION) {
                if (!unfinished) {
                    const int n_mot = __builtin_amdgcn_readfirstlane(__float_as_int(image[P.off_cam + 3].w));
                    const float4 *mot = image + __builtin_amdgcn_readfirstlane(__float_as_int(image[P.off_cam + 4].w));
                    for (int m = 0; m < n_mot; ++m) {
                        const float4 g0 = mot[RT_MOTION_STRIDE * m], g1 = mot[RT_MOTION_STRIDE * m + 1];
                        float t;
                        if (moving_sphere_hit(g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, mot_s, ox, oy, oz, dx, dy, dz, ra, rinv_a, best_t, t))
                            best_t = t, mot_i = m;
                    }
                }
            }
            // the shadow query's verdict (CLEAR: nothing lies between the vertex and its light point): the light sample counts or is
            // lost, then the continuation comes back (or, behind an absorbed metal vertex, the path ends).  One text for its two
            // places -- here, and in the winner's branch of the alpha kernels, where an occluder may be a hole; as text
            // and not as a lambda, which changed the register allocation of every instance
#define RT_SHADOW_VERDICT(CLEAR)                                        \
    {                                                                   \
        nee_add = (CLEAR);                                              \
        L_r = pend_r, L_g = pend_g, L_b = pend_b;                       \
        if ((ENV ? (shadow & 3) : shadow) == 2) active = false;         \
        dx = cdx, dy = cdy, dz = cdz;                                   \
        ra = dot3(dx, dy, dz, dx, dy, dz);                              \
        rinv_a = 1.0f / ra;                                             \
        shadow = 0;                                                     \
    }
            if (unfinished) {
            } else if (NEE && shadow != 0 && !(ALPHA && has_alpha && best_id >= 0)) {
                // the shadow query's verdict: the light sample counts when nothing lies between the vertex and its light
                // point; then the continuation comes back (or, behind an absorbed metal vertex, the path ends)
                // (ALPHA: in a scene with masks an occluder may be a hole: such a lane takes the winner's branch below, which
                //  needs the hit's material and (u, v), and its verdict there.  A ray that got here through holes starts its
                //  continuation from the vertex it left)
                if constexpr (ALPHA) {
                    if (has_alpha) {
                        if (__float_as_int(al_state[0]) != 0) ox = al_state[AL_OX], oy = al_state[AL_OY], oz = al_state[AL_OZ];
                        al_state[0] = __int_as_float(0), al_state[AL_T] = 0.0f;
                    }
                }
                RT_SHADOW_VERDICT(best_id < 0)
                // MEDIA: what the media between the vertex and its light point let through; tau = 0: exactly 1
                if constexpr (MEDIA && NEE) {
                    const float T = media_transmittance(med_t);
                    L_r *= T, L_g *= T, L_b *= T;
                }
            } else if (MEDIA && med_i >= 0) {
                // a medium event: a vertex without a normal and without a material record (the scatter step takes the albedo
                // from the medium's record), which emits nothing.  Where a surface vertex keeps its normal's x, a medium vertex
                // keeps its medium's asymmetry: 0 -- the normal n = 0 of the isotropic medium -- or g != 0, which the
                // rejection loop (5) and the scatter step (6a) ask, and nothing else reads
                px = fmaf(med_t, dx, ox), py = fmaf(med_t, dy, oy), pz = fmaf(med_t, dz, oz);
                nx = med_g, ny = nz = 0.0f;
                mat = med_i;
                kind = MK_MEDIUM;
            } else if (best_id >= 0 || (MOTION && mot_i >= 0)) {
                // hit record of the winner only (the reference fills one per candidate)
                if (MOTION && mot_i >= 0) {  // a moving sphere: the static sphere's record about the centre at the shutter time
                    const float4 *g = image + __builtin_amdgcn_readfirstlane(__float_as_int(image[P.off_cam + 4].w)) + RT_MOTION_STRIDE * mot_i;
                    const float4 g0 = g[0], g1 = g[1], g2 = g[2];
                    const float cx = fmaf(mot_s, g1.x, g0.x), cy = fmaf(mot_s, g1.y, g0.y), cz = fmaf(mot_s, g1.z, g0.z);
                    px = fmaf(best_t, dx, ox), py = fmaf(best_t, dy, oy), pz = fmaf(best_t, dz, oz);
                    const float onx = g1.w * (px - cx), ony = g1.w * (py - cy), onz = g1.w * (pz - cz);
                    front = dot3(dx, dy, dz, onx, ony, onz) < 0.0f;
                    nx = front ? onx : -onx, ny = front ? ony : -ony, nz = front ? onz : -onz;
                    mat = __float_as_int(g2.x);
                    kind = __float_as_int(g2.y);
                } else if (SPH || best_id < ns) {
                    const float4 s = sph[best_id];
                    const float4 cold = *rec_at(image + P.off_sph_cold, (uint32_t)best_id << 4);  // (fewer than 2^28 slots: lay_out_image)
                    px = fmaf(best_t, dx, ox), py = fmaf(best_t, dy, oy), pz = fmaf(best_t, dz, oz);
                    const float onx = cold.x * (px - s.x), ony = cold.x * (py - s.y), onz = cold.x * (pz - s.z);
                    front = dot3(dx, dy, dz, onx, ony, onz) < 0.0f;
                    nx = front ? onx : -onx, ny = front ? ony : -ony, nz = front ? onz : -onz;
                    mat = __float_as_int(cold.y);
                    kind = __float_as_int(cold.w);
                } else if (best_id < ns + nr) {
                    const int j = best_id - ns;
                    const int axis = __float_as_int(rect[2 * j + 1].y);
                    px = fmaf(best_t, dx, ox), py = fmaf(best_t, dy, oy), pz = fmaf(best_t, dz, oz);
                    const float dk = axis == 0 ? dz : (axis == 1 ? dy : dx);
                    front = dk < 0.0f;
                    // front ? (0,0,1) : -(0,0,1), zeros keep their sign as in the reference
                    const float sgn = front ? 1.0f : -1.0f, zer = front ? 0.0f : -0.0f;
                    nx = axis == 2 ? sgn : zer, ny = axis == 1 ? sgn : zer, nz = axis == 0 ? sgn : zer;
                    const float4 rc = image[P.off_rect_cold + j];
                    mat = __float_as_int(rc.x);
                    kind = __float_as_int(rc.z);
                } else if (best_id < ns + nr + nc) {
                    const int k = best_id - ns - nr;
                    const float4 r0 = cyl[RT_CYL_STRIDE * k], r1 = cyl[RT_CYL_STRIDE * k + 1], r2 = cyl[RT_CYL_STRIDE * k + 2];
                    const float4 *cc4 = image + P.off_cyl_cold + 4 * k;
                    const float4 m0 = cc4[0], m1 = cc4[1], m2 = cc4[2];
                    const float oox = fmaf(r0.x, ox, fmaf(r0.y, oy, fmaf(r0.z, oz, r0.w)));
                    const float ooy = fmaf(r1.x, ox, fmaf(r1.y, oy, fmaf(r1.z, oz, r1.w)));
                    const float ooz = fmaf(r2.x, ox, fmaf(r2.y, oy, fmaf(r2.z, oz, r2.w)));
                    const float odx = fmaf(r0.x, dx, fmaf(r0.y, dy, r0.z * dz));
                    const float ody = fmaf(r1.x, dx, fmaf(r1.y, dy, r1.z * dz));
                    const float odz = fmaf(r2.x, dx, fmaf(r2.y, dy, r2.z * dz));
                    const float opx = fmaf(best_t, odx, oox), opy = fmaf(best_t, ody, ooy), opz = fmaf(best_t, odz, ooz);
                    const float len = rt_sqrtf<ROOT_VOTE>(fmaf(opx, opx, opy * opy));
                    const float onx = opx / len, ony = opy / len;
                    px = fmaf(m0.x, opx, fmaf(m0.y, opy, fmaf(m0.z, opz, m0.w)));
                    py = fmaf(m1.x, opx, fmaf(m1.y, opy, fmaf(m1.z, opz, m1.w)));
                    pz = fmaf(m2.x, opx, fmaf(m2.y, opy, fmaf(m2.z, opz, m2.w)));
                    const float wnx = fmaf(r0.x, onx, r1.x * ony);
                    const float wny = fmaf(r0.y, onx, r1.y * ony);
                    const float wnz = fmaf(r0.z, onx, r1.z * ony);
                    front = dot3(dx, dy, dz, wnx, wny, wnz) < 0.0f;
                    nx = front ? wnx : -wnx, ny = front ? wny : -wny, nz = front ? wnz : -wnz;
                    mat = __float_as_int(cc4[3].x);
                    kind = __float_as_int(cc4[3].z);
                } else if (EXT) {  // triangle, taichi-version/hittable.py:254-259: the stored unit normal, turned against the ray
                    const int k = best_id - ns - nr - nc;
                    const float tnx = tri[RT_TRI_STRIDE * k].w, tny = tri[RT_TRI_STRIDE * k + 1].w, tnz = tri[RT_TRI_STRIDE * k + 2].w;
                    px = fmaf(best_t, dx, ox), py = fmaf(best_t, dy, oy), pz = fmaf(best_t, dz, oz);
                    front = dot3(dx, dy, dz, tnx, tny, tnz) < 0.0f;
                    nx = front ? tnx : -tnx, ny = front ? tny : -tny, nz = front ? tnz : -tnz;
                    mat = __float_as_int(image[P.off_tri_cold + 2 * k].x);
                    kind = __float_as_int(image[P.off_mat + 3 * mat].x);
                }
                // (the material kind rides in the primitive's cold record: one dependent load, not two)
                const float4 *M = image + P.off_mat + 3 * mat;
                // a noise texture (rt_noise.h): a solid texture, evaluated here at the hit point the checker reads and
                // left where an image's texel is left.  From here on the vertex IS the image-textured one of its material --
                // scatter, emitter, albedo feature, the counters and every ordered comparison of kinds see the kind they know --
                // except plastic, whose light sample needs the colour again (step (7) evaluates it again from the same point).
                // (Its value is formed further down, behind the (u, v): here the vertex only learns what it is.)
                // The metallic-roughness material (rt_pbr.h) has two textures of any type: its base colour in the
                // material's own rows and its map in the rows of a side record.  pbr_t: base type | map type << 4 (-1: not pbr)
                bool noise_tex = false;
                int pbr_t = -1;
                if constexpr (EXT && !QUERY) {
                    if (kind == MK_PBR) pbr_t = __float_as_int(M[0].w);
                    if (kind >= MK_LAMBERT_NOISE && kind <= MK_PLASTIC_NOISE) {  // (rough glass, above them, has no texture)
                        noise_tex = true;
                        if (kind != MK_PLASTIC_NOISE) kind = kind == MK_LAMBERT_NOISE ? MK_LAMBERT_IMAGE : MK_LIGHT_IMAGE;
                    }
                }
                const bool pbr_uv = EXT && !QUERY && pbr_t >= 0 && ((pbr_t & 15) == 2 || (pbr_t >> 4) == 2);
                // the hit record's (u, v) -- only where the material's texture reads them (an image texture); every
                // other texture of the reference ignores them, and acos / atan2 per candidate hit (object.cuh:87-93)
                // would be the most expensive part of sphere::hit
                // (QUERY: for every hit, they are part of the record)
                // (and where the material carries a normal map, DESIGN 7u: a negative word where a bump's record offset sits)
                // (has_maps: a bit of the parameter block, so a scene without maps takes one scalar branch around all of it)
                bool nmap_uv = false;
                const bool has_maps = EXT && !QUERY && (P.flags & RT_PFLAG_NORMAL_MAPS) != 0u;
                if constexpr (EXT && !QUERY) {
                    if (has_maps) nmap_uv = __float_as_int(M[2].w) < 0 && !(MOTION && mot_i >= 0);
                }
                // (and where the material carries an alpha mask, DESIGN 7v: its record {texel word offset, rows, cols, c8} stands
                //  behind the material table, at off_mat + 3 nm + material, rows = 0: none.  A query that has used up its passes reads no mask: the hit is opaque.
                //  al_shadow: a shadow ray came here only to learn whether its occluder is a hole -- nothing else of the hit is formed)
                bool al_mask = false, al_pass = false;
                float4 al_rec = {0.0f, 0.0f, 0.0f, 0.0f};
                const bool al_shadow = ALPHA && NEE && shadow != 0;
                if constexpr (ALPHA) {
                    if (has_alpha && !(MOTION && mot_i >= 0)) {
                        al_rec = image[P.off_mat + 3 * P.nm + mat];
                        al_mask = __float_as_int(al_rec.y) != 0 && __float_as_int(al_state[0]) < RT_ALPHA_MAX_PASSES;
                    }
                }
                const bool want_uv = EXT && (al_shadow ? al_mask : (QUERY || pbr_uv || nmap_uv || al_mask || (!noise_tex && (kind == MK_LAMBERT_IMAGE || kind == MK_LIGHT_IMAGE || kind == MK_PLASTIC_IMAGE))));
                // a triangle's area weights (hittable.py:54-58), stated once: of the plane point for (u, v), and -- smooth shading,
                // DESIGN 7l -- of the vertex normals.  The NORMALS part (device_scene.h) is there only when the scene has a triangle
                // with vertex normals: where it lies is a wave-uniform word of the camera block, as for the media and the movers.
                // The shading normal replaces the face-turned geometric one where the material scatters, in a query's record and
                // in a feature pass; an emitter keeps the geometric normal (its light pdf below reads nx, ny, nz).
                float w1 = 0.0f, w2 = 0.0f, w3 = 0.0f;
                if constexpr (EXT) {
                    if (!(MOTION && mot_i >= 0) && best_id >= ns + nr + nc) {
                        const int k = best_id - ns - nr - nc;
                        const int off_nrm = __builtin_amdgcn_readfirstlane(__float_as_int(image[P.off_cam + 5].w));
                        bool smooth = false;
                        if (k >= nt) {
                            // a quad: no vertex normals; its (u, v) are the coordinates (a, b) of the hit point, left
                            // where the triangle's first two weights are left
                            if (want_uv) {
                                const float4 *qr = tri + RT_TRI_STRIDE * k;  // (one table: the quads follow the triangles)
                                const float4 r0 = qr[0], r1 = qr[1], r2 = qr[2];
                                quad_uv(r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r2.x, r2.y, r2.z, px, py, pz, w1, w2);
                            }
                        } else
                        if (off_nrm != 0 && (QUERY || AOV || kind < MK_LIGHT_SOLID || kind >= MK_ROUGH_METAL)) smooth = __float_as_int(image[off_nrm + 3 * k].w) != 0;
                        if (k < nt && (want_uv || smooth)) {
                            const float4 r0 = tri[RT_TRI_STRIDE * k], r1 = tri[RT_TRI_STRIDE * k + 1], r2 = tri[RT_TRI_STRIDE * k + 2];
                            float rix, riy, riz, root;
                            tri_plane(r0, r1, r2, rix, riy, riz, root);
                            const float a1x = rix - r0.x, a1y = riy - r0.y, a1z = riz - r0.z;
                            const float a2x = rix - r1.x, a2y = riy - r1.y, a2z = riz - r1.z;
                            const float a3x = rix - r2.x, a3y = riy - r2.y, a3z = riz - r2.z;
                            float cx, cy, cz, ex, ey, ez;
                            cross3(a1x, a1y, a1z, a2x, a2y, a2z, cx, cy, cz);
                            cross3(r2.x - r0.x, r2.y - r0.y, r2.z - r0.z, r2.x - r1.x, r2.y - r1.y, r2.z - r1.z, ex, ey, ez);
                            w1 = rt_sqrtf<ROOT_VOTE>(dot3(cx, cy, cz, cx, cy, cz)) / rt_sqrtf<ROOT_VOTE>(dot3(ex, ey, ez, ex, ey, ez));
                            cross3(a1x, a1y, a1z, a3x, a3y, a3z, cx, cy, cz);
                            cross3(r1.x - r0.x, r1.y - r0.y, r1.z - r0.z, r1.x - r2.x, r1.y - r2.y, r1.z - r2.z, ex, ey, ez);
                            w2 = rt_sqrtf<ROOT_VOTE>(dot3(cx, cy, cz, cx, cy, cz)) / rt_sqrtf<ROOT_VOTE>(dot3(ex, ey, ez, ex, ey, ez));
                            cross3(a3x, a3y, a3z, a2x, a2y, a2z, cx, cy, cz);
                            cross3(r0.x - r2.x, r0.y - r2.y, r0.z - r2.z, r0.x - r1.x, r0.y - r1.y, r0.z - r1.z, ex, ey, ez);
                            w3 = rt_sqrtf<ROOT_VOTE>(dot3(cx, cy, cz, cx, cy, cz)) / rt_sqrtf<ROOT_VOTE>(dot3(ex, ey, ez, ex, ey, ez));
                        }
                        if (smooth) {
                            // each corner's normal by the area of the sub-triangle OPPOSITE that corner (the barycentric weight
                            // that is 1 at the corner): w1 is (r, v1, v2) over the whole and goes with n3, w2 is (r, v1, v3) and
                            // goes with n2, w3 is (r, v3, v2) and goes with n1.  (u, v) above keeps the reference's pairing, u1
                            // with w1: under that pairing a normal would be n3 at v1 and jump across every edge.)  Normalised,
                            // turned into the geometric normal's hemisphere; zero or not finite: the geometric normal stays
                            const float4 *nr3 = image + off_nrm + 3 * k;
                            const float4 n1 = nr3[0], n2 = nr3[1], n3 = nr3[2];
                            const float sx = fmaf(n1.x, w3, fmaf(n2.x, w2, n3.x * w1));
                            const float sy = fmaf(n1.y, w3, fmaf(n2.y, w2, n3.y * w1));
                            const float sz = fmaf(n1.z, w3, fmaf(n2.z, w2, n3.z * w1));
                            const float l2 = dot3(sx, sy, sz, sx, sy, sz);
                            if (l2 > 0.0f && l2 < INFINITY) {
                                const float inv = 1.0f / rt_sqrtf<ROOT_VOTE>(l2);
                                const float ux = inv * sx, uy = inv * sy, uz = inv * sz;
                                const bool turn = dot3(ux, uy, uz, nx, ny, nz) < 0.0f;
                                nx = turn ? -ux : ux, ny = turn ? -uy : uy, nz = turn ? -uz : uz;
                            }
                        }
                    }
                }
                float tu = 0.0f, tv = 0.0f;
                if (want_uv) {
                    if ((MOTION && mot_i >= 0) || best_id < ns) {  // get_sphere_uv(outward_normal), object.cuh:87-93
                        const float onx = front ? nx : -nx, ony = front ? ny : -ny, onz = front ? nz : -nz;
                        const float theta = rt_acosf(-ony);
                        const float phi = rt_atan2f(-onz, onx) + 3.1415927410125732421875f;
                        tu = phi / 6.283185482025146484375f;
                        tv = theta / 3.1415927410125732421875f;
                    } else if (best_id < ns + nr) {  // object.cuh:113-114, 150-151, 183-184
                        const int j = best_id - ns;
                        const float4 q0r = rect[2 * j];
                        const int axis = __float_as_int(rect[2 * j + 1].y);
                        const float pa = axis == 2 ? py : px, pb = axis == 0 ? py : pz;
                        tu = (pa - q0r.x) / (q0r.y - q0r.x);
                        tv = (pb - q0r.z) / (q0r.w - q0r.z);
                    } else if (best_id < ns + nr + nc) {  // object.cuh:283-288, in the cylinder's object space
                        const int k = best_id - ns - nr;
                        const float4 r0 = cyl[RT_CYL_STRIDE * k], r1 = cyl[RT_CYL_STRIDE * k + 1], r2 = cyl[RT_CYL_STRIDE * k + 2], pr = cyl[RT_CYL_STRIDE * k + 3];
                        const float oox = fmaf(r0.x, ox, fmaf(r0.y, oy, fmaf(r0.z, oz, r0.w)));
                        const float ooy = fmaf(r1.x, ox, fmaf(r1.y, oy, fmaf(r1.z, oz, r1.w)));
                        const float ooz = fmaf(r2.x, ox, fmaf(r2.y, oy, fmaf(r2.z, oz, r2.w)));
                        const float odx = fmaf(r0.x, dx, fmaf(r0.y, dy, r0.z * dz));
                        const float ody = fmaf(r1.x, dx, fmaf(r1.y, dy, r1.z * dz));
                        const float odz = fmaf(r2.x, dx, fmaf(r2.y, dy, r2.z * dz));
                        const float opx = fmaf(best_t, odx, oox), opy = fmaf(best_t, ody, ooy), opz = fmaf(best_t, odz, ooz);
                        const float phi = rt_atan2f(opy, opx) + 6.283185482025146484375f;
                        tu = phi / 12.56637096405029296875f;
                        tv = (opz - pr.y) / (pr.z - pr.y);
                    } else {  // hittable.py:233: uv = u1 w1 + u2 w2 + u3 w3, with the area weights from above
                        const int k = best_id - ns - nr - nc;
                        const float4 c0 = image[P.off_tri_cold + 2 * k], c1 = image[P.off_tri_cold + 2 * k + 1];
                        tu = fmaf(c1.z, w3, fmaf(c1.x, w2, c0.z * w1));
                        tv = fmaf(c1.w, w3, fmaf(c1.y, w2, c0.w * w1));
                        if (k >= nt) tu = w1, tv = w2;  // a quad's (a, b)
                    }
                    // the mask's verdict (rt_alpha.h): the texel of the mask's image at this (u, v), its alpha byte against c8
                    if constexpr (ALPHA) {
                        if (al_mask) al_pass = alpha_transparent(image_texel_word(image, al_rec, tu, tv), (uint32_t)__float_as_int(al_rec.w));
                    }
                    if constexpr (QUERY) {
                        // the query's answer: the record as it stands here, the primitive by its index in the scene's list
                        put_record(q_ray, best_t, list_index_of(P, image, best_id), mat, front ? 1 : 0, nx, ny, nz, tu, px, py, pz, tv);
                        active = false;
                        kind = -1;
                    } else
                    if (!pbr_uv && (kind == MK_LAMBERT_IMAGE || kind == MK_LIGHT_IMAGE || kind == MK_PLASTIC_IMAGE) && !noise_tex && !al_pass && !al_shadow) image_texel(image, M[1], tu, tv, tex_r, tex_g, tex_b);
                }
                // ALPHA: the transition.  A hole: the query starts again from p = o + t d with everything else of the lane as it
                // is -- no vertex, no draw, no bounce.  A surface: the query ends; if it came through holes, the origin it set
                // out from comes back and t counts from there.  A shadow ray takes its verdict here (occluded) and is done.
                if constexpr (ALPHA) {
                    if (has_alpha) {
                        const int al_n = __float_as_int(al_state[0]);
                        if (al_pass) {
                            if (al_n == 0) al_state[AL_OX] = ox, al_state[AL_OY] = oy, al_state[AL_OZ] = oz;
                            ox = fmaf(best_t, dx, ox), oy = fmaf(best_t, dy, oy), oz = fmaf(best_t, dz, oz);
                            al_state[AL_T] += best_t;
                            al_state[0] = __int_as_float(al_n + 1);
                            kind = -1;
                        } else {
                            if (al_n != 0) {
                                ox = al_state[AL_OX], oy = al_state[AL_OY], oz = al_state[AL_OZ];
                                best_t += al_state[AL_T];
                            }
                            al_state[0] = __int_as_float(0), al_state[AL_T] = 0.0f;
                            if (al_shadow) {  // (an opaque occluder: the light sample is lost)
                                RT_SHADOW_VERDICT(false)
                                kind = -1;
                            }
                        }
                    }
                }
                if (!(ALPHA && kind < 0)) {  // (a hole and a shadow ray's occluder: nothing of the material is evaluated)
                // The solid textures' values: a noise texture under a lambertian, an emitter or a plastic, and both textures of a
                // pbr material -- ONE copy of the noise code: a second pass of the same call site evaluates a pbr material's
                // noise map.  Then a pbr hit's parameters (rt_pbr.h): its image, solid and checker sources, and everything to
                // bytes.  From here on tex holds the base colour c8 / 255, and r8 and m8 ride in the kind's upper bits (kind =
                // MK_PBR | r8 << 8 | m8 << 16) until the scatter step (6) has made the vertex a plastic or a rough-metal one: every
                // ordered comparison of kinds in between sees a glossy kind, and nothing more stays live than for an
                // image-textured plastic
                if constexpr (EXT && !QUERY) {
                    const bool pbr = pbr_t >= 0;
                    if (noise_tex || pbr) {
                        const float4 *PS = pbr ? image + __float_as_int(M[0].y) : M;
                        float pm_g = 1.0f, pm_b = 1.0f;  // the map's G and B channels
                        const bool n_base = !pbr || (pbr_t & 15) == 3, n_map = pbr && (pbr_t >> 4) == 3;
#pragma clang loop unroll(disable)
                        for (int pass = 0; pass < 2; ++pass) {
                            if (pass == 0 ? n_base : n_map) {
                                const float4 *R = pass == 0 ? M : PS;
                                const float4 c = noise_texel(image, R[1], R[2], px, py, pz);
                                if (pass == 0) tex_r = c.x, tex_g = c.y, tex_b = c.z;
                                else pm_g = c.y, pm_b = c.z;
                            }
                        }
                        if (pbr) {
                            float mr;
                            if ((pbr_t & 15) == 2) image_texel(image, M[1], tu, tv, tex_r, tex_g, tex_b);
                            if ((pbr_t >> 4) == 2) image_texel(image, PS[1], tu, tv, mr, pm_g, pm_b);
                            const float4 q1 = M[1], q2 = M[2], s0 = PS[0], s1 = PS[1], s2 = PS[2];
                            const bool odd = checker_odd(px, py, pz);
                            if ((pbr_t & 15) < 2) {
                                const bool o = odd && (pbr_t & 15) == 1;
                                tex_r = o ? q2.x : q1.x, tex_g = o ? q2.y : q1.y, tex_b = o ? q2.z : q1.z;
                            }
                            if ((pbr_t >> 4) < 2) {
                                const bool o = odd && (pbr_t >> 4) == 1;
                                pm_g = o ? s2.y : s1.y, pm_b = o ? s2.z : s1.z;
                            }
                            uint32_t m8;
                            const uint32_t c8 = pbr_params(tex_r, tex_g, tex_b, pm_g, pm_b, s0.y, s0.x, m8);
                            tex_r = pbr_unit(c8 & 255u), tex_g = pbr_unit((c8 >> 8) & 255u), tex_b = pbr_unit((c8 >> 16) & 255u);
                            kind = MK_PBR | (int)((c8 >> 24) << 8) | (int)(m8 << 16);
                        }
                    }
                }
                // a bump or a normal map (7u; a material carries one of them): the material's noise height field, or its
                // map's texel in the tangent frame, tilts the shading normal, behind the smooth-shading normal
                // and the (u, v) above (a sphere's read its normal) and before everything that shades: the feature pass, the
                // scatter step, the light sample's cosine and frame.  The hit point, front, t and an emitter's normal (a
                // diffuse_light takes no bump) stay geometric; a query never comes here.
                if constexpr (EXT && !QUERY) {
                    const int boff = __float_as_int(M[2].w);
                    if (boff != 0 && !(MOTION && mot_i >= 0)) {
                        float gnx = nx, gny = ny, gnz = nz;  // the face-turned geometric normal: a triangle's may have been replaced
                        if (best_id >= ns + nr + nc) {
                            const int k = best_id - ns - nr - nc;
                            const float tnx = tri[RT_TRI_STRIDE * k].w, tny = tri[RT_TRI_STRIDE * k + 1].w, tnz = tri[RT_TRI_STRIDE * k + 2].w;
                            gnx = front ? tnx : -tnx, gny = front ? tny : -tny, gnz = front ? tnz : -tnz;
                        }
                        if (boff > 0) {
                            const float4 nb = bump_normal(image, boff, front, nx, ny, nz, gnx, gny, gnz, dx, dy, dz, px, py, pz);
                            nx = nb.x, ny = nb.y, nz = nb.z;
                        } else if (has_maps) {
                            // a normal map (rt_tangent.h): the word is minus the offset of the record {texel word
                            // offset, rows, cols, scale}.  The texel at the (u, v) above, then -- only where it tilts anything --
                            // the raw tangents dp/du, dp/dv of the winner's primitive type from the records the blocks above read
                            const float4 mr = image[-boff];
                            float mx, my, mz;
                            if (tangent_decode(image_texel_word(image, mr, tu, tv), mx, my, mz)) {
                                float Tx, Ty, Tz, Bx, By, Bz;
                                if (best_id < ns) {
                                    tangent_sphere(front ? nx : -nx, front ? ny : -ny, front ? nz : -nz, Tx, Ty, Tz, Bx, By, Bz);
                                } else if (best_id < ns + nr) {
                                    const int j = best_id - ns;
                                    const float4 q0r = rect[2 * j];
                                    tangent_rect(__float_as_int(rect[2 * j + 1].y), q0r.x, q0r.y, q0r.z, q0r.w, Tx, Ty, Tz, Bx, By, Bz);
                                } else if (best_id < ns + nr + nc) {
                                    const int k = best_id - ns - nr;
                                    const float4 r2 = cyl[RT_CYL_STRIDE * k + 2], pr = cyl[RT_CYL_STRIDE * k + 3];
                                    tangent_cylinder(r2.x, r2.y, r2.z, front ? nx : -nx, front ? ny : -ny, front ? nz : -nz, pr.y, pr.z, Tx, Ty, Tz, Bx, By, Bz);
                                } else {
                                    const int k = best_id - ns - nr - nc;
                                    const float4 r0 = tri[RT_TRI_STRIDE * k], r1 = tri[RT_TRI_STRIDE * k + 1], r2 = tri[RT_TRI_STRIDE * k + 2];
                                    if (k >= nt) {  // a quad's record: {Q, n.x} {A, n.y} {B, n.z}
                                        tangent_quad(r0.w, r1.w, r2.w, r1.x, r1.y, r1.z, r2.x, r2.y, r2.z, Tx, Ty, Tz, Bx, By, Bz);
                                    } else {
                                        const float4 c0 = image[P.off_tri_cold + 2 * k], c1 = image[P.off_tri_cold + 2 * k + 1];
                                        tangent_triangle(r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r2.x, r2.y, r2.z, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, Tx, Ty,
                                                         Tz, Bx, By, Bz);
                                    }
                                }
                                const float4 nb = mapped_normal(front, mr.w, nx, ny, nz, gnx, gny, gnz, dx, dy, dz, Tx, Ty, Tz, Bx, By, Bz, mx, my, mz);
                                nx = nb.x, ny = nb.y, nz = nb.z;
                            }
                        }
                    }
                }
                if (COUNT) {
                    c_hits++;
                    // (the glossy materials, DESIGN 7m: plastic counts with the lambertians, rough metal with the metals)
                    // (rough glass, DESIGN 7r, with the dielectrics)
                    if (kind <= MK_LAMBERT_IMAGE || (EXT && kind >= MK_PLASTIC_SOLID && kind != MK_ROUGH_GLASS)) c_scatter0++;
                    else if (kind == MK_METAL || (EXT && kind == MK_ROUGH_METAL)) c_scatter1++;
                    else if (kind == MK_DIELECTRIC || (EXT && kind == MK_ROUGH_GLASS)) c_scatter2++;
                    else c_scatter3++;
                }
                if constexpr (QUERY) {
                } else
                if constexpr (AOV) {
                    // first-hit feature (render_feature_kernel): the path ends here and adds one triple in place of radiance --
                    // the texture value under the hit (metal: its albedo, dielectric: white), the face-turned normal, or (t, 1, 0)
                    if (P.feature == RT_FEATURE_ALBEDO) {
                        const float4 q1 = M[1], q2 = M[2];
                        // (rough metal: F0, where metal keeps its albedo; plastic: the body's texture)
                        const bool odd = (kind == MK_LAMBERT_CHECKER || kind == MK_LIGHT_CHECKER || kind == MK_PLASTIC_CHECKER) && checker_odd(px, py, pz);
                        L_r = odd ? q2.x : q1.x, L_g = odd ? q2.y : q1.y, L_b = odd ? q2.z : q1.z;
                        if (kind == MK_LAMBERT_IMAGE || kind == MK_LIGHT_IMAGE || kind == MK_PLASTIC_IMAGE || kind == MK_PLASTIC_NOISE || (EXT && pbr_t >= 0)) L_r = tex_r, L_g = tex_g, L_b = tex_b;  // (pbr: the base colour, c8 / 255)
                        if (kind == MK_DIELECTRIC || (EXT && kind == MK_ROUGH_GLASS)) L_r = L_g = L_b = 1.0f;  // (c0 of rough glass is its sigma)
                    } else if (P.feature == RT_FEATURE_NORMAL) {
                        L_r = nx, L_g = ny, L_b = nz;
                    } else {
                        L_r = best_t, L_g = 1.0f, L_b = 0.0f;
                    }
                    path_done = true;
                    kind = -1;
                } else
                if (kind >= MK_LIGHT_SOLID && (!EXT || kind <= MK_LIGHT_IMAGE)) {  // diffuse_light: emitted, never scatters (material.cuh:161-182, main.cu:48-58)
                    const float4 q1 = M[1], q2 = M[2];
                    const bool odd = kind == MK_LIGHT_CHECKER && checker_odd(px, py, pz);
                    float er = odd ? q2.x : q1.x, eg = odd ? q2.y : q1.y, eb = odd ? q2.z : q1.z;
                    if (EXT && kind == MK_LIGHT_IMAGE) er = tex_r, eg = tex_g, eb = tex_b;
                    L_r = er * beta_r, L_g = eg * beta_g, L_b = eb * beta_b;
                    if (NEE && mis_pdf >= 0.0f) {
                        // MIS on a BSDF hit: pdf_b^2 / (pdf_b^2 + p_l^2), p_l the light strategy's solid-angle density here
                        const int slot = lslot[best_id];
                        if (slot >= 0) {
                            const float4 *lr = image + P.off_light + RT_LIGHT_STRIDE * slot;
                            const float4 h = lr[0];
                            float pl;
                            if (__float_as_int(h.x) == 0) {  // sphere: uniform in the cone it subtends at the origin
                                const float4 g = lr[3];
                                const float wx = g.x - ox, wy = g.y - oy, wz = g.z - oz;
                                const float c2 = dot3(wx, wy, wz, wx, wy, wz), r2 = g.w * g.w;
                                pl = c2 > r2 ? h.z / ((2.0f * kPi) * cone_one_minus_cos(r2, c2)) : 0.0f;
                            } else {  // by area: selection x 1/area x dist^2 / |cos_l|
                                pl = ((h.z * h.w) * (best_t * best_t * ra)) / (fabsf(dot3(nx, ny, nz, dx, dy, dz)) * inv_len);
                            }
                            if (pl > 0.0f) {
                                const float q = pl / mis_pdf;
                                const float w = mis_pdf > 0.0f ? 1.0f / fmaf(q, q, 1.0f) : 0.0f;
                                L_r *= w, L_g *= w, L_b *= w;
                            }
                        }
                    }
                    path_done = true;  // absorbed: main.cu:55-58
                    kind = -1;
                }
                }  // if (!(ALPHA && kind < 0))
            } else if (QUERY) {
                put_record(q_ray, INFINITY, -1, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
                active = false;
            } else {
                // miss: main.cpp:36-38 (sky) or main.cu:63 (constant background)
                if constexpr (ALPHA) {
                    if (has_alpha) al_state[0] = __int_as_float(0), al_state[AL_T] = 0.0f;  // (the path ends here: the origin is of no use any more)
                }
                float bg_r, bg_g, bg_b;
                float env_w = 1.0f;  // ENV + NEE: the MIS weight of a BSDF ray that escapes
                if constexpr (ENV) {
                    // the environment in place of both: radiance and the light strategy's density through the one lookup
                    const EnvView EV = env_view();
                    float pe;
                    env_eval(EV, inv_len * dx, inv_len * dy, inv_len * dz, bg_r, bg_g, bg_b, pe);
                    if (NEE && mis_pdf >= 0.0f) {
                        const float pl = P.env_sel * pe;
                        if (pl > 0.0f) {
                            const float q = pl / mis_pdf;
                            env_w = mis_pdf > 0.0f ? 1.0f / fmaf(q, q, 1.0f) : 0.0f;
                        }
                    }
                } else
                if (P.flags & RT_FLAG_SKY_GRADIENT) {
                    const float t = 0.5f * (inv_len * dy + 1.0f);
                    const float omt = 1.0f - t;
                    bg_r = fmaf(t, 0.5f, omt), bg_g = fmaf(t, 0.7f, omt), bg_b = fmaf(t, 1.0f, omt);
                } else {
                    bg_r = P.background[0], bg_g = P.background[1], bg_b = P.background[2];
                }
                L_r = beta_r * bg_r, L_g = beta_g * bg_g, L_b = beta_b * bg_b;
                if constexpr (ENV && NEE) L_r *= env_w, L_g *= env_w, L_b *= env_w;
                if constexpr (AOV) {  // a miss: the albedo pass keeps the background (beta = 1), normal and depth add zeros
                    if (P.feature != RT_FEATURE_ALBEDO) L_r = L_g = L_b = 0.0f;
                }
                path_done = true;
                if (COUNT) c_misses++;
            }
#undef RT_SHADOW_VERDICT
            }  // if (active): rects, cylinders, triangles, shading part 1
          }
        }
        tick(3);
        // ---- (3) res += ray_color(...), main.cu:100 -- exact fixed-point add into the tile
        if (!QUERY && (path_done || (NEE && nee_add))) {
            {
                const unsigned long long fr = radiance_to_fixed(L_r), fg = radiance_to_fixed(L_g), fb = radiance_to_fixed(L_b);
                if (cur_p < 0) {
                    unsigned long long *g = acc + (size_t)(~cur_p) * 3;
                    if (fr) atomicAdd(g + 0, fr);
                    if (fg) atomicAdd(g + 1, fg);
                    if (fb) atomicAdd(g + 2, fb);
                } else {
                    // (an LDS address and cur_p < 64: a 24-bit multiply-add on the low word, where `c_acc + cur_p * 3` was a
                    //  quarter-rate v_mad_u64_u32)
                    unsigned long long *a = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(c_acc) + __umul24((uint32_t)cur_p, 24u));
                    atomicAdd(a + 0, fr);
                    atomicAdd(a + 1, fg);
                    atomicAdd(a + 2, fb);
                }
            }
            if (!NEE || path_done) active = false;
        }
        tick(4);
        if (RT_PRIO_H != RT_PRIO_F) __builtin_amdgcn_s_setprio(RT_PRIO_F);
        // ---- (4) refill: lanes without a live path take new samples
        // (render()'s sample loop, main.cu:95-101; camera::get_ray camera.h:32-39)
        float u = 0, v = 0;    // jitter of the sample a lane starts (main.cu:96-97)
        bool started = false;  // this lane starts a new path in this iteration
        // ... and those lanes as a lane mask, from the compares that decide it (each a ballot of its own, combined as scalars),
        // so that the vote below needs no round trip through a vector register
        unsigned long long started_m = 0ull;
        const bool need = !active;
        const unsigned long long idle = __ballot(need);
        // is the current item handed out completely?
        bool exhausted = !c_valid;
        if (c_valid) {
            if (POOL) exhausted = cursor >= c_pool;
            else exhausted = __builtin_amdgcn_ballot_w64(c_hvalid != 0 && mine * 64 < c_pool) == 0ull;
        }
        // The pool is handed out and idle lanes want the next item: retire the current one.  Its
        // accumulator is flushed for reuse and every path still alive becomes an orphan (three 64-bit global atomics
        // when it ends: one more dirty 64-byte line for 24 useful bytes).  So the item is only retired once at most
        // P.orphan_max paths are left, the idle lanes wait meanwhile.  Measured 12 / 32 / 63 (never wait): whole frame
        // 147.9 / 147.9 / 147.3 ms and 1.16 / - / 2.0 GB of HBM writes, a 1/8 row shard (short items) 20.36 / 20.11 /
        // 19.97 ms: the host sets 12 for launches with many tiles per wave and 63 for small ones.
        bool fetch = exhausted && !queue_empty;
        if (QUERY) {
            // (the lanes still tracing carry their ray's index: an item that is handed out has nothing left to wait for)
            if (idle != 0ull && fetch) c_valid = false;
        } else if (c_valid && idle != 0ull && fetch) {
            if (mask_count(~idle) <= P.orphan_max) {
                if (active && cur_p >= 0) cur_p = ~((c_band * 8 + (cur_p >> 3)) * P.width + c_x0 + (cur_p & 7));
                flush_tile(c_acc, c_x0, c_band);
                c_valid = false;
            } else {
                fetch = false;
            }
        }
        if (idle) {  // wave-uniform
            if (fetch) {
                unsigned int item = 0;
                if (lane == 0) item = atomicAdd(queue, 1u);
                item = __builtin_amdgcn_readfirstlane(item);
                if constexpr (QUERY) {
                    // item i is the rays [i * RT_TRACE_ITEM, + RT_TRACE_ITEM) of the batch (n < 2^31, and the counter
                    // passes the last item by at most one per wave: 32 bits hold it)
                    const uint32_t base = item * (uint32_t)RT_TRACE_ITEM;
                    if (base >= TQ.n) {
                        queue_empty = true;
                    } else {
                        c_sbegin = (int)base;
                        c_pool = (int)min((uint32_t)RT_TRACE_ITEM, TQ.n - base);
                        cursor = 0;
                        c_valid = true;
                    }
                } else {
                const int4 ia = ipar4(0), ib = ipar4(1), ic = ipar4(2);
                if (item >= (unsigned int)ia.z) {
                    queue_empty = true;  // the counter only grows: every wave gets here
                    if (COUNT) t_qe = __builtin_amdgcn_s_memrealtime();
                } else {
                    const unsigned int tiles_x = (unsigned int)ia.x, bands = (unsigned int)ia.y;
                    const int sample_first = ia.w, sample_count = ib.x, spp_chunk = ib.y;
                    const int n_big = ib.z, n_med = ib.w, q_med = ic.x, q_small = ic.y;
                    c_x0 = (int)(item % tiles_x) * 8;
                    c_band = (int)((item / tiles_x) % bands);
                    const int chunk = (int)(item / (tiles_x * bands));
                    if (ic.w != 0) {
                        // a tile list of n_list = ic.w tiles (adaptive sampling, device_scene.h).  The host sets tiles_x = n_list
                        // and bands = 1 for such a launch, so c_x0 / 8 is item % n_list and chunk is item / n_list: no division
                        // of its own, one scalar 16-byte load (the list word's quad) behind the ipar4 barrier
                        const int4 t = ipar4((RT_TILE_LIST_AT - RT_ITEM_PARAMS_AT) / 4 + (c_x0 >> 5));
                        const int q = (c_x0 >> 3) & 3;
                        const int w = q == 0 ? t.x : q == 1 ? t.y : q == 2 ? t.z : t.w;
                        c_x0 = w & 0xffff, c_band = w >> 16;
                    }
                    int s_stop;  // sample range: big chunks first, shorter and shorter ones towards the end of the queue
                    if (chunk < n_big) {
                        c_sbegin = sample_first + chunk * spp_chunk;
                        s_stop = c_sbegin + spp_chunk;
                    } else if (chunk < n_big + n_med) {
                        c_sbegin = sample_first + n_big * spp_chunk + (chunk - n_big) * q_med;
                        s_stop = c_sbegin + q_med;
                    } else {
                        c_sbegin = sample_first + n_big * spp_chunk + n_med * q_med + (chunk - n_big - n_med) * q_small;
                        s_stop = c_sbegin + q_small;
                    }
                    const int s_end = sample_first + sample_count;
                    if (s_stop > s_end) s_stop = s_end;
                    c_pool = (s_stop - c_sbegin) * 64;  // pool item k = (pixel k & 63, sample c_sbegin + (k >> 6))
                    // (the item's values are the same in every lane; said so, they live in scalar registers instead of five of
                    //  the 72 vector registers this kernel spills from)
                    c_x0 = __builtin_amdgcn_readfirstlane(c_x0), c_band = __builtin_amdgcn_readfirstlane(c_band);
                    c_sbegin = __builtin_amdgcn_readfirstlane(c_sbegin), c_pool = __builtin_amdgcn_readfirstlane(c_pool);
                    cursor = 0;
                    if constexpr (TRACE) slab_for = -1;
                    mine = 0;
                    c_valid = true;
                    int hx_unused, hlr_unused;
                    home_pixel(c_x0, c_band, hx_unused, hlr_unused, c_hy, c_hvalid);
                    // (POOL: a pixel's row is read across lanes in the refill; an off-image pixel says so through it)
                    if (POOL && c_hvalid == 0) c_hy = -1;
                }
                }
            }
            bool start = false;
            int sp = 0, spx = 0, spy = 0, ss = 0;
            if constexpr (QUERY) {
                // an idle lane takes ray c_sbegin + cursor + rank: two 16-byte loads, the guard (rt_trace.h), and what every new
                // ray needs.  A ray that fails the guard gets its record here and never enters the walk; its lane stays idle.
                const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                const int k = cursor + rank;
                if (c_valid) cursor = min(cursor + mask_count(idle), c_pool);
                const unsigned long long takes = c_valid ? idle & __builtin_amdgcn_ballot_w64(k < c_pool) : 0ull;
                bool ok = false;
                if (__builtin_amdgcn_inverse_ballot_w64(takes)) {
                    const uint32_t ray = (uint32_t)(c_sbegin + k);
                    const float4 r0 = TQ.rays[(size_t)ray * 2], r1 = TQ.rays[(size_t)ray * 2 + 1];
                    ok = ray_valid(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z);
                    if (ok) {
                        q_ray = ray, q_tmax = r0.w;
                        ox = r0.x, oy = r0.y, oz = r0.z, dx = r1.x, dy = r1.y, dz = r1.z;
                        ra = dot3(dx, dy, dz, dx, dy, dz);
                        rinv_a = 1.0f / ra;
                        active = true;
                    } else {
                        put_record(ray, INFINITY, RT_HIT_INVALID, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
                    }
                }
                started_m = takes & __builtin_amdgcn_ballot_w64(ok);
            } else
            if constexpr (BURST) {
                // Paths start from the wave's slab.  The pool's order is the other builds': entry k is pixel k & 63, sample
                // c_sbegin + (k >> 6), so entries [64 b, 64 b + 64) are ONE sample of every pixel of the tile: batch b.  When the
                // cursor stands on a multiple of 64 the slab is used up (or the item is new), and all 64 lanes prepare batch
                // cursor >> 6 -- lane l its home pixel's sample: seed, the two jitter draws, the lens disk's rejection loop and the
                // camera ray, each what a starting lane of the other builds computes, from the same counter in the same
                // order -- at full occupancy instead of for the dozen lanes that happen to be idle.  An idle lane of rank r then
                // takes slot (cursor + r) & 63: three reads.  Its stored generator state goes on with the roulette draw.
                // A hand-out that reaches the end of a batch serves the rest of the idle lanes from the next one in the same
                // iteration (at most two passes: a batch has a slot for every lane).
                // TRACE (kernels.h, RT_BURST_TRACE; render_burst.h): the burst also runs the FIRST closest-hit query of its 64
                // paths -- stage (1)'s text, render_query.h -- and settles the paths that end there: the sky or the background,
                // an emitter, and with rr_p > 0 the roulette's first draw, which moves in front of the query.  Such a slot is
                // dead (the NaN in d.x that an off-image slot carries); a scattering hit's slot is {p, d, state}, 10 words as
                // before, and the winner's id rides in the upper half of lane l's home-row register c_hy.  A lane that pops a
                // live slot rebuilds stage (2)'s hit record and joins the rejection loop and the scatter step of this
                // iteration; one that pops a dead slot stays in `want` and is served from the following slots (REPOP).
                // The traced burst does not run here but at the top of the next iteration, where no hit record is live
                // across its query: the lanes still unserved when the slab runs out wait one iteration.  (Inside the refill
                // the second query site cost the main loop 20 more spilled registers and 5 % of the frame)
                unsigned long long want = c_valid ? idle : 0ull;  // idle lanes not served yet
                while (want != 0ull && cursor < c_pool) {
                    if constexpr (TRACE) {
                        // (the slab does not hold the cursor's batch: the lanes still unserved wait for the burst at the top
                        //  of the next iteration)
                        if ((cursor >> 6) != slab_for) break;
                    } else {
                        // (without TRACE the burst prepares camera rays only, here, where the slab runs out)
                        if ((cursor & 63) == 0) {
                            __builtin_amdgcn_wave_barrier();
#include "render_burst.h"
                            __builtin_amdgcn_wave_barrier();
                        }
                    }
                    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(want >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)want, 0u));
                    const int room = 64 - (cursor & 63);
                    const unsigned long long takes = want & __builtin_amdgcn_ballot_w64(rank < room);
                    bool on_image = false;
                    // TRACE: the winner's id of slot s waits in the upper half of lane s's home-row register: one cross-lane
                    // read in which every lane takes part, as the 4-wave builds read the row
                    int hid = 0;
                    if constexpr (TRACE) hid = __shfl(c_hy, (cursor + rank) & 63, 64);
                    if (__builtin_amdgcn_inverse_ballot_w64(takes)) {
                        const int slot = (cursor + rank) & 63;
                        const float4 a = slab_a[slot], b = slab_b[slot];
                        const float2 c = slab_c[slot];
                        on_image = a.w == a.w;
                        if constexpr (TRACE) {
                            // a live slot: the path stands at its first vertex.  What stage (2) would have left of the winner, by
                            // stage (2)'s expressions -- the normal from the cold record, front, 1 / |d|, material and kind -- and
                            // what stage (6b) gives a path that starts; the lane joins the rejection loop and the scatter step of
                            // this iteration, and its first query in the main loop is its second ray.  A dead slot (the path ended
                            // in the burst, or the pixel is off the image) leaves the lane as it is.
                            if (on_image) {
                                px = a.x, py = a.y, pz = a.z, dx = a.w, dy = b.x, dz = b.y;
                                rng.g.x = __float_as_uint(b.z), rng.g.y = __float_as_uint(b.w);
                                rng.g.z = __float_as_uint(c.x), rng.g.w = __float_as_uint(c.y);
                                cur_p = slot;
                                const int id = hid >> 16;
                                const float4 s = sph[id];
                                const float4 cold = *rec_at(image + P.off_sph_cold, (uint32_t)id << 4);
                                const float onx = cold.x * (px - s.x), ony = cold.x * (py - s.y), onz = cold.x * (pz - s.z);
                                front = dot3(dx, dy, dz, onx, ony, onz) < 0.0f;
                                nx = front ? onx : -onx, ny = front ? ony : -ony, nz = front ? onz : -onz;
                                mat = __float_as_int(cold.y);
                                kind = __float_as_int(cold.w);
                                inv_len = 1.0f / rt_sqrtf<ROOT_VOTE>(dot3(dx, dy, dz, dx, dy, dz));
                                beta_r = beta_g = beta_b = P.rr_p > 0.0f ? 1.0f / P.rr_p : 1.0f;
                                depth = P.max_depth;
                                active = true;
                            }
                        } else {
                        ox = a.x, oy = a.y, oz = a.z, dx = a.w, dy = b.x, dz = b.y;
                        rng.g.x = __float_as_uint(b.z), rng.g.y = __float_as_uint(b.w);
                        rng.g.z = __float_as_uint(c.x), rng.g.w = __float_as_uint(c.y);
                        cur_p = slot;
                        }
                    }
                    const unsigned long long served = takes & __builtin_amdgcn_ballot_w64(on_image);
                    started_m |= served;
                    cursor += min(mask_count(want), room);
                    // (REPOP: a lane that popped a dead slot stays in `want`: the loop serves it from the following slots, and
                    //  runs the next burst when the batch ends, until it is served or the pool is empty -- a sample whose
                    //  camera ray leaves the scene costs no lane slot of an iteration, and a tile of sky is a loop of bursts)
                    want &= REPOP ? ~served : ~takes;
                }
            } else
            if (POOL) {
                const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                const int k = cursor + rank;
                if (c_valid) cursor = min(cursor + mask_count(idle), c_pool);
                sp = k & 63;
                // row and validity of pixel sp live in lane sp's registers (all lanes take part): one cross-lane read, the row
                // of an off-image pixel is -1.  (As a wave-uniform mask of on-image bits beside the row, the bit of pixel sp cost a
                //  select between the mask's halves, a bit-field extract and a compare, and the mask two scalar registers.)
                spy = __shfl(c_hy, sp, 64);
                spx = c_x0 + (sp & 7);
                ss = c_sbegin + (k >> 6);
                started_m = c_valid ? idle & __builtin_amdgcn_ballot_w64(k < c_pool) & __builtin_amdgcn_ballot_w64(spy >= 0) : 0ull;
                start = __builtin_amdgcn_inverse_ballot_w64(started_m);
            } else {
                started_m = c_valid ? idle & __builtin_amdgcn_ballot_w64(mine * 64 < c_pool) & __builtin_amdgcn_ballot_w64(c_hvalid != 0) : 0ull;
                start = __builtin_amdgcn_inverse_ballot_w64(started_m);
                sp = lane, spx = c_x0 + (lane & 7), spy = c_hy, ss = c_sbegin + mine;
                if (start) mine++;
            }
            if (start) {
                cur_p = sp;
                // (row and width are at most 65536, scene_validate: a 24-bit multiply, full rate; its low 32 bits are the id's)
                const uint32_t pixel = __umul24((uint32_t)spy, (uint32_t)P.width) + (uint32_t)spx;
                rng_start(rng, pixel, (uint32_t)ss, k0, k1);
                if constexpr (MOTION) {  // (the key behind the same barrier as in rng_start: its schedule stays scalar)
                    uint32_t m0 = k0, m1 = k1;
                    asm volatile("" : "+s"(m0), "+s"(m1));
                    mot_s = shutter_time(pixel, (uint32_t)ss, m0, m1);
                }
                u = ((float)spx + rng_next<COUNT>(rng)) * P.inv_wm1;
                v = ((float)spy + rng_next<COUNT>(rng)) * P.inv_hm1;
                if (COUNT) c_samples++;
            }
        }
        started = __builtin_amdgcn_inverse_ballot_w64(started_m);
        tick(0);
        // (`active` has not changed since `idle` was taken: the live lanes are the others of this wave)
        if (((__builtin_amdgcn_ballot_w64(true) & ~idle) | started_m) == 0ull) {
            // nothing in flight.  Out of work when the queue is dry, the current item is handed out and no sample
            // waits to be added; otherwise loop: the refill above makes progress every time (takes an item,
            // marks the queue empty, or skips off-image pool entries).  (TRACE: or it has stopped at a batch the slab does
            // not hold yet, or has popped dead slots only; then the progress is the burst that the `continue` below
            // reaches at the top of the next iteration, and the cursor, which every pop moves on.)
            bool exhausted = !c_valid;
            if (c_valid) {
                if (POOL) exhausted = cursor >= c_pool;
                else exhausted = __builtin_amdgcn_ballot_w64(c_hvalid != 0 && mine * 64 < c_pool) == 0ull;
            }
            if (queue_empty && exhausted) {
                if (!QUERY && c_valid) flush_tile(c_acc, c_x0, c_band);
                break;
            }
            continue;
        }
        // ---- (5) rejection sampling, one converged loop: random_in_unit_sphere (vec3.h:121-129: three draws, for the
        // lanes whose material scatters with one: lambertian, metal) and random_in_unit_disk (vec3.h:157-165: two
        // draws, for the lens sample of the paths that start)
        // (QUERY: a ray is traced once and answered: no scatter step, no camera, no roulette -- nothing from here on)
        // (MEDIA: an anisotropic medium vertex -- nx = g != 0 -- takes no attempt: its two draws come in (6a))
        const bool need_s = !QUERY && ((kind >= 0 && kind <= MK_METAL) || (MEDIA && kind == MK_MEDIUM && nx == 0.0f));
        const bool need_d = !QUERY && !BURST && started && (P.flags & RT_FLAG_DEFOCUS_BLUR) != 0u;  // (BURST: the burst's own loop)
        float sx = 0, sy = 0, sz = 0, sl2 = 1;
        asm volatile("" : "=v"(sx), "=v"(sy), "=v"(sz), "=v"(sl2));  // (read by the lanes that ran the loop below, which sets all four)
        if (need_s || need_d) {
            if (RT_PRIO_R != RT_PRIO_F) __builtin_amdgcn_s_setprio(RT_PRIO_R);
            // The three draws of an attempt written out on the generator's four state words (xor128_next, philox.h): every
            // lane computes the third value, and the lanes that sample a disk do not keep it -- their state advances by two
            // draws, the others' by three, through four selects on a loop-invariant mask.  With the third draw behind a
            // branch the loop carried the rotating state through ten register moves per pass: 46 VALU per pass, 39 now.
            // (Measured twice: before the wave priorities it was 0.5 % SLOWER than the branch, with them 1.7 % faster.)
            uint32_t x = rng.g.x, y = rng.g.y, z = rng.g.z, w = rng.g.w;
            do {
                const uint32_t tx = x ^ (x << 11), ty = y ^ (y << 11), tz = z ^ (z << 11);
                const uint32_t n1 = (w ^ (w >> 19)) ^ (tx ^ (tx >> 8));
                const uint32_t n2 = (n1 ^ (n1 >> 19)) ^ (ty ^ (ty >> 8));
                const uint32_t n3 = (n2 ^ (n2 >> 19)) ^ (tz ^ (tz >> 8));
                sx = fmaf((float)(n1 >> 8), 1.0f / 8388608.0f, -1.0f);
                sy = fmaf((float)(n2 >> 8), 1.0f / 8388608.0f, -1.0f);
                const float s3 = fmaf((float)(n3 >> 8), 1.0f / 8388608.0f, -1.0f);
                sz = need_s ? s3 : 0.0f;
                x = need_s ? w : z, y = need_s ? n1 : w, z = need_s ? n2 : n1, w = need_s ? n3 : n2;
                if (COUNT) rng.draws += need_s ? 3u : 2u;
                sl2 = dot3(sx, sy, sz, sx, sy, sz);  // disk: fma(x, x, y * y) -- the product with sz = 0 adds an exact zero
            } while (sl2 >= 1.0f);
            rng.g.x = x, rng.g.y = y, rng.g.z = z, rng.g.w = w;
            if (RT_PRIO_R != RT_PRIO_F) __builtin_amdgcn_s_setprio(RT_PRIO_F);
        }
        if (RT_PRIO_S != RT_PRIO_F) __builtin_amdgcn_s_setprio(RT_PRIO_S);
        // ---- (6a) the scatter step of the paths that go on
        bool fresh = false;  // this lane has a new ray
        // NEE: does this vertex take a light sample (before the depth and roulette checks), does the path end after it (an
        // absorbed metal vertex), the throughput the continuation carries, the metal's reflected direction and fuzz (0: lambertian)
        bool nee_v = false, nee_end = false;
        float vb_r = 0, vb_g = 0, vb_b = 0, mrx = 0, mry = 0, mrz = 0, mfz = 0;
        float glossy_pdf = 0;  // (EXT, NEE) pdf_b of the direction a glossy vertex drew
        uint32_t gtex = 0u;    // (EXT, NEE) an image-textured plastic vertex: its texel, 8 bits a channel, for the light-sample step
        float gv_r = 1.0f, gv_g = 1.0f, gv_b = 1.0f;  // (EXT) a rough-glass back hit: its tint, until it is folded into vb below
        if (!QUERY && kind >= 0) {
            const float4 *M = rec_at(image + P.off_mat, __umul24((uint32_t)mat, 48u));  // (below 2^24 materials: scene_validate)
            if constexpr (MEDIA) {  // (a medium's record 1 is {albedo, density}: where a material keeps c0)
                if (kind == MK_MEDIUM) M = image + __builtin_amdgcn_readfirstlane(__float_as_int(image[P.off_cam + 2].w)) + RT_MEDIUM_STRIDE * mat;
            }
            const float4 q0 = M[0], q1 = M[1], q2 = M[2];
                float g_rough = q0.w;          // (EXT) a glossy vertex's roughness: the record's, or a pbr hit's own
                float ndx, ndy, ndz;           // scattered direction
                float at_r, at_g, at_b;        // attenuation
                bool scattered = true;
                if (MEDIA && kind == MK_MEDIUM && nx != 0.0f) {
                    // an anisotropic medium vertex (rt_phase.h): two draws, u1 for the polar angle about the direction of
                    // travel and u2 for the azimuth; the sample's density is the phase function, so the weight is the albedo
                    const float u1 = rng_next<COUNT>(rng), u2 = rng_next<COUNT>(rng);
                    phase_hg_sample(nx, inv_len * dx, inv_len * dy, inv_len * dz, u1, u2, ndx, ndy, ndz);
                    at_r = q1.x, at_g = q1.y, at_b = q1.z;
                } else if (kind <= MK_LAMBERT_IMAGE || (MEDIA && kind == MK_MEDIUM)) {  // lambertian::scatter, material.h:25-35 (MEDIA: a medium vertex, n = 0)
                    const float inv = 1.0f / rt_sqrtf<ROOT_VOTE>(sl2);
                    ndx = nx + inv * sx, ndy = ny + inv * sy, ndz = nz + inv * sz;
                    const float eps = 1e-8f;
                    if (fabsf(ndx) < eps && fabsf(ndy) < eps && fabsf(ndz) < eps) ndx = nx, ndy = ny, ndz = nz;
                    const bool odd = kind == MK_LAMBERT_CHECKER && checker_odd(px, py, pz);
                    at_r = odd ? q2.x : q1.x, at_g = odd ? q2.y : q1.y, at_b = odd ? q2.z : q1.z;
                    if (EXT && kind == MK_LAMBERT_IMAGE) at_r = tex_r, at_g = tex_g, at_b = tex_b;
                } else if (kind == MK_METAL) {  // metal::scatter, material.h:47-53
                    const float ux = inv_len * dx, uy = inv_len * dy, uz = inv_len * dz;
                    const float k2 = 2.0f * dot3(ux, uy, uz, nx, ny, nz);
                    const float rx = fmaf(-k2, nx, ux), ry = fmaf(-k2, ny, uy), rz = fmaf(-k2, nz, uz);
                    ndx = fmaf(q0.y, sx, rx), ndy = fmaf(q0.y, sy, ry), ndz = fmaf(q0.y, sz, rz);
                    at_r = q1.x, at_g = q1.y, at_b = q1.z;
                    if (NEE) mrx = rx, mry = ry, mrz = rz, mfz = q0.y;
                    scattered = dot3(ndx, ndy, ndz, nx, ny, nz) > 0.0f;
                } else if (EXT && kind >= MK_ROUGH_METAL) {
                    // the glossy materials (rt_glossy.h): two draws for the lobe's visible normal, plastic one more
                    // in front of them for the choice between coat and body.  A vertex seen from below its shading normal
                    // (wo.z <= 0) is absorbed without a draw and takes no light sample; one whose direction comes out below
                    // (wi.z <= 0) is absorbed as a metal vertex is.
                    const float ux = inv_len * dx, uy = inv_len * dy, uz = inv_len * dz;
                    float gpdf = 0.0f;
                    bool below = false, lobe = false;
                    at_r = at_g = at_b = 0.0f, ndx = ndy = ndz = 0.0f;
                    // Rough glass (rt_glass.h) goes through the same body as a rough metal with F0 = 1: uf where plastic
                    // draws ul, then the same two.  The tint of a back hit is formed here, from the hit point and the origin of
                    // the ray that arrived (both still live: t |d| = |p - o|), so that nothing of it is carried through the walk;
                    // it goes into the attenuation and into the throughput the light sample starts from (gv), nowhere else.
                    const bool glass = kind == MK_ROUGH_GLASS;
                    if (glass && !front) {
                        const float ex = px - ox, ey = py - oy, ez = pz - oz;
                        const float dist = rt_sqrtf(dot3(ex, ey, ez, ex, ey, ez));
                        gv_r = glass_tint(q1.x, dist), gv_g = glass_tint(q1.y, dist), gv_b = glass_tint(q1.z, dist);
                    }
                    // The metallic-roughness material (rt_pbr.h): its bytes come out of the kind's upper bits, and
                    // from its first draw on the vertex is a plastic or a rough-metal one of roughness r8 / 255 -- in `kind` too
                    // (MK_PBR: plastic, MK_PBR + 1: metal), which the packed word below hands to the light sample
                    const bool pbr = (kind & 255) == MK_PBR;
                    float g_alpha = q0.y;
                    uint32_t pbr_m8 = 0u;
                    if (pbr) {
                        pbr_m8 = ((uint32_t)kind >> 16) & 255u;
                        gtex = ((uint32_t)kind >> 8) << 24;  // (r8; m8 falls off the top)
                        g_rough = pbr_unit(gtex >> 24);
                        g_alpha = pbr_alpha(g_rough);
                        kind = MK_PBR;
                    }
                    if (-dot3(ux, uy, uz, nx, ny, nz) > 0.0f) {
                        bool plastic = kind != MK_ROUGH_METAL && !glass;
                        // F0, or the coat's r0 in every channel with the body's colour beside it
                        float f_r = q1.x, f_g = q1.y, f_b = q1.z, rh_r = 0.0f, rh_g = 0.0f, rh_b = 0.0f, ul = 0.0f;
                        if (plastic) {
                            const bool odd = kind == MK_PLASTIC_CHECKER && checker_odd(px, py, pz);
                            rh_r = odd ? q2.x : q1.x, rh_g = odd ? q2.y : q1.y, rh_b = odd ? q2.z : q1.z;
                            if (kind == MK_PLASTIC_IMAGE || kind == MK_PLASTIC_NOISE) rh_r = tex_r, rh_g = tex_g, rh_b = tex_b;
                            f_r = f_g = f_b = q0.z;
                        }
                        if (glass) f_r = f_g = f_b = 1.0f;  // (its c0 is sigma)
                        if (plastic || glass) ul = rng_next<COUNT>(rng);  // (pbr is a plastic so far: three draws, whatever it chooses)
                        if (pbr) {
                            rh_r = tex_r, rh_g = tex_g, rh_b = tex_b;
                            if (pbr_choose(pbr_m8, ul, ul)) {
                                plastic = false, kind = MK_PBR + 1;
                                f_r = tex_r, f_g = tex_g, f_b = tex_b;
                            }
                        }
                        const float u1 = rng_next<COUNT>(rng), u2 = rng_next<COUNT>(rng);
                        scattered = glossy_sample_body(glass ? GLOSSY_GLASS : (plastic ? GLOSSY_PLASTIC : GLOSSY_METAL), nx, ny, nz, ux, uy, uz, g_alpha,
                                                       f_r, f_g, f_b, rh_r, rh_g, rh_b, front ? q0.z : q1.w, ul, u1, u2, ndx, ndy, ndz, at_r, at_g,
                                                       at_b, gpdf, below, lobe, NEE && !ENV);  // (the Fresnel term behind a call there: DESIGN 7r)
                        if (glass) at_r *= gv_r, at_g *= gv_g, at_b *= gv_b;
                    } else {
                        scattered = false, below = true;
                    }
                    if (glass && !front) kind = MK_ROUGH_GLASS + 1;  // (what the packed word below tells the light sample: eta = ir)
                    if (NEE) {
                        // the light sample's f cos is not albedo x pdf_b here: step (7) evaluates the material for the light's
                        // direction, from -unit(d) (kept where metal keeps its mirror direction) and the throughput in FRONT
                        // of this vertex.  Where metal keeps its fuzz, a NEGATIVE number says "glossy" and carries in its bits what
                        // that step needs to find the material again -- sign | below << 30 | kind << 24 | material (below 2^24:
                        // scene_validate; a small normal number, never a NaN) -- so that neither kind nor mat nor the texel's
                        // three floats stay live across the roulette section and the light's sample
                        mrx = ux, mry = uy, mrz = uz;
                        mfz = __uint_as_float(0x80000000u | (below ? 0x40000000u : 0u) | ((uint32_t)kind << 24) | (uint32_t)mat);
                        // (a pbr vertex: its colour bytes beside r8, which is there already -- all the light sample takes of it)
                        if (kind == MK_PLASTIC_IMAGE || pbr)
                            gtex |= (uint32_t)fmaf(tex_r, 255.0f, 0.5f) | (uint32_t)fmaf(tex_g, 255.0f, 0.5f) << 8 | (uint32_t)fmaf(tex_b, 255.0f, 0.5f) << 16;
                        glossy_pdf = gpdf;
                    }
                } else {  // dielectric::scatter, material.h:66-95
                    const float ratio = front ? q0.z : q0.y;
                    const float ux = inv_len * dx, uy = inv_len * dy, uz = inv_len * dz;
                    const float udn = dot3(ux, uy, uz, nx, ny, nz);
                    const float cos_t = fminf(-udn, 1.0f);
                    const float sin_t = rt_sqrtf<ROOT_VOTE>(fmaf(-cos_t, cos_t, 1.0f));
                    bool refl = ratio * sin_t > 1.0f;
                    if (!refl) {
                        const float r0 = front ? q0.w : q1.w;
                        const float xx = 1.0f - cos_t;
                        const float x2 = xx * xx;
                        const float x5 = (x2 * x2) * xx;
                        refl = fmaf(1.0f - r0, x5, r0) > rng_next<COUNT>(rng);
                    }
                    if (refl) {  // reflect(), vec3.h:144-147
                        const float k2 = 2.0f * udn;
                        ndx = fmaf(-k2, nx, ux), ndy = fmaf(-k2, ny, uy), ndz = fmaf(-k2, nz, uz);
                    } else {  // refract(), vec3.h:149-155
                        const float ppx = ratio * fmaf(cos_t, nx, ux);
                        const float ppy = ratio * fmaf(cos_t, ny, uy);
                        const float ppz = ratio * fmaf(cos_t, nz, uz);
                        const float kk = -rt_sqrtf<ROOT_VOTE>(fabsf(1.0f - dot3(ppx, ppy, ppz, ppx, ppy, ppz)));
                        ndx = fmaf(kk, nx, ppx), ndy = fmaf(kk, ny, ppy), ndz = fmaf(kk, nz, ppz);
                    }
                    at_r = at_g = at_b = 1.0f;
                }

            if (NEE) {
                // light-sampled vertices: lambertian, and metal fuzzy enough for its lobe to meet a light; the continuation's pdf
                // is kept for the MIS weight of an emitter it hits
                nee_v = kind <= MK_LAMBERT_IMAGE || (kind == MK_METAL && q0.y >= 0.05f);
                const bool glossy = EXT && mfz < 0.0f;
                if (glossy) nee_v = g_rough >= RT_GLOSSY_MIN_ROUGHNESS && (__float_as_uint(mfz) & 0x40000000u) == 0u;  // (pbr: the per-hit r)
                float cpdf = -1.0f;
                if (glossy) {
                    if (nee_v && scattered) cpdf = glossy_pdf;
                } else
                if (nee_v && scattered) {
                    const float il = 1.0f / sqrtf(dot3(ndx, ndy, ndz, ndx, ndy, ndz));
                    const float wx = ndx * il, wy = ndy * il, wz = ndz * il;
                    cpdf = kind == MK_METAL ? metal_pdf(wx, wy, wz, mrx, mry, mrz, mfz) : fmaxf(0.0f, dot3(wx, wy, wz, nx, ny, nz)) * kInvPi;
                }
                // MEDIA: a medium vertex takes a light sample.  Its pdf_b is the phase function's -- 1 / (4 pi) for the
                // stored g = 0 (the rejection loop's normalize(s) is uniform), phase_hg_eval(g, cos) otherwise, cos between the unit
                // direction of travel w = inv_len d and the unit direction drawn -- and w waits where metal keeps its mirror
                // direction, for the light's direction in step (7)
                if constexpr (MEDIA && NEE) {
                    if (kind == MK_MEDIUM) {
                        nee_v = true;
                        mrx = inv_len * dx, mry = inv_len * dy, mrz = inv_len * dz;
                        const float il = 1.0f / sqrtf(dot3(ndx, ndy, ndz, ndx, ndy, ndz));
                        cpdf = nx == 0.0f ? RT_PHASE_ISOTROPIC : phase_hg_eval(nx, dot3(ndx * il, ndy * il, ndz * il, mrx, mry, mrz));
                    }
                }
                mis_pdf = cpdf;
                vb_r = beta_r * at_r, vb_g = beta_g * at_g, vb_b = beta_b * at_b;
                // (the throughput in front of a glossy vertex; rough glass: times its tint, which is not part of glass_eval)
                if (glossy) vb_r = beta_r * gv_r, vb_g = beta_g * gv_g, vb_b = beta_b * gv_b;
                // an absorbed metal vertex still samples its light when its continuation would have been traced: the light
                // sample may not depend on the direction the BSDF drew
                nee_end = !scattered;
                if (nee_end) nee_v = nee_v && depth > 1;
            }
            if (scattered) {
                beta_r *= at_r, beta_g *= at_g, beta_b *= at_b;
                ox = px, oy = py, oz = pz;
                dx = ndx, dy = ndy, dz = ndz;
                depth--;
                fresh = true;
                if (depth <= 0) active = false;  // main.cpp:42 / main.cu:69: black
            } else {
                active = false;  // absorbed: main.cpp:32 / main.cu:55-58: black
            }
        }
        // ---- (6b) the camera ray of the paths that start (camera::get_ray, camera.h:32-39)
        if constexpr (BURST) {
            // (the ray and the generator came out of the slab in the refill; the lane joins `fresh` for what every new ray needs)
            // (TRACE: a popped path is at its first vertex, with throughput and depth set at the pop; the scatter step above
            //  has made its second ray)
            if (!TRACE && started) {
                beta_r = beta_g = beta_b = 1.0f;
                depth = P.max_depth;
                active = true;
                fresh = true;
            }
        } else
        if constexpr (CAMERA) {
            // CAMERA (camera projections, DESIGN 7w, rt_camera.h; a constant of the including kernel, true in the instances of
            // camera_kernel.h alone, which the host picks for a scene whose projection is not the perspective one): the six
            // camera records mean what rt_camera.h says for the model, which is a kernel argument -- the switch is scalar.  The
            // draws before this point are the perspective camera's.  A fisheye sample outside the image circle has no path: the
            // lane took its draws, adds nothing and is idle again at the next refill.
            if (started) {
                float offx = 0.0f, offy = 0.0f, offz = 0.0f;
                const float4 *cv = hot + P.off_cam;
                const float4 c_org = cv[0], c_u = cv[4], c_v = cv[5];
                if (P.flags & RT_FLAG_DEFOCUS_BLUR) camera_lens_offset(c_org.w, c_u, c_v, sx, sy, offx, offy, offz);
                const int model = (int)((P.flags >> RT_PFLAG_PROJ_SHIFT) & 3u);
                const bool seen = camera_ray(model, c_org, cv[1], cv[2], cv[3], c_u, c_v, u, v, offx, offy, offz, ox, oy, oz, dx, dy, dz);
                beta_r = beta_g = beta_b = 1.0f;
                depth = P.max_depth;
                active = seen;
                fresh = seen;
                if (NEE) mis_pdf = -1.0f;
            }
        } else
        if (!QUERY && started) {
                float offx = 0.0f, offy = 0.0f, offz = 0.0f;
                // the camera's derived vectors come from the hot table (wave-uniform reads, used here only),
                // not from kernel arguments that would sit in SGPRs for the whole launch
                const float4 *cv = hot + P.off_cam;
                const float4 c_org = cv[0];  // origin, lens_radius
                if (P.flags & RT_FLAG_DEFOCUS_BLUR) {
                    const float4 c_u = cv[4], c_v = cv[5];
                    float rdx = c_org.w * sx, rdy = c_org.w * sy;
                    offx = fmaf(c_u.x, rdx, c_v.x * rdy);
                    offy = fmaf(c_u.y, rdx, c_v.y * rdy);
                    offz = fmaf(c_u.z, rdx, c_v.z * rdy);
                }
                const float4 c_ll = cv[1], c_hor = cv[2], c_ver = cv[3];
                dx = fmaf(v, c_ver.x, fmaf(u, c_hor.x, c_ll.x));
                dy = fmaf(v, c_ver.y, fmaf(u, c_hor.y, c_ll.y));
                dz = fmaf(v, c_ver.z, fmaf(u, c_hor.z, c_ll.z));
                dx = (dx - c_org.x) - offx;
                dy = (dy - c_org.y) - offy;
                dz = (dz - c_org.z) - offz;
                ox = c_org.x + offx;
                oy = c_org.y + offy;
                oz = c_org.z + offz;
                beta_r = beta_g = beta_b = 1.0f;
                depth = P.max_depth;
                active = true;
                fresh = true;
                if (NEE) mis_pdf = -1.0f;
        }
        // ---- (6c) what every new ray needs, however it came about
        if (fresh) {
            ra = dot3(dx, dy, dz, dx, dy, dz);
            rinv_a = 1.0f / ra;
        }
        // Russian roulette before the next query (4_0_path_tracing.py:45-46; include/rtmi.h,
        // rt_scene_set_russian_roulette): a path that does not survive keeps what it has collected (a new one:
        // nothing, so there is nothing to add); a survivor's throughput is divided by p at once
        if (!AOV && !QUERY && P.rr_p > 0.0f) {  // (a feature sample ends at its first query: no roulette draw)
            if (!TRACE && started) {  // (TRACE: a starting path's draw is the burst's, and its 1 / p is set at the pop)
                if (rng_next<COUNT>(rng) > P.rr_p) active = false;
                beta_r = beta_g = beta_b = 1.0f / P.rr_p;
            } else if (fresh && active) {
                if (rng_next<COUNT>(rng) > P.rr_p) active = false;
                beta_r = beta_r / P.rr_p, beta_g = beta_g / P.rr_p, beta_b = beta_b / P.rr_p;
            }
        }
        if (NEE && nee_v) {
            // ---- (7) the light sample of this vertex (next-event estimation), drawn after the roulette from the same stream:
            // alias draw, then two for the point.  It only happens where the BSDF continuation is traced (or, at an absorbed
            // metal vertex, would be), with the throughput that continuation carries.
            if (nee_end) {
                if (P.rr_p > 0.0f) {
                    if (rng_next<COUNT>(rng) > P.rr_p) nee_v = false;
                    vb_r = vb_r / P.rr_p, vb_g = vb_g / P.rr_p, vb_b = vb_b / P.rr_p;
                }
            } else {
                nee_v = active;
                if (EXT && mfz < 0.0f) {  // (a glossy vertex: the throughput in front of it, the roulette's division included)
                    if (P.rr_p > 0.0f) vb_r = vb_r / P.rr_p, vb_g = vb_g / P.rr_p, vb_b = vb_b / P.rr_p;
                } else
                vb_r = beta_r, vb_g = beta_g, vb_b = beta_b;
            }
        }
        if (NEE && nee_v) {
            const float u0 = rng_next<COUNT>(rng), u1 = rng_next<COUNT>(rng), u2 = rng_next<COUNT>(rng);
            const float xs = u0 * (float)P.nl;
            int li = min((int)xs, P.nl - 1);
            const float4 al = image[P.off_alias + li];
            if (xs - (float)li >= al.x) li = __float_as_int(al.y);
            const float4 *lr = image + P.off_light + RT_LIGHT_STRIDE * li;
            const float4 h = lr[0];
            const int shape = __float_as_int(h.x);
            float ldx = 0, ldy = 0, ldz = 0, pl = 0;  // y - p and the light strategy's solid-angle density of that direction
            float ev_r = 0, ev_g = 0, ev_b = 0;       // ENV: the environment's radiance in the sampled direction
            if (ENV && shape == 3) {
                // the environment: u1 -> row and cos(theta) within its band, u2 -> column and azimuth within the texel; radiance
                // and density of the direction as it came out, through the lookup a BSDF ray that escapes goes through
                const EnvView EV = env_view();
                float pe;
                env_sample(EV, u1, u2, ldx, ldy, ldz);
                env_eval(EV, ldx, ldy, ldz, ev_r, ev_g, ev_b, pe);
                pl = h.z * pe;
            } else if (shape == 0 || shape == 8) {
                // sphere: a direction uniform in the cone it subtends, then the nearer intersection.  A distant light
                // goes through the same cone code (light_cone_direction, rt_lights.h: one copy of the sincosf and the frame)
                // with the record's axis t and 1 - cos(alpha); its ld is D e and its density the selection probability alone
                const float4 g = lr[3];
                const bool far = shape == 8;
                float ax = g.x, ay = g.y, az = g.z, omc = g.w, c = 0.0f, c2 = 0.0f, r2 = 0.0f;
                bool cone = true;
                if (!far) {
                    const float wx = g.x - px, wy = g.y - py, wz = g.z - pz;
                    c2 = dot3(wx, wy, wz, wx, wy, wz), r2 = g.w * g.w;
                    cone = c2 > r2;
                    omc = cone_one_minus_cos(r2, c2);
                    c = sqrtf(c2);
                    const float ic = 1.0f / c;
                    ax = wx * ic, ay = wy * ic, az = wz * ic;
                }
                if (cone) {
                    float ex, ey, ez, cth, sth;
                    light_cone_direction(ax, ay, az, omc, u1, u2, ex, ey, ez, cth, sth);
                    float tt = c * cth - sqrtf(fmaxf(0.0f, r2 - c2 * (sth * sth)));
                    pl = h.z / ((2.0f * kPi) * omc);
                    if (far) tt = lr[4].x, pl = h.z;
                    ldx = tt * ex, ldy = tt * ey, ldz = tt * ez;
                }
            } else if (shape >= 6) {  // point and spot lights (rt_lights.h): ld = x - p, density psel d^2 (/ falloff)
                const float4 g = lr[3];
                ldx = g.x - px, ldy = g.y - py, ldz = g.z - pz;
                const float d2 = dot3(ldx, ldy, ldz, ldx, ldy, ldz);
                pl = point_light_density(h.z, d2);
                if (shape == 7) {
                    const float4 a = lr[4], k = lr[5];
                    pl = spot_light_density(h.z, d2, spot_falloff(a.x, a.y, a.z, ldx, ldy, ldz, d2, k.x, k.y));
                }
            } else {
                float lnx, lny, lnz;  // the light's normal at y
                if (shape == 1) {  // rect: uniform by area
                    const float4 g = lr[3], g2 = lr[4];
                    const float a = fmaf(u1, g.y - g.x, g.x), b = fmaf(u2, g.w - g.z, g.z);
                    const int axis = __float_as_int(g2.y);  // 0: z = k, 1: y = k, 2: x = k
                    const float yx = axis == 2 ? g2.x : a, yy = axis == 0 ? b : (axis == 1 ? g2.x : a), yz = axis == 0 ? g2.x : b;
                    ldx = yx - px, ldy = yy - py, ldz = yz - pz;
                    lnx = axis == 2 ? 1.0f : 0.0f, lny = axis == 1 ? 1.0f : 0.0f, lnz = axis == 0 ? 1.0f : 0.0f;
                } else {
                    // the four geometry records of a tube or a triangle, loaded once for both: nothing of the triangle's is
                    // live outside its branch
                    const float4 m0 = lr[3], m1 = lr[4], m2 = lr[5], g = lr[6];
                    if (shape == 4 || shape == 5) {  // triangle (mesh lights): uniform by area, y = v1 + b1 e1 + b2 e2 with
                        // {v1, e1, e2, n} = {m0, m1, m2, g}; quad (quad_light_point, rt_quad.h): y = Q + u1 u + u2 v
                        // with {Q, u, v, n} in the same records -- the triangle's expression with b1 = u1, b2 = u2
                        const float s = sqrtf(u1);
                        const float b1 = shape == 5 ? u1 : 1.0f - s, b2 = shape == 5 ? u2 : u2 * s;
                        ldx = fmaf(b2, m2.x, fmaf(b1, m1.x, m0.x)) - px;
                        ldy = fmaf(b2, m2.y, fmaf(b1, m1.y, m0.y)) - py;
                        ldz = fmaf(b2, m2.z, fmaf(b1, m1.z, m0.z)) - pz;
                        lnx = g.x, lny = g.y, lnz = g.z;  // the geometric normal, whatever the vertex normals (the hit side's too)
                    } else {  // cylinder tube: uniform by area in object space, through the (rigid) object-to-world transform
                        float sp, cp;
                        sincosf((2.0f * kPi) * u1, &sp, &cp);
                        const float qx = g.x * cp, qy = g.x * sp, qz = fmaf(u2, g.z - g.y, g.y);
                        ldx = fmaf(m0.x, qx, fmaf(m0.y, qy, fmaf(m0.z, qz, m0.w))) - px;
                        ldy = fmaf(m1.x, qx, fmaf(m1.y, qy, fmaf(m1.z, qz, m1.w))) - py;
                        ldz = fmaf(m2.x, qx, fmaf(m2.y, qy, fmaf(m2.z, qz, m2.w))) - pz;
                        lnx = fmaf(m0.x, cp, m0.y * sp), lny = fmaf(m1.x, cp, m1.y * sp), lnz = fmaf(m2.x, cp, m2.y * sp);
                    }
                }
                const float d2 = dot3(ldx, ldy, ldz, ldx, ldy, ldz);
                pl = ((h.z * h.w) * (d2 * sqrtf(d2))) / fabsf(dot3(lnx, lny, lnz, ldx, ldy, ldz));
            }
            // the BSDF's density of that direction (its f cos is albedo x pdf_b for both materials)
            const float d2 = dot3(ldx, ldy, ldz, ldx, ldy, ldz);
            const float il = 1.0f / sqrtf(d2);
            const float wx = ldx * il, wy = ldy * il, wz = ldz * il;
            const float wn = dot3(wx, wy, wz, nx, ny, nz);
            float pb = 0.0f;
            float gf_r = 1.0f, gf_g = 1.0f, gf_b = 1.0f;  // a glossy vertex: f cos of the light's direction
            const bool glossy = EXT && mfz < 0.0f;
            if (glossy) {
                // the material again, from its record and the hit (the frame is rebuilt from n: nothing of it is kept live
                // across the roulette section); which record and which kind: the bits of mfz
                const uint32_t gbits = __float_as_uint(mfz);
                const int gkind = (int)((gbits >> 24) & 63u);
                const float4 *M = rec_at(image + P.off_mat, __umul24(gbits & 0xffffffu, 48u));
                const float4 q0 = M[0], q1 = M[1], q2 = M[2];
                const bool glass = (gkind & ~1) == MK_ROUGH_GLASS;  // (bit 0 of the kind: a back hit)
                // a vertex of pbr origin (bit 0: it chose the metal lobe): alpha, r and the colour are the hit's own,
                // from gtex, not the record's
                const bool pbr = gkind >= MK_PBR;
                const bool plastic = gkind != MK_ROUGH_METAL && !glass && gkind != MK_PBR + 1;
                const float g_alpha = pbr ? pbr_alpha(pbr_unit(gtex >> 24)) : q0.y;
                float f_r = q1.x, f_g = q1.y, f_b = q1.z, rh_r = 0.0f, rh_g = 0.0f, rh_b = 0.0f;
                if (gkind == MK_PBR + 1) f_r = pbr_unit(gtex & 255u), f_g = pbr_unit((gtex >> 8) & 255u), f_b = pbr_unit((gtex >> 16) & 255u);
                if (glass) f_r = f_g = f_b = 1.0f;  // (its c0 is sigma; its tint is in vb already)
                if (plastic) {
                    const bool odd = gkind == MK_PLASTIC_CHECKER && checker_odd(px, py, pz);
                    rh_r = odd ? q2.x : q1.x, rh_g = odd ? q2.y : q1.y, rh_b = odd ? q2.z : q1.z;
                    if (gkind == MK_PLASTIC_IMAGE || pbr)  // (the texel as image_texel made it: the same byte over 255)
                        rh_r = (float)(gtex & 255u) / 255.0f, rh_g = (float)((gtex >> 8) & 255u) / 255.0f, rh_b = (float)((gtex >> 16) & 255u) / 255.0f;
                    // (a noise texture: 8 bits a channel would lose it.  Evaluated again at the hit point, which is still in
                    //  px, py, pz: the same operations on the same floats, so the rho the vertex scattered with, bit for bit)
                    if (gkind == MK_PLASTIC_NOISE) {
                        const float4 c = noise_texel(image, q1, q2, px, py, pz);
                        rh_r = c.x, rh_g = c.y, rh_b = c.z;
                    }
                    f_r = f_g = f_b = q0.z;
                }
                glossy_eval_body(glass ? GLOSSY_GLASS : (plastic ? GLOSSY_PLASTIC : GLOSSY_METAL), nx, ny, nz, mrx, mry, mrz, g_alpha, f_r, f_g, f_b, rh_r,
                                 rh_g, rh_b, (gkind & 1) ? q1.w : q0.z, wx, wy, wz, gf_r, gf_g, gf_b, pb, !ENV);
            } else
            if (MEDIA && NEE && kind == MK_MEDIUM) {
                // a medium vertex: the phase function's density of the light's direction about the direction of travel
                // (kept in mr); no cosine, so f = albedo x pdf_b and the lambertian form below holds
                pb = nx == 0.0f ? RT_PHASE_ISOTROPIC : phase_hg_eval(nx, dot3(mrx, mry, mrz, wx, wy, wz));
            } else
            if (wn > 0.0f) pb = mfz > 0.0f ? metal_pdf(wx, wy, wz, mrx, mry, mrz, mfz) : wn * kInvPi;
            // f cos / p_l x the power heuristic's p_l^2 / (p_l^2 + pdf_b^2) = albedo x pdf_b p_l / (p_l^2 + pdf_b^2)
            // (glossy: f cos x p_l / (p_l^2 + pdf_b^2), f cos per channel)
            // An analytic light (shapes 6, 7, 8) is sampled by this strategy alone: weight 1, f cos / p_l
            const bool delta = shape >= 6;
            float wgt = (pl > 0.0f && pb > 0.0f && d2 > 0.0f) ? pb / (delta ? pl : pl + pb * (pb / pl)) : 0.0f;
            if (glossy) {
                wgt = (pl > 0.0f && pb > 0.0f && d2 > 0.0f) ? 1.0f / (delta ? pl : pl + pb * (pb / pl)) : 0.0f;
                vb_r *= gf_r, vb_g *= gf_g, vb_b *= gf_b;
            }
            if (wgt > 0.0f) {
                const float lx = px + ldx, ly = py + ldy, lz = pz + ldz;
                const float4 e0 = lr[1], e1 = lr[2];
                const bool odd = __float_as_int(e0.w) != 0 && checker_odd(lx, ly, lz);
                pend_r = vb_r * (odd ? e1.x : e0.x) * wgt;
                pend_g = vb_g * (odd ? e1.y : e0.y) * wgt;
                pend_b = vb_b * (odd ? e1.z : e0.z) * wgt;
                // the lane's next query is the shadow ray from p to y; the continuation waits
                shadow = nee_end ? 2 : 1;
                if (ENV && shape == 3) {
                    pend_r = vb_r * ev_r * wgt, pend_g = vb_g * ev_g * wgt, pend_b = vb_b * ev_b * wgt;
                    shadow |= 4;
                }
                cdx = dx, cdy = dy, cdz = dz;
                ox = px, oy = py, oz = pz;
                dx = ldx, dy = ldy, dz = ldz;
                ra = d2;
                rinv_a = 1.0f / ra;
                active = true;
            }
        }
    }

    if (COUNT) {
        // one atomic per wave per counter
        auto wave_add = [&](unsigned long long *p, uint32_t v) {
            unsigned long long t = v;
            for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
            if (lane == 0 && t) atomicAdd(p, t);
        };
        wave_add(&counters->samples, c_samples);
        wave_add(&counters->queries, c_queries);
        wave_add(&counters->hits, c_hits);
        wave_add(&counters->misses, c_misses);
        wave_add(&counters->scatter[0], c_scatter0);
        wave_add(&counters->scatter[1], c_scatter1);
        wave_add(&counters->scatter[2], c_scatter2);
        wave_add(&counters->scatter[3], c_scatter3);
        wave_add(&counters->rng_draws, rng.draws);
        wave_add(&counters->cand_lanes, c_cand);
        wave_add(&counters->cand_waves, c_cand_wave);
        if (lane == 0 && c_clusters) atomicAdd(&counters->clusters_visited, (unsigned long long)c_clusters);
        if (lane == 0 && c_groups) atomicAdd(&counters->groups_visited, (unsigned long long)c_groups);
        wave_add(&counters->lane_clusters, c_lane_clusters);
        wave_add(&counters->lane_groups, c_lane_groups);
        wave_add(&counters->lane_cands, c_lane_cands);
        wave_add(&counters->group_maxpop, c_group_maxpop);
        wave_add(&counters->query_maxpop, c_query_maxpop);
        wave_add(&counters->walk_resumed, c_walk_resumed);
        if (lane == 0) {
            for (int i = 0; i < 6; ++i) atomicAdd(&counters->cycles[i], cyc[i]);
            const unsigned long long t = __builtin_amdgcn_s_memrealtime();
            atomicMin(&counters->t_end_min, t);
            atomicMax(&counters->t_end_max, t);
            atomicAdd(&counters->life_cycles, __builtin_amdgcn_s_memtime() - c_begin);
            atomicAdd(&counters->life_ticks, t - t_begin);
            atomicMin(&counters->t_qe_min, t_qe);
            atomicMax(&counters->t_qe_max, t_qe);
            const unsigned long long bin = (t - t_qe) / 5000ull;  // 100 MHz ticks -> 50 us bins
            atomicAdd(&counters->drain_hist[bin < 31 ? bin : 31], 1u);
            const unsigned long long b1 = (t_qe - t_begin) / 6400ull, b2 = (t - t_begin) / 6400ull;
            atomicAdd(&counters->qe_hist[b1 < 1023 ? b1 : 1023], 1u);
            atomicAdd(&counters->exit_hist[b2 < 1023 ? b2 : 1023], 1u);
        }
        wave_add(&counters->wave_queries, c_wave_queries);
    }
