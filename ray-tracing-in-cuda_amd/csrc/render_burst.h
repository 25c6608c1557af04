// The burst of render_body.h (variants 2 and 6, kernels.h): all 64 lanes of the wave prepare batch cursor >> 6 of the current
// item -- lane l one sample of its home pixel -- and fill the wave's slab.  Text of its own because it has two places, of which an
// instance compiles one: inside the refill, where the slab runs out (RT_BURST_TRACE=0: camera rays only), and at the
// top of the main loop's iteration (the default).  The including site puts a wave barrier on either side.
// Slot l afterwards, 10 words: {o.xyz, d.x} {d.yz, g.xy} {g.zw} without TRACE; with it {p.xyz, d.x} ... for a path whose camera
// ray hit a surface that scatters, p the hit point and the winner's id in bits 16 .. 30 of lane l's c_hy, and a NaN in d.x for
// every other slot: off the image, ended by the roulette, gone to the sky or the background, or ended on an emitter (both
// added to the tile accumulator here).
                        // TRACE: the lane's camera ray stays in registers for the query below; b_live: a path continues from it
                        float b_ox = 0.0f, b_oy = 0.0f, b_oz = 0.0f, b_dx = 0.0f, b_dy = 0.0f, b_dz = 1.0f;
                        bool b_live = false;
                        // LISTS (kernels.h, RT_BURST_LISTS; rt_beam.h): the tile's record of the beam table -- the staged spheres a camera
                        // ray of this tile can be flagged for at all -- by two wave-uniform loads, the table's address from behind the
                        // item parameters and the record at whole-frame tile (x0 / 8, home row of lane 0 / 8).  Issued here, so that
                        // they travel while the lanes seed their streams; read and dead inside the burst.  (Lane 0's pixel is on the
                        // image whenever the item is: its c_hy is a row.)
                        [[maybe_unused]] unsigned long long b_w0 = kBeamOverflow, b_w1 = 0ull, b_w2 = 0ull, b_w3 = 0ull;  // (no table: as the mark)
                        if constexpr (LISTS) {
                            typedef const __attribute__((address_space(4))) unsigned long long *BeamWords;
                            asm volatile("" ::: "memory");
                            const unsigned long long b_table = *(BeamWords)(uintptr_t)(queue + RT_BEAMS_AT);
                            if (b_table != 0ull) {
                                const int b_ty = (__builtin_amdgcn_readfirstlane(c_hy) & 0xffff) >> 3;
                                const uint32_t b_tile = __umul24((uint32_t)b_ty, (uint32_t)P.tiles_x) + (uint32_t)(c_x0 >> 3);
                                BeamWords b_rec = (BeamWords)(uintptr_t)(b_table + (unsigned long long)b_tile * (kBeamRecordWords * 2));
                                b_w0 = b_rec[0], b_w1 = b_rec[1], b_w2 = b_rec[2], b_w3 = b_rec[3];
                            }
                        }
                        if (c_hy >= 0) {
                            const int bx = c_x0 + (lane & 7);
                            const int by = TRACE ? (c_hy & 0xffff) : c_hy;  // (TRACE: a winner's id above the row, below)
                            const uint32_t pixel = __umul24((uint32_t)by, (uint32_t)P.width) + (uint32_t)bx;
                            LaneRng br;
                            br.draws = 0;
                            rng_start(br, pixel, (uint32_t)(c_sbegin + (cursor >> 6)), k0, k1);
                            const float bu = ((float)bx + rng_next<false>(br)) * P.inv_wm1;
                            const float bv = ((float)by + rng_next<false>(br)) * P.inv_hm1;
                            float offx = 0.0f, offy = 0.0f, offz = 0.0f;
                            const float4 *cv = hot + P.off_cam;
                            const float4 c_org = cv[0];  // origin, lens_radius
                            if (P.flags & RT_FLAG_DEFOCUS_BLUR) {
                                // random_in_unit_disk (vec3.h:157-165): two draws per attempt; x^2 + y^2 as the merged loop forms it
                                float bsx, bsy;
                                do {
                                    bsx = rng_pm1<false>(br);
                                    bsy = rng_pm1<false>(br);
                                } while (fmaf(bsx, bsx, bsy * bsy) >= 1.0f);
                                const float4 c_u = cv[4], c_v = cv[5];
                                const float rdx = c_org.w * bsx, rdy = c_org.w * bsy;
                                offx = fmaf(c_u.x, rdx, c_v.x * rdy);
                                offy = fmaf(c_u.y, rdx, c_v.y * rdy);
                                offz = fmaf(c_u.z, rdx, c_v.z * rdy);
                            }
                            const float4 c_ll = cv[1], c_hor = cv[2], c_ver = cv[3];
                            float bdx = fmaf(bv, c_ver.x, fmaf(bu, c_hor.x, c_ll.x));
                            float bdy = fmaf(bv, c_ver.y, fmaf(bu, c_hor.y, c_ll.y));
                            float bdz = fmaf(bv, c_ver.z, fmaf(bu, c_hor.z, c_ll.z));
                            bdx = (bdx - c_org.x) - offx;
                            bdy = (bdy - c_org.y) - offy;
                            bdz = (bdz - c_org.z) - offz;
                            if constexpr (TRACE) {
                                // the roulette draw of a starting path (stage (6c) without TRACE): the next draw of the same state,
                                // before anything is added for the path -- one the roulette ends adds nothing.  The slot keeps the
                                // state after the draw
                                b_live = true;
                                if (P.rr_p > 0.0f) {
                                    if (rng_next<false>(br) > P.rr_p) b_live = false;
                                }
                                b_ox = c_org.x + offx, b_oy = c_org.y + offy, b_oz = c_org.z + offz;
                                b_dx = bdx, b_dy = bdy, b_dz = bdz;
                            } else {
                                slab_a[lane] = make_float4(c_org.x + offx, c_org.y + offy, c_org.z + offz, bdx);
                            }
                            slab_b[lane] = make_float4(bdy, bdz, __uint_as_float(br.g.x), __uint_as_float(br.g.y));
                            slab_c[lane] = make_float2(__uint_as_float(br.g.z), __uint_as_float(br.g.w));
                        } else {
                            if constexpr (!TRACE) slab_a[lane] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0x7fc00000u));
                        }
                        if constexpr (TRACE) {
                            // ---- the first closest-hit query of the 64 paths: one sample of every pixel of the tile, the most
                            // coherent query the kernel runs, at full occupancy.  It is the text of stage (1) (render_query.h), on
                            // this block's own ray behind the names that text reads; the walk runs to completion.  The query takes
                            // no draw, so every sample's stream is what it was.
                            const float ox = b_ox, oy = b_oy, oz = b_oz, dx = b_dx, dy = b_dy, dz = b_dz;
                            const float ra = dot3(dx, dy, dz, dx, dy, dz), rinv_a = 1.0f / ra;  // (stage (6c)'s expressions)
                            const bool active = b_live;
                            [[maybe_unused]] const bool b_listed = LISTS && (uint32_t)(b_w0 & 0xffffull) != (uint32_t)kBeamOverflow;
                            float t_res = 0.0f;
                            float4 rec = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0x7fc00000u));  // (nobody continues from here)
                            {
#define RT_QUERY_CUT false
#define RT_QUERY_SKIP (LISTS && b_listed)
#include "render_query.h"
#undef RT_QUERY_SKIP
#undef RT_QUERY_CUT
                                // LISTS: behind a record without the overflow mark the query is one wave-uniform loop over its ids --
                                // the test, the resolve, the tie rule and kTMin of the text above; no prefix, no grid clip, no walk
                                // (RT_QUERY_SKIP took them out).  An empty record: every live lane misses
                                if constexpr (LISTS) {
                                    if (b_listed) {
                                        for (int b_n = (int)(b_w0 & 0xffffull); b_n > 0; --b_n) {
                                            b_w0 = (b_w0 >> 16) | (b_w1 << 48), b_w1 = (b_w1 >> 16) | (b_w2 << 48);
                                            b_w2 = (b_w2 >> 16) | (b_w3 << 48), b_w3 >>= 16;
                                            const int b_id = (int)(b_w0 & 0xffffull);
                                            const float4 b_s = sph[b_id];
                                            if (active) RT_SPHERE_TEST(b_s, b_id)
                                        }
                                    }
                                }
#undef RT_SPHERE_TEST
                                // ---- the outcome, stage (2)'s expressions.  A path that ends here -- the sky or the background on
                                // a miss, an emitter -- adds its sample to the lane's OWN pixel of the tile (lane = home pixel: no
                                // two lanes meet) with the exact fixed-point add of stage (3), and leaves a dead slot.  A hit that
                                // scatters leaves {p, d, state}; the origin is dead once p exists.
                                if (active) {
                                    const float bb = P.rr_p > 0.0f ? 1.0f / P.rr_p : 1.0f;  // the throughput of a path that starts
                                    float e_r = 0.0f, e_g = 0.0f, e_b = 0.0f;
                                    bool ends = true;
                                    if (best_id >= 0) {
                                        const float4 cold = *rec_at(image + P.off_sph_cold, (uint32_t)best_id << 4);
                                        const float hx = fmaf(best_t, dx, ox), hy = fmaf(best_t, dy, oy), hz = fmaf(best_t, dz, oz);
                                        const int hkind = __float_as_int(cold.w);
                                        if (hkind >= MK_LIGHT_SOLID && (!EXT || hkind <= MK_LIGHT_IMAGE)) {  // diffuse_light: emitted, never scatters (stage (2)'s test)
                                            const float4 *M = image + P.off_mat + 3 * __float_as_int(cold.y);
                                            const float4 q1 = M[1], q2 = M[2];
                                            const bool odd = hkind == MK_LIGHT_CHECKER && checker_odd(hx, hy, hz);
                                            e_r = (odd ? q2.x : q1.x) * bb, e_g = (odd ? q2.y : q1.y) * bb, e_b = (odd ? q2.z : q1.z) * bb;
                                        } else {
                                            ends = false;
                                            rec = make_float4(hx, hy, hz, dx);
                                            c_hy = (c_hy & 0xffff) | (best_id << 16);
                                        }
                                    } else {
                                        float bg_r, bg_g, bg_b;
                                        if (P.flags & RT_FLAG_SKY_GRADIENT) {
                                            const float il = 1.0f / rt_sqrtf<ROOT_VOTE>(ra);
                                            const float t = 0.5f * (il * dy + 1.0f);
                                            const float omt = 1.0f - t;
                                            bg_r = fmaf(t, 0.5f, omt), bg_g = fmaf(t, 0.7f, omt), bg_b = fmaf(t, 1.0f, omt);
                                        } else {
                                            bg_r = P.background[0], bg_g = P.background[1], bg_b = P.background[2];
                                        }
                                        e_r = bb * bg_r, e_g = bb * bg_g, e_b = bb * bg_b;
                                    }
                                    if (ends) {
                                        unsigned long long *a = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(c_acc) + __umul24((uint32_t)lane, 24u));
                                        atomicAdd(a + 0, radiance_to_fixed(e_r));
                                        atomicAdd(a + 1, radiance_to_fixed(e_g));
                                        atomicAdd(a + 2, radiance_to_fixed(e_b));
                                    }
                                }
                            }
                            slab_a[lane] = rec;
                            if (RT_PRIO_H != RT_PRIO_F) __builtin_amdgcn_s_setprio(RT_PRIO_F);
                        }
