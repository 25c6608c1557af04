// The closest-hit query of render_body.h -- the always-tested prefix and the instance's candidate search -- as text of its own,
// because the kernels with bursts (variants 2 and 6, kernels.h) run it at TWO places: in the main loop, stage (1), for every
// live lane, and in the burst of the refill, for the 64 camera rays the wave has just prepared.  One text, so the two cannot
// drift apart: the same tests, the same resolve, the same tie rule, the same kTMin.  It reads the ray of the lanes with `active`
// set from the names ox, oy, oz, dx, dy, dz, ra, rinv_a of the scope that includes it and a cut-short walk's resumption point
// from t_res (the burst declares its own behind those names); it leaves best_t, best_id, far_scan, far_m and blim in that
// scope.  RT_QUERY_CUT, defined by the including site: may a walk's stragglers be cut short and go on in the next iteration
// (RT_WALK_TAIL)?  The main loop: true.  A burst has no next iteration: false, its walk runs to completion.
// RT_QUERY_SKIP, likewise: a wave-uniform condition under which the prefix and the candidate search are left out and the
// site tests its own candidates with the text's RT_SPHERE_TEST and resolve.  The main loop: false.  A burst whose tile has a
// list (render_burst.h, RT_BURST_LISTS): true.
            // ---- closest-hit query over the LDS-resident list (hittable_list::hit,
            // object.cuh:23-37).  Wave-uniform trip counts; `best_id` is the grouped id.
            // (a shadow ray ends just short of its light point y = o + d: any hit before that occludes)
            // (ENV: the shadow ray towards the environment -- shadow bit 2 -- has no far end)
            // (QUERY: the ray's own far end)
            // (ALPHA: ... less what the query has covered on its way through holes; al_t is 0 otherwise)
            float best_t = QUERY ? q_tmax : (NEE && shadow != 0 && !(ENV && (shadow & 4) != 0)) ? 0.999f : INFINITY;
            if constexpr (ALPHA && NEE) {
                if (shadow != 0 && !(ENV && (shadow & 4) != 0)) best_t = 0.999f - al_state[AL_T];
            }
            int best_id = -1;

            // spheres: sphere::hit, object.cuh:47-75.  Early-outs that need no sqrt:
            //   disc < 0                      -> no real root
            //   hb >= 0 and c >= 0            -> both roots <= 0 < t_min  (then
            //     sqrt(disc) <= sqrt(fl(hb*hb)) = hb, so (-hb + sqrtd) <= 0 exactly)
            // The closest hit does not depend on the visiting order (ties go to the later
            // list entry, resolved through list_index_of), so the device table is sorted
            // big-spheres-first.
            auto resolve = [&](int idx, float hb, float disc) {
                if (COUNT) {  // diagnostic: candidate lanes, and entries of this block per wave
                    c_cand++;
                    const unsigned long long em = __builtin_amdgcn_ballot_w64(true);
                    if ((int)__builtin_ctzll(em) == lane) c_cand_wave++;
                }
                const float sq = rt_sqrtf<ROOT_VOTE>(disc);
                float root = (-hb - sq) * rinv_a;
                if (root < kTMin || best_t < root) root = (-hb + sq) * rinv_a;
                // straight-line: the winner by two selects, and the tie rule -- which reads global memory and practically
                // never runs -- behind one vote of the wave.  (As three nested lane-level `if`s -- range, tie, take -- every
                // entry paid three exec-mask save / branch / restore groups.)
                bool take = !(root < kTMin || best_t < root);
                const bool tie = take && root == best_t && best_id >= 0;
                if (__builtin_expect(__builtin_amdgcn_ballot_w64(tie) != 0ull, 0)) {
                    if (tie) take = lidx(idx) > lidx(best_id);
                }
                best_t = take ? root : best_t;
                best_id = take ? idx : best_id;
            };
            // the point where the ray meets a triangle's plane and its ray parameter (hittable.py:44-52, 61):
            // n = the unit normal turned towards the origin, theta = d.n / |d| < 0, r = o - d/|d| (oc.n) / theta
            // (|d| and d / |d| belong to the ray, not to the triangle: one square root and three divisions per query instead of per
            //  test -- a triangle test is about 190 instructions, 41 of them these)
            float tq_a = 1.0f, tq_ux = 0.0f, tq_uy = 0.0f, tq_uz = 0.0f;
            if (EXT && nt > 0 && active) {
                tq_a = rt_sqrtf<ROOT_VOTE>(ra);
                tq_ux = dx / tq_a, tq_uy = dy / tq_a, tq_uz = dz / tq_a;
            }
            auto tri_plane = [&](const float4 r0, const float4 r1, const float4 r2, float &rix, float &riy, float &riz,
                                 float &root) -> bool {
                float tnx = r0.w, tny = r1.w, tnz = r2.w;
                float ocn = dot3(ox - r0.x, oy - r0.y, oz - r0.z, tnx, tny, tnz);
                if (ocn < 0.0f) tnx = -tnx, tny = -tny, tnz = -tnz, ocn = -ocn;
                const float theta = dot3(dx, dy, dz, tnx, tny, tnz) / tq_a;
                if (!(theta < 0.0f)) return false;
                rix = ox - (tq_ux * ocn) / theta;
                riy = oy - (tq_uy * ocn) / theta;
                riz = oz - (tq_uz * ocn) / theta;
                root = ((-ocn) / theta) / tq_a;
                return true;
            };
#define RT_SPHERE_TEST(S, IDX)                                                                 \
    {                                                                                          \
        const float ocx = ox - S.x, ocy = oy - S.y, ocz = oz - S.z;                            \
        const float hb = dot3(ocx, ocy, ocz, dx, dy, dz);                                      \
        const float cc = fmaf(ocx, ocx, fmaf(ocy, ocy, fmaf(ocz, ocz, -S.w)));                 \
        const float disc = fmaf(hb, hb, -(ra * cc));                                           \
        const bool cand = RT_CAND(disc, hb, cc);                                                \
        if (__builtin_expect(cand, 0)) resolve(IDX, hb, disc);                                 \
    }
            // the same test with the candidate PARKED in (p_idx, p_hb, p_disc) instead of resolved on the spot: the cold block
            // (IEEE sqrt, both roots, range and tie rules: ~45 instructions) runs once for the candidates of several
            // records.  The closest hit does not depend on the order in which candidates are resolved (a candidate's root
            // is its smallest one >= t_min, accepted while it is <= best_t: the outcome is the minimum over candidates, ties
            // by list index), so parking is free to reorder.  A lane that finds a second candidate resolves the first there.
#define RT_SPHERE_PARK(S, IDX)                                                                 \
    {                                                                                          \
        const float ocx = ox - S.x, ocy = oy - S.y, ocz = oz - S.z;                            \
        const float hb = dot3(ocx, ocy, ocz, dx, dy, dz);                                      \
        const float cc = fmaf(ocx, ocx, fmaf(ocy, ocy, fmaf(ocz, ocz, -S.w)));                 \
        const float disc = fmaf(hb, hb, -(ra * cc));                                           \
        const bool cand = RT_CAND(disc, hb, cc);                                                \
        if (__builtin_expect(cand, 0)) {                                                       \
            if (p_idx >= 0) resolve(p_idx, p_hb, p_disc);                                      \
            p_idx = IDX, p_hb = hb, p_disc = disc;                                             \
        }                                                                                      \
    }
            if (RT_PRIO_Q != RT_PRIO_S) __builtin_amdgcn_s_setprio(RT_PRIO_Q);
            if (active && !RT_QUERY_SKIP) {
            // the always-tested prefix (big spheres, largest first), four records at a time: the first one -- in RTIOW the
            // ground, a candidate for half of the lanes -- is resolved at once, the other three share one resolve
            for (int i = 0; i < P.np; i += 4) {
                const float4 s0 = sph[i], s1 = sph[i + 1], s2 = sph[i + 2], s3 = sph[i + 3];
                RT_SPHERE_TEST(s0, i)
                int p_idx = -1;
                float p_hb = 0.0f, p_disc = 0.0f;
                asm volatile("" : "=v"(p_hb), "=v"(p_disc));  // (read only where p_idx >= 0, which comes with their values)
                RT_SPHERE_PARK(s1, i + 1)
                RT_SPHERE_PARK(s2, i + 2)
                RT_SPHERE_PARK(s3, i + 3)
                if (p_idx >= 0) resolve(p_idx, p_hb, p_disc);
            }
            if (!CULL) {
                // flat scan (the reference's hittable_list loop) of every cluster's 8 records (clusters are 9 slots apart,
                // see the packer): 16 records per iteration -- two clusters, the never-hit slot between them skipped -- in two
                // register sets of four fetched half a step ahead of their use; the table ends with all-padding clusters, so
                // the last read-ahead stays inside it
                {
                    constexpr int kStep = 2 * (CSIZE + 1);
#define RT_OFF(k) ((k) + ((k) >= CSIZE ? 1 : 0))
                    const int iters = (P.ncl * CSIZE + 15) / 16;
                    int base = P.np;
                    float4 a0 = sph[base], a1 = sph[base + 1], a2 = sph[base + 2], a3 = sph[base + 3];
                    for (int it = 0; it < iters; ++it) {
#pragma unroll
                        for (int k = 0; k < 16; k += 8) {
                            const float4 b0 = sph[base + RT_OFF(k + 4)], b1 = sph[base + RT_OFF(k + 5)],
                                         b2 = sph[base + RT_OFF(k + 6)], b3 = sph[base + RT_OFF(k + 7)];
                            RT_SPHERE_TEST(a0, base + RT_OFF(k))
                            RT_SPHERE_TEST(a1, base + RT_OFF(k + 1))
                            RT_SPHERE_TEST(a2, base + RT_OFF(k + 2))
                            RT_SPHERE_TEST(a3, base + RT_OFF(k + 3))
                            const int nxt = k + 8 < 16 ? RT_OFF(k + 8) : kStep;
                            a0 = sph[base + nxt], a1 = sph[base + nxt + 1], a2 = sph[base + nxt + 2], a3 = sph[base + nxt + 3];
                            RT_SPHERE_TEST(b0, base + RT_OFF(k + 4))
                            RT_SPHERE_TEST(b1, base + RT_OFF(k + 5))
                            RT_SPHERE_TEST(b2, base + RT_OFF(k + 6))
                            RT_SPHERE_TEST(b3, base + RT_OFF(k + 7))
                        }
                        base += kStep;
                    }
#undef RT_OFF
                }
            }
            }
            tick(1);
            // ---- culling set-up (CULL): aabb::hit (aabb.hpp:15-29) for every live lane, then one wave-wide
            // vote per box; used for the sphere clusters and for each cylinder's bounding box
            // 1-ulp reciprocals are enough here: the box test only has to be conservative, and the
            // margin below is five orders of magnitude larger than their error
            // Clamped to +-1e18: a direction component that is exactly 0 (a fuzz-free mirror produces them)
            // would give inf, and the fma form below inf - inf = NaN on the face behind the origin, which
            // min/max then drop together with the slab.  With a huge finite value the axis keeps its
            // meaning: origin inside the slab -> (-huge, +huge), outside -> both of one sign -> dead.
            // The values are only needed around the box tests; they are derived where those sit (per window of
            // clusters, and once more for the cylinders' and triangles' boxes) instead of once per query, so that
            // the ten registers are free while the wave walks its clusters -- the kernel's register peak.
            struct BoxP {
                float idx, idy, idz, nxm, nym, nzm, nxp, nyp, nzp, marg;
            };
            auto box_params = [&]() -> BoxP {
                BoxP b;
                b.idx = __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(dx), -1e18f, 1e18f);
                b.idy = __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(dy), -1e18f, 1e18f);
                b.idz = __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(dz), -1e18f, 1e18f);
                // per-lane box margin covering the fp32 error of the sphere test at this origin's
                // distance (derivation in render_host.hip): two shifted origins, nothing per box
                b.marg = 4e-3f * (fmaxf(fmaxf(fabsf(ox), fabsf(oy)), fabsf(oz)) + P.cull_extent1);
                // slab distances as one fma per face: t = b * (1/d) - (o +- marg) * (1/d).  The products
                // cancel to an absolute error ~ eps |o/d|, i.e. ~1e-7 |o| in space: four orders of
                // magnitude inside the margin.
                b.nxm = -(ox + b.marg) * b.idx, b.nym = -(oy + b.marg) * b.idy, b.nzm = -(oz + b.marg) * b.idz;
                b.nxp = -(ox - b.marg) * b.idx, b.nyp = -(oy - b.marg) * b.idy, b.nzp = -(oz - b.marg) * b.idz;
                return b;
            };
            const float4 *box = hot + (P.off_box - gap);
            const float4 *gbox = hot + (P.off_gbox - gap);
            // best_t (1 + 1e-4), refreshed whenever spheres have been tested (a stale, larger value only
            // culls less)
            float blim = best_t * 1.0001f;
            auto slab_live = [&](const BoxP &b, const float4 bmn, const float4 bmx) -> bool {
                const float lx = fmaf(bmn.x, b.idx, b.nxm), ux = fmaf(bmx.x, b.idx, b.nxp);
                const float ly = fmaf(bmn.y, b.idy, b.nym), uy = fmaf(bmx.y, b.idy, b.nyp);
                const float lz = fmaf(bmn.z, b.idz, b.nzm), uz = fmaf(bmx.z, b.idz, b.nzp);
                // live  <=>  tn <= tf, tf >= 0, tn <= best_t (1 + 1e-4)
                //       <=>  max(tn, 0) <= min(tf, best_t (1 + 1e-4))          (NaN -> live)
                const float tn = fmaxf(fmaxf(fmaxf(fminf(lx, ux), fminf(ly, uy)), 0.0f), fminf(lz, uz));
                const float tf = fminf(fminf(fminf(fmaxf(lx, ux), fmaxf(ly, uy)), blim), fmaxf(lz, uz));
                return !(tn > tf);
            };
            // ---- the other primitives' tests (one primitive, index uniform or per lane)
            // axis-aligned rects: xy_rect/xz_rect/yz_rect::hit, object.cuh:105-192
            auto test_rect = [&](int j) {
                const float4 q0 = rect[2 * j], q1 = rect[2 * j + 1];
                const int axis = __float_as_int(q1.y);  // 0: z = k, 1: y = k, 2: x = k
                float ok, dk, oa, da, ob, db;
                if (axis == 0) ok = oz, dk = dz, oa = ox, da = dx, ob = oy, db = dy;
                else if (axis == 1) ok = oy, dk = dy, oa = ox, da = dx, ob = oz, db = dz;
                else ok = ox, dk = dx, oa = oy, da = dy, ob = oz, db = dz;
                const float t = (q1.x - ok) / dk;
                if (!(t < kTMin || t > best_t)) {
                    const float pa = fmaf(t, da, oa), pb = fmaf(t, db, ob);
                    if (!(pa < q0.x || pa > q0.y || pb < q0.z || pb > q0.w)) {
                        bool take = true;
                        if (t == best_t && best_id >= 0)  // tie: the later list entry wins
                            take = list_index_of(P, image, ns + j) > list_index_of(P, image, best_id);
                        if (take) {
                            best_t = t;
                            best_id = ns + j;
                        }
                    }
                }
            };
            // cylinders: cylinder::hit + quadratic, object.cuh:199-214, 233-290
            auto test_cyl = [&](int k) {
                const float4 r0 = cyl[RT_CYL_STRIDE * k], r1 = cyl[RT_CYL_STRIDE * k + 1], r2 = cyl[RT_CYL_STRIDE * k + 2], pr = cyl[RT_CYL_STRIDE * k + 3];
                const float oox = fmaf(r0.x, ox, fmaf(r0.y, oy, fmaf(r0.z, oz, r0.w)));
                const float ooy = fmaf(r1.x, ox, fmaf(r1.y, oy, fmaf(r1.z, oz, r1.w)));
                const float ooz = fmaf(r2.x, ox, fmaf(r2.y, oy, fmaf(r2.z, oz, r2.w)));
                const float odx = fmaf(r0.x, dx, fmaf(r0.y, dy, r0.z * dz));
                const float ody = fmaf(r1.x, dx, fmaf(r1.y, dy, r1.z * dz));
                const float odz = fmaf(r2.x, dx, fmaf(r2.y, dy, r2.z * dz));
                const float qa = fmaf(odx, odx, ody * ody);
                const float qb = 2.0f * fmaf(odx, oox, ody * ooy);
                const float qc = fmaf(oox, oox, fmaf(ooy, ooy, -pr.x));
                const float delta = fmaf(qb, qb, -((4.0f * qa) * qc));
                if (!(delta < 0.0f)) {
                    const float sq = rt_sqrtf<ROOT_VOTE>(delta);
                    float t0 = (-0.5f * (qb - sq)) / qa;
                    float t1 = (-0.5f * (qb + sq)) / qa;
                    if (t0 > t1) {
                        const float tmp = t0;
                        t0 = t1;
                        t1 = tmp;
                    }
                    bool ok = !(t0 > best_t || t1 < kTMin);
                    float t = t0;
                    if (ok && t0 < kTMin) {
                        t = t1;
                        if (t > best_t) ok = false;
                    }
                    if (ok) {
                        float opz = fmaf(t, odz, ooz);
                        if (opz < pr.y || opz > pr.z) {
                            if (t == t1) ok = false;
                            else {
                                t = t1;
                                if (t > best_t || t < kTMin) ok = false;
                                else {
                                    opz = fmaf(t, odz, ooz);
                                    if (opz < pr.y || opz > pr.z) ok = false;
                                }
                            }
                        }
                    }
                    if (ok) {
                        bool take = true;
                        if (t == best_t && best_id >= 0)
                            take = list_index_of(P, image, ns + nr + k) > list_index_of(P, image, best_id);
                        if (take) {
                            best_t = t;
                            best_id = ns + nr + k;
                        }
                    }
                }
            };
            // triangles: hit_triangle, taichi-version/hittable.py:38-71 -- the plane of the triangle (its unit normal
            // turned towards the ray origin), then four same-side tests of the plane point
            auto test_tri = [&](int k) {
                const float4 r0 = tri[RT_TRI_STRIDE * k], r1 = tri[RT_TRI_STRIDE * k + 1], r2 = tri[RT_TRI_STRIDE * k + 2];
                float rix, riy, riz, root;
                if (tri_plane(r0, r1, r2, rix, riy, riz, root) && !(root < kTMin || root > best_t)) {
                    const float e21x = r1.x - r0.x, e21y = r1.y - r0.y, e21z = r1.z - r0.z;
                    const float e31x = r2.x - r0.x, e31y = r2.y - r0.y, e31z = r2.z - r0.z;
                    const float e32x = r2.x - r1.x, e32y = r2.y - r1.y, e32z = r2.z - r1.z;
                    const float a1x = rix - r0.x, a1y = riy - r0.y, a1z = riz - r0.z;
                    const float a2x = rix - r1.x, a2y = riy - r1.y, a2z = riz - r1.z;
                    float px_, py_, pz_, qx_, qy_, qz_;
                    cross3(a1x, a1y, a1z, e21x, e21y, e21z, px_, py_, pz_);
                    cross3(e31x, e31y, e31z, e21x, e21y, e21z, qx_, qy_, qz_);
                    const float n1 = dot3(px_, py_, pz_, qx_, qy_, qz_);
                    cross3(a2x, a2y, a2z, -e21x, -e21y, -e21z, px_, py_, pz_);
                    cross3(e32x, e32y, e32z, -e21x, -e21y, -e21z, qx_, qy_, qz_);
                    const float n2 = dot3(px_, py_, pz_, qx_, qy_, qz_);
                    cross3(a1x, a1y, a1z, e31x, e31y, e31z, px_, py_, pz_);
                    cross3(e21x, e21y, e21z, e31x, e31y, e31z, qx_, qy_, qz_);
                    const float n3 = dot3(px_, py_, pz_, qx_, qy_, qz_);
                    cross3(a2x, a2y, a2z, e32x, e32y, e32z, px_, py_, pz_);
                    cross3(-e21x, -e21y, -e21z, e32x, e32y, e32z, qx_, qy_, qz_);
                    const float n4 = dot3(px_, py_, pz_, qx_, qy_, qz_);
                    if (n1 > 0.0f && n2 > 0.0f && n3 > 0.0f && n4 > 0.0f) {
                        bool take = true;
                        if (root == best_t && best_id >= 0)
                            take = list_index_of(P, image, ns + nr + nc + k) > list_index_of(P, image, best_id);
                        if (take) {
                            best_t = root;
                            best_id = ns + nr + nc + k;
                        }
                    }
                }
            };
            // quads: quad_hit, rt_quad.h.  Nothing is live across the test but best_t / best_id, as in test_tri
            auto test_quad = [&](int k) {
                if constexpr (EXT) {
                    const float4 *qr = tri + RT_TRI_STRIDE * nt + RT_QUAD_STRIDE * k;
                    const float4 r0 = qr[0], r1 = qr[1], r2 = qr[2];
                    float t, qa, qb;
                    if (quad_hit(r0.x, r0.y, r0.z, r0.w, r1.w, r2.w, r1.x, r1.y, r1.z, r2.x, r2.y, r2.z, ox, oy, oz, dx, dy, dz, kTMin,
                                 best_t, t, qa, qb)) {
                        bool take = true;
                        if (t == best_t && best_id >= 0)
                            take = list_index_of(P, image, ns + nr + nc + nt + k) > list_index_of(P, image, best_id);
                        if (take) {
                            best_t = t;
                            best_id = ns + nr + nc + nt + k;
                        }
                    }
                }
            };
            bool far_scan = false;  // GRID: this lane's origin lies beyond the reach of the cells' lists: it scans what they list
            unsigned long long far_m = 0ull;  // VOTE_MASKS: ... and those lanes as a lane mask
            if (active && !RT_QUERY_SKIP) {
            if (GRID && P.grid_cells != 0) {  // (no cells: a scene small enough for every primitive to be tested per query)
                // ---- uniform grid, 3-D DDA per lane (the default).  The clustered spheres -- and, in the wide tables, the
                // rectangles, cylinders and triangles that are not oversized -- are listed in the cells their (error-grown, see
                // the packer) boxes touch; a lane walks the cells its ray crosses in the order it crosses them and tests what
                // they list, so the nearest hit ends the walk: a cell is only entered while its entry distance is within
                // best_t (1 + 1e-4).
                const float4 *gh = hot + P.off_grid;
                const float4 g_min = gh[0], g_inv = gh[1], g_size = gh[2];
                const int gnx = __float_as_int(gh[3].x), gny = __float_as_int(gh[3].y), gnz = __float_as_int(gh[3].z);
                const uint32_t *g_cells = reinterpret_cast<const uint32_t *>(hot + P.off_grid_cells);
                const uint16_t *g_items = reinterpret_cast<const uint16_t *>(hot + P.off_grid_items);
                const BoxP bp = box_params();
                // which tier of the cells' lists covers this lane's origin (the packer: |o| against ob_near, ob_far)
                const float o2 = fmaf(ox, ox, fmaf(oy, oy, oz * oz));
                const bool tier_far = o2 > g_min.w, beyond = o2 > g_inv.w;
                // cell header, compact: (first << 12) | (n_near << 6) | n_all;  wide: {first, n_near | n_all << 10 | n_other << 20}:
                // the sphere entries [first, + n_near) serve near origins, [first, + n_all) far ones, and the n_other entries
                // behind them are the cell's other primitives (grouped ids)
                const int cnt_shift = tier_far ? (WIDE ? 10 : 0) : (WIDE ? 0 : 6);
                constexpr int REM_BITS = WIDE ? 10 : 8;            // steps left per axis, packed in one register
                constexpr uint32_t REM_MASK = (1u << REM_BITS) - 1u, CNT_MASK = WIDE ? 1023u : 63u;
                constexpr bool OTHERS = WIDE && !SPH;
                const uint32_t *g_items32 = reinterpret_cast<const uint32_t *>(g_items);
                int ko = 0, koend = 0;  // OTHERS: the entries of the cell's other primitives still to test
                // NEST: a nested cell's header is {its sub-grid, 1023} (n_near = 1023 > n_all = 0: no list looks like that).  A lane
                // that steps into one walks the sub-grid front to back, clipped to its stay in the outer cell, and then takes up
                // the outer walk where it left it.  sub >= 0: the sub-grid this lane is about to enter; in_sub: it walks one, and
                // o_*: the outer walk's state meanwhile; t_cur: the ray parameter at which the lane entered its outer cell.
                int sub = -1;
                bool in_sub = false;
                float t_cur = 0.0f, o_tmx = 0.0f, o_tmy = 0.0f, o_tmz = 0.0f, o_texit = 0.0f;
                uint32_t o_rem = 0;
                int o_ci = 0;
                auto cell_list = [&](int cell, int &first, int &end) {  // a cell's list entries [first, end) of this lane's tier
                    if (WIDE) {
                        const uint2 h = reinterpret_cast<const uint2 *>(g_cells)[cell];
                        if constexpr (NEST) {
                            if (h.y == 1023u) {
                                sub = (int)h.x, first = end = 0, ko = koend = 0;
                                return;
                            }
                        }
                        first = (int)h.x, end = first + (int)((h.y >> cnt_shift) & CNT_MASK);
                        if (OTHERS) ko = (int)h.x + (int)((h.y >> 10) & CNT_MASK), koend = ko + (int)(h.y >> 20);
                    } else {
                        const uint32_t h = g_cells[cell];
                        first = (int)(h >> 12), end = first + (int)((h >> cnt_shift) & CNT_MASK);
                    }
                };
                // the grid's bounds (un-grown: the lists carry the growth); the near tier's lie g_size.w further in
                const float shrink = tier_far ? 0.0f : g_size.w;
                const float bx0 = g_min.x + shrink, by0 = g_min.y + shrink, bz0 = g_min.z + shrink;
                const float bx1 = fmaf((float)gnx, g_size.x, g_min.x) - shrink, by1 = fmaf((float)gny, g_size.y, g_min.y) - shrink,
                            bz1 = fmaf((float)gnz, g_size.z, g_min.z) - shrink;
                blim = best_t * 1.0001f;
                // a walk that was cut short goes on a few ulps past the cell boundary it stopped at: inside the next cell (the
                // lists' margin of 0.004 cell covers the sliver), so that every resumption ends at a later boundary
                const float t_from = t_res * 1.000002f;
                bool enters = false;
                int ci = 0, k = 0, kend = 0;
                uint32_t rem = 0;  // steps left before the ray leaves the grid: x | y << 8 | z << 16
                float tmx = INFINITY, tmy = INFINITY, tmz = INFINITY, t_exit = 0.0f;
                // (only the lanes in `live` read these, and entering the grid sets them: "undefined" values spare their v_mov
                //  in both set-up paths.  k and kend stay 0: ballot(k < kend) below is asked of every lane.)
                asm volatile("" : "=v"(tmx), "=v"(tmz), "=v"(t_exit), "=v"(ci), "=v"(rem));
                // VOTE_MASKS: the lanes beyond the lists' reach as a mask, the scan's lanes inside a wave-uniform branch; every
                // other lane evaluates the entry test (a lane beyond: for nothing), and the mask of who enters is the walk's `live`
                unsigned long long m_beyond = 0ull, m_enters = 0ull;
                if (VOTE_MASKS) {
                    m_beyond = __builtin_amdgcn_ballot_w64(o2 > g_inv.w);
                    if (m_beyond != 0ull) {
                        const float4 fmn = {bx0, by0, bz0, 0.0f}, fmx = {bx1, by1, bz1, 0.0f};
                        far_m = m_beyond & __builtin_amdgcn_ballot_w64(slab_live(bp, fmn, fmx));
                        far_scan = __builtin_amdgcn_inverse_ballot_w64(far_m);
                    }
                }
                if (!VOTE_MASKS && beyond) {
                    const float4 fmn = {bx0, by0, bz0, 0.0f}, fmx = {bx1, by1, bz1, 0.0f};
                    far_scan = slab_live(bp, fmn, fmx);
                } else {
                    // exact slab distances here (no margin): t = (b - o) * (1 / d), reciprocals clamped as in box_params
                    const float lx = (bx0 - ox) * bp.idx, ux = (bx1 - ox) * bp.idx;
                    const float ly = (by0 - oy) * bp.idy, uy = (by1 - oy) * bp.idy;
                    const float lz = (bz0 - oz) * bp.idz, uz = (bz1 - oz) * bp.idz;
                    const float tn = fmaxf(fmaxf(fmaxf(fminf(lx, ux), fminf(ly, uy)), t_from), fminf(lz, uz));
                    t_exit = fminf(fminf(fmaxf(lx, ux), fmaxf(ly, uy)), fmaxf(lz, uz));
                    if (VOTE_MASKS) {
                        m_enters = __builtin_amdgcn_ballot_w64(!(tn > fminf(t_exit, blim))) & ~m_beyond;
                        enters = __builtin_amdgcn_inverse_ballot_w64(m_enters);
                    } else {
                        enters = !(tn > fminf(t_exit, blim));
                    }
                    if (enters) {
                        // the cell of the entry point
                        const float px = fmaf(tn, dx, ox), py = fmaf(tn, dy, oy), pz = fmaf(tn, dz, oz);
                        const int ix = min(max((int)floorf((px - g_min.x) * g_inv.x), 0), gnx - 1);
                        // (SHEET: one layer of cells.  A ray that leaves it through the top or the bottom ends its walk at t_exit,
                        // the exit from the grid's bounds, which comes no later than the layer's own faces; so the walk needs
                        // neither a y cell index nor a y leave distance, and visits the cells the 3-D walk would visit)
                        const int iy = SHEET ? 0 : min(max((int)floorf((py - g_min.y) * g_inv.y), 0), gny - 1);
                        const int iz = min(max((int)floorf((pz - g_min.z) * g_inv.z), 0), gnz - 1);
                        // (24-bit multiplies, full rate: at most 1023 cells per axis and 2^21 in all, pack.hip size_grid)
                        ci = SHEET ? __mul24(iz, gnx) + ix : __mul24(__mul24(iz, gny) + iy, gnx) + ix;
                        // ray parameter at which the ray leaves the cell along each axis (a component of exactly 0
                        // never leaves), and how many steps are left before it leaves the grid
                        tmx = dx == 0.0f ? INFINITY : (fmaf((float)(ix + (dx > 0.0f ? 1 : 0)), g_size.x, g_min.x) - ox) * bp.idx;
                        if (!SHEET) tmy = dy == 0.0f ? INFINITY : (fmaf((float)(iy + (dy > 0.0f ? 1 : 0)), g_size.y, g_min.y) - oy) * bp.idy;
                        tmz = dz == 0.0f ? INFINITY : (fmaf((float)(iz + (dz > 0.0f ? 1 : 0)), g_size.z, g_min.z) - oz) * bp.idz;
                        rem = (uint32_t)(dx > 0.0f ? gnx - 1 - ix : ix) | (SHEET ? 0u : (uint32_t)(dy > 0.0f ? gny - 1 - iy : iy) << REM_BITS) |
                              (uint32_t)(dz > 0.0f ? gnz - 1 - iz : iz) << (2 * REM_BITS);
                        cell_list(ci, k, kend);
                        if constexpr (NEST) t_cur = tn;
                        if (COUNT && t_res == 0.0f) c_lane_groups++, c_group_maxpop += tier_far ? 1u : 0u;
                    }
                }
                if (COUNT && far_scan) c_query_maxpop++;
                if (COUNT && t_res != 0.0f) c_walk_resumed++;
                t_res = 0.0f;
                // The lanes that are still walking, as a lane mask in scalar registers: the loops below ask "any lane?"
                // and "how many?" of it with scalar instructions, a lane that stops is cleared from it with one scalar and-not, and
                // a lane-level `if` takes it as its exec mask.  (As a bool per lane, carried round the loops, it lived in a vector
                // register as 0 / 1 and was compared back into a mask at the head of the walk, after every pass over the lists
                // and before the tail's decision.)
                unsigned long long live = VOTE_MASKS ? m_enters : __builtin_amdgcn_ballot_w64(enters);
                // |size / d| per axis: what one step adds to the leave distance
                float dtx = g_size.x * fabsf(bp.idx), dty = g_size.y * fabsf(bp.idy), dtz = g_size.z * fabsf(bp.idz);
                int sx = dx > 0.0f ? 1 : -1, sy = dy > 0.0f ? gnx : -gnx, sz = SHEET ? (dz > 0.0f ? gnx : -gnx) : (dz > 0.0f ? gnx * gny : -(gnx * gny));
                // cell by cell: the wave first drains the lists of the cells its lanes stand in (one sphere per lane and
                // pass), then every lane steps (measured: 47.4 ms against 54.8 for one flattened loop in which a lane either
                // tests or steps, RTIOW 256 spp)
#ifndef RT_STEP_AT
#define RT_STEP_AT 16  /* lanes that must be waiting before the wave runs a step pass while others still test (65: never; 16 / 24 / 32 / 65: 145.4 / 146.0 / 145.8 / 147.9 ms) */
#endif
#ifndef RT_WALK_TAIL
#define RT_WALK_TAIL 20     /* at most this many lanes still walking ...            (0: never cut; 0 / 8 / 12 / 20: 149.0 / 146.5 / 146.0 / 145.0 ms) */
#define RT_WALK_WAITING 32  /* ... and at least this many live lanes done: the stragglers go on next iteration */
#endif
                if (RT_PRIO_W != RT_PRIO_Q) __builtin_amdgcn_s_setprio(RT_PRIO_W);
                while (live != 0ull) {
                    if constexpr (NEST) {
                        if (__builtin_amdgcn_inverse_ballot_w64(live) && sub >= 0) {
                            // into the sub-grid of the nested cell this lane stands in: one 64-byte line per lane {min, first
                            // cell} {1 / size} {size} {n}.  The sub-grid spans what the cell's entries reach of the outer cell
                            // (grown, like the lists); the walk through it is the outer walk's code on this state, over the
                            // part of the ray's stay in the outer cell that lies inside those bounds.  Sub-cells are never nested.
                            const float4 *sg = image + (__float_as_int(gh[3].w) + 4 * sub);
                            const float4 s_min = sg[0], s_inv = sg[1], s_size = sg[2], s_n = sg[3];
                            const int snx = __float_as_int(s_n.x), sny = __float_as_int(s_n.y), snz = __float_as_int(s_n.z);
                            o_tmx = tmx, o_tmy = tmy, o_tmz = tmz, o_texit = t_exit, o_rem = rem, o_ci = ci;
                            // (exact slab distances, as at the grid's bounds; a ray that misses the sub-grid gets t_exit = -inf,
                            //  which ends the sub-grid's walk at its first step)
                            const float lx = (s_min.x - ox) * bp.idx, ux = (fmaf((float)snx, s_size.x, s_min.x) - ox) * bp.idx;
                            const float ly = (s_min.y - oy) * bp.idy, uy = (fmaf((float)sny, s_size.y, s_min.y) - oy) * bp.idy;
                            const float lz = (s_min.z - oz) * bp.idz, uz = (fmaf((float)snz, s_size.z, s_min.z) - oz) * bp.idz;
                            const float t_in = fmaxf(fmaxf(fmaxf(fminf(lx, ux), fminf(ly, uy)), t_cur), fminf(lz, uz));
                            // (fminf here, quieting and all: once per nested cell a lane enters, and not on the headline kernel's
                            //  path -- min_arith is kept to the step pass, where the compiler has nothing to fold into it)
                            t_exit = fminf(fminf(fminf(t_exit, fminf(fminf(tmx, tmy), tmz)), fminf(fmaxf(lx, ux), fmaxf(ly, uy))), fmaxf(lz, uz));
                            const bool miss = t_in > fminf(t_exit, best_t * 1.0001f);
                            const float px = fmaf(t_in, dx, ox), py = fmaf(t_in, dy, oy), pz = fmaf(t_in, dz, oz);
                            const int ix = min(max((int)floorf((px - s_min.x) * s_inv.x), 0), snx - 1);
                            const int iy = min(max((int)floorf((py - s_min.y) * s_inv.y), 0), sny - 1);
                            const int iz = min(max((int)floorf((pz - s_min.z) * s_inv.z), 0), snz - 1);
                            ci = __float_as_int(s_min.w) + __mul24(__mul24(iz, sny) + iy, snx) + ix;
                            tmx = dx == 0.0f ? INFINITY : (fmaf((float)(ix + (dx > 0.0f ? 1 : 0)), s_size.x, s_min.x) - ox) * bp.idx;
                            tmy = dy == 0.0f ? INFINITY : (fmaf((float)(iy + (dy > 0.0f ? 1 : 0)), s_size.y, s_min.y) - oy) * bp.idy;
                            tmz = dz == 0.0f ? INFINITY : (fmaf((float)(iz + (dz > 0.0f ? 1 : 0)), s_size.z, s_min.z) - oz) * bp.idz;
                            rem = (uint32_t)(dx > 0.0f ? snx - 1 - ix : ix) | (uint32_t)(dy > 0.0f ? sny - 1 - iy : iy) << REM_BITS |
                                  (uint32_t)(dz > 0.0f ? snz - 1 - iz : iz) << (2 * REM_BITS);
                            dtx = s_size.x * fabsf(bp.idx), dty = s_size.y * fabsf(bp.idy), dtz = s_size.z * fabsf(bp.idz);
                            sx = dx > 0.0f ? 1 : -1, sy = dy > 0.0f ? snx : -snx, sz = dz > 0.0f ? snx * sny : -(snx * sny);
                            in_sub = true, sub = -1;
                            if (miss) t_exit = -INFINITY;
                            else cell_list(ci, k, kend);
                            if (COUNT) c_lane_cands++;
                        }
                    }
                    while (__builtin_amdgcn_ballot_w64(k < kend) != 0ull) {
                        if (COUNT) c_clusters++;
                        // two list entries per pass: both index reads, then both record reads, are in flight together, and a
                        // cell's list costs the wave ceil(n / 2) passes (each a dependent LDS round trip, exec-mask
                        // bookkeeping and a taken branch) instead of n.  A list of odd length reads the never-hit slot
                        // behind the first cluster for its second half.
                        if (k < kend) {
                            const int idx = WIDE ? (int)g_items32[k] : (int)g_items[k];
                            const int j_raw = WIDE ? (int)g_items32[k + 1] : (int)g_items[k + 1];  // (one entry past the list at worst: the next list, or the padding entry behind the last one)
                            // (the compact tables of the product instances take the entry as it is: a sphere of the next list,
                            //  whose test finds a true hit or none -- the closest hit is a minimum over true hits, so a
                            //  candidate nobody needs changes nothing, and the select and its compare are gone from every
                            //  pair pass.  The wide tables list other primitives behind a cell's spheres, and the counting
                            //  builds count tests: both keep the never-hit slot.)
                            const int jdx = ((!COUNT && !WIDE) || k + 1 < kend) ? j_raw : P.np + CSIZE;
                            if (COUNT) c_lane_clusters += k + 1 < kend ? 2u : 1u;
                            k += 2;
                            const float4 S = sph[idx], T = sph[jdx];
                            int p_idx = -1;
                            float p_hb = 0.0f, p_disc = 0.0f;
                            asm volatile("" : "=v"(p_hb), "=v"(p_disc));
                            RT_SPHERE_PARK(S, idx)
                            RT_SPHERE_PARK(T, jdx)
                            if (p_idx >= 0) resolve(p_idx, p_hb, p_disc);
                        }
                        // (the masks of the two conditions are combined as scalars, and the count is declared wave-uniform:
                        //  ballot(a && b) of two lane masks goes through a VGPR, and its popcount is compared as a vector)
                        if (RT_STEP_AT < 65 &&
                            mask_count(live & ~__builtin_amdgcn_ballot_w64(k < kend)) >= RT_STEP_AT)
                            break;
                    }
                    // the cell's other primitives, one per lane and pass, for the lanes that are through with its spheres
                    if (OTHERS) {
                        while ((live & ~__builtin_amdgcn_ballot_w64(k < kend) & __builtin_amdgcn_ballot_w64(ko < koend)) != 0ull) {
                            if (__builtin_amdgcn_inverse_ballot_w64(live) && !(k < kend) && ko < koend) {
                                const int id = (int)g_items32[ko];
                                ++ko;
                                if (COUNT) c_lane_clusters++;
                                if (id < ns + nr) {
                                    test_rect(id - ns);
                                } else {
                                    // behind the primitive's (host-grown) box: exact slab distances, as at the grid's bounds.  (The box
                                    // lies behind the primitive's records, in the same lines of memory.  Reading all of them at
                                    // once, so that the test's operands travel while the box is tested, costs 24 registers and
                                    // lost: 20000 triangles 30.5 -> 31.7 ms, the DNA frame 7.05 -> 7.47 ms.)
                                    const bool is_cyl = id < ns + nr + nc;
                                    const int kk = is_cyl ? id - ns - nr : id - ns - nr - nc;
                                    const float4 *bb = is_cyl ? cyl + RT_CYL_STRIDE * kk + 4 : tri + RT_TRI_STRIDE * kk + 3;
                                    const float4 bmn = bb[0], bmx = bb[1];
                                    const float lx = (bmn.x - ox) * bp.idx, ux = (bmx.x - ox) * bp.idx;
                                    const float ly = (bmn.y - oy) * bp.idy, uy = (bmx.y - oy) * bp.idy;
                                    const float lz = (bmn.z - oz) * bp.idz, uz = (bmx.z - oz) * bp.idz;
                                    const float tn = fmaxf(fmaxf(fmaxf(fminf(lx, ux), fminf(ly, uy)), 0.0f), fminf(lz, uz));
                                    const float tf = fminf(fminf(fminf(fmaxf(lx, ux), fmaxf(ly, uy)), best_t * 1.0001f), fmaxf(lz, uz));
                                    if (!(tn > tf)) {
                                        if (is_cyl) test_cyl(kk);
                                        else if (EXT) {
                                            // (the quad's test laid out behind the triangle's: a mesh's walk falls through.
                                            //  Without the hint the 20 000-triangle mesh ran 1.5 % slower)
                                            if (__builtin_expect(kk < nt, 1)) test_tri(kk);
                                            else test_quad(kk - nt);
                                        }
                                    }
                                }
                            }
                        }
                    }
                    if (COUNT) c_groups++;
                    // The tail: a wave's walk lasts as long as its slowest lane's (11 test and 4 step passes for 2.8 tests
                    // and 0.7 steps per lane).  When only a few lanes are still walking while most of the wave waits for
                    // its shading, the stragglers stop at their next cell boundary and go on from there in the next
                    // iteration, together with the new queries (the walk is front to back: nothing nearer than the
                    // boundary was found, and whatever was found beyond it is found again in its own cell).
                    const bool cut = RT_QUERY_CUT && RT_WALK_TAIL > 0 && mask_count(live) <= RT_WALK_TAIL &&
                                     mask_count(__builtin_amdgcn_ballot_w64(active) & ~live) >= RT_WALK_WAITING;
                    // the lanes that are through with their cell's lists: they step, or stop.  (Every lane evaluates the step's
                    // conditions; they count for these lanes alone, as masks: who stops, who is cut short, who goes on.)
                    unsigned long long stepping = live & ~__builtin_amdgcn_ballot_w64(k < kend);
                    if (OTHERS) stepping &= ~__builtin_amdgcn_ballot_w64(ko < koend);
                    {
                        if constexpr (NEST) {
                            if (__builtin_amdgcn_inverse_ballot_w64(stepping) && in_sub) {
                                // the sub-grid's walk is over where the outer walk's would be (past the ray's stay in the outer
                                // cell, which is t_exit here, or past a hit, or at the sub-grid's last cell): back to the outer one
                                const float tn_s = min3_arith(tmx, tmy, tmz);
                                const int sh_s = tmx == tn_s ? 0 : (tmy == tn_s ? REM_BITS : 2 * REM_BITS);
                                if (tn_s > min_arith(t_exit, best_t * 1.0001f) || ((rem >> sh_s) & REM_MASK) == 0u) {
                                    tmx = o_tmx, tmy = o_tmy, tmz = o_tmz, t_exit = o_texit, rem = o_rem, ci = o_ci;
                                    dtx = g_size.x * fabsf(bp.idx), dty = g_size.y * fabsf(bp.idy), dtz = g_size.z * fabsf(bp.idz);
                                    sx = dx > 0.0f ? 1 : -1, sy = dy > 0.0f ? gnx : -gnx, sz = dz > 0.0f ? gnx * gny : -(gnx * gny);
                                    in_sub = false;
                                }
                            }
                        }
                        // (the leave distances and t_exit are sums, products and minima of such, or +-inf, carried round the loop:
                        //  min_arith, where fminf would first quiet all three, one v_max_f32 each)
                        const float tnext = SHEET ? min_arith(tmx, tmz) : min3_arith(tmx, tmy, tmz);
                        const bool xle = tmx == tnext, yle = !SHEET && !xle && tmy == tnext;
                        const int sh = xle ? 0 : (yle ? REM_BITS : 2 * REM_BITS);
                        const unsigned long long ends = __builtin_amdgcn_ballot_w64(tnext > min_arith(t_exit, best_t * 1.0001f)) |
                                                        __builtin_amdgcn_ballot_w64(((rem >> sh) & REM_MASK) == 0u);
                        // (a hit inside the cell being left stays: the walk ends at the next boundary test)
                        const unsigned long long cuts =
                            cut ? __builtin_amdgcn_ballot_w64(tnext > t_from) & ~__builtin_amdgcn_ballot_w64(best_t < tnext) & ~ends : 0ull;
                        live &= ~(stepping & (ends | cuts));
                        if (__builtin_amdgcn_inverse_ballot_w64(stepping & cuts)) t_res = tnext;
                        if (__builtin_amdgcn_inverse_ballot_w64(stepping & ~(ends | cuts))) {
                            ci += xle ? sx : (yle ? sy : sz);
                            tmx += xle ? dtx : 0.0f, tmz += (xle || yle) ? 0.0f : dtz;
                            if (!SHEET) tmy += yle ? dty : 0.0f;
                            rem -= 1u << sh;
                            if constexpr (NEST) {
                                if (!in_sub) t_cur = tnext;
                            }
                            cell_list(ci, k, kend);
                            if (COUNT) c_lane_cands++;
                        }
                    }
                }
                if (RT_PRIO_W != RT_PRIO_H) __builtin_amdgcn_s_setprio(RT_PRIO_H);
                // far origins that can reach the grid at all: every clustered sphere (the flat scan)
                if (VOTE_MASKS ? far_m != 0ull : __builtin_amdgcn_ballot_w64(far_scan) != 0ull) {
                    const int end = P.np + (CSIZE + 1) * P.ncl;
                    for (int i = P.np; i < end; i += 4) {
                        const float4 s0 = sph[i], s1 = sph[i + 1], s2 = sph[i + 2], s3 = sph[i + 3];
                        if (far_scan) {
                            RT_SPHERE_TEST(s0, i)
                            RT_SPHERE_TEST(s1, i + 1)
                            RT_SPHERE_TEST(s2, i + 2)
                            RT_SPHERE_TEST(s3, i + 3)
                        }
                    }
                }
                blim = best_t * 1.0001f;
            } else if (CULL == 3) {
                // windows of 64 clusters: one mask bit per cluster
                for (int w0 = 0; w0 < P.nwin; ++w0) {
                    // clip the ray to the window box (the union of its cluster boxes; same margin as every box test)
                    const BoxP bp = box_params();
                    const float idx = bp.idx, idy = bp.idy, idz = bp.idz, marg = bp.marg;
                    const float4 *wb = hot + (P.off_wbox - gap) + 2 * w0;
                    const float4 wmn = wb[0], wmx = wb[1];
                    blim = best_t * 1.0001f;  // what the prefix and the previous windows found
                    const float lx = fmaf(wmn.x, idx, bp.nxm), ux = fmaf(wmx.x, idx, bp.nxp);
                    const float ly = fmaf(wmn.y, idy, bp.nym), uy = fmaf(wmx.y, idy, bp.nyp);
                    const float lz = fmaf(wmn.z, idz, bp.nzm), uz = fmaf(wmx.z, idz, bp.nzp);
                    const float tn = fmaxf(fmaxf(fmaxf(fminf(lx, ux), fminf(ly, uy)), 0.0f), fminf(lz, uz));
                    const float tf = fminf(fminf(fminf(fmaxf(lx, ux), fmaxf(ly, uy)), blim), fmaxf(lz, uz));
                    const bool wlive = !(tn > tf);
                    if (__builtin_amdgcn_ballot_w64(wlive) == 0ull) continue;
                    if (COUNT) c_lane_groups += wlive ? 1u : 0u;
                    // phase 1: candidate clusters of the clipped segment [tn, tf]: the slab ranges of its bounding box
                    // (grown by the margin) select one precomputed mask per axis -- R_a[i0][i1] = clusters whose box
                    // overlaps the slabs i0..i1 of the window along axis a; a cluster the ray can reach overlaps the
                    // segment's box on every axis, so it is in the intersection of the three masks
                    unsigned long long cand = 0ull;
                    if (wlive) {
                        const float4 *hd = hot + (P.off_rtab - gap) + w0 * P.rt_stride;
                        const float4 gmn = hd[0], giw = hd[1];
                        const unsigned long long *tab = reinterpret_cast<const unsigned long long *>(hd + 2);
                        cand = ~0ull;
                        const float top = (float)(RT_SLABS - 1);
                        if (P.rt_axes & 1) {
                            const float a = fmaf(tn, dx, ox), b = fmaf(tf, dx, ox);
                            const int i0 = (int)__builtin_amdgcn_fmed3f(((fminf(a, b) - marg) - gmn.x) * giw.x, 0.0f, top);
                            const int i1 = (int)__builtin_amdgcn_fmed3f(((fmaxf(a, b) + marg) - gmn.x) * giw.x, 0.0f, top);
                            cand &= tab[i0 * RT_SLABS + i1];
                            tab += RT_SLABS * RT_SLABS;
                        }
                        if (P.rt_axes & 2) {
                            const float a = fmaf(tn, dy, oy), b = fmaf(tf, dy, oy);
                            const int i0 = (int)__builtin_amdgcn_fmed3f(((fminf(a, b) - marg) - gmn.y) * giw.y, 0.0f, top);
                            const int i1 = (int)__builtin_amdgcn_fmed3f(((fmaxf(a, b) + marg) - gmn.y) * giw.y, 0.0f, top);
                            cand &= tab[i0 * RT_SLABS + i1];
                            tab += RT_SLABS * RT_SLABS;
                        }
                        if (P.rt_axes & 4) {
                            const float a = fmaf(tn, dz, oz), b = fmaf(tf, dz, oz);
                            const int i0 = (int)__builtin_amdgcn_fmed3f(((fminf(a, b) - marg) - gmn.z) * giw.z, 0.0f, top);
                            const int i1 = (int)__builtin_amdgcn_fmed3f(((fmaxf(a, b) + marg) - gmn.z) * giw.z, 0.0f, top);
                            cand &= tab[i0 * RT_SLABS + i1];
                        }
                        const int left = P.ncl - w0 * 64;  // the last window may hold fewer than 64 clusters
                        if (left < 64) cand &= (1ull << left) - 1ull;
                        if (COUNT) c_lane_cands += (uint32_t)__popcll(cand);
                    }
                    // phase 2: keep the candidates whose own box the ray reaches (per-lane box reads)
                    unsigned long long mine = 0ull;
                    while (__builtin_amdgcn_ballot_w64(cand != 0ull) != 0ull) {
                        if (cand != 0ull) {
                            const unsigned long long low = cand & (0ull - cand);
                            const int q = (int)__builtin_ctzll(cand);
                            cand ^= low;
                            const float4 *b = box + 2 * (w0 * 64 + q);
                            if (slab_live(bp, b[0], b[1])) mine |= low;
                        }
                        if (COUNT) c_groups++;
                    }
                    if (COUNT) {
                        c_lane_clusters += (uint32_t)__popcll(mine);
                        uint32_t m = (uint32_t)__popcll(mine);
                        for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
                        if (lane == 0) c_query_maxpop += m;
                    }
                    // phase 3: every lane walks its own clusters; lanes that are done wait masked off
                    while (__builtin_amdgcn_ballot_w64(mine != 0ull) != 0ull) {
                        if (mine != 0ull) {
                            const int q = (int)__builtin_ctzll(mine);
                            mine &= mine - 1ull;
                            const int base = P.np + (CSIZE + 1) * (w0 * 64 + q);
                            const float4 *cs = sph + base;
#pragma unroll
                            for (int h = 0; h < CSIZE; h += 4) {
                                const float4 r0 = cs[h], r1 = cs[h + 1], r2 = cs[h + 2], r3 = cs[h + 3];
                                RT_SPHERE_TEST(r0, base + h)
                                RT_SPHERE_TEST(r1, base + h + 1)
                                RT_SPHERE_TEST(r2, base + h + 2)
                                RT_SPHERE_TEST(r3, base + h + 3)
                            }
                        }
                        if (COUNT) c_clusters++;
                    }
                }
                blim = best_t * 1.0001f;
            } else if (CULL == 2) {
                const BoxP bp = box_params();
                // windows of 64 clusters (16 outer boxes): one mask bit per cluster
                for (int g0 = 0; g0 < P.ngr; g0 += 64 / RT_GROUP) {
                    // big scenes: one box around the whole window first (third level of the hierarchy)
                    if (P.nwin > 1) {
                        const float4 *wb = hot + (P.off_wbox - gap) + 2 * (g0 / (64 / RT_GROUP));
                        if (__builtin_amdgcn_ballot_w64(slab_live(bp, wb[0], wb[1])) == 0ull) continue;
                        blim = best_t * 1.0001f;  // what the previous windows found tightens this one
                    }
                    // phase 1: which clusters can this lane's ray reach?  (wave-uniform box reads)
                    unsigned long long mine = 0ull;
                    const int g_end = min(P.ngr, g0 + 64 / RT_GROUP);
                    for (int g = g0; g < g_end; ++g) {
                        const bool glive = slab_live(bp, gbox[2 * g], gbox[2 * g + 1]);
                        if (__builtin_amdgcn_ballot_w64(glive) == 0ull) continue;
                        if (COUNT) c_groups++, c_lane_groups += glive ? 1u : 0u;
                        const int nj = min(RT_GROUP, P.ncl - g * RT_GROUP);
                        uint32_t gm = 0;
#pragma unroll
                        for (int j = 0; j < RT_GROUP; ++j) {
                            if (j < nj) {
                                const int q = g * RT_GROUP + j;
                                if (slab_live(bp, box[2 * q], box[2 * q + 1])) gm |= 1u << j;
                            }
                        }
                        if (COUNT) c_lane_clusters += __popc(gm);
                        mine |= (unsigned long long)gm << (RT_GROUP * (g - g0));
                    }
                    if (COUNT) {
                        uint32_t m = (uint32_t)__popcll(mine);
                        for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
                        if (lane == 0) c_query_maxpop += m;
                    }
                    // phase 2: every lane walks its own clusters; lanes that are done wait masked off
                    while (__builtin_amdgcn_ballot_w64(mine != 0ull) != 0ull) {
                        if (mine != 0ull) {
                            const int q = (int)__builtin_ctzll(mine);
                            mine &= mine - 1ull;
                            const int base = P.np + (CSIZE + 1) * (g0 * RT_GROUP + q);
                            const float4 *cs = sph + base;
                            // four records at a time: eight in flight cost 20 spilled VGPRs at 6 waves/SIMD
#pragma unroll
                            for (int h = 0; h < CSIZE; h += 4) {
                                const float4 r0 = cs[h], r1 = cs[h + 1], r2 = cs[h + 2], r3 = cs[h + 3];
                                RT_SPHERE_TEST(r0, base + h)
                                RT_SPHERE_TEST(r1, base + h + 1)
                                RT_SPHERE_TEST(r2, base + h + 2)
                                RT_SPHERE_TEST(r3, base + h + 3)
                            }
                        }
                        if (COUNT) c_clusters++;
                    }
                }
                blim = best_t * 1.0001f;
            } else if (CULL == 1) {
                const BoxP bp = box_params();
                for (int g = 0; g < P.ngr; ++g) {
                const bool glive = slab_live(bp, gbox[2 * g], gbox[2 * g + 1]);
                if (__builtin_amdgcn_ballot_w64(glive) == 0ull) continue;
                if (COUNT) c_groups++, c_lane_groups += glive ? 1u : 0u;
                const int q_end = min(P.ncl, (g + 1) * RT_GROUP);
                for (int q = g * RT_GROUP; q < q_end; ++q) {
                    const bool live = slab_live(bp, box[2 * q], box[2 * q + 1]);
                    if (COUNT && live) c_lane_clusters++;
                    if (__builtin_amdgcn_ballot_w64(live) != 0ull) {
                        const int base = P.np + (CSIZE + 1) * q;
                        const float4 *cs = sph + base;
#pragma unroll
                        for (int h = 0; h < CSIZE; h += 4) {
                            const float4 r0 = cs[h], r1 = cs[h + 1], r2 = cs[h + 2], r3 = cs[h + 3];
                            RT_SPHERE_TEST(r0, base + h)
                            RT_SPHERE_TEST(r1, base + h + 1)
                            RT_SPHERE_TEST(r2, base + h + 2)
                            RT_SPHERE_TEST(r3, base + h + 3)
                        }
                        blim = best_t * 1.0001f;
                        if (COUNT) c_clusters++;
                    }
                }
                }
            }
            }  // if (active): candidate search
