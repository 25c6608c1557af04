// The scene packer: the scene's primitives, materials and textures -> the device image (device_scene.h) and the packer's
// fields of RenderParams.  One round runs five stages, each handing the next a small struct:
//   1. sphere_slots:  the sphere table's slots (big-sphere prefix, then Morton-ordered clusters)
//   2. other_prims:   the boxes of the rects, cylinders and triangles, which of them the grid lists, their table order
//   3. build_grid:    the uniform grid's cells and lists, compact or wide
//   4. lay_out_image: every offset of the image, in image order
//   5. write_*:       one writer per section of the image
// A round fails when the grid forces more primitives to be tested for every query; pack_scene then runs another.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

#include "pack.h"
#include "rt_motion.h"  // (before rt_media.h: philox.h defines RTMI_HD, rt_trig.h takes it as it finds it)
#include "rt_media.h"
#include "rt_noise.h"
#include "rt_alpha.h"

namespace rtmi {
namespace {

inline float bits(int32_t v) {
    float f;
    memcpy(&f, &v, 4);
    return f;
}

inline float *rec4(float *I, int idx) { return I + (size_t)idx * 4; }

struct OBox {
    double lo[3], hi[3];
};

// ---- stage 1: sphere slots ------------------------------------------------------------
struct SphereSlots {
    std::vector<int> slots;  // prim index per slot, -1 = padding
    std::vector<int> rest;   // the clustered spheres in Morton order: rest[k] sits in cluster k / RT_CLUSTER
    int np = 0;              // prefix slots (the always-tested big spheres), a multiple of 4
    int n_clusters = 0;
    int axes = 0;            // range tables: the axes along which the clustered spheres spread (bit a)
    int ns() const { return (int)slots.size(); }
    int slot_of(size_t k) const { return np + (int)(k / RT_CLUSTER) * (RT_CLUSTER + 1) + (int)(k % RT_CLUSTER); }
};

// Range tables (ablation variant 128: candidate clusters of a ray segment without testing every box): per window of 64
// clusters and per enabled axis, R[i0 * 16 + i1] = the clusters whose box overlaps the slabs i0..i1 of the window box cut
// into RT_SLABS slabs along that axis (64-bit mask).  An axis along which the clustered spheres do not spread (a sheet:
// RTIOW's y) carries no information and is left out (2 KB of LDS).
int range_axes(const Scene &s, const std::vector<int> &rest) {
    int axes = 0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i : rest) {
        const float r = std::fabs(s.prims[i].f[3]);
        for (int a = 0; a < 3; ++a) lo[a] = std::min(lo[a], s.prims[i].f[a] - r), hi[a] = std::max(hi[a], s.prims[i].f[a] + r);
    }
    float ext[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    const float big = std::max(ext[0], std::max(ext[1], ext[2]));
    for (int a = 0; a < 3; ++a)
        if (!rest.empty() && ext[a] > 0.05f * big) axes |= 1 << a;
    return axes;
}

// The closest hit does not depend on the visiting order (ties are resolved through the stored list index), so the table is
// laid out for the kernel:
//   prefix   : the big spheres (|r| > 4 x median), largest first -- the likeliest closest hits, tested unconditionally, so
//              best_t is tight before anything else;
//   clusters : the rest in Morton order of their centres, 8 per cluster (what the grid's cells list; the clusters and their
//              boxes serve the cluster searches of the ablation builds and the scan of far origins).
// Both parts are padded with never-hit records (r*r = -inf).
SphereSlots sphere_slots(const Scene &s, std::vector<int> sph, const std::vector<char> &forced) {
    SphereSlots S;
    std::vector<int> &slots = S.slots, &rest = S.rest;
    std::stable_sort(sph.begin(), sph.end(), [&](int a, int b) {
        return std::fabs(s.prims[a].f[3]) > std::fabs(s.prims[b].f[3]);
    });
    {
        float big = 0.0f;  // 0: every sphere is tested for every query (16 spheres or fewer)
        if (sph.size() > 16) {
            std::vector<float> radii;
            for (int i : sph) radii.push_back(std::fabs(s.prims[i].f[3]));
            std::nth_element(radii.begin(), radii.begin() + radii.size() / 2, radii.end());
            big = 4.0f * radii[radii.size() / 2];
        }
        for (int i : sph) {
            if (big == 0.0f || std::fabs(s.prims[i].f[3]) > big || forced[i]) slots.push_back(i);
            else rest.push_back(i);
        }
    }
    while (slots.size() % 4) slots.push_back(-1);  // the prefix is walked four records at a time
    S.np = (int)slots.size();
    if (!rest.empty()) {
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int i : rest)
            for (int a = 0; a < 3; ++a) lo[a] = std::min(lo[a], s.prims[i].f[a]), hi[a] = std::max(hi[a], s.prims[i].f[a]);
        auto spread = [](uint32_t v) {  // 10 bits -> every third bit
            v = (v | (v << 16)) & 0x030000FFu;
            v = (v | (v << 8)) & 0x0300F00Fu;
            v = (v | (v << 4)) & 0x030C30C3u;
            v = (v | (v << 2)) & 0x09249249u;
            return v;
        };
        auto morton = [&](int i) {
            uint32_t q[3];
            for (int a = 0; a < 3; ++a) {
                float ext = hi[a] - lo[a];
                float t = ext > 0 ? (s.prims[i].f[a] - lo[a]) / ext : 0.0f;
                q[a] = (uint32_t)std::min(1023.0f, std::max(0.0f, t * 1023.0f));
            }
            return spread(q[0]) | (spread(q[1]) << 1) | (spread(q[2]) << 2);
        };
        std::stable_sort(rest.begin(), rest.end(), [&](int a, int b) { return morton(a) < morton(b); });
    }
    // Cluster q occupies the slots [np + 9 q, + 8) followed by ONE never-hit slot: with a stride of 9 records, record h of
    // clusters q and q' lies (q - q') records apart modulo 16, so the lanes of a wave that read different clusters hit
    // different LDS banks with the same instruction (a ds_read_b128 serves 16 lanes per cycle, one 16-byte record per 4
    // banks; with stride 16 every cluster's record h shared one bank group: 19.5 % of the LDS cycles were conflicts).
    // All-padding clusters end the table (read-ahead of the flat scan; the pair test's never-hit partner).
    const int csize = RT_CLUSTER;
    S.n_clusters = ((int)rest.size() + csize - 1) / csize;
    const int cstride = csize + 1;
    for (int q = 0; q < S.n_clusters + 3; ++q)  // + 3 all-padding clusters: the flat scan reads 16 records a step and one ahead
        for (int h = 0; h < cstride; ++h) {
            const size_t j = (size_t)q * csize + h;
            slots.push_back((q < S.n_clusters && h < csize && j < rest.size()) ? rest[j] : -1);
        }
    while (slots.size() % 4) slots.push_back(-1);
    S.axes = range_axes(s, rest);
    return S;
}

// ---- stage 2: the other primitives ------------------------------------------------------
// world boxes in double precision (grown by the grid where they are listed)
OBox rect_box(const rt_prim &p) {
    OBox b;
    const int axis = p.type - RT_PRIM_XY_RECT;  // 0: z = k (x, y extents), 1: y = k (x, z), 2: x = k (y, z)
    const int ia = axis == 2 ? 1 : 0, ib = axis == 0 ? 1 : 2, ik = axis == 0 ? 2 : (axis == 1 ? 1 : 0);
    b.lo[ia] = std::min(p.f[0], p.f[1]), b.hi[ia] = std::max(p.f[0], p.f[1]);
    b.lo[ib] = std::min(p.f[2], p.f[3]), b.hi[ib] = std::max(p.f[2], p.f[3]);
    b.lo[ik] = b.hi[ik] = p.f[4];
    return b;
}

// cylinders: world box of the open tube = union of the boxes of its two end circles
// (centre M (0,0,z), radius R, normal = the tube axis a: half-extent R sqrt(1 - a_i^2) on axis i)
OBox cyl_box(const rt_prim &p, double R, double zpad) {
    OBox b;
    double ax[3] = {p.m[2], p.m[6], p.m[10]};  // image of the object z axis
    const double an = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    const double z0 = std::min((double)p.f[1], (double)p.f[2]) - zpad, z1 = std::max((double)p.f[1], (double)p.f[2]) + zpad;
    for (int a = 0; a < 3; ++a) {
        const double ai = an > 0 ? ax[a] / an : 0.0;
        const double half = R * std::sqrt(std::max(0.0, 1.0 - ai * ai));
        const double c0 = p.m[a * 4 + 2] * z0 + p.m[a * 4 + 3];
        const double c1 = p.m[a * 4 + 2] * z1 + p.m[a * 4 + 3];
        b.lo[a] = std::min(c0, c1) - half, b.hi[a] = std::max(c0, c1) + half;
    }
    return b;
}

OBox tri_box(const rt_prim &p) {
    OBox b;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = std::min((double)p.m[a], std::min((double)p.m[3 + a], (double)p.m[6 + a]));
        b.hi[a] = std::max((double)p.m[a], std::max((double)p.m[3 + a], (double)p.m[6 + a]));
    }
    return b;
}

// a quad's box: the bounds of its four corners Q, Q + u, Q + u + v, Q + v
OBox quad_box(const rt_prim &p) {
    OBox b;
    for (int a = 0; a < 3; ++a) {
        const double q = p.m[a], u = p.m[3 + a], v = p.m[6 + a];
        b.lo[a] = q + std::min(0.0, u) + std::min(0.0, v);
        b.hi[a] = q + std::max(0.0, u) + std::max(0.0, v);
    }
    return b;
}

struct OtherPrims {
    std::vector<int> rec, cyl, tri, quad;  // prim indices per table, the always-tested ones first
    int nr_a = 0, nc_a = 0, nt_a = 0, nq_a = 0;
    std::vector<int> others;         // rects, cylinders, triangles in list order: the index k of the per-k vectors below
    std::vector<int> oidx;           // per prim: its k, -1 for spheres
    std::vector<OBox> obox;          // world box
    std::vector<char> listed;        // listed in the grid's cells (else tested for every query)
    std::vector<int> gid;            // per prim: grouped id (its position in the tables behind the sphere slots)
    int prim_of_gid(int g, int ns) const {  // (a grouped id of a rect, cylinder, triangle or quad)
        const int k = g - ns, nr = (int)rec.size(), nc = (int)cyl.size(), nt = (int)tri.size();
        return k < nr ? rec[k] : (k < nr + nc ? cyl[k - nr] : (k < nr + nc + nt ? tri[k - nr - nc] : quad[k - nr - nc - nt]));
    }
};

OtherPrims other_prims(const Scene &s, const SphereSlots &S, std::vector<int> rec, std::vector<int> cyl, std::vector<int> tri,
                       std::vector<int> quad, const std::vector<char> &forced) {
    OtherPrims O;
    std::vector<int> &others = O.others;
    others.insert(others.end(), rec.begin(), rec.end());
    others.insert(others.end(), cyl.begin(), cyl.end());
    others.insert(others.end(), tri.begin(), tri.end());
    others.insert(others.end(), quad.begin(), quad.end());
    O.oidx.assign(s.prims.size(), -1);
    for (size_t k = 0; k < others.size(); ++k) O.oidx[others[k]] = (int)k;
    std::vector<OBox> &obox = O.obox;
    obox.resize(others.size());
    for (size_t k = 0; k < others.size(); ++k) {
        const rt_prim &p = s.prims[others[k]];
        obox[k] = p.type == RT_PRIM_CYLINDER ? cyl_box(p, std::fabs((double)p.f[0]), 0.0) : (p.type == RT_PRIM_TRIANGLE ? tri_box(p) : (p.type == RT_PRIM_QUAD ? quad_box(p) : rect_box(p)));
    }
    // Which of them go into the grid's cells?  Like the spheres: none while the scene is small (16 primitives outside the
    // sphere prefix or fewer: the per-query loops are the cheaper search), and not the oversized ones (largest box edge > 8 x
    // the median of what would be listed: a room's walls, a ground plane), which every ray has to test anyway.
    std::vector<char> &listed = O.listed;
    listed.assign(others.size(), 0);
    if (S.rest.size() + others.size() > 16) {
        std::vector<double> sizes;
        for (int i : S.rest) sizes.push_back(2.0 * std::fabs((double)s.prims[i].f[3]));
        auto edge = [&](size_t k) {
            return std::max(obox[k].hi[0] - obox[k].lo[0], std::max(obox[k].hi[1] - obox[k].lo[1], obox[k].hi[2] - obox[k].lo[2]));
        };
        for (size_t k = 0; k < others.size(); ++k) sizes.push_back(edge(k));
        std::nth_element(sizes.begin(), sizes.begin() + sizes.size() / 2, sizes.end());
        const double big = 8.0 * sizes[sizes.size() / 2];
        for (size_t k = 0; k < others.size(); ++k) listed[k] = (edge(k) <= big || !(big > 0.0)) && !forced[others[k]];
    }
    // the other primitives' tables: the always-tested ones first (the kernel's per-query loops run over that prefix)
    auto order_table = [&](std::vector<int> &v, int &n_always) {
        std::vector<int> a, b;
        for (int i : v) (listed[O.oidx[i]] ? b : a).push_back(i);
        n_always = (int)a.size();
        v = a;
        v.insert(v.end(), b.begin(), b.end());
    };
    order_table(rec, O.nr_a), order_table(cyl, O.nc_a), order_table(tri, O.nt_a), order_table(quad, O.nq_a);
    const int ns = S.ns(), nr = (int)rec.size(), nc = (int)cyl.size(), nt = (int)tri.size();
    O.gid.assign(s.prims.size(), -1);
    for (size_t k = 0; k < rec.size(); ++k) O.gid[rec[k]] = ns + (int)k;
    for (size_t k = 0; k < cyl.size(); ++k) O.gid[cyl[k]] = ns + nr + (int)k;
    for (size_t k = 0; k < tri.size(); ++k) O.gid[tri[k]] = ns + nr + nc + (int)k;
    for (size_t k = 0; k < quad.size(); ++k) O.gid[quad[k]] = ns + nr + nc + nt + (int)k;
    O.rec = std::move(rec), O.cyl = std::move(cyl), O.tri = std::move(tri), O.quad = std::move(quad);
    return O;
}

// ---- stage 3: the uniform grid ----------------------------------------------------------
// The candidate search: every lane walks the cells its ray crosses front to back -- 3-D DDA -- and tests what they list.  A
// primitive is listed in every cell its GROWN box touches.  The growth covers the fp32 error of its test, so that the walk
// finds every hit the linear scan would find:
//   spheres: |disc_fp32 - disc| <= K eps a |oc|^2 (K = 32 bounds the operation-by-operation sum, about 15 eps |oc|^2), so a
//     ray the fp32 test can accept passes within r' = sqrt(r^2 + K eps |oc|^2) of the centre, and its fp32 hit point lies
//     inside that ball too.  |oc| <= |o| + |c|, so the growth depends on how far from the coordinate origin a ray starts;
//     the lists come in two tiers:
//       near  |o| <= ob_near (the cloud, the camera; RTIOW 23.4): the first n_near entries of a cell's list
//       far   |o| <= ob_far  (hits on distant ground; 8x the cloud, at least 64): all n_all entries
//   cylinders (object.cuh:233-290): the same quadratic in the tube's object space, K = 64 (the transform's rounding rides
//     along): tube radius R' = sqrt(R^2 + K eps (ob_far + |corner|)^2), ends moved out by the term below;
//   rectangles, triangles: the accepted point lies on the ray within a few eps (|o| + |p|) of the primitive's plane (the
//     triangle's plane point r = o - d/|d| (oc.n)/theta carries the error of oc.n, which does not grow with 1/theta) and, in
//     projection, inside its outline to the same order: 64 eps (ob_far + |corner|);
//   one tier (the far one) for these three: their growth is 1e-4 of a cell.
// Lanes further out than ob_far test the grid's bounds with the per-lane margin of the box tests and, if they can reach it
// at all, test everything the cells list: rare, and the flat scan is the definition of the result.
// (0.004 cell + 1e-5 (max|c| + 1)) more covers the walk's own rounding: the entry point, the cell boundaries, up to
// 1023 accumulated leave distances.)
// Two table formats: COMPACT (sphere-only scenes that fit LDS: 16-bit entries, one word per cell, <= 255 cells per axis,
// <= 63 entries per cell) and WIDE (everything else: 32-bit entries, two words per cell, <= 1023 cells per axis, <= 1023
// sphere entries per tier and <= 4095 other entries per cell).
struct Grid {
    bool wide = false;
    std::vector<uint32_t> cells;  // compact: (first item << 12) | (n_near << 6) | n_all;  wide: {first item, n_near | n_all << 10 | n_other << 20}
    std::vector<uint32_t> items;  // sphere slots (a cell's near-tier entries first), then grouped ids of the other primitives
    float min[3] = {0, 0, 0}, size[3] = {1, 1, 1};
    int n[3] = {0, 0, 0};
    float ob2[2] = {0.0f, 0.0f}, shrink = 0.0f;
    std::vector<OBox> listed_box;  // grown boxes of the listed others (also what their box tests read)
    // nested cells (build_grid with a nesting threshold): the cells of every sub-grid follow the top-level ones in `cells`,
    // their lists are in `items`; subs: 4 records per nested cell, in the order of the top-level header {min.xyz, first
    // cell (bits)} {1/size.xyz, 0} {size.xyz, 0} {nx, ny, nz (bits), 0}
    std::vector<float> subs;
    int top_cells = 0;  // cells of the top level (= cells.size() / 2 without nested cells)
    size_t sub_items = 0, longest = 0;  // list entries of the sub-cells; the longest list (near + far + others) a walk can meet
    bool demoted = false;               // fill_cells forced the members of an overflowing cell
};

// a nested cell's header word 1 (n_near = 1023 > n_all = 0 never occurs in a plain cell); word 0 = its sub-grid (index into subs / 16)
constexpr uint32_t kNestedMark = 1023u;

// per clustered sphere: the radius of its near-tier and far-tier listing
struct Growth {
    std::vector<double> near, far;
};

// The tiers' reach, the cell size and the grown boxes: fills g's header values and listed_box
Growth size_grid(const Scene &s, const SphereSlots &S, const OtherPrims &O, size_t n_listed, Grid &g) {
    const std::vector<int> &rest = S.rest;
    const double cell_factor = knob("RTMI_GRID_CELL", 1.0);
    const double ob_env = knob("RTMI_GRID_OB", 0.0);  // experiments
    // (steps left per axis in 10 / 8 bits of one register; the walk's entry cell index is put together with 24-bit
    //  multiplies, which these bounds keep far inside their range: (z n_y + y) n_x + x < 2^21)
    const double max_dim = g.wide ? 1023.0 : 255.0;
    const long long max_cells = g.wide ? (1LL << 21) : (1LL << 18);
    // centres (spheres) and box centres (others): the cloud the cells are sized for
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, cmax = 0.0, cmax2 = 0.0;
    double slo[3] = {1e300, 1e300, 1e300}, shi[3] = {-1e300, -1e300, -1e300};  // of the sphere centres alone
    auto add_point = [&](const double *c) {
        double c2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], c[a]), hi[a] = std::max(hi[a], c[a]);
            cmax = std::max(cmax, std::fabs(c[a])), c2 += c[a] * c[a];
        }
        cmax2 = std::max(cmax2, std::sqrt(c2));
    };
    for (int i : rest) {
        const double c[3] = {s.prims[i].f[0], s.prims[i].f[1], s.prims[i].f[2]};
        add_point(c);
        for (int a = 0; a < 3; ++a) slo[a] = std::min(slo[a], c[a]), shi[a] = std::max(shi[a], c[a]);
    }
    const std::vector<OBox> &obox = O.obox;
    for (size_t k = 0; k < O.others.size(); ++k) {
        if (!O.listed[k]) continue;
        const double c[3] = {0.5 * (obox[k].lo[0] + obox[k].hi[0]), 0.5 * (obox[k].lo[1] + obox[k].hi[1]), 0.5 * (obox[k].lo[2] + obox[k].hi[2])};
        add_point(c);
        // (the far corners count towards the reach of the tiers: |oc| <= |o| + |corner|)
        double far2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double m = std::max(std::fabs(obox[k].lo[a]), std::fabs(obox[k].hi[a]));
            far2 += m * m, cmax = std::max(cmax, m);
        }
        cmax2 = std::max(cmax2, std::sqrt(far2));
    }
    const double cam = std::sqrt(s.cam.lookfrom[0] * s.cam.lookfrom[0] + s.cam.lookfrom[1] * s.cam.lookfrom[1] +
                                 s.cam.lookfrom[2] * s.cam.lookfrom[2]) + std::fabs(s.cam.aperture);
    const double ob_near = ob_env > 0.0 ? ob_env : std::max(1.5 * cmax2, 1.1 * cam + 1.0);
    const double ob_far = std::max(std::max(64.0, 8.0 * cmax2), 4.0 * ob_near);
    g.ob2[0] = (float)(ob_near * ob_near * (1.0 - 1e-5)), g.ob2[1] = (float)(ob_far * ob_far * (1.0 - 1e-5));
    double ext[3], big = 0.0;
    for (int a = 0; a < 3; ++a) ext[a] = hi[a] - lo[a], big = std::max(big, ext[a]);
    int dims = 0;
    double measure = 1.0;
    bool spread[3];
    for (int a = 0; a < 3; ++a) {
        spread[a] = ext[a] > 0.05 * big;
        if (spread[a]) ++dims, measure *= ext[a];
    }
    // cell edge: a multiple of the spacing of the centres.  Measured: RTIOW (a sheet, one sphere per unit square)
    // 1.0 / 1.25 / 1.5 / 2.0 x -> 41.5 / 39.9 / 42.0 / 42.0 ms per 256 spp; 4000 spheres in a volume 0.7 / 1.0 /
    // 1.4 x -> 6.4 / 6.7 / 7.3 ms, 20000: 12.3 / 12.7 / 15.1 ms (RTMI_GRID_CELL scales the choice).
    double cell = dims ? std::pow(measure / (double)n_listed, 1.0 / dims) * (dims == 3 ? 0.85 : 1.25) * cell_factor : 1.0;
    if (!(cell > 0.0)) cell = 1.0;
    Growth gr{std::vector<double>(rest.size()), std::vector<double>(rest.size())};
    g.listed_box.assign(O.others.size(), OBox{});
    double rmax_near = 0.0, rmax_far = 0.0;
    double blo[3], bhi[3], nlo[3], nhi[3];  // bounds of the far-tier boxes (the grid's), of the near-tier boxes
    const double eps = std::ldexp(1.0, -24);
    for (;;) {
        rmax_near = rmax_far = 0.0;
        const double walk = 4e-3 * cell + 1e-5 * (cmax + 1.0);
        for (size_t k = 0; k < rest.size(); ++k) {
            const float *sp = s.prims[rest[k]].f;
            const double r = std::fabs((double)sp[3]);
            const double cn = std::sqrt((double)sp[0] * sp[0] + (double)sp[1] * sp[1] + (double)sp[2] * sp[2]);
            const double K = 32.0 * eps;
            gr.near[k] = std::sqrt(r * r + K * (ob_near + cn) * (ob_near + cn)) + walk;
            gr.far[k] = std::sqrt(r * r + K * (ob_far + cn) * (ob_far + cn)) + walk;
            rmax_near = std::max(rmax_near, gr.near[k]), rmax_far = std::max(rmax_far, gr.far[k]);
        }
        for (int a = 0; a < 3; ++a) {  // (empty without spheres: slo = +huge, shi = -huge)
            blo[a] = slo[a] - rmax_far, bhi[a] = shi[a] + rmax_far;
            nlo[a] = slo[a] - rmax_near, nhi[a] = shi[a] + rmax_near;
        }
        for (size_t k = 0; k < O.others.size(); ++k) {
            if (!O.listed[k]) continue;
            const rt_prim &p = s.prims[O.others[k]];
            double corner2 = 0.0;
            for (int a = 0; a < 3; ++a) {
                const double m = std::max(std::fabs(obox[k].lo[a]), std::fabs(obox[k].hi[a]));
                corner2 += m * m;
            }
            const double reach = ob_far + std::sqrt(corner2);
            const double gw = 64.0 * eps * reach + walk;
            OBox b = obox[k];
            if (p.type == RT_PRIM_CYLINDER) {
                const double R = std::fabs((double)p.f[0]);
                b = cyl_box(p, std::sqrt(R * R + 64.0 * eps * reach * reach), 64.0 * eps * reach);
            }
            for (int a = 0; a < 3; ++a) {
                b.lo[a] -= gw, b.hi[a] += gw;
                blo[a] = std::min(blo[a], b.lo[a]), bhi[a] = std::max(bhi[a], b.hi[a]);
                nlo[a] = std::min(nlo[a], b.lo[a]), nhi[a] = std::max(nhi[a], b.hi[a]);
            }
            g.listed_box[k] = b;
        }
        long long total = 1;
        for (int a = 0; a < 3; ++a) {
            const double span = bhi[a] - blo[a];
            g.n[a] = spread[a] ? (int)std::min(max_dim, std::max(1.0, std::ceil(span / cell))) : 1;
            g.min[a] = (float)blo[a];
            g.size[a] = (float)(span / g.n[a]);
            total *= g.n[a];
        }
        if (total <= max_cells) break;
        cell *= 1.3;
    }
    // near-tier lanes clip their rays to the bounds of the near-tier boxes: the far tier's, this much further in
    double shrink = 1e300;
    for (int a = 0; a < 3; ++a) shrink = std::min(shrink, std::min(nlo[a] - blo[a], bhi[a] - nhi[a]));
    g.shrink = (float)(std::max(0.0, shrink) * (1.0 - 1e-6));
    return gr;
}

enum class Fill {
    built,        // every cell's list fits the format
    overflow,     // a compact cell's list does not: try the wide format
    more_forced,  // primitives were added to `forced`: pack again
};

// One nested cell's sub-grid.  It spans the part of the cell that its entries' grown balls / boxes reach (a mesh is a thin
// slab of its cell) and is sized from the entries by the spacing rule of size_grid (their centres, clipped to that box), at
// most `cap` cells per axis and 8 sub-cells per entry; every entry is listed in the sub-cells its grown ball / box touches --
// the growth of the top level, whose walk term is that of the larger cell.  Appends to g.cells / items / subs.
// False: a sub-cell's list overflows the wide format (its members are then in `forced`).
bool nest_cell(const Scene &s, const SphereSlots &S, const OtherPrims &O, const Growth &gr, Grid &g, std::vector<char> &forced,
               const int cell_idx[3], const std::vector<uint32_t> &near, const std::vector<uint32_t> &far,
               const std::vector<uint32_t> &others, int cap) {
    double clo[3], chi[3];
    for (int a = 0; a < 3; ++a)
        clo[a] = (double)g.min[a] + (double)g.size[a] * cell_idx[a], chi[a] = (double)g.min[a] + (double)g.size[a] * (cell_idx[a] + 1);
    const int ns = S.ns();
    const double cell_lo[3] = {clo[0], clo[1], clo[2]}, cell_hi[3] = {chi[0], chi[1], chi[2]};
    auto rest_of = [&](uint32_t slot) { return (size_t)(((int)slot - S.np) / (RT_CLUSTER + 1) * RT_CLUSTER + ((int)slot - S.np) % (RT_CLUSTER + 1)); };
    {  // what the entries reach of the cell
        double rlo[3] = {1e300, 1e300, 1e300}, rhi[3] = {-1e300, -1e300, -1e300};
        for (const std::vector<uint32_t> *v : {&near, &far})
            for (uint32_t slot : *v) {
                const size_t k = rest_of(slot);
                for (int a = 0; a < 3; ++a) {
                    const double c = (double)s.prims[S.rest[k]].f[a];
                    rlo[a] = std::min(rlo[a], c - gr.far[k]), rhi[a] = std::max(rhi[a], c + gr.far[k]);
                }
            }
        for (uint32_t gid : others) {
            const OBox &b = g.listed_box[(size_t)O.oidx[O.prim_of_gid((int)gid, ns)]];
            for (int a = 0; a < 3; ++a) rlo[a] = std::min(rlo[a], b.lo[a]), rhi[a] = std::max(rhi[a], b.hi[a]);
        }
        for (int a = 0; a < 3; ++a) {
            clo[a] = std::min(std::max(rlo[a], cell_lo[a]), cell_hi[a]), chi[a] = std::max(std::min(rhi[a], cell_hi[a]), cell_lo[a]);
            if (!(chi[a] - clo[a] > 1e-6 * (cell_hi[a] - cell_lo[a]))) clo[a] = cell_lo[a], chi[a] = cell_hi[a];  // (degenerate: the whole cell)
        }
    }
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    auto add_point = [&](const double *c) {
        for (int a = 0; a < 3; ++a) {
            const double x = std::min(std::max(c[a], clo[a]), chi[a]);
            lo[a] = std::min(lo[a], x), hi[a] = std::max(hi[a], x);
        }
    };
    for (const std::vector<uint32_t> *v : {&near, &far})
        for (uint32_t slot : *v) {
            const float *sp = s.prims[S.slots[slot]].f;
            const double c[3] = {sp[0], sp[1], sp[2]};
            add_point(c);
        }
    for (uint32_t gid : others) {
        const OBox &b = O.obox[(size_t)O.oidx[O.prim_of_gid((int)gid, ns)]];
        const double c[3] = {0.5 * (b.lo[0] + b.hi[0]), 0.5 * (b.lo[1] + b.hi[1]), 0.5 * (b.lo[2] + b.hi[2])};
        add_point(c);
    }
    const size_t count = near.size() + far.size() + others.size();
    double ext[3], big = 0.0, measure = 1.0;
    for (int a = 0; a < 3; ++a) ext[a] = hi[a] - lo[a], big = std::max(big, ext[a]);
    int dims = 0, n[3];
    bool spread[3];
    for (int a = 0; a < 3; ++a) {
        spread[a] = ext[a] > 0.05 * big;
        if (spread[a]) ++dims, measure *= ext[a];
    }
    double cell = dims ? std::pow(measure / (double)count, 1.0 / dims) * (dims == 3 ? 0.85 : 1.25) : 1.0;
    if (!(cell > 0.0)) cell = 1.0;
    for (;;) {
        long long total = 1;
        for (int a = 0; a < 3; ++a) {
            n[a] = spread[a] ? (int)std::min((double)cap, std::max(1.0, std::ceil((chi[a] - clo[a]) / cell))) : 1;
            total *= n[a];
        }
        if (total <= 8LL * (long long)count) break;
        cell *= 1.3;
    }
    float smin[3], ssize[3];
    for (int a = 0; a < 3; ++a) smin[a] = (float)clo[a], ssize[a] = (float)((chi[a] - clo[a]) / n[a]);
    auto cell_of = [&](int a, double x) {
        const int i = (int)std::floor((x - (double)smin[a]) / (double)ssize[a]);
        return std::min(std::max(i, 0), n[a] - 1);
    };
    const size_t n_sub = (size_t)n[0] * n[1] * n[2];
    std::vector<std::vector<uint32_t>> lists(n_sub), extra(n_sub), olist(n_sub);
    for (int tier = 0; tier < 2; ++tier)
        for (uint32_t slot : tier ? far : near) {
            const size_t k = rest_of(slot);
            int c0[3], c1[3], n0[3], n1[3];
            for (int a = 0; a < 3; ++a) {
                const double c = (double)s.prims[S.rest[k]].f[a];
                c0[a] = cell_of(a, c - gr.far[k]), c1[a] = cell_of(a, c + gr.far[k]);
                n0[a] = cell_of(a, c - gr.near[k]), n1[a] = cell_of(a, c + gr.near[k]);
            }
            for (int iz = c0[2]; iz <= c1[2]; ++iz)
                for (int iy = c0[1]; iy <= c1[1]; ++iy)
                    for (int ix = c0[0]; ix <= c1[0]; ++ix) {
                        // (an entry of the outer cell's far tier stays in the far tier of every sub-cell)
                        const bool nr = tier == 0 && ix >= n0[0] && ix <= n1[0] && iy >= n0[1] && iy <= n1[1] && iz >= n0[2] && iz <= n1[2];
                        (nr ? lists : extra)[((size_t)iz * n[1] + iy) * n[0] + ix].push_back(slot);
                    }
        }
    for (uint32_t gid : others) {
        const OBox &b = g.listed_box[(size_t)O.oidx[O.prim_of_gid((int)gid, ns)]];
        int c0[3], c1[3];
        for (int a = 0; a < 3; ++a) c0[a] = cell_of(a, b.lo[a]), c1[a] = cell_of(a, b.hi[a]);
        for (int iz = c0[2]; iz <= c1[2]; ++iz)
            for (int iy = c0[1]; iy <= c1[1]; ++iy)
                for (int ix = c0[0]; ix <= c1[0]; ++ix) olist[((size_t)iz * n[1] + iy) * n[0] + ix].push_back(gid);
    }
    const uint32_t first_cell = (uint32_t)(g.cells.size() / 2);
    bool ok = true;
    for (size_t c = 0; c < n_sub; ++c) {
        const size_t n_near = lists[c].size(), n_all = n_near + extra[c].size(), n_other = olist[c].size();
        if (n_all > 1023 || n_other > 4095 || g.items.size() + n_all + n_other >= ((size_t)1 << 30)) {
            ok = false;  // one level of nesting: a clump even here is tested for every query, as in the flat tables
            for (uint32_t slot : lists[c]) forced[S.slots[slot]] = 1;
            for (uint32_t slot : extra[c]) forced[S.slots[slot]] = 1;
            for (uint32_t gid : olist[c]) forced[O.prim_of_gid((int)gid, ns)] = 1;
            continue;
        }
        g.cells.push_back((uint32_t)g.items.size());
        g.cells.push_back((uint32_t)n_near | ((uint32_t)n_all << 10) | ((uint32_t)n_other << 20));
        g.items.insert(g.items.end(), lists[c].begin(), lists[c].end());
        g.items.insert(g.items.end(), extra[c].begin(), extra[c].end());
        g.items.insert(g.items.end(), olist[c].begin(), olist[c].end());
        g.sub_items += n_all + n_other;
        g.longest = std::max(g.longest, n_all + n_other);
    }
    float rec[16] = {};
    for (int a = 0; a < 3; ++a) rec[a] = smin[a], rec[4 + a] = ssize[a] > 0.0f ? 1.0f / ssize[a] : 0.0f, rec[8 + a] = ssize[a], rec[12 + a] = bits(n[a]);
    rec[3] = bits((int32_t)first_cell);
    g.subs.insert(g.subs.end(), rec, rec + 16);
    return ok;
}

// The cells' lists in g's format.  nest_over > 0 (wide tables): a cell whose list is longer becomes a nested cell (nest_cell).
Fill fill_cells(const Scene &s, const SphereSlots &S, const OtherPrims &O, const Growth &gr, Grid &g, std::vector<char> &forced,
                size_t nest_over = 0, int nest_cap = 0) {
    const size_t max_per_cell = g.wide ? 1023 : 63, max_other = 4095;
    const size_t max_items = g.wide ? ((size_t)1 << 30) : ((size_t)1 << 20);
    const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
    std::vector<std::vector<uint32_t>> lists((size_t)nx * ny * nz), extra((size_t)nx * ny * nz), olist((size_t)nx * ny * nz);
    auto cell_of = [&](int a, double x) {
        const int i = (int)std::floor((x - (double)g.min[a]) / (double)g.size[a]);
        return std::min(std::max(i, 0), g.n[a] - 1);
    };
    for (size_t k = 0; k < S.rest.size(); ++k) {
        const int slot = S.slot_of(k);
        int c0[3], c1[3], n0[3], n1[3];
        for (int a = 0; a < 3; ++a) {
            const double c = (double)s.prims[S.rest[k]].f[a];
            c0[a] = cell_of(a, c - gr.far[k]), c1[a] = cell_of(a, c + gr.far[k]);
            n0[a] = cell_of(a, c - gr.near[k]), n1[a] = cell_of(a, c + gr.near[k]);
        }
        for (int iz = c0[2]; iz <= c1[2]; ++iz)
            for (int iy = c0[1]; iy <= c1[1]; ++iy)
                for (int ix = c0[0]; ix <= c1[0]; ++ix) {
                    const bool near = ix >= n0[0] && ix <= n1[0] && iy >= n0[1] && iy <= n1[1] && iz >= n0[2] && iz <= n1[2];
                    (near ? lists : extra)[((size_t)iz * ny + iy) * nx + ix].push_back((uint32_t)slot);
                }
    }
    // the other primitives; one that would be listed in more than 4096 cells is tested for every query instead
    bool too_wide = false;
    for (size_t k = 0; k < O.others.size(); ++k) {
        if (!O.listed[k]) continue;
        int c0[3], c1[3];
        long long cells = 1;
        for (int a = 0; a < 3; ++a) {
            c0[a] = cell_of(a, g.listed_box[k].lo[a]), c1[a] = cell_of(a, g.listed_box[k].hi[a]);
            cells *= c1[a] - c0[a] + 1;
        }
        if (cells > 4096) {
            forced[O.others[k]] = 1, too_wide = true;
            continue;
        }
        for (int iz = c0[2]; iz <= c1[2]; ++iz)
            for (int iy = c0[1]; iy <= c1[1]; ++iy)
                for (int ix = c0[0]; ix <= c1[0]; ++ix) olist[((size_t)iz * ny + iy) * nx + ix].push_back((uint32_t)O.gid[O.others[k]]);
    }
    if (too_wide) return Fill::more_forced;
    g.cells.resize(lists.size() * (g.wide ? 2 : 1));
    g.top_cells = (int)lists.size();
    if (nest_over > 0 && (lists.size() & 1)) g.cells.resize(g.cells.size() + 2), ++g.top_cells;  // (an empty cell: the sub-cells start on a record)
    bool overflow = false;
    for (size_t cidx = 0; cidx < lists.size(); ++cidx) {
        const size_t n_near = lists[cidx].size(), n_all = n_near + extra[cidx].size(), n_other = olist[cidx].size();
        if (nest_over > 0 && n_all + n_other > nest_over) {
            const int cell_idx[3] = {(int)(cidx % (size_t)nx), (int)(cidx / (size_t)nx % (size_t)ny), (int)(cidx / ((size_t)nx * ny))};
            g.cells[2 * cidx] = (uint32_t)(g.subs.size() / 16), g.cells[2 * cidx + 1] = kNestedMark;
            if (!nest_cell(s, S, O, gr, g, forced, cell_idx, lists[cidx], extra[cidx], olist[cidx], nest_cap)) overflow = true, g.demoted = true;
            continue;
        }
        g.longest = std::max(g.longest, n_all + n_other);
        if (n_all > max_per_cell || n_other > max_other || g.items.size() + n_all + n_other >= max_items) {
            overflow = true;
            if (g.wide) {  // a clump even for the wide tables: its members are tested for every query from now on
                g.demoted = true;
                for (uint32_t slot : lists[cidx]) forced[S.slots[slot]] = 1;
                for (uint32_t slot : extra[cidx]) forced[S.slots[slot]] = 1;
                for (uint32_t gid : olist[cidx]) forced[O.prim_of_gid((int)gid, S.ns())] = 1;
            }
            continue;
        }
        if (g.wide)
            g.cells[2 * cidx] = (uint32_t)g.items.size(),
                          g.cells[2 * cidx + 1] = (uint32_t)n_near | ((uint32_t)n_all << 10) | ((uint32_t)n_other << 20);
        else
            g.cells[cidx] = ((uint32_t)g.items.size() << 12) | ((uint32_t)n_near << 6) | (uint32_t)n_all;
        g.items.insert(g.items.end(), lists[cidx].begin(), lists[cidx].end());
        g.items.insert(g.items.end(), extra[cidx].begin(), extra[cidx].end());
        g.items.insert(g.items.end(), olist[cidx].begin(), olist[cidx].end());
    }
    if (!overflow) return Fill::built;
    return g.wide ? Fill::more_forced : Fill::overflow;
}

int lay_out_hot(RenderParams &L, const Grid &g);

// The grid in the wide format if `wide`, else compact, falling back to wide when a compact list overflows or the compact
// tables would not leave the kernel its full occupancy.  L: the counts.  False: more primitives were forced, pack again.
// nest_over > 0 (with `wide`): cells with longer lists become nested cells.
bool build_grid(const Scene &s, const SphereSlots &S, const OtherPrims &O, const RenderParams &L, bool wide,
                std::vector<char> &forced, Grid &g, size_t nest_over, int nest_cap) {
    size_t n_listed = S.rest.size();
    for (char l : O.listed) n_listed += l ? 1 : 0;
    g = Grid();
    g.wide = wide;
    if (n_listed == 0) return true;  // no grid: empty tables, n = {0, 0, 0}
    for (;;) {
        const Growth gr = size_grid(s, S, O, n_listed, g);
        const Fill f = fill_cells(s, S, O, gr, g, forced, g.wide ? nest_over : 0, nest_cap);
        if (f == Fill::more_forced) return false;
        if (g.wide) return true;
        RenderParams with = L;  // (the offsets these compact tables would give)
        const size_t hot = (size_t)lay_out_hot(with, g) * 16;
        if (f == Fill::built && hot <= (size_t)knob("RTMI_GLOBAL_TABLE_BYTES", (double)kLdsTableBytes)) return true;
        g = Grid();  // once more, in the wide format
        g.wide = true;
    }
}

// ---- stage 4: the offsets -----------------------------------------------------------------
// The hot part through the grid tables, in image order; fills those offsets of L from its counts and returns the record
// count (hot_vec4_grid).  build_grid asks it whether compact tables fit LDS.
int lay_out_hot(RenderParams &L, const Grid &g) {
    int off = 0;
    off += L.ns + 4;  // sphere hot (+ never-hit padding)
    L.off_rect_hot = off;
    off += 2 * L.nr;
    L.off_cyl_hot = off;
    off += RT_CYL_STRIDE * L.nc;  // (each followed by its box)
    L.off_tri_hot = off;
    off += RT_TRI_STRIDE * L.nt;
    off += RT_QUAD_STRIDE * L.nq;  // (the quads' records, DESIGN 7q: one table with the triangles')
    L.off_cam = off;  // camera::camera's derived vectors (camera.h:9-31): read once per new sample
    off += 6;
    L.off_grid = off;  // 4 records {min.xyz, ob_near^2} {1/size.xyz, ob_far^2} {size.xyz, shrink} {nx, ny, nz, -}, then cells, then items
    off += 4;
    L.off_grid_cells = off;
    off += ((int)g.cells.size() + 3) / 4;
    L.off_grid_items = off;
    off += g.wide ? ((int)g.items.size() + 1 + 3) / 4 : ((int)g.items.size() + 1 + 7) / 8;  // (+ 1: the pair test reads one entry past a list)
    if (!g.subs.empty()) {  // the sub-grid records of the nested cells, each one 64-byte line (the header's record 3 holds the offset)
        off = (off + 3) & ~3;
        off += (int)(g.subs.size() / 4);
    }
    return off;
}

// Every offset of the image, in image order: the one place that says what the image looks like.  Returns the record count;
// image_word[k]: the first 32-bit word of image texture k's texels.
// off_media: the first record of the MEDIA part (rt_media.h; 0: the scene has no media); off_motion: of the MOTION part
// (rt_motion.h; 0: no moving spheres); off_normals: of the NORMALS part (device_scene.h; 0: no triangle has vertex normals).  -1: the environment's words would not fit an int32 offset; -2: 2^28 sphere slots or more.
// off_noise: the first record of the noise textures' parameters (device_scene.h; 0: the scene has no noise texture).
// off_bump: the first bump record (device_scene.h; 0: no material carries a bump).
// off_nmap: the first normal-map record (device_scene.h; 0: no material carries a normal map).
// off_pbr: the first side record of the pbr materials (device_scene.h, MK_PBR; 0: the scene has none).
int lay_out_image(RenderParams &L, const Grid &g, const Scene &s, std::vector<int> &image_word, int &off_media, int &off_motion,
                  int &off_normals, int &off_noise, int &off_bump, int &off_nmap, int &off_pbr) {
    // The kernels read the winner's cold record at a 32-bit BYTE offset from the cold table, 16 x its slot (rec_at,
    // render_device.h): the slots end below 2^28.  This is the check that bound rests on; pack_scene refuses with RT_ERR_LIMIT.
    if ((long long)L.ns >= RT_MAX_SPHERE_SLOTS) return -2;
    int off = lay_out_hot(L, g);
    L.hot_vec4_grid = off;  // what the grid-walk kernels stage into LDS
    // the boxes of the cluster searches (ablation builds) lie behind the grid tables, so that the grid walk does not stage
    // them (RTIOW: 2.5 KB of 15.2 KB)
    L.off_box = off;
    off += 2 * L.ncl;
    L.off_wbox = off;
    off += 2 * L.nwin;
    L.off_gbox = off;  // outer boxes: the box-hierarchy variant reads them
    off += 2 * L.ngr;
    L.hot_vec4 = off;  // what the box-hierarchy and flat-scan variants stage into LDS
    const int n_axes = (L.rt_axes & 1) + ((L.rt_axes >> 1) & 1) + ((L.rt_axes >> 2) & 1);
    L.rt_stride = 2 + n_axes * (RT_SLABS * RT_SLABS / 2);  // float4 records per window: {min, 1/width} + masks (2 per record)
    L.off_rtab = off;
    off += L.nwin * L.rt_stride;
    L.hot_vec4_tables = off;  // ... and the range-table kernel: the same plus the tables
    L.off_sph_cold = off;
    off += L.ns;
    L.off_rect_cold = off;
    off += L.nr;
    L.off_cyl_cold = off;
    off += 4 * L.nc;
    L.off_tri_cold = off;
    off += 2 * L.nt;
    off += 2 * L.nq;  // (the quads' cold records: behind the triangles', and as wide)
    L.off_mat = off;
    off += 3 * L.nm;
    // the alpha masks' records: one per material, straight behind the material table; no mask in the scene: not a byte
    if (scene_has_alpha(s)) off += L.nm;
    // texels of the image textures: one 32-bit word each, every image starts on a float4 record
    image_word.assign(s.images.size(), 0);
    for (size_t k = 0; k < s.images.size(); ++k) {
        image_word[k] = off * 4;
        off += (int)(((size_t)s.images[k].rows * s.images[k].cols + 3) / 4);
    }
    // the noise textures' parameters: one record each, in texture order; none: not a byte
    off_noise = 0;
    for (const rt_texture &t : s.texs)
        if (t.type == RT_TEX_NOISE) {
            if (!off_noise) off_noise = off;
            ++off;
        }
    // the bump records: one per bumped material, in material order, behind the noise records; none: not a byte
    off_bump = 0;
    for (const SceneBump &b : s.bumps)
        if (b.texture >= 0) {
            if (!off_bump) off_bump = off;
            ++off;
        }
    // the normal-map records: one per mapped material, in material order, behind the bump records; none: not a byte
    off_nmap = 0;
    for (const SceneNormalMap &b : s.normal_maps)
        if (b.texture >= 0) {
            if (!off_nmap) off_nmap = off;
            ++off;
        }
    // the pbr materials' side records: three rows each, in material order, behind those; none: not a byte
    off_pbr = 0;
    for (const rt_material &m : s.mats)
        if (m.type == RT_MAT_PBR) {
            if (!off_pbr) off_pbr = off;
            off += 3;
        }
    // the LIGHT part (device_scene.h): light records, alias table, light slot of every grouped primitive id
    if (L.nl > 0) {
        L.off_light = off;
        off += RT_LIGHT_STRIDE * L.nl;
        L.off_alias = off;
        off += L.nl;
        L.off_lslot = off;
        off += (L.ns + L.nr + L.nc + L.nt + L.nq + 3) / 4;
    }
    // the ENVIRONMENT part (rt_env.h): texels, then the sampler's tables -- fp32 WORD offsets; global memory only, read by the
    // environment kernels.  -1: the words would not fit an int32 offset
    if (s.env) {
        const long long R = s.env->rows, C = s.env->cols;
        long long w = (long long)off * 4;
        L.env_rows = (int)R, L.env_cols = (int)C;
        const long long tex = w, marg = tex + 3 * R * C, cond = marg + (R + 1), band = cond + R * (C + 1), ct = band + R, end = ct + (R + 1);
        if (end + 4 > (long long)INT32_MAX) return -1;
        L.off_env_tex = (int)tex, L.off_env_marg = (int)marg, L.off_env_cond = (int)cond, L.off_env_band = (int)band, L.off_env_ct = (int)ct;
        off = (int)((end + 3) / 4);
    }
    // the MEDIA part (rt_media.h): the media's records, behind everything else; global memory only, read by the media kernels
    off_media = 0;
    if (!s.media.empty()) {
        off_media = off;
        off += RT_MEDIUM_STRIDE * (int)s.media.size();
    }
    // the MOTION part (rt_motion.h): the moving spheres' records, last of all; global memory only, read by the motion kernels
    off_motion = 0;
    if (!s.movers.empty()) {
        off_motion = off;
        off += RT_MOTION_STRIDE * (int)s.movers.size();
    }
    // the NORMALS part (smooth shading): three records per triangle, only when a triangle has vertex normals; global
    // memory only, read by the winner section of the general kernels
    off_normals = 0;
    for (const rt_prim &p : s.prims)
        if (p.type == RT_PRIM_TRIANGLE && tri_has_normals(p)) {
            off_normals = off;
            off += 3 * L.nt;
            break;
        }
    return off;
}

// ---- stage 5: the writers -------------------------------------------------------------------
void write_camera(float *I, const RenderParams &L, const Scene &s) {
    if (s.cam.projection != RT_PROJ_PERSPECTIVE) {  // (the same six records, holding what rt_camera.h says for the model)
        float rec[6][3], lens_radius;
        camera_records(s, rec, &lens_radius);
        for (int k = 0; k < 6; ++k) {
            float *h = rec4(I, L.off_cam + k);
            h[0] = rec[k][0], h[1] = rec[k][1], h[2] = rec[k][2];
        }
        rec4(I, L.off_cam)[3] = lens_radius;
        return;
    }
    rt_camera cam;
    derive_camera(s, &cam);
    const float *src[6] = {cam.origin, cam.lower_left, cam.horizontal, cam.vertical, cam.u, cam.v};
    for (int k = 0; k < 6; ++k) {
        float *h = rec4(I, L.off_cam + k);
        h[0] = src[k][0], h[1] = src[k][1], h[2] = src[k][2];
    }
    rec4(I, L.off_cam)[3] = cam.lens_radius;
}

void write_spheres(float *I, const RenderParams &L, const Scene &s, const SphereSlots &S) {
    for (int k = 0; k < L.ns + 4; ++k) {
        float *h = rec4(I, k);
        const int pi = k < L.ns ? S.slots[k] : -1;
        if (pi < 0) {
            h[3] = -INFINITY;  // c = +inf, disc = -inf: never a candidate
            continue;
        }
        const rt_prim &p = s.prims[pi];
        h[0] = p.f[0], h[1] = p.f[1], h[2] = p.f[2];
        h[3] = p.f[3] * p.f[3];  // r*r in fp32, as sphere::hit evaluates it
        float *cd = rec4(I, L.off_sph_cold + k);
        cd[0] = 1.0f / p.f[3];   // (p - c) / r  ==  (1/r) * (p - c), vec3.cuh:105
        cd[1] = bits(p.material);
        cd[2] = bits(pi);
    }
}

// Boxes tested per lane with a margin (the cluster boxes of the ablation searches; the boxes of the cylinders and
// triangles that are tested for every query).  Skipping a box must never change the result of the fp32 test behind
// it, whose rounding error grows with the distance |oc| from the ray origin: with unit roundoff e = 2^-24,
// |disc_fp32 - disc| <= 15 e a |oc|^2, so a ray the sphere test can accept passes within r + sqrt(15 e)|oc| ~ r + 1e-3 |oc|
// of the centre, and its fp32 root lies within the same distance of that approach point: the hit point is inside the
// sphere's box grown by 2e-3 |oc|.  |oc| <= sqrt(3) (max|o_i| + extent), so the KERNEL grows every such box per lane by
//     m = 4e-3 (max|o_i| + extent + 1)
// (two shifted ray origins per query, no extra work per box); a ray that leaked 2000 units inside the ground sphere
// thereby visits everything, exactly like the noise it would hit.  The stored boxes only carry a 1e-5-relative pad
// for their own rounding (the listed cylinders and triangles: their grid growth, which is larger).
// Returns the extent: max |coordinate| reached by a clustered sphere, a cylinder or a triangle.
float box_extent(const Scene &s, const SphereSlots &S, const OtherPrims &O) {
    float extent = 0.0f;
    for (int k = S.np; k < S.ns(); ++k) {
        if (S.slots[k] < 0) continue;
        const rt_prim &p = s.prims[S.slots[k]];
        for (int a = 0; a < 3; ++a) extent = std::max(extent, std::fabs(p.f[a]) + std::fabs(p.f[3]));
    }
    for (int prim : O.cyl) {
        const OBox &b = O.obox[(size_t)O.oidx[prim]];
        for (int a = 0; a < 3; ++a) extent = std::max(extent, (float)std::max(std::fabs(b.lo[a]), std::fabs(b.hi[a])));
    }
    for (int prim : O.tri) {
        const rt_prim &p = s.prims[prim];
        for (int cc = 0; cc < 9; ++cc) extent = std::max(extent, std::fabs(p.m[cc]));
    }
    for (int prim : O.quad) {
        const OBox &b = O.obox[(size_t)O.oidx[prim]];
        for (int a = 0; a < 3; ++a) extent = std::max(extent, (float)std::max(std::fabs(b.lo[a]), std::fabs(b.hi[a])));
    }
    return extent;
}

// cluster boxes, their outer (group) boxes and the window boxes over those
void write_cluster_boxes(float *I, const RenderParams &L, const Scene &s, const SphereSlots &S, float inflate) {
    for (int q = 0; q < L.ncl; ++q) {
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = 0; k < RT_CLUSTER; ++k) {
            const int pi = S.slots[S.np + (RT_CLUSTER + 1) * q + k];
            if (pi < 0) continue;
            const rt_prim &p = s.prims[pi];
            const float r = std::fabs(p.f[3]);
            for (int a = 0; a < 3; ++a) lo[a] = std::min(lo[a], p.f[a] - r), hi[a] = std::max(hi[a], p.f[a] + r);
        }
        float *b = rec4(I, L.off_box + 2 * q);
        for (int a = 0; a < 3; ++a) {
            b[a] = lo[a] - inflate;
            b[4 + a] = hi[a] + inflate;
        }
    }
    for (int g = 0; g < L.ngr; ++g) {  // outer boxes: union of the (already inflated) cluster boxes
        float *gb = rec4(I, L.off_gbox + 2 * g);
        for (int a = 0; a < 3; ++a) gb[a] = INFINITY, gb[4 + a] = -INFINITY;
        for (int q = g * RT_GROUP; q < std::min(L.ncl, (g + 1) * RT_GROUP); ++q) {
            const float *b = rec4(I, L.off_box + 2 * q);
            for (int a = 0; a < 3; ++a) gb[a] = std::min(gb[a], b[a]), gb[4 + a] = std::max(gb[4 + a], b[4 + a]);
        }
    }
    const int groups_per_window = 64 / RT_GROUP;  // one 64-bit cluster mask per window in the kernel
    for (int w = 0; w < L.nwin; ++w) {  // third level (big scenes): union of the window's outer boxes
        float *wb = rec4(I, L.off_wbox + 2 * w);
        for (int a = 0; a < 3; ++a) wb[a] = INFINITY, wb[4 + a] = -INFINITY;
        for (int g = w * groups_per_window; g < std::min(L.ngr, (w + 1) * groups_per_window); ++g) {
            const float *b = rec4(I, L.off_gbox + 2 * g);
            for (int a = 0; a < 3; ++a) wb[a] = std::min(wb[a], b[a]), wb[4 + a] = std::max(wb[4 + a], b[4 + a]);
        }
    }
}

// range tables of every window (what they hold: range_axes); reads the cluster and window boxes
void write_range_tables(float *I, const RenderParams &L) {
    for (int w = 0; w < L.nwin; ++w) {
        const float *wb = rec4(I, L.off_wbox + 2 * w);
        float *hd = rec4(I, L.off_rtab + w * L.rt_stride);
        uint64_t *masks = reinterpret_cast<uint64_t *>(hd + 8);
        const int q0 = w * 64, q1 = std::min(L.ncl, q0 + 64);
        int ai = 0;
        for (int a = 0; a < 3; ++a) {
            const float lo = wb[a], hi = wb[4 + a];
            const float width = (hi - lo) / (float)RT_SLABS;
            hd[a] = lo;
            hd[4 + a] = width > 0.0f ? 1.0f / width : 0.0f;  // a window that is flat on this axis: every point -> slab 0
            if (!((L.rt_axes >> a) & 1)) continue;
            uint64_t slab[RT_SLABS];
            // the kernel finds a point's slab as floor((x - lo) * (1 / width)) in fp32: grow every slab by a tolerance
            // far above that rounding so that a cluster touching a slab boundary is listed on both sides
            const float tol = 1e-3f * width + 1e-5f * (std::fabs(lo) + std::fabs(hi));
            for (int i = 0; i < RT_SLABS; ++i) {
                const float a0 = lo + width * (float)i - tol, a1 = lo + width * (float)(i + 1) + tol;
                uint64_t m = 0;
                for (int q = q0; q < q1; ++q) {
                    const float *b = rec4(I, L.off_box + 2 * q);
                    // the first and last slab also stand for everything outside the window box on their side
                    const bool over = (i == 0 || b[4 + a] >= a0) && (i == RT_SLABS - 1 || b[a] <= a1);
                    if (over || !(width > 0.0f)) m |= 1ull << (q - q0);
                }
                slab[i] = m;
            }
            uint64_t *R = masks + (size_t)ai * RT_SLABS * RT_SLABS;
            for (int i0 = 0; i0 < RT_SLABS; ++i0) {
                uint64_t m = 0;
                for (int i1 = 0; i1 < RT_SLABS; ++i1) {
                    if (i1 >= i0) m |= slab[i1];
                    R[i0 * RT_SLABS + i1] = i1 >= i0 ? m : 0;
                }
            }
            ++ai;
        }
    }
}

void write_grid(float *I, const RenderParams &L, const Grid &gr) {
    float *g = rec4(I, L.off_grid);
    for (int a = 0; a < 3; ++a) {
        g[a] = gr.min[a];
        g[4 + a] = gr.size[a] > 0.0f ? 1.0f / gr.size[a] : 0.0f;
        g[8 + a] = gr.size[a];
        g[12 + a] = bits(gr.n[a]);
    }
    g[3] = gr.ob2[0], g[7] = gr.ob2[1], g[11] = gr.shrink;
    if (!gr.subs.empty()) {
        const int off_sub = (L.off_grid_items + ((int)gr.items.size() + 1 + 3) / 4 + 3) & ~3;
        g[15] = bits(off_sub);
        memcpy(rec4(I, off_sub), gr.subs.data(), gr.subs.size() * sizeof(float));
    }
    if (!gr.cells.empty()) memcpy(rec4(I, L.off_grid_cells), gr.cells.data(), gr.cells.size() * sizeof(uint32_t));
    if (gr.items.empty()) return;
    if (gr.wide) {
        memcpy(rec4(I, L.off_grid_items), gr.items.data(), gr.items.size() * sizeof(uint32_t));
    } else {
        uint16_t *dst = reinterpret_cast<uint16_t *>(rec4(I, L.off_grid_items));
        for (size_t i = 0; i < gr.items.size(); ++i) dst[i] = (uint16_t)gr.items[i];
    }
}

// rects, cylinders and triangles: hot and cold records, the boxes of the cylinders and triangles
void write_others(float *I, const RenderParams &L, const Scene &s, const OtherPrims &O, const Grid &g, float inflate) {
    auto store_box = [&](float *b, int prim) {
        const size_t k = (size_t)O.oidx[prim];
        const bool grown = O.listed[k] && !g.cells.empty();
        const OBox &src = grown ? g.listed_box[k] : O.obox[k];
        for (int a = 0; a < 3; ++a) {
            // (rounded outwards: the grown box is a double-precision bound)
            b[a] = std::nextafterf((float)src.lo[a], -INFINITY) - inflate;
            b[4 + a] = std::nextafterf((float)src.hi[a], INFINITY) + inflate;
        }
    };
    for (int k = 0; k < L.nr; ++k) {
        const rt_prim &p = s.prims[O.rec[k]];
        float *h = rec4(I, L.off_rect_hot + 2 * k);
        h[0] = p.f[0], h[1] = p.f[1], h[2] = p.f[2], h[3] = p.f[3];
        h[4] = p.f[4];
        h[5] = bits(p.type - RT_PRIM_XY_RECT);
        float *cd = rec4(I, L.off_rect_cold + k);
        cd[0] = bits(p.material);
        cd[1] = bits(O.rec[k]);
    }
    for (int k = 0; k < L.nc; ++k) {
        const rt_prim &p = s.prims[O.cyl[k]];
        float *h = rec4(I, L.off_cyl_hot + RT_CYL_STRIDE * k);
        memcpy(h, p.m_inv, 12 * sizeof(float));
        h[12] = p.f[0] * p.f[0], h[13] = p.f[1], h[14] = p.f[2];
        store_box(h + 16, O.cyl[k]);  // (records 4 and 5)
        float *cd = rec4(I, L.off_cyl_cold + 4 * k);
        memcpy(cd, p.m, 12 * sizeof(float));
        cd[12] = bits(p.material);
        cd[13] = bits(O.cyl[k]);
    }
    for (int k = 0; k < L.nt; ++k) {
        const rt_prim &p = s.prims[O.tri[k]];
        float *h = rec4(I, L.off_tri_hot + RT_TRI_STRIDE * k);
        for (int cc = 0; cc < 3; ++cc) {
            h[4 * cc] = p.m[3 * cc], h[4 * cc + 1] = p.m[3 * cc + 1], h[4 * cc + 2] = p.m[3 * cc + 2];
            h[4 * cc + 3] = p.m[9 + cc];
        }
        store_box(h + 12, O.tri[k]);  // (records 3 and 4)
        float *cd = rec4(I, L.off_tri_cold + 2 * k);
        cd[0] = bits(p.material), cd[1] = bits(O.tri[k]);
        cd[2] = p.m_inv[0], cd[3] = p.m_inv[1];
        cd[4] = p.m_inv[2], cd[5] = p.m_inv[3], cd[6] = p.m_inv[4], cd[7] = p.m_inv[5];
    }
    // quads: {Q, n.x} {A, n.y} {B, n.z}, the box; cold {material, list index, 0, 0} {0, 0, 0, 0}
    for (int k = 0; k < L.nq; ++k) {
        const rt_prim &p = s.prims[O.quad[k]];
        float *h = rec4(I, L.off_tri_hot + RT_TRI_STRIDE * L.nt + RT_QUAD_STRIDE * k);
        for (int cc = 0; cc < 3; ++cc) {
            h[cc] = p.m[cc], h[4 + cc] = p.m_inv[cc], h[8 + cc] = p.m_inv[3 + cc];
            h[4 * cc + 3] = p.m[9 + cc];
        }
        store_box(h + 12, O.quad[k]);  // (records 3 and 4)
        float *cd = rec4(I, L.off_tri_cold + 2 * (L.nt + k));
        cd[0] = bits(p.material), cd[1] = bits(O.quad[k]);
    }
}

void write_texels(float *I, const Scene &s, const std::vector<int> &image_word) {
    for (size_t k = 0; k < s.images.size(); ++k) {
        const SceneImage &im = s.images[k];
        uint32_t *w = reinterpret_cast<uint32_t *>(I) + image_word[k];
        for (size_t t = 0; t < (size_t)im.rows * im.cols; ++t)
            w[t] = (uint32_t)im.rgb[3 * t] | ((uint32_t)im.rgb[3 * t + 1] << 8) | ((uint32_t)im.rgb[3 * t + 2] << 16);
        // an alpha plane (rt_alpha.h): 255 - a8 in the top byte, so that an opaque texel keeps the word it had
        if (!im.alpha.empty())
            for (size_t t = 0; t < (size_t)im.rows * im.cols; ++t) w[t] |= alpha_word_bits(im.alpha[t]);
    }
}

// the alpha masks' records: material m's at off_alpha + m (off_alpha = off_mat + 3 nm), {word offset of the mask's texels (bits), rows (bits),
// cols (bits), c8 (bits)}; a material without a mask keeps zeros (rows = 0)
void write_alphas(float *I, const Scene &s, int off_alpha, const std::vector<int> &image_word) {
    for (size_t m = 0; m < s.alphas.size() && m < s.mats.size(); ++m) {
        if (s.alphas[m].texture < 0) continue;
        const size_t im = (size_t)s.texs[(size_t)s.alphas[m].texture].c0[0];
        float *q = rec4(I, off_alpha + (int)m);
        q[0] = bits(image_word[im]), q[1] = bits(s.images[im].rows), q[2] = bits(s.images[im].cols);
        q[3] = bits((int)alpha_cutoff_byte((double)s.alphas[m].cutoff));
    }
}

// the noise textures' records {scale, distortion, seed, style | axis << 2 | octaves << 4}; noise_rec[i]: texture i's record
void write_noise(float *I, const Scene &s, int off_noise, std::vector<int> &noise_rec) {
    noise_rec.assign(s.texs.size(), 0);
    int at = off_noise;
    for (size_t i = 0; i < s.texs.size(); ++i) {
        if (s.texs[i].type != RT_TEX_NOISE) continue;
        const rt_noise &n = s.noise[i];
        float *q = rec4(I, at);
        q[0] = n.scale, q[1] = n.distortion, q[3] = bits((int32_t)noise_pack(n.style, n.axis, n.octaves));
        memcpy(q + 2, &n.seed, 4);  // (any 32 bits: never through a float register)
        noise_rec[i] = at++;
    }
}

// the bump records {offset of the texture's noise record (bits), strength, 0, 0}; bump_rec[m]: material m's record, 0: none
void write_bumps(float *I, const Scene &s, int off_bump, const std::vector<int> &noise_rec, std::vector<int> &bump_rec) {
    bump_rec.assign(s.mats.size(), 0);
    int at = off_bump;
    for (size_t m = 0; m < s.bumps.size() && m < s.mats.size(); ++m) {
        if (s.bumps[m].texture < 0) continue;
        float *q = rec4(I, at);
        q[0] = bits(noise_rec[(size_t)s.bumps[m].texture]), q[1] = s.bumps[m].strength;
        bump_rec[m] = at++;
    }
}

// the normal-map records {word offset of the image's texels (bits), rows (bits), cols (bits), scale} -- the first three as an
// image-textured material's second row holds them; bump_rec[m] = MINUS material m's record (a material carries a bump or a map)
void write_normal_maps(float *I, const Scene &s, int off_nmap, const std::vector<int> &image_word, std::vector<int> &bump_rec) {
    int at = off_nmap;
    for (size_t m = 0; m < s.normal_maps.size() && m < s.mats.size(); ++m) {
        if (s.normal_maps[m].texture < 0) continue;
        const size_t im = (size_t)s.texs[(size_t)s.normal_maps[m].texture].c0[0];
        float *q = rec4(I, at);
        q[0] = bits(image_word[im]), q[1] = bits(s.images[im].rows), q[2] = bits(s.images[im].cols), q[3] = s.normal_maps[m].scale;
        bump_rec[m] = -(at++);
    }
}

void write_materials(float *I, const RenderParams &L, const Scene &s, const SphereSlots &S, const OtherPrims &O,
                     const std::vector<int> &image_word, const std::vector<int> &noise_rec, const std::vector<int> &bump_rec, int off_pbr) {
    // a noise texture under a material: the two colours where a checker keeps them, the record's offset in c0.w
    auto noise_words = [&](float *q, const rt_material &m, const rt_texture &t) {
        q[4] = t.c0[0], q[5] = t.c0[1], q[6] = t.c0[2], q[7] = bits(noise_rec[(size_t)m.texture]);
        q[8] = t.c1[0], q[9] = t.c1[1], q[10] = t.c1[2];
    };
    // a pbr material's texture of any type into rows 1 and 2 of q, as the textured kinds keep theirs -> its type code
    // (0 solid, 1 checker, 2 image, 3 noise); texture -1 (no map): solid white
    auto pbr_texture = [&](float *q, int texture) {
        if (texture < 0) {
            q[4] = q[5] = q[6] = 1.0f;
            return 0;
        }
        const rt_texture &t = s.texs[(size_t)texture];
        if (t.type == RT_TEX_IMAGE) {
            const size_t im = (size_t)t.c0[0];
            q[4] = bits(image_word[im]), q[5] = bits(s.images[im].rows), q[6] = bits(s.images[im].cols);
            return 2;
        }
        q[4] = t.c0[0], q[5] = t.c0[1], q[6] = t.c0[2];
        q[8] = t.c1[0], q[9] = t.c1[1], q[10] = t.c1[2];
        if (t.type == RT_TEX_NOISE) q[7] = bits(noise_rec[(size_t)texture]);
        return t.type == RT_TEX_NOISE ? 3 : (t.type == RT_TEX_CHECKER ? 1 : 0);
    };
    int pbr_at = off_pbr;
    for (int k = 0; k < L.nm; ++k) {
        const rt_material &m = s.mats[k];
        float *q = rec4(I, L.off_mat + 3 * k);
        int kind = MK_LAMBERT_SOLID;
        const rt_texture *t = (m.texture >= 0 && m.texture < (int)s.texs.size()) ? &s.texs[m.texture] : nullptr;
        switch (m.type) {
        case RT_MAT_LAMBERTIAN:
        case RT_MAT_DIFFUSE_LIGHT: {
            bool light = m.type == RT_MAT_DIFFUSE_LIGHT;
            bool checker = t && t->type == RT_TEX_CHECKER;
            kind = light ? (checker ? MK_LIGHT_CHECKER : MK_LIGHT_SOLID) : (checker ? MK_LAMBERT_CHECKER : MK_LAMBERT_SOLID);
            if (t && t->type == RT_TEX_IMAGE) {
                kind = light ? MK_LIGHT_IMAGE : MK_LAMBERT_IMAGE;
                const size_t im = (size_t)t->c0[0];
                q[4] = bits(image_word[im]), q[5] = bits(s.images[im].rows), q[6] = bits(s.images[im].cols);
            } else if (t && t->type == RT_TEX_NOISE) {
                kind = light ? MK_LIGHT_NOISE : MK_LAMBERT_NOISE;
                noise_words(q, m, *t);
            } else if (t) {
                q[4] = t->c0[0], q[5] = t->c0[1], q[6] = t->c0[2];
                q[8] = t->c1[0], q[9] = t->c1[1], q[10] = t->c1[2];
            }
            break;
        }
        case RT_MAT_METAL:
            kind = MK_METAL;
            q[1] = m.fuzz;
            q[4] = m.albedo[0], q[5] = m.albedo[1], q[6] = m.albedo[2];
            break;
        case RT_MAT_DIELECTRIC: {
            kind = MK_DIELECTRIC;
            float ir = m.ir, inv_ir = 1.0f / m.ir;
            // reflectance()'s r0 for both refraction ratios, material.cuh:175-178
            float r0f = (1.0f - inv_ir) / (1.0f + inv_ir);
            r0f = r0f * r0f;
            float r0b = (1.0f - ir) / (1.0f + ir);
            r0b = r0b * r0b;
            q[1] = ir, q[2] = inv_ir, q[3] = r0f, q[7] = r0b;
            break;
        }
        case RT_MAT_ROUGH_METAL:  // alpha = max(r^2, 1e-3), and r itself for the light-sample threshold
            kind = MK_ROUGH_METAL;
            q[1] = std::max(m.fuzz * m.fuzz, 1e-3f), q[3] = m.fuzz;
            q[4] = m.albedo[0], q[5] = m.albedo[1], q[6] = m.albedo[2];
            break;
        case RT_MAT_PLASTIC: {
            float r0 = (m.ir - 1.0f) / (m.ir + 1.0f);
            r0 = r0 * r0;
            q[1] = std::max(m.fuzz * m.fuzz, 1e-3f), q[2] = r0, q[3] = m.fuzz;
            kind = (t && t->type == RT_TEX_CHECKER) ? MK_PLASTIC_CHECKER : MK_PLASTIC_SOLID;
            if (t && t->type == RT_TEX_IMAGE) {
                kind = MK_PLASTIC_IMAGE;
                const size_t im = (size_t)t->c0[0];
                q[4] = bits(image_word[im]), q[5] = bits(s.images[im].rows), q[6] = bits(s.images[im].cols);
            } else if (t && t->type == RT_TEX_NOISE) {
                kind = MK_PLASTIC_NOISE;
                noise_words(q, m, *t);
            } else if (t) {
                q[4] = t->c0[0], q[5] = t->c0[1], q[6] = t->c0[2];
                q[8] = t->c1[0], q[9] = t->c1[1], q[10] = t->c1[2];
            }
            break;
        }
        case RT_MAT_ROUGH_GLASS:  // eta of a front hit in p1, of a back hit in c0.w; albedo holds sigma
            kind = MK_ROUGH_GLASS;
            q[1] = std::max(m.fuzz * m.fuzz, 1e-3f), q[2] = 1.0f / m.ir, q[3] = m.fuzz;
            q[4] = m.albedo[0], q[5] = m.albedo[1], q[6] = m.albedo[2], q[7] = m.ir;
            break;
        case RT_MAT_PBR: {  // the base texture here, the factors and the map in the side record
            kind = MK_PBR;
            float r0 = (m.ir - 1.0f) / (m.ir + 1.0f);
            r0 = r0 * r0;
            float *sd = rec4(I, pbr_at);
            sd[0] = m.albedo[0], sd[1] = m.fuzz;
            const int base = pbr_texture(q, m.texture), map = pbr_texture(sd, scene_pbr_map(s, k));
            q[1] = bits(pbr_at), q[2] = r0, q[3] = bits(base | map << 4);
            pbr_at += 3;
            break;
        }
        default: break;
        }
        q[0] = bits(kind);
        // a bump: its record's offset in c1.w, the one word no kind above uses; 0: none.  (A normal map, DESIGN 7u:
        // minus its record's offset)
        if (bump_rec[(size_t)k]) q[11] = bits(bump_rec[(size_t)k]);
    }
    // The material kind of every sphere, rect and cylinder sits in its cold record too: the shading then knows after ONE
    // dependent load (the primitive's cold record) whether the path ends, scatters or needs a rejection sample, instead
    // of two (cold record -> material record).
    auto kind_of = [&](int material) { return I[(size_t)(L.off_mat + 3 * material) * 4]; };  // the bits, as a float
    for (int k = 0; k < L.ns; ++k)
        if (S.slots[k] >= 0) rec4(I, L.off_sph_cold + k)[3] = kind_of(s.prims[S.slots[k]].material);
    for (int k = 0; k < L.nr; ++k) rec4(I, L.off_rect_cold + k)[2] = kind_of(s.prims[O.rec[k]].material);
    for (int k = 0; k < L.nc; ++k) rec4(I, L.off_cyl_cold + 4 * k)[14] = kind_of(s.prims[O.cyl[k]].material);
}

// light records, the alias table and the light slot of every grouped primitive id
void write_lights(float *I, const RenderParams &L, const Scene &s, const SphereSlots &S, const OtherPrims &O,
                  const std::vector<SceneLight> &lights) {
    std::vector<int> group_id(s.prims.size(), -1);
    for (int k = 0; k < L.ns; ++k)
        if (S.slots[k] >= 0) group_id[(size_t)S.slots[k]] = k;
    for (int k = 0; k < L.nr; ++k) group_id[(size_t)O.rec[k]] = L.ns + k;
    for (int k = 0; k < L.nc; ++k) group_id[(size_t)O.cyl[k]] = L.ns + L.nr + k;
    for (int k = 0; k < L.nt; ++k) group_id[(size_t)O.tri[k]] = L.ns + L.nr + L.nc + k;
    for (int k = 0; k < L.nq; ++k) group_id[(size_t)O.quad[k]] = L.ns + L.nr + L.nc + L.nt + k;
    int32_t *slot = reinterpret_cast<int32_t *>(rec4(I, L.off_lslot));
    for (int k = 0; k < L.ns + L.nr + L.nc + L.nt + L.nq; ++k) slot[k] = -1;
    for (int i = 0; i < L.nl; ++i) {
        const SceneLight &l = lights[(size_t)i];
        if (l.analytic >= 0) {  // point / spot / distant (rt_lights.h): shapes 6 / 7 / 8, no primitive, no slot
            const rt_analytic_light &al = s.alights[(size_t)l.analytic];
            const AnalyticRecord a = analytic_record(al, scene_bound_radius(s));
            float *r = rec4(I, L.off_light + RT_LIGHT_STRIDE * i);
            r[0] = bits(al.type == RT_LIGHT_POINT ? 6 : (al.type == RT_LIGHT_SPOT ? 7 : 8)), r[1] = bits(-1);
            r[2] = (float)l.prob, r[3] = (float)(1.0 / l.area);
            for (int c3 = 0; c3 < 3; ++c3) r[4 + c3] = r[8 + c3] = a.color[c3];
            float *g = r + 12;
            if (al.type == RT_LIGHT_DISTANT) {
                for (int c3 = 0; c3 < 3; ++c3) g[c3] = (float)a.dir[c3];
                g[3] = a.omc, g[4] = a.dist;
            } else {
                for (int c3 = 0; c3 < 3; ++c3) g[c3] = al.position[c3];
                if (al.type == RT_LIGHT_SPOT) {
                    for (int c3 = 0; c3 < 3; ++c3) g[4 + c3] = (float)a.dir[c3];
                    g[8] = a.cos_o, g[9] = a.inv;
                }
            }
            continue;
        }
        if (l.prim < 0) {  // the environment: shape 3, no primitive, no geometry (rt_env.h samples it)
            float *r = rec4(I, L.off_light + RT_LIGHT_STRIDE * i);
            r[0] = bits(3), r[1] = bits(-1), r[2] = (float)l.prob, r[3] = (float)(1.0 / l.area);
            continue;
        }
        const rt_prim &p = s.prims[(size_t)l.prim];
        const int gid = group_id[(size_t)l.prim];
        slot[gid] = i;
        float *r = rec4(I, L.off_light + RT_LIGHT_STRIDE * i);
        const int shape = p.type == RT_PRIM_SPHERE ? 0 : (p.type == RT_PRIM_CYLINDER ? 2 : (p.type == RT_PRIM_TRIANGLE ? 4 : (p.type == RT_PRIM_QUAD ? 5 : 1)));
        r[0] = bits(shape), r[1] = bits(gid), r[2] = (float)l.prob, r[3] = (float)(1.0 / l.area);
        for (int c3 = 0; c3 < 3; ++c3) r[4 + c3] = l.even[c3], r[8 + c3] = l.odd[c3];
        r[7] = bits(l.checker ? 1 : 0);
        float *g = r + 12;
        if (shape == 0) {
            g[0] = p.f[0], g[1] = p.f[1], g[2] = p.f[2], g[3] = std::fabs(p.f[3]);
        } else if (shape == 1) {
            g[0] = p.f[0], g[1] = p.f[1], g[2] = p.f[2], g[3] = p.f[3];
            g[4] = p.f[4], g[5] = bits(p.type - RT_PRIM_XY_RECT);
        } else if (shape == 2) {
            memcpy(g, p.m, 12 * sizeof(float));
            g[12] = std::fabs(p.f[0]), g[13] = p.f[1], g[14] = p.f[2];
        } else if (shape == 5) {  // quad: Q, u, v and the unit normal
            for (int c3 = 0; c3 < 3; ++c3) g[c3] = p.m[c3], g[4 + c3] = p.m[3 + c3], g[8 + c3] = p.m[6 + c3], g[12 + c3] = p.m[9 + c3];
        } else {  // triangle (mesh lights): v1, the edges from it (fp32 differences) and the GEOMETRIC unit normal
            for (int c3 = 0; c3 < 3; ++c3) {
                g[c3] = p.m[c3], g[4 + c3] = p.m[3 + c3] - p.m[c3], g[8 + c3] = p.m[6 + c3] - p.m[c3];
                g[12 + c3] = p.m[9 + c3];
            }
        }
    }
    // alias table (Vose): one uniform draw picks bucket i = floor(u n), then i itself below the threshold, else its alias
    std::vector<double> w(lights.size());
    std::vector<int> small, large;
    for (size_t i = 0; i < lights.size(); ++i) {
        w[i] = lights[i].prob * (double)L.nl;
        (w[i] < 1.0 ? small : large).push_back((int)i);
    }
    std::vector<float> thr(lights.size(), 1.0f);
    std::vector<int> alias(lights.size());
    for (size_t i = 0; i < lights.size(); ++i) alias[i] = (int)i;
    while (!small.empty() && !large.empty()) {
        const int a = small.back(), b = large.back();
        small.pop_back();
        thr[(size_t)a] = (float)w[(size_t)a], alias[(size_t)a] = b;
        w[(size_t)b] -= 1.0 - w[(size_t)a];
        if (w[(size_t)b] < 1.0) large.pop_back(), small.push_back(b);
    }
    for (int i = 0; i < L.nl; ++i) {
        float *a = rec4(I, L.off_alias + i);
        a[0] = thr[(size_t)i], a[1] = bits(alias[(size_t)i]);
    }
}

// the media's records, and in the camera block how many there are and where (rt_media.h)
void write_media(float *I, const RenderParams &L, const Scene &s, int off_media) {
    const int32_t n = (int32_t)s.media.size(), off = off_media;
    memcpy(rec4(I, L.off_cam + 1) + 3, &n, 4);
    memcpy(rec4(I, L.off_cam + 2) + 3, &off, 4);
    for (int i = 0; i < n; ++i) {
        const rt_medium &m = s.media[(size_t)i];
        float *r0 = rec4(I, off_media + RT_MEDIUM_STRIDE * i), *r1 = r0 + 4, *r2 = r0 + 8;
        for (int k = 0; k < 4; ++k) r0[k] = m.f[k];
        for (int c = 0; c < 3; ++c) r1[c] = m.albedo[c];
        r1[3] = m.density;
        r2[0] = m.f[4], r2[1] = m.f[5];
        memcpy(r2 + 2, &m.shape, 4);
        r2[3] = s.media_g[(size_t)i];  // (0: the isotropic medium, the word this place always held)
    }
}

// the moving spheres' records, and in the camera block how many there are and where (rt_motion.h).  After write_materials:
// a record carries its material's kind, as the primitives' cold records do.
void write_motion(float *I, const RenderParams &L, const Scene &s, int off_motion) {
    const int32_t n = (int32_t)s.movers.size(), off = off_motion;
    memcpy(rec4(I, L.off_cam + 3) + 3, &n, 4);
    memcpy(rec4(I, L.off_cam + 4) + 3, &off, 4);
    for (int i = 0; i < n; ++i) {
        const rt_moving_sphere &m = s.movers[(size_t)i];
        float *r0 = rec4(I, off_motion + RT_MOTION_STRIDE * i), *r1 = r0 + 4, *r2 = r0 + 8;
        for (int k = 0; k < 3; ++k) r0[k] = m.center0[k], r1[k] = m.center1[k] - m.center0[k];  // v, once, in fp32
        r0[3] = m.radius;
        r1[3] = 1.0f / m.radius;  // (p - c) / r  ==  (1/r) * (p - c), as for the static spheres
        r2[0] = bits(m.material);
        r2[1] = I[(size_t)(L.off_mat + 3 * m.material) * 4];  // the material's kind (bits)
        r2[2] = r2[3] = 0.0f;
    }
}

// the triangles' vertex normals in the order of the triangle tables, and in the camera block where they lie (device_scene.h)
void write_normals(float *I, const RenderParams &L, const Scene &s, const OtherPrims &O, int off_normals) {
    const int32_t off = off_normals;
    memcpy(rec4(I, L.off_cam + 5) + 3, &off, 4);
    for (int k = 0; k < L.nt; ++k) {
        const rt_prim &p = s.prims[O.tri[k]];
        float *r = rec4(I, off_normals + 3 * k);
        const float *n[3] = {p.f, p.f + 3, p.m_inv + 6};
        for (int c = 0; c < 3; ++c) r[4 * c] = n[c][0], r[4 * c + 1] = n[c][1], r[4 * c + 2] = n[c][2];
        r[3] = bits(tri_has_normals(p) ? 1 : 0);  // (a flat triangle's records are zeros)
    }
}

// the environment's texels and sampling tables, as the host evaluation reads them
void write_environment(float *I, const RenderParams &L, const Scene &s) {
    const SceneEnvironment &e = *s.env;
    memcpy(I + L.off_env_tex, e.rgb.data(), e.rgb.size() * sizeof(float));
    memcpy(I + L.off_env_marg, e.marg.data(), e.marg.size() * sizeof(float));
    memcpy(I + L.off_env_cond, e.cond.data(), e.cond.size() * sizeof(float));
    memcpy(I + L.off_env_band, e.band.data(), e.band.size() * sizeof(float));
    memcpy(I + L.off_env_ct, e.ct.data(), e.ct.size() * sizeof(float));
}

// what a round tells pack_scene beside the image
struct PackNote {
    bool too_large = false;  // the environment's tables end beyond an int32 word offset
    bool too_many_slots = false;  // RT_MAX_SPHERE_SLOTS sphere slots or more (lay_out_image)
    bool demoted = false;  // (this or an earlier round) the members of an overflowing cell were forced
    size_t longest = 0;    // the longest list (near + far + others) of a cell a walk can meet
    NestedInfo nested;
};

// ---- one round ---------------------------------------------------------------------------------
// forced: primitives that must be tested for every query whatever their size (members of a cell whose list overflowed in an
// earlier round).  False, with more primitives added to `forced`, when the grid could not list them.
bool pack_round(const Scene &s, std::vector<char> &forced, std::vector<float> &image, RenderParams &L, size_t nest_over, int nest_cap,
                PackNote &note) {
    std::vector<int> sph, rec, cyl, tri, quad;
    for (size_t i = 0; i < s.prims.size(); ++i) {
        switch (s.prims[i].type) {
        case RT_PRIM_SPHERE: sph.push_back((int)i); break;
        case RT_PRIM_CYLINDER: cyl.push_back((int)i); break;
        case RT_PRIM_TRIANGLE: tri.push_back((int)i); break;
        case RT_PRIM_QUAD: quad.push_back((int)i); break;
        default: rec.push_back((int)i); break;
        }
    }
    // (a glossy material, DESIGN 7m, a noise texture, 7o, and a bump, 7p, run in the general kernels alone, as an image texture does;
    // a normal map, 7u, is an image texture)
    const bool sphere_only = rec.empty() && cyl.empty() && tri.empty() && quad.empty() && s.images.empty() && !scene_has_glossy(s) && !scene_has_noise(s) && !scene_has_bump(s);
    const SphereSlots S = sphere_slots(s, std::move(sph), forced);
    const OtherPrims O = other_prims(s, S, std::move(rec), std::move(cyl), std::move(tri), std::move(quad), forced);
    // light sampling runs in the general kernels alone (render_nee_kernel: the linear scan and the wide-table walks), so a
    // sphere-only scene that has lights to sample gets the wide tables; with nothing to sample the image stays as it was
    const std::vector<SceneLight> lights = s.light_sampling ? scene_lights(s) : std::vector<SceneLight>();

    memset(&L, 0, sizeof L);
    L.ns = S.ns(), L.feature = 0, L.np = S.np, L.ncl = S.n_clusters, L.cluster = RT_CLUSTER;
    L.nr = (int)O.rec.size(), L.nc = (int)O.cyl.size(), L.nt = (int)O.tri.size(), L.nm = (int)s.mats.size();
    L.nr_a = O.nr_a, L.nc_a = O.nc_a, L.nt_a = O.nt_a;
    L.nq = (int)O.quad.size(), L.nq_a = O.nq_a;
    L.ngr = (S.n_clusters + RT_GROUP - 1) / RT_GROUP;        // RT_GROUP consecutive clusters share an outer box
    L.nwin = (L.ngr + 64 / RT_GROUP - 1) / (64 / RT_GROUP);  // 64 clusters per window
    L.rt_axes = S.axes;
    L.nl = (int)lights.size();

    Grid g;
    // (an environment, media and moving spheres, like light sampling, run in general kernels of their own: wide tables)
    const bool wide = !sphere_only || S.ns() >= 65536 || !lights.empty() || s.env || !s.media.empty() || !s.movers.empty() || nest_over > 0 || knob_set("RTMI_FORCE_WIDE")  // (the knob: measurement)
                      || s.cam.projection != RT_PROJ_PERSPECTIVE;  // (a projection, DESIGN 7w: the instances of camera_kernel.h are general builds)
    const bool built = build_grid(s, S, O, L, wide, forced, g, nest_over, nest_cap);
    note.demoted = note.demoted || g.demoted;
    if (!built) return false;
    note.longest = g.longest;
    const bool nested = !g.subs.empty();
    L.grid_cells = nested ? g.n[0] * g.n[1] * g.n[2] : (int)(g.cells.size() / (g.wide ? 2 : 1));
    L.grid_wide = g.wide ? (nested ? 2 : 1) : 0;
    L.grid_sheet = (!g.cells.empty() && g.n[1] == 1 && !g.wide) ? 1 : 0;
    std::vector<int> image_word;
    std::vector<int> noise_rec, bump_rec;
    int off_media = 0, off_motion = 0, off_normals = 0, off_noise = 0, off_bump = 0, off_nmap = 0, off_pbr = 0;
    const int records = lay_out_image(L, g, s, image_word, off_media, off_motion, off_normals, off_noise, off_bump, off_nmap, off_pbr);
    if (records < 0) {
        (records == -2 ? note.too_many_slots : note.too_large) = true;
        return true;
    }
    if (s.env) {
        L.env_scale = s.env_scale, L.env_uoff = env_uoff(s.env_rotate);
        if (!lights.empty() && lights.back().type == RT_LIGHT_ENVIRONMENT) L.env_sel = (float)lights.back().prob;
    }

    image.assign((size_t)(records > 0 ? records : 1) * 4, 0.0f);
    float *I = image.data();
    const float extent = box_extent(s, S, O);
    L.cull_extent1 = extent + 1.0f;
    const float inflate = 1e-5f * (extent + 1.0f);
    write_camera(I, L, s);
    write_spheres(I, L, s, S);
    write_cluster_boxes(I, L, s, S, inflate);
    write_range_tables(I, L);
    write_grid(I, L, g);
    write_others(I, L, s, O, g, inflate);
    write_texels(I, s, image_word);
    write_noise(I, s, off_noise, noise_rec);
    write_bumps(I, s, off_bump, noise_rec, bump_rec);
    write_normal_maps(I, s, off_nmap, image_word, bump_rec);
    if (scene_has_alpha(s)) write_alphas(I, s, L.off_mat + 3 * L.nm, image_word);
    write_materials(I, L, s, S, O, image_word, noise_rec, bump_rec, off_pbr);
    if (L.nl > 0) write_lights(I, L, s, S, O, lights);
    if (s.env) write_environment(I, L, s);
    if (!s.media.empty()) write_media(I, L, s, off_media);
    if (!s.movers.empty()) write_motion(I, L, s, off_motion);
    if (off_normals) write_normals(I, L, s, O, off_normals);
    note.nested = NestedInfo();
    if (nested) {
        note.nested.cells = (int)(g.subs.size() / 16);
        note.nested.sub_cells = (int)(g.cells.size() / 2) - g.top_cells;
        note.nested.sub_items = (long long)g.sub_items;
        note.nested.off_sub_grids = __builtin_bit_cast(int32_t, rec4(I, L.off_grid)[15]);
        note.nested.off_sub_cells = L.off_grid_cells + g.top_cells / 2;  // (two cells per record; top_cells is even here)
        note.nested.first_sub_cell = g.top_cells;
        note.nested.threshold = (int)nest_over, note.nested.axis_cap = nest_cap;
        note.nested.longest = (int)g.longest;
    }
    return true;
}

}  // namespace

int pack_scene(const Scene &s, std::vector<float> &image, RenderParams &layout, NestedInfo *nested_out) {
    // a cell's list that overflows even the wide tables (more than a thousand primitives through one cell: a clump) moves its
    // members to the always-tested set and the tables are rebuilt: in the limit the scene is scanned, which is the reference's
    // algorithm.  Every round removes at least one primitive from the lists, and real scenes need none.
    std::vector<char> forced(s.prims.size(), 0);
    PackNote note;
    if (nested_out) *nested_out = NestedInfo();
    bool packed = false;
    for (size_t round = 0; round <= s.prims.size() && !packed; ++round) packed = pack_round(s, forced, image, layout, 0, 0, note);
    if (note.too_large) {
        set_error("the environment map's tables end beyond the int32 word offsets of the scene image");
        return RT_ERR_LIMIT;
    }
    if (note.too_many_slots) {
        set_error("the scene's spheres take %lld slots or more, beyond the 32-bit byte offsets of their cold records", RT_MAX_SPHERE_SLOTS);
        return RT_ERR_LIMIT;
    }
    // The nested grid (rt_scene_set_nested_grid): only a scene whose flat tables have a cell longer than the threshold, or lost
    // primitives to the always-tested set through an overflowing cell, is packed again -- wide, from a clean slate, with such
    // cells nested.  If that packing nests nothing (every clump was a clump in its sub-grid too), the flat tables stand.
    if (packed && s.nested_grid) {
        // Threshold and cap: an evenly spread mesh gives the flat grid lists of 17.8 entries on average, 32 at most, and the walk
        // is tuned to those; twice the longest keeps every such scene flat.  Sweep in DESIGN 7c.
        const size_t nest_over = (size_t)std::max(1.0, knob("RTMI_NEST_OVER", 64.0));
        const int nest_cap = (int)std::min(1023.0, std::max(1.0, knob("RTMI_NEST_CAP", 32.0)));
        if (note.demoted || note.longest > nest_over) {
            std::vector<char> forced2(s.prims.size(), 0);
            std::vector<float> image2;
            RenderParams layout2;
            PackNote note2;
            bool packed2 = false;
            for (size_t round = 0; round <= s.prims.size() && !packed2; ++round)
                packed2 = pack_round(s, forced2, image2, layout2, nest_over, nest_cap, note2);
            if (packed2 && !note2.too_large && !note2.too_many_slots && note2.nested.cells > 0) {
                image = std::move(image2), layout = layout2;
                if (nested_out) *nested_out = note2.nested;
            }
        }
    }
    if (packed) return RT_OK;
    set_error("packing the scene tables: %zu rounds left primitives unlisted", s.prims.size() + 1);
    return RT_ERR_LIMIT;
}

}  // namespace rtmi
