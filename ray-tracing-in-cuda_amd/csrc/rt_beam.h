// Tile beams: which staged sphere records can the camera rays of ONE 8x8 tile of the frame be flagged for by the
// fp32 sphere test (RT_CAND, render_device.h)?  Stated once, in fp64 with a fixed operation sequence (the build contracts
// nothing), for the kernel that builds the table (tile_beams.hip) and for the host evaluation (render_host.hip): both read
// the packed image -- the six camera records and the hot sphere table -- and give the same records bit for bit.
//
// The ray family of tile (tx, ty): every bx in [8 tx, 8 tx + 8), by in [8 ty, 8 ty + 8), every jitter in [0, 1) and every lens
// point of the disk of lens_radius (0 without RT_FLAG_DEFOCUS_BLUR).  A ray runs from L = org + off, |off| <= R, through
// F = ll + bu hor + bv ver; with A = org and D = Fc - org, Fc the focus-plane point of the tile's middle, and
// F = Fc + delta, |delta| <= rho (half the tile's diagonal on the focus plane),
//     L + t (F - L) = (A + t D) + (1 - t) off + t delta:      within |1 - t| R + t rho of the central ray at the same t.
// A sphere (c, r^2) can be flagged only if the ray passes within r' = sqrt(r^2 + K eps |oc|^2) of c at some t >= 0 (the
// packer's growth, pack.hip stage 3, K = 32, |oc| <= |A - c| + R; a flagged ray whose fp32 hb has the wrong sign has its
// origin inside that ball, t = 0).  The fp32 camera ray itself deviates from the exact one by at most m at the origin and
// m per unit of t (m = 64 eps x the 1-norms of the records, an order above the handful of roundings that form o and d).  So
//     reached  <=>  exists t >= 0:  |A + t D - c| <= r' + |1 - t| R + t rho + m (1 + t),
// the right-hand side linear on [0, 1] and on [1, inf): a quadratic's minimum over an interval, twice.  A superset costs
// time only; a sphere that is missing changes the image.
//
// A tile's record: kBeamRecordWords 16-bit words {count, id, id, ...}; the ids ascending, grouped ids as the walk leaves them
// in best_id (slots of the hot sphere table, prefix and clusters alike).  count = kBeamOverflow: more than kBeamCapacity
// spheres are reachable, and the burst runs the full query.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define RTMI_BEAM_HD __host__ __device__ inline
#else
#define RTMI_BEAM_HD inline
#endif

namespace rtmi {

constexpr int kBeamRecordWords = 16;                 // 32 bytes per tile
constexpr int kBeamCapacity = kBeamRecordWords - 1;  // ids a record holds
constexpr uint16_t kBeamOverflow = 0xffffu;

// what the lists of a frame depend on besides the hot sphere table: a launch value, and the key of the cached table
struct BeamFrame {
    int32_t off_cam;   // record offset of the camera block in the image
    int32_t nslots;    // slots of the hot sphere table: np + (RT_CLUSTER + 1) ncl
    int32_t width, height;
    float inv_wm1, inv_hm1;
    uint32_t defocus;  // RT_FLAG_DEFOCUS_BLUR set
};

struct Beam {
    double ax, ay, az, dx, dy, dz, dd;  // the central ray A + t D, |D|^2
    double lens, rho, m;
};

// the central ray of tile (tx, ty) and the beam's widths; image: the packed image as floats
RTMI_BEAM_HD Beam beam_of_tile(const float *image, const BeamFrame &f, int tx, int ty) {
    const float *cv = image + 4 * (size_t)f.off_cam;
    const double iw = (double)f.inv_wm1, ih = (double)f.inv_hm1;
    const double uc = (double)(8 * tx + 4) * iw, vc = (double)(8 * ty + 4) * ih;
    Beam b;
    b.ax = cv[0], b.ay = cv[1], b.az = cv[2];
    b.lens = f.defocus ? fabs((double)cv[3]) : 0.0;
    const double hx = cv[8], hy = cv[9], hz = cv[10], vx = cv[12], vy = cv[13], vz = cv[14];
    b.dx = ((double)cv[4] + uc * hx + vc * vx) - b.ax;
    b.dy = ((double)cv[5] + uc * hy + vc * vy) - b.ay;
    b.dz = ((double)cv[6] + uc * hz + vc * vz) - b.az;
    b.dd = b.dx * b.dx + b.dy * b.dy + b.dz * b.dz;
    // half the tile's diagonal on the focus plane: |4 iw hor +- 4 ih ver|, the larger one
    const double px = 4.0 * iw * hx, py = 4.0 * iw * hy, pz = 4.0 * iw * hz;
    const double qx = 4.0 * ih * vx, qy = 4.0 * ih * vy, qz = 4.0 * ih * vz;
    b.rho = sqrt((px * px + py * py + pz * pz) + (qx * qx + qy * qy + qz * qz) + 2.0 * fabs(px * qx + py * qy + pz * qz));
    double n1 = b.lens;
    for (int i = 0; i < 16; ++i)
        if ((i & 3) != 3) n1 += fabs((double)cv[i]);
    b.m = 64.0 * 5.9604644775390625e-08 * n1;
    return b;
}

// min over [lo, hi] (hi < 0: [lo, inf)) of a t^2 + 2 b t + c  <=  0 ?
RTMI_BEAM_HD bool beam_quad_reaches(double a, double b, double c, double lo, double hi) {
    if ((a * lo + 2.0 * b) * lo + c <= 0.0) return true;
    if (hi >= 0.0 && (a * hi + 2.0 * b) * hi + c <= 0.0) return true;
    if (a > 0.0) {
        const double tv = -b / a;
        return tv > lo && (hi < 0.0 || tv < hi) && (a * tv + 2.0 * b) * tv + c <= 0.0;
    }
    return hi < 0.0;  // (the beam widens faster than it advances: everything ahead is inside it)
}

// can a camera ray of the beam be flagged for the sphere (c, r2)?  r2: the record's fourth word (r^2 in fp32; a never-hit
// slot's -inf is the caller's to skip)
RTMI_BEAM_HD bool beam_reaches(const Beam &b, double cx, double cy, double cz, double r2) {
    const double wx = b.ax - cx, wy = b.ay - cy, wz = b.az - cz;
    const double ww = wx * wx + wy * wy + wz * wz, wd = wx * b.dx + wy * b.dy + wz * b.dz;
    const double reach = sqrt(ww) + b.lens;
    const double rp = sqrt(r2 + (32.0 * 5.9604644775390625e-08) * (reach * reach));
    {  // t in [0, 1]: r' + (1 - t) R + t rho + m (1 + t)
        const double al = rp + b.lens + b.m, be = b.rho - b.lens + b.m;
        if (beam_quad_reaches(b.dd - be * be, wd - al * be, ww - al * al, 0.0, 1.0)) return true;
    }
    {  // t >= 1: r' + (t - 1) R + t rho + m (1 + t)
        const double al = rp - b.lens + b.m, be = b.rho + b.lens + b.m;
        if (beam_quad_reaches(b.dd - be * be, wd - al * be, ww - al * al, 1.0, -1.0)) return true;
    }
    return false;
}

// the record of tile (tx, ty)
RTMI_BEAM_HD void beam_tile_record(const float *image, const BeamFrame &f, int tx, int ty, uint16_t *rec) {
    const Beam b = beam_of_tile(image, f, tx, ty);
    int n = 0;
    for (int k = 1; k < kBeamRecordWords; ++k) rec[k] = 0;
    for (int i = 0; i < f.nslots; ++i) {
        const float *s = image + 4 * (size_t)i;
        if (!(s[3] >= 0.0f)) continue;  // a never-hit slot (r^2 = -inf)
        if (!beam_reaches(b, (double)s[0], (double)s[1], (double)s[2], (double)s[3])) continue;
        if (n < kBeamCapacity) rec[1 + n] = (uint16_t)i;
        ++n;
    }
    if (n > kBeamCapacity) {
        for (int k = 1; k < kBeamRecordWords; ++k) rec[k] = 0;
        rec[0] = kBeamOverflow;
    } else {
        rec[0] = (uint16_t)n;
    }
}

}  // namespace rtmi
