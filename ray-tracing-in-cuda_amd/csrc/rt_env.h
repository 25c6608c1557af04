// The environment map: the lookup of a direction and the sampler, shared by the kernels (render_env.hip) and the
// host evaluations (rt_environment_eval / rt_environment_sample), like rt_trig.h, which both go through.  Every step of the
// lookup is one fp32 operation in a fixed order, so the host restates the device's texel index bit for bit.
//
// Tables (fp32 words of the scene image; built on the host in fp64, stored as fp32 -- scene.cpp):
//   tex    rows x cols x 3   the texels, row 0 = the zenith (+y)
//   marg   rows + 1          marginal CDF over rows: marg[0] = 0, marg[rows] = 1
//   cond   rows x (cols + 1) per row: conditional CDF over its columns, cond[0] = 0, cond[cols] = 1 (all zero in a black row)
//   band   rows              per row: the solid angle of one of its texels, (2 pi / cols)(cos theta_i - cos theta_i+1)
//   ct     rows + 1          cos(theta) at the row borders: 1 ... -1
// A texel whose stored CDF steps are zero is never chosen and has pdf 0.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rt_trig.h"

namespace rtmi {

struct EnvView {
    const float *tex, *marg, *cond, *band, *ct;
    int rows, cols;
    float scale, uoff;  // radiance = scale x texel; uoff = rotate / 360 in [0, 1), added to u
};

// the texel of a UNIT direction: v = acos(d.y) / pi, u = frac((atan2(-d.z, d.x) + pi) / 2 pi + uoff), nearest texel
RTMI_HD void env_texel(const EnvView &E, float dx, float dy, float dz, int &row, int &col) {
    const float v = rt_acosf(dy) / 3.1415927410125732421875f;
    row = (int)(v * (float)E.rows);
    row = row < E.rows - 1 ? row : E.rows - 1;
    row = row > 0 ? row : 0;
    float u = (rt_atan2f(-dz, dx) + 3.1415927410125732421875f) / 6.283185482025146484375f;
    u = u + E.uoff;
    u = u - floorf(u);
    col = (int)(u * (float)E.cols);
    col = col < E.cols - 1 ? col : E.cols - 1;
    col = col > 0 ? col : 0;
}

// solid-angle density with which the sampler draws directions inside texel (row, col), from the tables its search reads
RTMI_HD float env_texel_pdf(const EnvView &E, int row, int col) {
    const float pm = E.marg[row + 1] - E.marg[row];
    const float *c = E.cond + (size_t)row * (size_t)(E.cols + 1);
    const float pc = c[col + 1] - c[col];
    return (pm * pc) / E.band[row];
}

// THE lookup: radiance and sampling density of a unit direction (both MIS strategies evaluate a direction through it)
RTMI_HD void env_eval(const EnvView &E, float dx, float dy, float dz, float &r, float &g, float &b, float &pdf) {
    int row, col;
    env_texel(E, dx, dy, dz, row, col);
    const float *t = E.tex + 3 * ((size_t)row * (size_t)E.cols + (size_t)col);
    r = E.scale * t[0], g = E.scale * t[1], b = E.scale * t[2];
    pdf = env_texel_pdf(E, row, col);
}

// the last index i in [0, n) with cdf[i] <= u (cdf[0] = 0 <= u < 1 = cdf[n]): never an empty step
RTMI_HD int env_search(const float *cdf, int n, float u) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] <= u) lo = mid;
        else hi = mid;
    }
    return lo;
}

// One direction from two uniform draws: u1 picks the row (marginal CDF) and, by what is left of it, cos(theta) uniform over the
// row's band; u2 picks the column (the row's conditional CDF) and, by what is left of it, phi uniform over the texel.  The
// caller evaluates the direction through env_eval: one that rounds into a neighbouring texel gets that texel's values.
RTMI_HD void env_sample(const EnvView &E, float u1, float u2, float &dx, float &dy, float &dz) {
    const int row = env_search(E.marg, E.rows, u1);
    const float m0 = E.marg[row], m1 = E.marg[row + 1];
    const float a1 = m1 > m0 ? (u1 - m0) / (m1 - m0) : 0.5f;
    const float *c = E.cond + (size_t)row * (size_t)(E.cols + 1);
    const int col = env_search(c, E.cols, u2);
    const float c0 = c[col], c1 = c[col + 1];
    const float a2 = c1 > c0 ? (u2 - c0) / (c1 - c0) : 0.5f;
    const float ct0 = E.ct[row], ct1 = E.ct[row + 1];
    const float cth = fmaf(a1, ct1 - ct0, ct0);
    const float sth = sqrtf(fmaxf(0.0f, fmaf(-cth, cth, 1.0f)));
    float u = ((float)col + a2) / (float)E.cols - E.uoff;  // the lookup adds uoff
    u = u - floorf(u);
    const float phi = fmaf(6.283185482025146484375f, u, -3.1415927410125732421875f);  // = atan2(-d.z, d.x)
    const float sp = sinf(phi), cp = cosf(phi);
    dx = sth * cp, dy = cth, dz = -(sth * sp);
}

}  // namespace rtmi
