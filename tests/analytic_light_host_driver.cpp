// What csrc/rt_lights.h returns, on the host (test_analytic_lights.py builds this with the host compiler and -ffp-contract=off and
// holds it against the fp64 statement of the lights in include/rtmi.h).  The kernels compile the same text.
//
// usage: analytic_light_host_driver IN OUT.  IN: fp32 records of 16 words
//   type (101 point, 102 spot, 103 distant)  p.xyz (the vertex)  u1  u2
//   x.xyz (point, spot: the position; distant: the unit direction t towards the light)  a.xyz (spot: the unit axis)
//   cos_o  inv (spot)   omc = 1 - cos alpha   D (distant)
// OUT: fp32 records of 8 words
//   ld.xyz   1 / pl for selection probability 1 (the scalar part of the sample's weight; 0: no sample)   falloff (1 unless a spot)
//   0  0  0
#include <cmath>
#include <cstdio>
#include <vector>

#include "../ray-tracing-in-cuda_amd/csrc/rt_lights.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<float> in;
    float rec[16];
    while (fread(rec, sizeof rec, 1, f) == 1) in.insert(in.end(), rec, rec + 16);
    fclose(f);
    const size_t n = in.size() / 16;
    std::vector<float> out(n * 8, 0.0f);
    for (size_t i = 0; i < n; ++i) {
        const float *r = &in[i * 16];
        const float *p = r + 1, *x = r + 6, *a = r + 9;
        float *w = &out[i * 8];
        const int type = (int)r[0];
        float pl = 0.0f;
        w[4] = 1.0f;
        if (type == 103) {
            float ex, ey, ez, cth, sth;
            rtmi::light_cone_direction(x[0], x[1], x[2], r[14], r[4], r[5], ex, ey, ez, cth, sth);
            w[0] = r[15] * ex, w[1] = r[15] * ey, w[2] = r[15] * ez;
            pl = 1.0f;
        } else {
            w[0] = x[0] - p[0], w[1] = x[1] - p[1], w[2] = x[2] - p[2];
            const float d2 = rtmi::light_dot(w[0], w[1], w[2], w[0], w[1], w[2]);
            pl = rtmi::point_light_density(1.0f, d2);
            if (type == 102) {
                w[4] = rtmi::spot_falloff(a[0], a[1], a[2], w[0], w[1], w[2], d2, r[12], r[13]);
                pl = rtmi::spot_light_density(1.0f, d2, w[4]);
            }
        }
        w[3] = pl > 0.0f ? 1.0f / pl : 0.0f;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 4;
    fwrite(out.data(), sizeof(float), out.size(), f);
    fclose(f);
    return 0;
}
