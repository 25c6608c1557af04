// What csrc/rt_quad.h returns, on the host (test_quads.py builds this with the host compiler and -ffp-contract=off and holds it
// against the fp64 statement of the quad in include/rtmi.h).  The kernels compile the same text.
//
// usage: quad_host_driver IN OUT.  IN: fp32 records of 26 words
//   Q.xyz  u.xyz  v.xyz  n.xyz  A.xyz  B.xyz  (the rt_prim record's words)   o.xyz  d.xyz  (a ray, d any length)   u1  u2
// OUT: fp32 records of 16 words
//   hit (0 / 1)  t  a  b  p.xyz  normal.xyz (n turned against the ray)  front (0 / 1)        -- zeros after `hit` on a miss
//   y.xyz (the light point of u1, u2)  the light's density of y - o for selection / area = 1
#include <cmath>
#include <cstdio>
#include <vector>

#include "../ray-tracing-in-cuda_amd/csrc/rt_quad.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<float> in;
    float rec[26];
    while (fread(rec, sizeof rec, 1, f) == 1) in.insert(in.end(), rec, rec + 26);
    fclose(f);
    const size_t n = in.size() / 26;
    std::vector<float> out(n * 16, 0.0f);
    for (size_t i = 0; i < n; ++i) {
        const float *r = &in[i * 26];
        const float *Q = r, *u = r + 3, *v = r + 6, *nn = r + 9, *A = r + 12, *B = r + 15, *o = r + 18, *d = r + 21;
        float *w = &out[i * 16];
        float t = 0, a = 0, b = 0;
        const bool hit = rtmi::quad_hit(Q[0], Q[1], Q[2], nn[0], nn[1], nn[2], A[0], A[1], A[2], B[0], B[1], B[2], o[0], o[1], o[2], d[0], d[1],
                                        d[2], 0.001f, INFINITY, t, a, b);
        w[0] = hit ? 1.0f : 0.0f;
        if (hit) {
            const float px = fmaf(t, d[0], o[0]), py = fmaf(t, d[1], o[1]), pz = fmaf(t, d[2], o[2]);
            // (the winner's (u, v): from the hit point again, as the kernels' winner section takes them)
            rtmi::quad_uv(Q[0], Q[1], Q[2], A[0], A[1], A[2], B[0], B[1], B[2], px, py, pz, a, b);
            const bool front = rtmi::quad_dot(d[0], d[1], d[2], nn[0], nn[1], nn[2]) < 0.0f;
            w[1] = t, w[2] = a, w[3] = b, w[4] = px, w[5] = py, w[6] = pz;
            w[7] = front ? nn[0] : -nn[0], w[8] = front ? nn[1] : -nn[1], w[9] = front ? nn[2] : -nn[2];
            w[10] = front ? 1.0f : 0.0f;
        }
        rtmi::quad_light_point(Q[0], Q[1], Q[2], u[0], u[1], u[2], v[0], v[1], v[2], r[24], r[25], w[11], w[12], w[13]);
        w[14] = rtmi::quad_light_pdf(1.0f, nn[0], nn[1], nn[2], w[11] - o[0], w[12] - o[1], w[13] - o[2]);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 4;
    fwrite(out.data(), sizeof(float), out.size(), f);
    fclose(f);
    return 0;
}
