// What csrc/rt_glass.h returns, on the host (test_glass.py builds this with the host compiler and -ffp-contract=off and holds
// it against the numpy statement of tests/ref64_glass.py).  The kernels compile the same text.
//
// usage: glass_host_driver IN OUT.  IN: fp32 records of 20 words
//   n.xyz  d.xyz  alpha  ir  front  sigma.rgb  dist  uf  u1  u2  wl.xyz  _      (n and wl unit vectors, d any length)
// OUT: fp32 records of 16 words
//   branch (0 reflected, 1 refracted, 2 absorbed: wo.z <= 0, 3 absorbed: wi on the wrong side)  wi.xyz  attenuation.rgb  pdf_b
//   fcos(wl).rgb  pdf_b(wl)  Tr.rgb  F at normal incidence
// (Rows of an absorbed vertex hold zeros in wi, attenuation and pdf_b.)
#include <cmath>
#include <cstdio>
#include <vector>

#include "../ray-tracing-in-cuda_amd/csrc/rt_glass.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<float> in;
    float rec[20];
    while (fread(rec, sizeof rec, 1, f) == 1) in.insert(in.end(), rec, rec + 20);
    fclose(f);
    const size_t n = in.size() / 20;
    std::vector<float> out(n * 16, 0.0f);
    for (size_t i = 0; i < n; ++i) {
        const float *r = &in[i * 20];
        float *o = &out[i * 16];
        const float il = 1.0f / sqrtf(fmaf(r[3], r[3], fmaf(r[4], r[4], r[5] * r[5])));
        const float ux = il * r[3], uy = il * r[4], uz = il * r[5];
        const float alpha = r[6], ir = r[7];
        const bool front = r[8] != 0.0f;
        const float eta = front ? 1.0f / ir : ir;  // (the packer's two words)
        float tr[3] = {1.0f, 1.0f, 1.0f};
        if (!front)
            for (int k = 0; k < 3; ++k) tr[k] = rtmi::glass_tint(r[9 + k], r[12]);
        bool below = false, reflected = false;
        float wx = 0, wy = 0, wz = 0, ratio = 0, pdf = 0;
        const bool ok = rtmi::glass_sample(r[0], r[1], r[2], ux, uy, uz, alpha, eta, r[13], r[14], r[15], wx, wy, wz, ratio, pdf, below, reflected);
        o[0] = below ? 2.0f : (!ok ? 3.0f : (reflected ? 0.0f : 1.0f));
        if (ok) {
            o[1] = wx, o[2] = wy, o[3] = wz, o[7] = pdf;
            for (int k = 0; k < 3; ++k) o[4 + k] = tr[k] * ratio;
        }
        float fc = 0, pw = 0;
        rtmi::glass_eval(r[0], r[1], r[2], ux, uy, uz, alpha, eta, r[16], r[17], r[18], fc, pw);
        for (int k = 0; k < 3; ++k) o[8 + k] = tr[k] * fc, o[12 + k] = tr[k];
        o[11] = pw;
        float ct;
        o[15] = rtmi::glass_fresnel(eta, 1.0f, ct);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 4;
    const bool wrote = fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
    return fclose(f) == 0 && wrote ? 0 : 5;
}
