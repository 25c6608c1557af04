// What csrc/rt_glossy.h returns, on the host (test_glossy.py builds this with the host compiler and -ffp-contract=off and holds
// it against the numpy statement of tests/ref64_glossy.py).  The kernels compile the same text.
//
// usage: glossy_host_driver IN OUT.  IN: fp32 records of 20 words
//   n.xyz  d.xyz  alpha  F0.rgb  r0  rho.rgb  ul  u1  u2  wl.xyz        (n and wl unit vectors, d any length)
// OUT: fp32 records of 26 words, rough metal then plastic, each
//   state (0 scattered, 1 absorbed: wo.z <= 0, 2 absorbed: wi.z <= 0)  wi.xyz  attenuation.rgb  pdf_b  fcos(wl).rgb  pdf_b(wl)
// and for plastic one more word: 1 where the microfacet lobe was drawn.  (Rows of an absorbed vertex hold zeros.)
#include <cmath>
#include <cstdio>
#include <vector>

#include "../ray-tracing-in-cuda_amd/csrc/rt_glossy.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<float> in;
    float rec[20];
    while (fread(rec, sizeof rec, 1, f) == 1) in.insert(in.end(), rec, rec + 20);
    fclose(f);
    const size_t n = in.size() / 20;
    std::vector<float> out(n * 26, 0.0f);
    for (size_t i = 0; i < n; ++i) {
        const float *r = &in[i * 20];
        float *o = &out[i * 26];
        const float il = 1.0f / sqrtf(fmaf(r[3], r[3], fmaf(r[4], r[4], r[5] * r[5])));
        const float ux = il * r[3], uy = il * r[4], uz = il * r[5];
        const float alpha = r[6], r0 = r[10], ul = r[14], u1 = r[15], u2 = r[16];
        bool below = false, lobe = false;
        float wx = 0, wy = 0, wz = 0, ar = 0, ag = 0, ab = 0, pdf = 0;
        bool ok = rtmi::glossy_sample(false, r[0], r[1], r[2], ux, uy, uz, alpha, r[7], r[8], r[9], 0.0f, 0.0f, 0.0f, 0.0f, u1, u2, wx, wy, wz, ar, ag, ab,
                                      pdf, below, lobe);
        o[0] = ok ? 0.0f : (below ? 1.0f : 2.0f);
        if (ok) o[1] = wx, o[2] = wy, o[3] = wz, o[4] = ar, o[5] = ag, o[6] = ab, o[7] = pdf;
        rtmi::glossy_eval(false, r[0], r[1], r[2], ux, uy, uz, alpha, r[7], r[8], r[9], 0.0f, 0.0f, 0.0f, r[17], r[18], r[19], o[8], o[9], o[10], o[11]);
        o += 12;
        ok = rtmi::glossy_sample(true, r[0], r[1], r[2], ux, uy, uz, alpha, r0, r0, r0, r[11], r[12], r[13], ul, u1, u2, wx, wy, wz, ar, ag, ab, pdf,
                                 below, lobe);
        o[0] = ok ? 0.0f : (below ? 1.0f : 2.0f);
        if (ok) o[1] = wx, o[2] = wy, o[3] = wz, o[4] = ar, o[5] = ag, o[6] = ab, o[7] = pdf;
        rtmi::glossy_eval(true, r[0], r[1], r[2], ux, uy, uz, alpha, r0, r0, r0, r[11], r[12], r[13], r[17], r[18], r[19], o[8], o[9], o[10], o[11]);
        o[12] = lobe ? 1.0f : 0.0f;
        o[13] = 0.0f;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 4;
    const bool wrote = fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
    return fclose(f) == 0 && wrote ? 0 : 5;
}
