// What csrc/rt_pbr.h returns, on the host (test_pbr.py builds this with the host compiler and -ffp-contract=off and holds it
// against the numpy statement of tests/ref64_pbr.py).  The kernels compile the same text.
//
// usage: pbr_host_driver IN OUT.  IN: fp32 records of 8 words
//   base colour.rgb  G  B  rf  mf  ul          (G, B: the map's channels at the hit; rf, mf: the factors)
// OUT: fp32 records of 8 words
//   c8.rgb  r8  m8  metal (1: the vertex chose the rough-metal lobe)  ul'  alpha
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../ray-tracing-in-cuda_amd/csrc/rt_pbr.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<float> in;
    float rec[8];
    while (fread(rec, sizeof rec, 1, f) == 1) in.insert(in.end(), rec, rec + 8);
    fclose(f);
    const size_t n = in.size() / 8;
    std::vector<float> out(n * 8, 0.0f);
    for (size_t i = 0; i < n; ++i) {
        const float *r = &in[i * 8];
        float *o = &out[i * 8];
        uint32_t m8 = 0;
        const uint32_t c8 = rtmi::pbr_params(r[0], r[1], r[2], r[3], r[4], r[5], r[6], m8);
        o[0] = (float)(c8 & 255u), o[1] = (float)((c8 >> 8) & 255u), o[2] = (float)((c8 >> 16) & 255u), o[3] = (float)(c8 >> 24), o[4] = (float)m8;
        float ulp = 0.0f;
        o[5] = rtmi::pbr_choose(m8, r[7], ulp) ? 1.0f : 0.0f;
        o[6] = ulp;
        o[7] = rtmi::pbr_alpha(rtmi::pbr_unit(c8 >> 24));
    }
    f = fopen(argv[2], "wb");
    if (!f) return 4;
    const bool wrote = fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
    return fclose(f) == 0 && wrote ? 0 : 5;
}
