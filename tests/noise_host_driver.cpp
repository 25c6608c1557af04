// What csrc/rt_noise.h returns, on the host (test_noise.py builds this with the host compiler and -ffp-contract=off and holds it
// against the numpy statement of tests/ref64_noise.py; built once more with -fsanitize=undefined,address it is fed coordinates
// no scene should hold).  The kernels compile the same text.
//
// usage: noise_host_driver IN OUT.  IN: records of 8 32-bit words
//   p.xyz (fp32)  scale (fp32)  distortion (fp32)  seed (uint32)  style | axis << 2 | octaves << 4 (uint32)  0
// OUT: fp32 records of 4 words
//   n(p, seed) -- one evaluation at p itself, no scale --   s, the texture's scalar   the hash of (int) p.xyz as a float's bits   0
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ray-tracing-in-cuda_amd/csrc/rt_noise.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<uint32_t> in;
    uint32_t rec[8];
    while (fread(rec, sizeof rec, 1, f) == 1) in.insert(in.end(), rec, rec + 8);
    fclose(f);
    const size_t n = in.size() / 8;
    std::vector<uint32_t> out(n * 4, 0u);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t *r = &in[i * 8];
        float p[5];
        memcpy(p, r, sizeof p);
        const uint32_t seed = r[5], packed = r[6];
        const float one = rtmi::noise3(p[0], p[1], p[2], seed);
        const float s = rtmi::noise_value((int)(packed & 3u), p[3], (int)(packed >> 4) & 15, seed, (int)(packed >> 2) & 3, p[4], p[0], p[1], p[2]);
        int32_t c[3];
        for (int k = 0; k < 3; ++k) rtmi::noise_cell(p[k], c[k]);
        const uint32_t h = rtmi::noise_hash(c[0], c[1], c[2], seed);
        memcpy(&out[i * 4], &one, 4);
        memcpy(&out[i * 4 + 1], &s, 4);
        out[i * 4 + 2] = h;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 4;
    const bool wrote = fwrite(out.data(), sizeof(uint32_t), out.size(), f) == out.size();
    return fclose(f) == 0 && wrote ? 0 : 5;
}
