// What csrc/rt_noise.h returns for bump mapping, on the host: the gradient of a noise texture's scalar and the
// bumped normal (test_bump.py builds this with the host compiler and -ffp-contract=off and holds it against the numpy statement
// of tests/ref64_bump.py).  The kernels compile the same text, with their own square root.
//
// usage: bump_host_driver IN OUT.  IN: records of 16 32-bit words
//   p.xyz (fp32)  scale (fp32)  distortion (fp32)  seed (uint32)  style | axis << 2 | octaves << 4 (uint32)  k (fp32)
//   n.xyz (fp32, unit: shading and geometric normal alike)  d.xyz (fp32, the ray's direction)  front (uint32: 0 or 1)  0
// OUT: fp32 records of 8 words
//   grad s (3)   n' where the rule accepts it, else n (3)   accepted (uint32)   0
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
    uint32_t rec[16];
    while (fread(rec, sizeof rec, 1, f) == 1) in.insert(in.end(), rec, rec + 16);
    fclose(f);
    const size_t n = in.size() / 16;
    std::vector<uint32_t> out(n * 8, 0u);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t *r = &in[i * 16];
        float p[5], k, v[6];
        memcpy(p, r, sizeof p);
        memcpy(&k, r + 7, 4);
        memcpy(v, r + 8, sizeof v);
        const uint32_t seed = r[5], packed = r[6];
        float G[3];
        rtmi::noise_gradient((int)(packed & 3u), p[3], (int)(packed >> 4) & 15, seed, (int)(packed >> 2) & 3, p[4], p[0], p[1], p[2], G[0], G[1], G[2]);
        float nb[3] = {v[0], v[1], v[2]};
        const bool ok = rtmi::noise_bump(nb[0], nb[1], nb[2], v[0], v[1], v[2], v[3], v[4], v[5], r[14] ? k : -k, G[0], G[1], G[2],
                                         [](float x) { return sqrtf(x); });
        memcpy(&out[i * 8], G, sizeof G);
        memcpy(&out[i * 8 + 3], nb, sizeof nb);
        out[i * 8 + 6] = ok ? 1u : 0u;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 4;
    const bool wrote = fwrite(out.data(), sizeof(uint32_t), out.size(), f) == out.size();
    return fclose(f) == 0 && wrote ? 0 : 5;
}
