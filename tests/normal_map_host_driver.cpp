// What csrc/rt_tangent.h returns for a normal-mapped vertex, on the host: the decoded texel and the mapped normal
// from a raw tangent frame (test_normal_map.py builds this with the host compiler and -ffp-contract=off and holds it against the
// numpy statement of tests/ref64_normal_map.py).  The kernels compile the same text, with their own square root.
//
// usage: normal_map_host_driver IN OUT.  IN: records of 20 32-bit words
//   T.xyz (fp32)  B.xyz (fp32)  texel r8 | g8 << 8 | b8 << 16 (uint32)  s (fp32)
//   g.xyz (fp32: the face-turned geometric normal)  n.xyz (fp32: the face-turned shading normal)  d.xyz (fp32, the ray's direction)
//   front (uint32: 0 or 1)  0  0
// OUT: fp32 records of 4 words
//   n' where the rule accepts it, else n (3)   replaced (uint32)
//
// usage: normal_map_host_driver frames IN OUT: the raw tangents of the five primitive types, from what the kernel hands them.
// IN: records of 20 32-bit words, the shape (uint32) and then fp32 arguments in the functions' order:
//   0 sphere: o.xyz                       1 rectangle: axis (uint32: 0 xy, 1 xz, 2 yz), a0, a1, b0, b1
//   2 cylinder: third row of the world-to-object linear part (3), o.xyz (world), zmin, zmax
//   3 triangle: V1, V2, V3 (9), u1, v1, u2, v2, u3, v3          4 quad: n.xyz, A.xyz, B.xyz
// OUT: fp32 records of 8 words, T.xyz B.xyz 0 0
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ray-tracing-in-cuda_amd/csrc/rt_tangent.h"

static int frames(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) return 3;
    std::vector<float> out;
    uint32_t r[20];
    while (fread(r, sizeof r, 1, f) == 1) {
        float a[20], t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        memcpy(a, r, sizeof a);
        switch (r[0]) {
        case 0: rtmi::tangent_sphere(a[1], a[2], a[3], t[0], t[1], t[2], t[3], t[4], t[5]); break;
        case 1: rtmi::tangent_rect((int)r[1], a[2], a[3], a[4], a[5], t[0], t[1], t[2], t[3], t[4], t[5]); break;
        case 2: rtmi::tangent_cylinder(a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], t[0], t[1], t[2], t[3], t[4], t[5]); break;
        case 3:
            rtmi::tangent_triangle(a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15], t[0], t[1],
                                   t[2], t[3], t[4], t[5]);
            break;
        case 4: rtmi::tangent_quad(a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], t[0], t[1], t[2], t[3], t[4], t[5]); break;
        default: fclose(f); return 6;
        }
        out.insert(out.end(), t, t + 8);
    }
    fclose(f);
    f = fopen(out_path, "wb");
    if (!f) return 4;
    const bool wrote = fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
    return fclose(f) == 0 && wrote ? 0 : 5;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "frames")) return frames(argv[2], argv[3]);
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<uint32_t> in;
    uint32_t rec[20];
    while (fread(rec, sizeof rec, 1, f) == 1) in.insert(in.end(), rec, rec + 20);
    fclose(f);
    const size_t n = in.size() / 20;
    std::vector<uint32_t> out(n * 4, 0u);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t *r = &in[i * 20];
        float tb[6], s, v[9];
        memcpy(tb, r, sizeof tb);
        memcpy(&s, r + 7, 4);
        memcpy(v, r + 8, sizeof v);
        float nb[3] = {v[3], v[4], v[5]};
        float x, y, z;
        bool ok = rtmi::tangent_decode(r[6], x, y, z);
        if (ok)
            ok = rtmi::tangent_normal(nb[0], nb[1], nb[2], v[0], v[1], v[2], v[6], v[7], v[8], r[17] != 0, s, tb[0], tb[1], tb[2], tb[3], tb[4],
                                      tb[5], x, y, z, [](float a) { return sqrtf(a); });
        memcpy(&out[i * 4], nb, sizeof nb);
        out[i * 4 + 3] = ok ? 1u : 0u;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 4;
    const bool wrote = fwrite(out.data(), sizeof(uint32_t), out.size(), f) == out.size();
    return fclose(f) == 0 && wrote ? 0 : 5;
}
