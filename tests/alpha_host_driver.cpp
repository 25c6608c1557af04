// Alpha cutouts on the host, two programs in one file (test_alpha.py builds both):
//
// alpha_host_driver wrapper            (built against librtmi) include/rtmi.hpp: image_texture_rgba() and alpha_masked() carry
//                                      a mask through the scene's build; prints the scene's JSON
//
// alpha_host_driver pack FILE.png ...  (-DALPHA_DRIVER_PACK: a stand-alone program over csrc/png_read.hpp, scene.cpp, capi.cpp and
//                                      pack.hip as plain C++, which test_alpha.py builds with -fsanitize=address,undefined)
//   every file is read as an image texture; one with an alpha plane becomes the mask of a material on each of the five shapes,
//   cutoffs 1e-9, 0.5 and 1; the scene is packed (pack_scene) and the texel words' top bytes and the mask records are held
//   against csrc/rt_alpha.h: 255 - a8, {word offset, rows, cols, c8}; then every texel's verdict (rt_alpha.h, alpha_transparent)
//   through the record against a8 < c8.  Then malformed PNG bytes (truncations of every file, a flipped byte in each chunk) go through
//   the reader, which must refuse or read them without touching memory it does not own.  Prints "alpha driver ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#ifndef ALPHA_DRIVER_PACK
#include "rtmi.hpp"

int main(int argc, char **argv) {
    if (argc != 2 || strcmp(argv[1], "wrapper")) return 2;
    rtmi::scene s(16, 9, 1, 3);
    std::vector<uint8_t> px(2 * 3 * 4);
    for (size_t k = 0; k < 6; ++k) px[4 * k] = (uint8_t)(10 * k), px[4 * k + 1] = 200, px[4 * k + 2] = 50, px[4 * k + 3] = (uint8_t)(k % 2 ? 255 : 0);
    auto leaf = rtmi::image_texture_rgba(2, 3, px);
    auto green = rtmi::lambertian(leaf);
    s.add(rtmi::sphere(rtmi::point3(0, 0, 0), 1.0f, rtmi::alpha_masked(green, leaf)));  // (the material's own image: the RGBA leaf)
    s.add(rtmi::sphere(rtmi::point3(2, 0, 0), 1.0f, green));
    s.add(rtmi::sphere(rtmi::point3(4, 0, 0), 1.0f, rtmi::alpha_masked(rtmi::metal(rtmi::color(0.5f, 0.5f, 0.5f), 0.0f), leaf, 0.25f)));
    int bad = 0;
    try {
        s.add(rtmi::sphere(rtmi::point3(6, 0, 0), 1.0f, rtmi::alpha_masked(rtmi::diffuse_light(rtmi::color(1, 1, 1)), leaf)));
    } catch (const rtmi::error &) {
        bad = 1;
    }
    if (!bad) return 3;
    bad = 0;
    try {  // an image without an alpha plane is no mask
        auto plain = rtmi::image_texture(1, 1, std::vector<uint8_t>(3, 9));
        s.add(rtmi::sphere(rtmi::point3(8, 0, 0), 1.0f, rtmi::alpha_masked(rtmi::dielectric(1.5f), plain)));
    } catch (const rtmi::error &) {
        bad = 1;
    }
    if (!bad) return 4;
    std::vector<char> b(1 << 16);
    const size_t n = rt_scene_to_json(s.handle(), b.data(), b.size());
    if (n == 0 || n > b.size()) return 1;
    fputs(b.data(), stdout);
    return 0;
}

#else
#include "../ray-tracing-in-cuda_amd/csrc/pack.h"
#include "../ray-tracing-in-cuda_amd/csrc/png_read.hpp"
#include "../ray-tracing-in-cuda_amd/csrc/rt_alpha.h"
#include "rtmi.h"

// the nearest texel's index in a rows x cols image as the model states it (include/rtmi.h: the row from u, the column from v,
// clamped to the last row and column) -- the driver's own statement, not the kernels' lookup (render_device.h), which
// test_gpu_alpha.py holds to the fp64 reference
static int texel_index(float u, float v, int rows, int cols) {
    const float fx = (u - floorf(u)) * (float)rows, fy = (v - floorf(v)) * (float)cols;
    const int x = fx >= 0.0f ? (fx < (float)rows ? (int)fx : rows - 1) : 0;  // (not a number: the first row)
    const int y = fy >= 0.0f ? (fy < (float)cols ? (int)fy : cols - 1) : 0;
    return (x < rows - 1 ? x : rows - 1) * cols + (y < cols - 1 ? y : cols - 1);
}

static int fail(const char *what, int a = 0, int b = 0) {
    fprintf(stderr, "alpha driver: %s (%d, %d): %s\n", what, a, b, rt_last_error());
    return 1;
}

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> out;
    if (FILE *f = fopen(path, "rb")) {
        uint8_t chunk[4096];
        size_t n;
        while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) out.insert(out.end(), chunk, chunk + n);
        fclose(f);
    }
    return out;
}

int main(int argc, char **argv) {
    if (argc < 3 || strcmp(argv[1], "pack")) return 2;
    rt_scene *sc = rt_scene_new(32, 18, 1, 4);
    if (!sc) return fail("rt_scene_new");
    const float cutoffs[3] = {1e-9f, 0.5f, 1.0f};
    const float grey[3] = {0.5f, 0.5f, 0.5f};
    const int solid = rt_scene_add_solid_color(sc, grey);
    std::vector<int> masked_mats, masked_tex;
    int with_alpha = 0;
    for (int i = 2; i < argc; ++i) {
        const int tex = rt_scene_add_image_texture_file(sc, argv[i]);
        if (tex < 0) return fail("image file", i);
        int rows = 0, cols = 0;
        const int has = rt_scene_get_image_alpha(sc, tex, &rows, &cols, nullptr, 0);
        if (has < 0) return fail("get_image_alpha", i);
        const int m = rt_scene_add_lambertian(sc, i % 2 ? tex : solid);
        if (m < 0) return fail("material", i);
        const int rc = rt_scene_set_alpha(sc, m, tex, cutoffs[i % 3]);
        if (has != (rc == RT_OK ? 1 : 0)) return fail("a mask takes an image with alpha, and only that", i, rc);
        if (has) {
            ++with_alpha;
            masked_mats.push_back(m), masked_tex.push_back(tex);
            const float c[3] = {(float)i, 0.5f, 0.0f}, u[3] = {1, 0, 0}, v[3] = {0, 1, 0}, uv0[2] = {0, 0}, uv1[2] = {1, 0}, uv2[2] = {0, 1};
            const float a[3] = {(float)i, 0, 1}, b[3] = {(float)i + 1, 0, 1}, d[3] = {(float)i, 1, 1};
            if (rt_scene_add_sphere(sc, c, 0.4f, m) < 0 || rt_scene_add_rect(sc, 0, (float)i, (float)i + 1, 0, 1, -1, m) < 0 ||
                rt_scene_add_cylinder(sc, 0.3f, -0.5f, 0.5f, m, nullptr, 0.0f, c) < 0 || rt_scene_add_quad(sc, c, u, v, m, nullptr, 0.0f, nullptr) < 0 ||
                rt_scene_add_triangle(sc, a, b, d, uv0, uv1, uv2, m) < 0)
                return fail("primitive", i);
        }
    }
    if (!with_alpha) return fail("no file with alpha among the arguments");
    // a round trip through JSON keeps the planes and the masks
    std::vector<char> text(1 << 22);
    const size_t n = rt_scene_to_json(sc, text.data(), text.size());
    if (n == 0 || n > text.size()) return fail("to_json");

    std::vector<float> image;
    rtmi::RenderParams L{};
    if (rtmi::pack_scene(sc->s, image, L) != RT_OK) return fail("pack_scene");
    const int off_alpha = L.off_mat + 3 * L.nm;  // (the mask records: straight behind the material table)
    if (L.off_mat <= 0 || (size_t)(off_alpha + L.nm) * 4 > image.size()) return fail("off_alpha", off_alpha, L.nm);
    const uint32_t *words = reinterpret_cast<const uint32_t *>(image.data());
    long long holes = 0, solids = 0;
    for (int m = 0; m < L.nm; ++m) {
        const uint32_t *rec = words + 4 * (size_t)(off_alpha + m);
        size_t k = 0;
        while (k < masked_mats.size() && masked_mats[k] != m) ++k;
        if (k == masked_mats.size()) {
            if (rec[0] || rec[1] || rec[2] || rec[3]) return fail("a material without a mask has a record", m);
            continue;
        }
        int rows = 0, cols = 0;
        rt_scene_get_image_alpha(sc, masked_tex[k], &rows, &cols, nullptr, 0);
        std::vector<uint8_t> plane((size_t)rows * cols);
        if (rt_scene_get_image_alpha(sc, masked_tex[k], nullptr, nullptr, plane.data(), plane.size()) != 1) return fail("plane", m);
        float cutoff = 0;
        rt_scene_get_alpha(sc, m, nullptr, &cutoff);
        const uint32_t c8 = rtmi::alpha_cutoff_byte((double)cutoff);
        if ((int)rec[1] != rows || (int)rec[2] != cols || rec[3] != c8 || c8 < 1 || c8 > 255) return fail("mask record", m, (int)rec[3]);
        if ((size_t)rec[0] + plane.size() > image.size()) return fail("texels beyond the image", m);
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const float u = ((float)r + 0.5f) / (float)rows, v = ((float)c + 0.5f) / (float)cols;
                const int at = texel_index(u, v, rows, cols);
                if (at != r * cols + c) return fail("texel index", r, c);
                const uint32_t w = words[rec[0] + (size_t)at];
                if ((w >> 24) != 255u - plane[(size_t)at]) return fail("top byte", r, c);
                const bool hole = rtmi::alpha_transparent(w, c8);
                if (hole != (plane[(size_t)at] < c8)) return fail("verdict", r, c);
                (hole ? holes : solids)++;
            }
        // (u, v) outside [0, 1) wrap, the last row and column clamp, and a NaN reads a texel of the image
        const float odd[6] = {-0.25f, 1.0f, 7.75f, -0.0f, 1e30f, NAN};
        for (float u : odd)
            for (float v : odd) {
                const int at = texel_index(u, v, rows, cols);
                if (at < 0 || at >= rows * cols) return fail("texel index out of the image", at);
            }
    }
    rt_scene *back = rt_scene_parse_json(text.data(), strlen(text.data()));
    if (!back) return fail("parse_json");
    std::vector<float> image2;
    rtmi::RenderParams L2{};
    if (rtmi::pack_scene(back->s, image2, L2) != RT_OK || image2.size() != image.size() ||
        memcmp(image2.data(), image.data(), image.size() * sizeof(float)) != 0)
        return fail("the round trip packs to other bytes");
    rt_scene_free(back);
    rt_scene_free(sc);

    // malformed files: every truncation (in steps), and one flipped byte per position (in steps)
    long long refused = 0, read = 0;
    for (int i = 2; i < argc; ++i) {
        const std::vector<uint8_t> file = slurp(argv[i]);
        const size_t step = file.size() > 400 ? file.size() / 200 : 1;
        for (size_t cut = 0; cut < file.size(); cut += step) {
            std::vector<uint8_t> part(file.begin(), file.begin() + (long)cut), rgb, al;
            int rows, cols;
            std::string err;
            (rtmi::png::read(part, rows, cols, rgb, err, &al) ? read : refused)++;
        }
        for (size_t at = 8; at < file.size(); at += step) {
            std::vector<uint8_t> bent = file, rgb, al;
            bent[at] ^= 0x55;
            int rows = 0, cols = 0;
            std::string err;
            if (rtmi::png::read(bent, rows, cols, rgb, err, &al)) {
                ++read;
                if (rgb.size() != (size_t)rows * cols * 3 || (!al.empty() && al.size() != (size_t)rows * cols)) return fail("sizes of a bent file", i);
            } else
                ++refused;
        }
    }
    printf("alpha driver ok: %d images with alpha, %lld holes, %lld solid texels, malformed files: %lld refused, %lld read\n", with_alpha, holes,
           solids, refused, read);
    return 0;
}
#endif
