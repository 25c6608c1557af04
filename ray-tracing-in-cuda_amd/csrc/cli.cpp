// rtmi -- command-line renderer over the C ABI (include/rtmi.h).
//
// Drop-in for both reference executables:
//   gpu-version   `parallel_compute -f scene.json`            (main.cu:455-460) -> main.ppm
//   cmake-cpu     `ray_tracing -w W -h H -d DEPTH -spp N`     (main.cpp:71-81)  -> main.ppm
// plus --rtiow [--scene-seed S] (the hard-coded random_scene() of main.cpp:125-172),
// --seed, -o, --device, --chunk, --dump-json.  Timing goes to stderr like the reference's
// when() markers (rtweekend.cuh:40).
// --gpus N renders ONE frame on the first N GPUs of the node: row tiles dealt out to the devices, one
// RCCL gather (rt_render_hip_tiles); the image is the same bytes as with one GPU.  (The reference's blue.py
// instead starts one process per GPU per animation frame; rtmi-frames is that shape.)
// Resumable rendering: --acc-out FILE saves the exact pixel sums, --acc-in FILE continues from them
// (-spp is then the number of samples to ADD; --spp-begin overrides the first sample index).  Any
// split of a sample range into runs writes the same main.ppm as one run over the whole range.
// Adaptive sampling: --adaptive T [--min-spp N] [--max-spp N] gives every 8x8 tile samples until its noise estimate is
// within T (rt_render_hip_adaptive); each pixel is written rescaled to the scene's spp (sum * spp / n).
// Environment map: --env FILE [--env-scale S] [--env-rotate DEG] lights the scene with a lat-long .hdr / .pfm / .png / .ppm
// panorama (rt_scene_set_environment_file); with --nee its bright texels are sampled.
// Display stage (rt_display_hip): --tonemap clamp|reinhard|aces, --exposure EV (multiplier 2^EV), --auto-exposure
// [KEY], --white W, --bloom STRENGTH [--bloom-threshold T] [--bloom-levels L].  With any of them the PPM and the PNG are
// written from the stage's 8-bit output; without, the program writes what it always wrote.  --hdr-out FILE.hdr|FILE.pfm
// writes the mean image before the display stage (and after --denoise) as a float image (rt_write_hdr / rt_write_pfm).
// Ray queries (rt_trace_hip): --pick X,Y (X from the left, Y from the top) traces the ray through that pixel's
// centre and prints what it meets as one JSON line on stdout; no frame is rendered.  --focus-at X,Y traces the same ray and
// focuses the camera on what it meets (focus_dist = t |dir|, rt_scene_set_camera) before the render.
// Smooth shading: --mesh-normals flat|file|smooth[:DEG] gives every "mesh" of the scene file its vertex normals
// that way, whatever its own "normals" says (DEG: the crease angle of the generated normals, 180 without).
// Camera projections: --projection TYPE[:P1[,P2]] replaces the scene file's -- perspective, orthographic:HEIGHT,
// panoramic[:HFOV[,VFOV]], fisheye[:FOV] (degrees; rt_scene_set_projection).  --pick and --focus-at follow the scene's camera.
// Mesh lights: --mesh-lights lists emissive triangles among the emitters --nee samples (rt_scene_set_mesh_lights).
// Light sampling in media: --nee-media is --nee plus rt_scene_set_media_light_sampling.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtmi.h"

// exact pixel sums on disk: 40-byte header + int64[height][width][3], little endian
struct AccHeader {
    char magic[8];  // "RTMIACC2" (version 1 held sums in units of 2^-32)
    int32_t width, height;
    int64_t samples_done;  // samples [0, samples_done) are in the sums
    uint64_t seed;
    int64_t fix_bits;      // fractional bits of the sums (RT_ACC_FIX_BITS): a file in another scale is refused
};
static_assert(sizeof(AccHeader) == 40, "accumulator file header");

static double now_s() {
    using namespace std::chrono;
    return duration<double>(steady_clock::now().time_since_epoch()).count();
}

static int usage(const char *argv0) {
    fprintf(stderr,
            "usage: %s [-f scene.json | --rtiow] [-w W] [-h H] [-d DEPTH] [-spp N] [-o out.ppm]\n"
            "          [--seed S] [--scene-seed S] [--device N] [--chunk N] [--dump-json file] [--count] [--no-png]\n"
            "          [--acc-in sums.bin] [--acc-out sums.bin] [--spp-begin FIRST] [--rr SURVIVAL_PROBABILITY] [--nee | --nee-media]\n"
            "          [--mesh-lights] [--nested-grid] [--env map.hdr [--env-scale S] [--env-rotate DEG]]\n"
            "          [--gpus N] [--tile-rows R] [--adaptive THRESHOLD [--min-spp N] [--max-spp N]]\n"
            "          [--denoise] [--aov PREFIX] [--feature-spp N]\n"
            "          [--tonemap clamp|reinhard|aces] [--exposure EV] [--auto-exposure [KEY]] [--white W]\n"
            "          [--bloom STRENGTH] [--bloom-threshold T] [--bloom-levels L] [--hdr-out frame.hdr|frame.pfm]\n"
            "          [--pick X,Y] [--focus-at X,Y] [--mesh-normals flat|file|smooth[:DEG]]\n"
            "          [--projection perspective|orthographic:HEIGHT|panoramic[:HFOV[,VFOV]]|fisheye[:FOV]]\n",
            argv0);
    return 2;
}

// a whole-string number in [lo, hi]; false for anything else (NaN included)
static bool number(const char *v, double lo, double hi, double *out) {
    char *end = nullptr;
    const double x = strtod(v, &end);
    if (end == v || *end != '\0' || !(x >= lo && x <= hi)) return false;
    *out = x;
    return true;
}

static bool ends_with(const std::string &s, const char *tail) {
    const size_t n = strlen(tail);
    return s.size() > n && s.compare(s.size() - n, n, tail) == 0;
}

// "X,Y": two whole numbers >= 0
static bool pixel_pair(const char *v, int *x, int *y) {
    char *end = nullptr;
    const long a = strtol(v, &end, 10);
    if (end == v || *end != ',' || a < 0 || a > 1000000) return false;
    const char *w = end + 1;
    const long b = strtol(w, &end, 10);
    if (end == w || *end != '\0' || b < 0 || b > 1000000) return false;
    *x = (int)a, *y = (int)b;
    return true;
}

// The ray through the centre of pixel (x from the left, y from the top) and what it meets: the scene's camera as the kernels
// evaluate it, whatever its projection (rt_camera_ray) -- u = (x + 0.5) / (W - 1), v likewise from the bottom row -- and no
// lens offset.  A pixel outside a fisheye's image circle has no ray: reported as an invalid ray is.
static int trace_pixel(const rt_scene *sc, int device, int x, int y, rt_ray *ray, rt_hit *hit) {
    rt_scene_info info;
    if (rt_scene_get_info(sc, &info) != RT_OK) return RT_ERR_ARG;
    if (x >= info.width || y >= info.height) {
        fprintf(stderr, "rtmi: pixel %d,%d lies outside the %d x %d frame\n", x, y, info.width, info.height);
        return RT_ERR_ARG;
    }
    const float u = ((float)x + 0.5f) * (1.0f / (float)(info.width - 1));
    const float v = ((float)(info.height - 1 - y) + 0.5f) * (1.0f / (float)(info.height - 1));
    memset(ray, 0, sizeof *ray);
    if (rt_camera_ray(sc, u, v, 0.0f, 0.0f, ray, nullptr) != RT_OK) {
        fprintf(stderr, "rtmi: %s\n", rt_last_error());
        return RT_ERR_ARG;
    }
    rt_opts o;
    rt_opts_default(&o);
    o.device = device;
    const int rc = rt_trace_hip(sc, &o, RT_TRACE_CLOSEST, ray, 1, hit, nullptr);
    if (rc != RT_OK) fprintf(stderr, "rtmi: %s\n", rt_last_error());
    else if (hit->prim == RT_HIT_INVALID) fprintf(stderr, "rtmi: the camera's ray through pixel %d,%d is not a valid ray\n", x, y);
    return rc != RT_OK ? rc : hit->prim == RT_HIT_INVALID ? RT_ERR_ARG : RT_OK;
}

int main(int argc, char **argv) {
    std::string scene_file = "sample_scene.json";  // main.cu:456 default
    std::string out_file = "main.ppm";             // main.cu:512
    std::string dump_json, acc_in, acc_out;
    long long spp_begin = -1;
    double rr = -1.0;  // Russian roulette: keep the scene file's setting
    bool nee = false;  // light sampling: on if the scene file or --nee says so
    bool nee_media = false;    // light samples in participating media too: on if the scene file or --nee-media says so
    bool mesh_lights = false;  // emissive triangles are sampled too: on if the scene file or --mesh-lights says so
    bool nested = false;  // nested grid: on if the scene file or --nested-grid says so
    std::string env_file;  // environment map: replaces the scene file's
    double env_scale = 1.0, env_rotate = 0.0;
    bool have_env_opts = false;
    bool rtiow = false, have_file = false, count = false, no_png = false;
    double adaptive = -1.0;  // noise target of adaptive sampling, < 0: off
    bool have_adaptive = false;
    int min_spp = 16, max_spp = 0;
    bool denoise = false;     // filter what is written (rt_denoise_hip, default parameters)
    std::string aov_prefix;   // write PREFIX_albedo.png, PREFIX_normal.png, PREFIX_depth.png
    int feature_spp = 0;      // samples of the feature passes, 0: min(spp, 16)
    bool have_min = false, have_max = false;
    bool have_display = false;  // any display flag: the images are written from rt_display_hip's bytes
    rt_display dp;
    memset(&dp, 0, sizeof dp);
    std::string hdr_out;        // the mean image before the display stage, .hdr or .pfm
    int w = 0, h = 0, depth = 0, spp = 0, device = 0, chunk = 0, gpus = 0, tile_rows = 0;
    bool pick = false, focus_at = false;  // ray queries through a pixel's centre
    int projection = -1;                  // --projection: replaces the scene file's; -1: keep it
    float projection_params[2] = {0.0f, 0.0f};
    int projection_given = 0;             // how many parameters the flag carried
    int pick_x = 0, pick_y = 0, focus_x = 0, focus_y = 0;
    unsigned long long seed = 2023;
    unsigned scene_seed = 7;  // srand(7), main.cpp:119
    for (int i = 1; i < argc; ++i) {
        auto need = [&](const char *flag) -> const char * {
            if (i + 1 >= argc) {
                fprintf(stderr, "%s needs a value\n", flag);
                exit(2);
            }
            return argv[++i];
        };
        if (!strcmp(argv[i], "-f")) scene_file = need("-f"), have_file = true;
        else if (!strcmp(argv[i], "-w")) w = atoi(need("-w"));
        else if (!strcmp(argv[i], "-h")) h = atoi(need("-h"));
        else if (!strcmp(argv[i], "-d")) depth = atoi(need("-d"));
        else if (!strcmp(argv[i], "-spp")) spp = atoi(need("-spp"));
        else if (!strcmp(argv[i], "-o")) out_file = need("-o");
        else if (!strcmp(argv[i], "--seed")) seed = strtoull(need("--seed"), nullptr, 0);
        else if (!strcmp(argv[i], "--scene-seed")) scene_seed = (unsigned)strtoul(need("--scene-seed"), nullptr, 0);
        else if (!strcmp(argv[i], "--device")) device = atoi(need("--device"));
        else if (!strcmp(argv[i], "--chunk")) chunk = atoi(need("--chunk"));
        else if (!strcmp(argv[i], "--gpus")) gpus = atoi(need("--gpus"));
        else if (!strcmp(argv[i], "--tile-rows")) tile_rows = atoi(need("--tile-rows"));
        else if (!strcmp(argv[i], "--dump-json")) dump_json = need("--dump-json");
        else if (!strcmp(argv[i], "--acc-in")) acc_in = need("--acc-in");
        else if (!strcmp(argv[i], "--acc-out")) acc_out = need("--acc-out");
        else if (!strcmp(argv[i], "--spp-begin")) spp_begin = atoll(need("--spp-begin"));
        else if (!strcmp(argv[i], "--rr")) rr = atof(need("--rr"));
        else if (!strcmp(argv[i], "--nee")) nee = true;
        else if (!strcmp(argv[i], "--mesh-lights")) mesh_lights = true;
        else if (!strcmp(argv[i], "--nee-media")) nee = nee_media = true;
        else if (!strcmp(argv[i], "--nested-grid")) nested = true;
        else if (!strcmp(argv[i], "--projection")) {
            const std::string v = need("--projection");
            const size_t colon = v.find(':');
            const std::string name = v.substr(0, colon);
            static const char *const names[] = {"perspective", "orthographic", "panoramic", "fisheye"};
            for (int k = 0; k < 4; ++k)
                if (name == names[k]) projection = k;
            bool ok = projection >= 0;
            if (ok && colon != std::string::npos) {
                const std::string rest = v.substr(colon + 1);
                const size_t comma = rest.find(',');
                double a = 0, b = 0;
                ok = number(rest.substr(0, comma).c_str(), -1e30, 1e30, &a);
                projection_params[0] = (float)a, projection_given = 1;
                if (ok && comma != std::string::npos) {
                    ok = number(rest.substr(comma + 1).c_str(), -1e30, 1e30, &b);
                    projection_params[1] = (float)b, projection_given = 2;
                }
            }
            if (!ok) {
                fprintf(stderr, "rtmi: --projection takes perspective, orthographic:HEIGHT, panoramic[:HFOV[,VFOV]] or fisheye[:FOV], not %s\n", v.c_str());
                return 2;
            }
        }
        else if (!strcmp(argv[i], "--mesh-normals")) {
            const std::string v = need("--mesh-normals");
            double deg = 180.0;
            int mode = -1;
            if (v == "flat") mode = RT_MESH_NORMALS_FLAT;
            else if (v == "file") mode = RT_MESH_NORMALS_FILE;
            else if (v == "smooth") mode = RT_MESH_NORMALS_SMOOTH;
            else if (v.rfind("smooth:", 0) == 0 && number(v.c_str() + 7, 0.0, 180.0, &deg)) mode = RT_MESH_NORMALS_SMOOTH;
            if (mode < 0) {
                fprintf(stderr, "rtmi: --mesh-normals takes flat, file, smooth or smooth:DEG (0..180), not %s\n", v.c_str());
                return 2;
            }
            rt_set_mesh_normals_override(mode, (float)deg);
        }
        else if (!strcmp(argv[i], "--env")) env_file = need("--env");
        else if (!strcmp(argv[i], "--env-scale")) env_scale = atof(need("--env-scale")), have_env_opts = true;
        else if (!strcmp(argv[i], "--env-rotate")) env_rotate = atof(need("--env-rotate")), have_env_opts = true;
        else if (!strcmp(argv[i], "--adaptive")) {
            const char *v = need("--adaptive");
            char *end = nullptr;
            adaptive = strtod(v, &end);
            have_adaptive = true;
            if (end == v || *end != '\0' || !(adaptive >= 0.0) || adaptive > 3.4e38) {
                fprintf(stderr, "rtmi: --adaptive needs a finite threshold >= 0, got '%s'\n", v);
                return 2;
            }
        }
        else if (!strcmp(argv[i], "--min-spp")) min_spp = atoi(need("--min-spp")), have_min = true;
        else if (!strcmp(argv[i], "--max-spp")) max_spp = atoi(need("--max-spp")), have_max = true;
        else if (!strcmp(argv[i], "--denoise")) denoise = true;
        else if (!strcmp(argv[i], "--aov")) aov_prefix = need("--aov");
        else if (!strcmp(argv[i], "--feature-spp")) {
            const char *v = need("--feature-spp");
            char *end = nullptr;
            const long n = strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 1 || n > (1 << 23)) {
                fprintf(stderr, "rtmi: --feature-spp needs a sample count in 1 .. 8388608, got '%s'\n", v);
                return 2;
            }
            feature_spp = (int)n;
        }
        else if (!strcmp(argv[i], "--tonemap")) {
            const char *v = need("--tonemap");
            if (!strcmp(v, "clamp")) dp.tonemap = RT_TONEMAP_CLAMP;
            else if (!strcmp(v, "reinhard")) dp.tonemap = RT_TONEMAP_REINHARD;
            else if (!strcmp(v, "aces")) dp.tonemap = RT_TONEMAP_ACES;
            else {
                fprintf(stderr, "rtmi: --tonemap needs clamp, reinhard or aces, got '%s'\n", v);
                return 2;
            }
            have_display = true;
        }
        else if (!strcmp(argv[i], "--exposure")) {
            const char *v = need("--exposure");
            double ev;
            if (!number(v, -100.0, 100.0, &ev)) {
                fprintf(stderr, "rtmi: --exposure needs a number of stops in -100 .. 100, got '%s'\n", v);
                return 2;
            }
            dp.exposure = (float)std::exp2(ev);  // fp64, rounded once
            have_display = true;
        }
        else if (!strcmp(argv[i], "--auto-exposure")) {
            double key = 0.18;  // the value is optional: the next argument is taken if it is a number
            double x;
            if (i + 1 < argc && number(argv[i + 1], -1e30, 1e30, &x)) {
                if (!(x > 0.0)) {
                    fprintf(stderr, "rtmi: --auto-exposure needs a key > 0, got '%s'\n", argv[i + 1]);
                    return 2;
                }
                key = x, ++i;
            }
            dp.auto_key = (float)key;
            have_display = true;
        }
        else if (!strcmp(argv[i], "--white") || !strcmp(argv[i], "--bloom") || !strcmp(argv[i], "--bloom-threshold")) {
            const char *flag = argv[i], *v = need(flag);
            const bool white = !strcmp(flag, "--white");
            double x;
            if (!number(v, 0.0, 1e30, &x) || (white && !(x > 0.0))) {
                fprintf(stderr, "rtmi: %s needs a number %s 0, got '%s'\n", flag, white ? ">" : ">=", v);
                return 2;
            }
            (white ? dp.white : !strcmp(flag, "--bloom") ? dp.bloom_strength : dp.bloom_threshold) = (float)x;
            have_display = true;
        }
        else if (!strcmp(argv[i], "--bloom-levels")) {
            const char *v = need("--bloom-levels");
            double x;
            if (!number(v, 1.0, 8.0, &x) || x != (double)(int)x) {
                fprintf(stderr, "rtmi: --bloom-levels needs a whole number in 1 .. 8, got '%s'\n", v);
                return 2;
            }
            dp.bloom_levels = (int)x;
            have_display = true;
        }
        else if (!strcmp(argv[i], "--hdr-out")) {
            hdr_out = need("--hdr-out");
            if (!ends_with(hdr_out, ".hdr") && !ends_with(hdr_out, ".pfm")) {
                fprintf(stderr, "rtmi: --hdr-out needs a file name ending in .hdr or .pfm, got '%s'\n", hdr_out.c_str());
                return 2;
            }
        }
        else if (!strcmp(argv[i], "--pick") || !strcmp(argv[i], "--focus-at")) {
            const char *flag = argv[i], *v = need(flag);
            const bool p = !strcmp(flag, "--pick");
            if (!pixel_pair(v, p ? &pick_x : &focus_x, p ? &pick_y : &focus_y)) {
                fprintf(stderr, "rtmi: %s needs a pixel X,Y (X from the left, Y from the top), got '%s'\n", flag, v);
                return 2;
            }
            (p ? pick : focus_at) = true;
        }
        else if (!strcmp(argv[i], "--rtiow")) rtiow = true;
        else if (!strcmp(argv[i], "--count")) count = true;
        else if (!strcmp(argv[i], "--no-png")) no_png = true;
        else if (!strcmp(argv[i], "--help")) return usage(argv[0]);
        else {
            fprintf(stderr, "unknown argument '%s'\n", argv[i]);
            return usage(argv[0]);
        }
    }
    const bool progressive = !acc_in.empty() || !acc_out.empty() || spp_begin >= 0;
    if (!have_adaptive && (have_min || have_max)) {
        fprintf(stderr, "rtmi: --min-spp and --max-spp belong to --adaptive\n");
        return 2;
    }
    if (have_adaptive && (gpus > 0 || progressive || count)) {
        fprintf(stderr, "rtmi: --adaptive renders one frame on one device: it cannot be combined with %s\n",
                gpus > 0 ? "--gpus" : (count ? "--count" : "--acc-in/--acc-out/--spp-begin"));
        return 2;
    }
    if (have_adaptive && (min_spp < 2 || max_spp < 0 || (max_spp > 0 && max_spp < min_spp))) {
        fprintf(stderr, "rtmi: --min-spp must be >= 2 and --max-spp 0 (the scene's spp) or >= --min-spp\n");
        return 2;
    }
    if (have_env_opts && env_file.empty()) {
        fprintf(stderr, "rtmi: --env-scale and --env-rotate belong to --env\n");
        return 2;
    }
    if (feature_spp > 0 && !denoise && aov_prefix.empty()) {
        fprintf(stderr, "rtmi: --feature-spp belongs to --denoise or --aov\n");
        return 2;
    }
    if ((denoise || !aov_prefix.empty()) && (gpus > 0 || count)) {
        fprintf(stderr, "rtmi: --denoise and --aov render their feature passes on one device: drop %s\n", gpus > 0 ? "--gpus" : "--count");
        return 2;
    }
    double t0 = now_s();
    rt_scene *sc;
    if (rtiow && !have_file) sc = rt_scene_rtiow(scene_seed, w > 0 ? w : 400, h > 0 ? h : 225, spp > 0 ? spp : 50,
                                                  depth > 0 ? depth : 50);  // defaults: main.cpp:64-68
    else sc = rt_scene_load_json(scene_file.c_str());
    if (!sc) {
        fprintf(stderr, "rtmi: %s\n", rt_last_error());
        return 1;
    }
    if (rt_scene_override(sc, w, h, spp, depth) != RT_OK) {
        fprintf(stderr, "rtmi: %s\n", rt_last_error());
        return 1;
    }
    if (nee && rt_scene_set_light_sampling(sc, 1) != RT_OK) {
        fprintf(stderr, "rtmi: %s\n", rt_last_error());
        return 1;
    }
    if (rt_scene_get_light_sampling(sc) == 0 && rt_scene_get_analytic_lights(sc, nullptr, 0) > 0)
        fprintf(stderr, "rtmi: light sampling is off: the scene's %d point / spot / distant lights light nothing (--nee switches it on)\n",
                rt_scene_get_analytic_lights(sc, nullptr, 0));
    if (nee_media && rt_scene_set_media_light_sampling(sc, 1) != RT_OK) {
        fprintf(stderr, "rtmi: %s\n", rt_last_error());
        return 1;
    }
    if (mesh_lights && rt_scene_set_mesh_lights(sc, 1) != RT_OK) {
        fprintf(stderr, "rtmi: %s\n", rt_last_error());
        return 1;
    }
    if (!env_file.empty() && rt_scene_set_environment_file(sc, env_file.c_str(), (float)env_scale, (float)env_rotate) != RT_OK) {
        fprintf(stderr, "rtmi: %s\n", rt_last_error());
        return 1;
    }
    if (projection >= 0) {
        if (projection == RT_PROJ_PANORAMIC && projection_given == 1) projection_params[1] = 180.0f;
        if (rt_scene_set_projection(sc, projection, projection_given ? projection_params : nullptr) != RT_OK) {
            fprintf(stderr, "rtmi: %s\n", rt_last_error());
            return 1;
        }
    }
    if (nested && rt_scene_set_nested_grid(sc, 1) != RT_OK) {
        fprintf(stderr, "rtmi: %s\n", rt_last_error());
        return 1;
    }
    if (rr >= 0.0 && rt_scene_set_russian_roulette(sc, (float)rr) != RT_OK) {
        fprintf(stderr, "rtmi: %s\n", rt_last_error());
        return 1;
    }
    if (focus_at) {
        rt_ray ray;
        rt_hit hit;
        if (trace_pixel(sc, device, focus_x, focus_y, &ray, &hit) != RT_OK) return 1;
        if (hit.prim < 0) {
            fprintf(stderr, "rtmi: --focus-at %d,%d: the ray through that pixel meets nothing to focus on\n", focus_x, focus_y);
            return 1;
        }
        rt_camera cam;
        rt_scene_get_camera(sc, &cam);
        const float len = sqrtf(fmaf(ray.dir[0], ray.dir[0], fmaf(ray.dir[1], ray.dir[1], ray.dir[2] * ray.dir[2])));
        const float focus = hit.t * len;
        if (rt_scene_set_camera(sc, cam.lookfrom, cam.lookat, cam.vup, cam.vfov, cam.aspect, cam.aperture, focus) != RT_OK) {
            fprintf(stderr, "rtmi: %s\n", rt_last_error());
            return 1;
        }
        fprintf(stderr, "focus: pixel %d,%d meets primitive %d at distance %.9g\n", focus_x, focus_y, hit.prim, (double)focus);
    }
    rt_scene_info info;
    rt_scene_get_info(sc, &info);
    fprintf(stderr, "scene: %dx%d, %d spp, depth %d, %d objects, %d materials, %d textures\n", info.width,
            info.height, info.samples_per_pixel, info.max_depth, info.num_prims, info.num_materials,
            info.num_textures);
    if (!dump_json.empty()) {
        size_t n = rt_scene_to_json(sc, nullptr, 0);
        std::vector<char> buf(n);
        rt_scene_to_json(sc, buf.data(), n);
        FILE *fp = fopen(dump_json.c_str(), "w");
        if (!fp) {
            fprintf(stderr, "rtmi: cannot write %s\n", dump_json.c_str());
            return 1;
        }
        fwrite(buf.data(), 1, n - 1, fp);
        fclose(fp);
    }
    if (pick) {
        rt_ray ray;
        rt_hit hit;
        if (trace_pixel(sc, device, pick_x, pick_y, &ray, &hit) != RT_OK) return 1;
        if (hit.prim < 0) {
            printf("{\"prim\": -1}\n");
        } else {
            std::vector<rt_prim> prims((size_t)info.num_prims);
            rt_scene_get_prims(sc, prims.data(), info.num_prims);
            static const char *const types[] = {"sphere", "xy_rect", "xz_rect", "yz_rect", "cylinder", "triangle"};
            const int ty = prims[(size_t)hit.prim].type;
            const float len = sqrtf(fmaf(ray.dir[0], ray.dir[0], fmaf(ray.dir[1], ray.dir[1], ray.dir[2] * ray.dir[2])));
            // (%.9g: every fp32 value reads back as itself)
            printf("{\"prim\": %d, \"type\": \"%s\", \"material\": %d, \"t\": %.9g, \"distance\": %.9g, \"point\": [%.9g, %.9g, %.9g], "
                   "\"normal\": [%.9g, %.9g, %.9g], \"front\": %d, \"uv\": [%.9g, %.9g], \"origin\": [%.9g, %.9g, %.9g], \"dir\": [%.9g, %.9g, %.9g]}\n",
                   hit.prim, ty >= 0 && ty < 6 ? types[ty] : "?", hit.material, (double)hit.t, (double)(hit.t * len), (double)hit.point[0],
                   (double)hit.point[1], (double)hit.point[2], (double)hit.normal[0], (double)hit.normal[1], (double)hit.normal[2], hit.front,
                   (double)hit.u, (double)hit.v, (double)ray.origin[0], (double)ray.origin[1], (double)ray.origin[2], (double)ray.dir[0],
                   (double)ray.dir[1], (double)ray.dir[2]);
        }
        rt_scene_free(sc);
        return 0;
    }
    rt_opts o;
    rt_opts_default(&o);
    o.seed = seed;
    o.device = device;
    o.spp_chunk = chunk;
    if (tile_rows > 0) o.tile_rows = tile_rows;
    rt_stats st;
    std::vector<float> img((size_t)info.width * info.height * 3);
    int total_spp = info.samples_per_pixel;  // divisor of the written image
    int rc;
    if (progressive && gpus > 0) {
        fprintf(stderr, "rtmi: --gpus cannot be combined with --acc-in/--acc-out/--spp-begin\n");
        return 2;
    }
    if (progressive) {
        if (count) {
            fprintf(stderr, "rtmi: --count cannot be combined with --acc-in/--acc-out/--spp-begin\n");
            return 2;
        }
        std::vector<int64_t> acc(img.size(), 0);
        long long done = 0;
        if (!acc_in.empty()) {
            FILE *fp = fopen(acc_in.c_str(), "rb");
            AccHeader h;
            if (!fp || fread(&h, sizeof h, 1, fp) != 1 || memcmp(h.magic, "RTMIACC", 7) != 0) {
                fprintf(stderr, "rtmi: %s is not an accumulator file\n", acc_in.c_str());
                return 1;
            }
            if (h.magic[7] != '2' || h.fix_bits != RT_ACC_FIX_BITS) {
                fprintf(stderr, "rtmi: %s holds pixel sums in another fixed-point scale (format '%c', %lld fractional bits; this build: "
                        "'2', %d): it cannot be continued\n", acc_in.c_str(), h.magic[7], (long long)h.fix_bits, RT_ACC_FIX_BITS);
                return 1;
            }
            if (h.width != info.width || h.height != info.height || h.seed != seed) {
                fprintf(stderr, "rtmi: %s holds %dx%d sums of seed %llu, this run is %dx%d seed %llu\n", acc_in.c_str(),
                        h.width, h.height, (unsigned long long)h.seed, info.width, info.height, seed);
                return 1;
            }
            if (fread(acc.data(), sizeof(int64_t), acc.size(), fp) != acc.size()) {
                fprintf(stderr, "rtmi: %s is truncated\n", acc_in.c_str());
                return 1;
            }
            fclose(fp);
            done = h.samples_done;
        }
        if (spp_begin < 0) spp_begin = done;
        if (spp_begin != done) {
            fprintf(stderr, "rtmi: the sums hold samples [0, %lld) but --spp-begin is %lld\n", done, spp_begin);
            return 1;
        }
        if (spp_begin + info.samples_per_pixel > 0x7fffffffLL) {
            fprintf(stderr, "rtmi: sample index overflow\n");
            return 1;
        }
        o.sample_first = (int)spp_begin;
        o.sample_count = info.samples_per_pixel;
        rc = rt_render_hip_accumulate(sc, &o, acc.data(), img.data(), &st);
        total_spp = (int)(spp_begin + info.samples_per_pixel);
        if (rc == RT_OK && !acc_out.empty()) {
            AccHeader h = {{'R', 'T', 'M', 'I', 'A', 'C', 'C', '2'}, info.width, info.height, total_spp, seed, RT_ACC_FIX_BITS};
            FILE *fp = fopen(acc_out.c_str(), "wb");
            if (!fp || fwrite(&h, sizeof h, 1, fp) != 1 ||
                fwrite(acc.data(), sizeof(int64_t), acc.size(), fp) != acc.size() || fclose(fp) != 0) {
                fprintf(stderr, "rtmi: cannot write %s\n", acc_out.c_str());
                return 1;
            }
        }
        if (rc == RT_OK)
            fprintf(stderr, "progressive: samples [%lld, %d) added, image holds %d spp\n", spp_begin, total_spp, total_spp);
    } else if (have_adaptive) {
        rt_adaptive a = {min_spp, max_spp, (float)adaptive};
        rt_adaptive_stats ast;
        std::vector<int32_t> spp_map((size_t)info.width * info.height);
        rc = rt_render_hip_adaptive(sc, &o, &a, img.data(), spp_map.data(), &ast);
        if (rc == RT_OK) {
            // rescale every pixel to the scene's spp, so that the writers' division applies
            for (size_t p = 0; p < spp_map.size(); ++p)
                for (int c = 0; c < 3; ++c)
                    img[p * 3 + c] = (float)((double)img[p * 3 + c] * total_spp / spp_map[p]);
            const int cap = max_spp > 0 ? max_spp : info.samples_per_pixel;
            const double full = (double)info.width * info.height * cap;
            fprintf(stderr, "adaptive: threshold %g, %d passes, active tiles per pass (of %d):", adaptive, ast.passes, ast.tiles);
            for (int k = 0; k < ast.passes; ++k) fprintf(stderr, " %d@%d", ast.active[k], ast.spp_after[k]);
            fprintf(stderr, "\nadaptive: %llu pixel samples of %.0f at %d spp (%.1f %% saved), %.3f ms\n", (unsigned long long)ast.samples,
                    full, cap, 100.0 * (1.0 - (double)ast.samples / full), ast.kernel_ms);
            st.kernel_ms = ast.kernel_ms, st.upload_ms = 0;
        }
    } else if (gpus > 0) {
        if (count) {
            fprintf(stderr, "rtmi: --count is a single-device diagnostic; drop --gpus\n");
            return 2;
        }
        rc = rt_render_hip_tiles(sc, &o, nullptr, gpus, img.data(), &st);
        if (rc == RT_OK)
            fprintf(stderr, "tiles: %d device(s), slowest render %.3f ms, gather + placement %.3f ms\n", st.devices_used,
                    st.kernel_ms, st.gather_ms);
    } else {
        rc = count ? rt_render_hip_count(sc, &o, img.data(), &st) : rt_render_hip(sc, &o, img.data(), &st);
    }
    if (rc != RT_OK) {
        fprintf(stderr, "rtmi: render failed: %s: %s\n", rt_status_string(rc), rt_last_error());
        return 1;
    }
    double samples = (double)info.width * info.height * info.samples_per_pixel;
    fprintf(stderr, "render: %.3f ms kernel (%.1f Msamples/s), %.3f ms upload\n", st.kernel_ms,
            samples / (st.kernel_ms * 1e3), st.upload_ms);
    if (count)
        fprintf(stderr, "counts: samples %llu queries %llu prim_tests %llu hits %llu misses %llu draws %llu\n",
                (unsigned long long)st.samples, (unsigned long long)st.queries, (unsigned long long)st.prim_tests,
                (unsigned long long)st.hits, (unsigned long long)st.misses, (unsigned long long)st.rng_draws);
    if (denoise || !aov_prefix.empty()) {
        // the three first-hit feature passes (same seed: the samples [0, n) of the frame's own streams), then the filter
        const int nf = feature_spp > 0 ? feature_spp : std::min(info.samples_per_pixel, 16);
        rt_opts fo = o;
        fo.sample_first = 0, fo.sample_count = nf;
        std::vector<float> feat[3];
        double feat_ms = 0.0;
        for (int f = 0; f < 3; ++f) {
            feat[f].resize(img.size());
            rt_stats fs;
            if (rt_render_hip_feature(sc, &fo, f, feat[f].data(), &fs) != RT_OK) {
                fprintf(stderr, "rtmi: feature pass failed: %s\n", rt_last_error());
                return 1;
            }
            feat_ms += fs.kernel_ms;
        }
        fprintf(stderr, "features: albedo, normal, depth at %d spp, %.3f ms\n", nf, feat_ms);
        if (denoise) {
            std::vector<float> out(img.size());
            double ms = 0.0;
            if (rt_denoise_hip(info.width, info.height, img.data(), total_spp, nullptr, feat[0].data(), feat[1].data(), feat[2].data(), nf,
                               nullptr, device, out.data(), &ms) != RT_OK) {
                fprintf(stderr, "rtmi: denoise failed: %s\n", rt_last_error());
                return 1;
            }
            img.swap(out);
            fprintf(stderr, "denoise: %.3f ms\n", ms);
        }
        if (!aov_prefix.empty()) {
            // normal: 0.5 n + 0.5; depth: mean t scaled so that the frame's largest is 1, in every channel
            float tmax = 0.0f;
            for (size_t p = 0; p < img.size(); p += 3) tmax = std::max(tmax, feat[2][p]);
            for (size_t p = 0; p < img.size(); p += 3) {
                const float t = tmax > 0.0f ? feat[2][p] / tmax * (float)nf : 0.0f;
                for (int c = 0; c < 3; ++c) feat[1][p + c] = 0.5f * feat[1][p + c] + 0.5f * (float)nf;
                feat[2][p] = feat[2][p + 1] = feat[2][p + 2] = t;
            }
            const char *names[3] = {"_albedo.png", "_normal.png", "_depth.png"};
            for (int f = 0; f < 3; ++f)
                if (rt_write_png((aov_prefix + names[f]).c_str(), feat[f].data(), info.width, info.height, nf, 0) != RT_OK) {
                    fprintf(stderr, "rtmi: %s\n", rt_last_error());
                    return 1;
                }
        }
    }
    if (!hdr_out.empty()) {
        const bool pfm = ends_with(hdr_out, ".pfm");
        if ((pfm ? rt_write_pfm : rt_write_hdr)(hdr_out.c_str(), img.data(), info.width, info.height, total_spp) != RT_OK) {
            fprintf(stderr, "rtmi: %s\n", rt_last_error());
            return 1;
        }
    }
    // what is written: with a display flag the stage's bytes, in both files; else the frame through the reference's writers
    // (write_image(..., data["output_file"]), main.cu:514: a LINEAR PNG next to the PPM).  The PNG is skipped when the
    // directory of output_file does not exist, which the reference would crash on.
    std::vector<uint8_t> rgb8;
    if (have_display) {
        rgb8.resize(img.size());
        rt_display_stats ds;
        if (rt_display_hip(info.width, info.height, img.data(), total_spp, nullptr, &dp, device, nullptr, rgb8.data(), &ds) != RT_OK) {
            fprintf(stderr, "rtmi: display stage failed: %s\n", rt_last_error());
            return 1;
        }
        fprintf(stderr, "display: exposure x%g, %.3f ms\n", (double)ds.exposure_used, ds.ms);
    }
    const int ppm_rc = have_display ? rt_write_ppm_rgb8(out_file.c_str(), rgb8.data(), info.width, info.height)
                                    : rt_write_ppm(out_file.c_str(), img.data(), info.width, info.height, total_spp);
    if (ppm_rc != RT_OK) {
        fprintf(stderr, "rtmi: %s\n", rt_last_error());
        return 1;
    }
    if (!no_png) {
        const char *png = rt_scene_output_file(sc);
        const int png_rc = have_display ? rt_write_png_rgb8(png, rgb8.data(), info.width, info.height)
                                        : rt_write_png(png, img.data(), info.width, info.height, total_spp, 0);
        if (png_rc != RT_OK) fprintf(stderr, "rtmi: PNG not written: %s\n", rt_last_error());
    }
    fprintf(stderr, "Program finish, cost: %f s\n", now_s() - t0);  // main.cu:519-520
    rt_scene_free(sc);
    return 0;
}
