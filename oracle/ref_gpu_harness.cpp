// ref_gpu_harness.cpp -- TEST INFRASTRUCTURE ONLY; builds into oracle/_ref/ (git-ignored).
//
// Compiles the HOST-COMPILABLE part of the reference's gpu-version as plain C++ -- camera.cuh, object.cuh (hittable_list, sphere,
// the three rects, cylinder and its transforms), material.cuh, texture.cuh and the text of ray_color -- from where the sources lie
// under $(REF); nothing is copied into this repository.  The Makefile passes the directory with -I, puts oracle/shim/ in front
// of it (cuda.h, curand_kernel.h and the two stb headers, written here from CUDA's public names) and cuts ray_color out of
// main.cu at build time, by pattern, into _ref/ref_gpu_ray_color.inc: main.cu as a whole needs a JSON library, kernels and a
// device.  What this gives and what it cannot:
//
//   * curandState is the hooked stream of one (seed; pixel, sample) (Philox4x32-10 block -> xorshift128, as ref_harness.cpp and
//     rt_oracle.c), curand_uniform its 24-bit uniform in [0, 1): cuRAND's generator and its (0, 1] are replaced, as rand() is for
//     the CPU reference.
//   * The sample loop of render() (main.cu:95-101) lives in a kernel that reads threadIdx, so refg_sample() STATES it: u, v from
//     (x + xi) / (W - 1), (y + xi) / (H - 1), camera::get_ray, ray_color.  Everything those four call is the reference's.
//   * gpu-version's random_in_unit_sphere draws from the positive octant only (vec3.cuh:135-136), this project follows the CPU
//     reference there: the streams part at the first lambertian or metal vertex, so whole paths are
//     compared on dielectric and diffuse_light alone.  refg_sample() refuses a scene with another material; refg_hit(), whose
//     records do not depend on the material, takes any.
//   * camera.cuh has the lens off (get_ray draws nothing): scenes with defocus_blur = false.  The background is the constant
//     colour render() is given; there is no sky gradient.
//   * math.h and stdlib.h are force-included (Makefile), so that sqrt, acos, atan2, sin, tan and abs of a float are the float
//     overloads, as they are for nvcc; the library behind them is the host's, not CUDA's.
//   * the scene is built with the reference's constructors, cylinders by rotate(axis, radians) then translate(offset), the unit
//     and order parser.hpp:423-440 gives our JSON.  Every object gets a material instance of its own, which is how the winner
//     of hittable_list::hit is known: rec.mat_ptr names it.  The instances are thin subclasses that count an event and then
//     call the reference's scatter(); they change nothing it computes.
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "camera.cuh"    // found through -I$(REF)/gpu-version; <cuda.h> & co. through -Ioracle/shim
#include "object.cuh"
#include "material.cuh"
#include "rtweekend.cuh"
#include "texture.cuh"
#include "color.cuh"

#include "ref_gpu_ray_color.inc"  // the text of ray_color, main.cu:17-70, cut out by the Makefile into _ref/

// ---- the hook -----------------------------------------------------------------
float curand_uniform(curandState *g) {
    uint32_t t = g->x ^ (g->x << 11);
    g->x = g->y, g->y = g->z, g->z = g->w;
    g->w = g->w ^ (g->w >> 19) ^ (t ^ (t >> 8));
    g->draws++;
    return (float)(g->w >> 8) * (1.0f / 16777216.0f);
}

namespace {
void hook_seed(curandState *g, uint64_t seed, uint32_t pixel, uint32_t sample) {
    uint32_t c0 = pixel, c1 = sample, c2 = 0, c3 = 0, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    g->x = c0, g->y = c1, g->z = c2, g->w = c3;
    if ((c0 | c1 | c2 | c3) == 0u) g->w = 0x9E3779B9u;
    g->draws = 0;
}

// what one sample did, counted by the material instances below
struct Tally {
    int scatters, dielectric, ended_by;
};
thread_local Tally g_tally;

struct counted_dielectric : dielectric {
    explicit counted_dielectric(float ir) : dielectric(ir) {}
    bool scatter(const ray &r_in, const hit_record &rec, color &attenuation, ray &scattered, curandState *state) const override {
        g_tally.scatters++, g_tally.dielectric++;
        return dielectric::scatter(r_in, rec, attenuation, scattered, state);
    }
};
struct counted_lambertian : lambertian {
    explicit counted_lambertian(mytexture *a) : lambertian(a) {}
    bool scatter(const ray &r_in, const hit_record &rec, color &attenuation, ray &scattered, curandState *state) const override {
        g_tally.scatters++;
        return lambertian::scatter(r_in, rec, attenuation, scattered, state);
    }
};
struct counted_metal : metal {
    counted_metal(const color &a, float f) : metal(a, f) {}
    bool scatter(const ray &r_in, const hit_record &rec, color &attenuation, ray &scattered, curandState *state) const override {
        const bool went_on = metal::scatter(r_in, rec, attenuation, scattered, state);
        if (went_on) g_tally.scatters++;
        return went_on;
    }
};
struct counted_light : diffuse_light {
    int index;
    counted_light(mytexture *a, int i) : diffuse_light(a), index(i) {}
    bool scatter(const ray &r_in, const hit_record &rec, color &attenuation, ray &scattered, curandState *state) const override {
        g_tally.ended_by = index;
        return diffuse_light::scatter(r_in, rec, attenuation, scattered, state);
    }
};

struct RefGpuScene {
    std::vector<hittable *> objects;
    std::vector<material *> mats;  // mats[i] belongs to objects[i] alone
    hittable_list list;
    hittable *list_ptr = &list;
    camera *cam = nullptr;
    color background{0, 0, 0};
    bool paths_ok = true;  // dielectric and diffuse_light only

    RefGpuScene() { relink(); }
    void relink() { list.objects = objects.data(), list.len = (int)objects.size(); }
};
}  // namespace

extern "C" {

// mat.type: 0 lambertian, 1 metal (albedo = c0), 2 dielectric, 3 diffuse_light; tex_type (lambertian, diffuse_light): 0 solid c0,
// 1 checker even = c0, odd = c1
struct refg_material {
    int type, tex_type;
    double c0[3], c1[3], fuzz, ir;
};

void *refg_scene_new(void) { return new RefGpuScene(); }

void refg_scene_free(void *h) {
    RefGpuScene *s = (RefGpuScene *)h;
    if (!s) return;
    delete s->cam;
    // objects, materials and textures are leaked on purpose: the reference's classes have no virtual destructors
    // (hittable.cuh:32) and the reference itself never frees them
    delete s;
}

void refg_scene_set_camera(void *h, const double lookfrom[3], const double lookat[3], const double vup[3], double vfov,
                           double aspect, double aperture, double focus_dist) {
    RefGpuScene *s = (RefGpuScene *)h;
    delete s->cam;
    s->cam = new camera(point3(lookfrom[0], lookfrom[1], lookfrom[2]), point3(lookat[0], lookat[1], lookat[2]),
                        vec3(vup[0], vup[1], vup[2]), vfov, aspect, aperture, focus_dist);
}

void refg_scene_set_background(void *h, const double rgb[3]) { ((RefGpuScene *)h)->background = color(rgb[0], rgb[1], rgb[2]); }

static material *make_material(RefGpuScene *s, const refg_material *m) {
    const int index = (int)s->objects.size();
    auto tex = [&]() -> mytexture * {
        if (m->tex_type == 0) return new solid_color(color(m->c0[0], m->c0[1], m->c0[2]));
        return new checker_texture(new solid_color(color(m->c0[0], m->c0[1], m->c0[2])),
                                   new solid_color(color(m->c1[0], m->c1[1], m->c1[2])));
    };
    if (m->tex_type != 0 && m->tex_type != 1) return nullptr;
    switch (m->type) {
    case 0: s->paths_ok = false; return new counted_lambertian(tex());
    case 1: s->paths_ok = false; return new counted_metal(color(m->c0[0], m->c0[1], m->c0[2]), m->fuzz);
    case 2: return new counted_dielectric(m->ir);
    case 3: return new counted_light(tex(), index);
    default: return nullptr;
    }
}

static int add(RefGpuScene *s, hittable *o, material *m) {
    s->objects.push_back(o);
    s->mats.push_back(m);
    s->relink();
    return (int)s->objects.size() - 1;
}

// each returns the object's list index, or -1 for a material the reference cannot express
int refg_scene_add_sphere(void *h, const double center[3], double radius, const refg_material *mat) {
    RefGpuScene *s = (RefGpuScene *)h;
    material *m = make_material(s, mat);
    if (!m) return -1;
    return add(s, new sphere(point3(center[0], center[1], center[2]), radius, m), m);
}

// axis 0: xy_rect(x0, x1, y0, y1, k), 1: xz_rect(x0, x1, z0, z1, k), 2: yz_rect(y0, y1, z0, z1, k)
int refg_scene_add_rect(void *h, int axis, double a0, double a1, double b0, double b1, double k, const refg_material *mat) {
    RefGpuScene *s = (RefGpuScene *)h;
    if (axis < 0 || axis > 2) return -1;
    material *m = make_material(s, mat);
    if (!m) return -1;
    hittable *o;
    if (axis == 0) o = new xy_rect(a0, a1, b0, b1, k, m);
    else if (axis == 1) o = new xz_rect(a0, a1, b0, b1, k, m);
    else o = new yz_rect(a0, a1, b0, b1, k, m);
    return add(s, o, m);
}

// cylinder(radius, zmin, zmax, m), then rotate(axis, radians) where has_rotate, then translate(offset) where has_translate
int refg_scene_add_cylinder(void *h, double radius, double zmin, double zmax, int has_rotate, const double axis[3], double radians,
                            int has_translate, const double offset[3], const refg_material *mat) {
    RefGpuScene *s = (RefGpuScene *)h;
    material *m = make_material(s, mat);
    if (!m) return -1;
    cylinder *c = new cylinder(radius, zmin, zmax, m);
    if (has_rotate) c->rotate(vec3(axis[0], axis[1], axis[2]), radians);
    if (has_translate) c->translate(vec3(offset[0], offset[1], offset[2]));
    return add(s, c, m);
}

int refg_scene_num_objects(void *h) { return (int)((RefGpuScene *)h)->objects.size(); }

// hittable_list::hit(r, 0.001, FLT_MAX, rec) of n rays.  rec9[i] = {t, p.xyz, normal.xyz, u, v}, front[i], index[i] = the
// winning list entry or -1 on a miss (the record is then left as it was given)
void refg_hit(void *h, int n, const float *origins, const float *dirs, float *rec9, int *front, int *index) {
    RefGpuScene *s = (RefGpuScene *)h;
    for (int i = 0; i < n; ++i) {
        const float *o = origins + 3 * i, *d = dirs + 3 * i;
        ray r(point3(o[0], o[1], o[2]), vec3(d[0], d[1], d[2]));
        hit_record got;
        index[i] = -1, front[i] = 0;
        if (!s->list.hit(r, 0.001, FLT_MAX, got)) continue;
        for (size_t k = 0; k < s->mats.size(); ++k)
            if (s->mats[k] == got.mat_ptr) index[i] = (int)k;
        float *q = rec9 + 9 * i;
        q[0] = got.t;
        q[1] = got.p.x(), q[2] = got.p.y(), q[3] = got.p.z();
        q[4] = got.normal.x(), q[5] = got.normal.y(), q[6] = got.normal.z();
        q[7] = got.u, q[8] = got.v;
        front[i] = got.front_face ? 1 : 0;
    }
}

// one sample of one pixel: the loop body of render() (main.cu:96-100) stated here, on the stream of (seed; pixel, sample).
// counters = {dielectric events, the list index of the light that ended the path or -1, cut at depth (0 / 1)}.  Returns the
// number of uniforms drawn, or -1 where the scene holds a material whose scattering this project does not take from gpu-version.
int refg_sample(void *h, uint64_t seed, int x, int y, int sample, int width, int height, int max_depth, float rgb[3],
                int counters[3]) {
    RefGpuScene *s = (RefGpuScene *)h;
    if (!s->cam || !s->paths_ok) return -1;
    curandState state;
    curandState *rng = &state;
    hook_seed(rng, seed, (uint32_t)(y * width + x), (uint32_t)sample);
    g_tally = {0, 0, -1};
    const float u = float(x + random_float(rng)) / (width - 1);  // fp32 sum, fp32 quotient, as main.cu:97-98
    const float v = float(y + random_float(rng)) / (height - 1);
    const ray first = s->cam->get_ray(u, v, rng);
    const color c = ray_color(first, s->background, &s->list_ptr, max_depth, rng);
    rgb[0] = c.x(), rgb[1] = c.y(), rgb[2] = c.z();
    if (counters) {
        counters[0] = g_tally.dielectric;
        counters[1] = g_tally.ended_by;
        counters[2] = (g_tally.ended_by < 0 && g_tally.scatters >= max_depth) ? 1 : 0;  // every scatter takes one off depth
    }
    return (int)state.draws;
}

// checker_texture::value at n points: out[i] = 1 where it returns the odd colour
void refg_checker(int n, const float *points, int *out) {
    static checker_texture *tex = new checker_texture(new solid_color(color(0, 0, 0)), new solid_color(color(1, 1, 1)));
    for (int i = 0; i < n; ++i)
        out[i] = tex->value(0.0f, 0.0f, point3(points[3 * i], points[3 * i + 1], points[3 * i + 2])).x() > 0.5f;
}

}  // extern "C"
