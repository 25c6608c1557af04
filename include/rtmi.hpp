// rtmi.hpp -- header-only C++ view of the C ABI (rtmi.h) with the reference's class names and
// constructor argument lists, so host code written against the reference's object model
// (gpu-version/{camera,object,material,texture}.cuh) builds a scene the same way:
//
//     rtmi::scene sc(400, 225, 100, 50);
//     sc.set_camera(rtmi::camera({-2,2,1}, {0,0,-1}, {0,1,0}, 20, 16.0f/9, 0.0f, 0.0f));
//     auto ground = rtmi::lambertian(rtmi::color(0.8f, 0.8f, 0.0f));
//     sc.add(rtmi::sphere({0,-100.5f,-1}, 100, ground));
//     auto tube = rtmi::cylinder(0.25f, -1, 1, rtmi::dielectric(1.5f));
//     tube.rotate({0,1,0}, 3.14159265f / 2);  tube.translate({0,0,0});       // object.cuh:225-231
//     sc.add(tube);
//     std::vector<float> image = sc.render();                                 // main.cu:505-513
//     rtmi::output_image(image, sc, "main.ppm");                              // main.cu:359-372
//
// Objects are value descriptors (no device pointers, no virtual calls); textures and materials
// are registered in the scene tables when the object that uses them is added.
#pragma once
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "rtmi.h"

namespace rtmi {

struct vec3 {  // vec3.cuh:9-79
    float e[3];
    vec3() : e{0, 0, 0} {}
    vec3(float x, float y, float z) : e{x, y, z} {}
    float x() const { return e[0]; }
    float y() const { return e[1]; }
    float z() const { return e[2]; }
};
using point3 = vec3;
using color = vec3;

struct error : std::runtime_error {
    int status;
    error(int st, const std::string &where)
        : std::runtime_error(where + ": " + rt_status_string(st) + ": " + rt_last_error()), status(st) {}
};

// ---- textures (texture.cuh) --------------------------------------------------------------
struct mytexture {
    int type = RT_TEX_SOLID;
    color c0, c1;
    // image texture (taichi-version/material.py:96-110, 137-144): rows x cols texels, R G B bytes
    int rows = 0, cols = 0;
    std::vector<uint8_t> rgb;
    std::vector<uint8_t> alpha;  // an alpha plane: rows x cols bytes, empty: none
    rt_noise noise{};  // noise texture: c0, c1 are its two colours
};
inline std::shared_ptr<mytexture> solid_color(color c) {  // texture.cuh:18-19
    auto t = std::make_shared<mytexture>();
    t->type = RT_TEX_SOLID, t->c0 = c, t->c1 = c;
    return t;
}
inline std::shared_ptr<mytexture> checker_texture(color even, color odd) {  // texture.cuh:40-42
    auto t = std::make_shared<mytexture>();
    t->type = RT_TEX_CHECKER, t->c0 = even, t->c1 = odd;
    return t;
}

inline std::shared_ptr<mytexture> image_texture(int rows, int cols, std::vector<uint8_t> rgb) {
    auto t = std::make_shared<mytexture>();
    t->type = RT_TEX_IMAGE, t->rows = rows, t->cols = cols, t->rgb = std::move(rgb);
    return t;
}

// an image with an alpha plane: rows x cols x 4 bytes R G B A; the plane serves as an alpha mask (alpha_masked)
inline std::shared_ptr<mytexture> image_texture_rgba(int rows, int cols, const std::vector<uint8_t> &rgba) {
    auto t = std::make_shared<mytexture>();
    t->type = RT_TEX_IMAGE, t->rows = rows, t->cols = cols;
    const size_t n = rgba.size() / 4;
    t->rgb.resize(3 * n), t->alpha.resize(n);
    for (size_t i = 0; i < n; ++i) {
        t->rgb[3 * i] = rgba[4 * i], t->rgb[3 * i + 1] = rgba[4 * i + 1], t->rgb[3 * i + 2] = rgba[4 * i + 2];
        t->alpha[i] = rgba[4 * i + 3];
    }
    return t;
}

// a procedural solid texture: c0 + s (c1 - c0) with s from fBm, turbulence or marble noise at the hit point
inline std::shared_ptr<mytexture> noise_texture(color c0, color c1, int style = RT_NOISE_STYLE_FBM, float scale = 1.0f, int octaves = 1,
                                                uint32_t seed = 0, int axis = 1, float distortion = 5.0f) {
    auto t = std::make_shared<mytexture>();
    t->type = RT_TEX_NOISE, t->c0 = c0, t->c1 = c1;
    t->noise.style = style, t->noise.octaves = octaves, t->noise.seed = seed, t->noise.axis = axis;
    t->noise.scale = scale, t->noise.distortion = distortion;
    return t;
}

// ---- materials (material.cuh) --------------------------------------------------------------
struct material {
    int type = RT_MAT_LAMBERTIAN;
    std::shared_ptr<mytexture> tex;  // lambertian albedo / diffuse_light emit
    color albedo;
    float fuzz = 0, ir = 1;
    std::shared_ptr<mytexture> bump;  // bump mapping: a noise texture as the height field, null: none
    float bump_strength = 0;
    std::shared_ptr<mytexture> normal_map;  // a tangent-space normal map: an image texture, null: none
    float normal_scale = 0;
    std::shared_ptr<mytexture> alpha;  // an alpha mask: an image texture with an alpha plane, null: none
    float alpha_cutoff = 0.5f;
    std::shared_ptr<mytexture> map;  // pbr: the metallic-roughness map (G scales the roughness, B the metalness), null: none
};
using material_ptr = std::shared_ptr<material>;
inline material_ptr lambertian(std::shared_ptr<mytexture> a) {  // material.cuh:34-35
    auto m = std::make_shared<material>();
    m->type = RT_MAT_LAMBERTIAN, m->tex = std::move(a);
    return m;
}
inline material_ptr lambertian(color a) { return lambertian(solid_color(a)); }  // material.cuh:31-32
inline material_ptr metal(color a, float f) {                                     // material.cuh:60-61
    auto m = std::make_shared<material>();
    m->type = RT_MAT_METAL, m->albedo = a, m->fuzz = f;
    return m;
}
// glossy materials: fuzz holds the roughness, albedo F0, ir the coat's index
inline material_ptr rough_metal(color f0, float roughness) {
    auto m = std::make_shared<material>();
    m->type = RT_MAT_ROUGH_METAL, m->albedo = f0, m->fuzz = roughness;
    return m;
}
inline material_ptr plastic(std::shared_ptr<mytexture> body, float ior = 1.5f, float roughness = 0.3f) {
    auto m = std::make_shared<material>();
    m->type = RT_MAT_PLASTIC, m->tex = std::move(body), m->ir = ior, m->fuzz = roughness;
    return m;
}
inline material_ptr plastic(color body, float ior = 1.5f, float roughness = 0.3f) { return plastic(solid_color(body), ior, roughness); }
// rough glass: ir the index, fuzz the roughness, albedo the absorption coefficient per unit length (0: clear)
inline material_ptr rough_glass(float ir = 1.5f, float roughness = 0.3f, color absorption = color(0, 0, 0)) {
    auto m = std::make_shared<material>();
    m->type = RT_MAT_ROUGH_GLASS, m->ir = ir, m->fuzz = roughness, m->albedo = absorption;
    return m;
}
// the metallic-roughness material: tex the base colour, albedo[0] the metallic factor, fuzz the roughness factor,
// ir the coat's index, map (optional) the metallic-roughness map
inline material_ptr pbr(std::shared_ptr<mytexture> base, float metallic = 0.0f, float roughness = 0.5f, float ior = 1.5f,
                        std::shared_ptr<mytexture> metallic_roughness = nullptr) {
    auto m = std::make_shared<material>();
    m->type = RT_MAT_PBR, m->tex = std::move(base), m->albedo = color(metallic, 0, 0), m->fuzz = roughness, m->ir = ior;
    m->map = std::move(metallic_roughness);
    return m;
}
inline material_ptr pbr(color base, float metallic = 0.0f, float roughness = 0.5f, float ior = 1.5f,
                        std::shared_ptr<mytexture> metallic_roughness = nullptr) {
    return pbr(solid_color(base), metallic, roughness, ior, std::move(metallic_roughness));
}
inline material_ptr dielectric(float index_of_refraction) {  // material.cuh:91-92
    auto m = std::make_shared<material>();
    m->type = RT_MAT_DIELECTRIC, m->ir = index_of_refraction;
    return m;
}
inline material_ptr diffuse_light(std::shared_ptr<mytexture> a) {  // material.cuh:163-164
    auto m = std::make_shared<material>();
    m->type = RT_MAT_DIFFUSE_LIGHT, m->tex = std::move(a);
    return m;
}
inline material_ptr diffuse_light(color c) { return diffuse_light(solid_color(c)); }  // material.cuh:166-167

// bump mapping: a copy of `m` whose shading normal is perturbed by the gradient of `height`'s scalar (a noise
// texture; only its height is used, not its colours) x `strength`.  Any material but diffuse_light.
inline material_ptr bumped(const material_ptr &m, std::shared_ptr<mytexture> height, float strength) {
    auto b = std::make_shared<material>(*m);
    b->bump = std::move(height), b->bump_strength = strength;
    return b;
}

// normal mapping: a copy of `m` whose shading normal is the texel of `map` (an image texture) read in the surface's
// tangent frame, its tangential part x `scale`.  Any material but diffuse_light, and not one that is bumped.
inline material_ptr normal_mapped(const material_ptr &m, std::shared_ptr<mytexture> map, float scale = 1.0f) {
    auto b = std::make_shared<material>(*m);
    b->normal_map = std::move(map), b->normal_scale = scale;
    return b;
}

// alpha cutouts: a copy of `m` with holes where the alpha byte of `mask` (an image texture with an alpha plane, which
// may be the material's own colour image) at the hit's (u, v) lies below ceil(255 x cutoff).  Any material but diffuse_light.
inline material_ptr alpha_masked(const material_ptr &m, std::shared_ptr<mytexture> mask, float cutoff = 0.5f) {
    auto b = std::make_shared<material>(*m);
    b->alpha = std::move(mask), b->alpha_cutoff = cutoff;
    return b;
}

// ---- participating media (include/rtmi.h: homogeneous media, isotropic or Henyey-Greenstein scattering) ------------
// constant_medium(boundary, density, albedo[, g]): the boundary is a sphere (centre, radius) or an axis-aligned box (min, max);
// g is the asymmetry of the phase function (0: isotropic)
struct constant_medium {
    rt_medium rec{};
    float g = 0.0f;
    constant_medium(point3 cen, float radius, float density, color albedo, float g_ = 0.0f) : g(g_) {
        rec.shape = RT_MEDIUM_SPHERE, rec.f[0] = cen.x(), rec.f[1] = cen.y(), rec.f[2] = cen.z(), rec.f[3] = radius;
        fill(density, albedo);
    }
    constant_medium(point3 bmin, point3 bmax, float density, color albedo, float g_ = 0.0f) : g(g_) {
        rec.shape = RT_MEDIUM_BOX, rec.f[0] = bmin.x(), rec.f[1] = bmin.y(), rec.f[2] = bmin.z();
        rec.f[3] = bmax.x(), rec.f[4] = bmax.y(), rec.f[5] = bmax.z();
        fill(density, albedo);
    }

private:
    void fill(float density, color albedo) {
        rec.density = density, rec.albedo[0] = albedo.x(), rec.albedo[1] = albedo.y(), rec.albedo[2] = albedo.z();
    }
};

// host evaluations of the device's phase function (include/rtmi.h: rt_phase_hg_sample, rt_phase_hg_eval)
inline vec3 phase_hg_sample(float g, vec3 dir, float u1, float u2) {
    vec3 out;
    const int rc = rt_phase_hg_sample(g, dir.e, u1, u2, out.e);
    if (rc != RT_OK) throw error(rc, "phase_hg_sample");
    return out;
}
inline float phase_hg_eval(float g, float cos_theta) { return rt_phase_hg_eval(g, cos_theta); }

// ---- motion blur (include/rtmi.h: moving spheres) ---------------------------------------------
// moving_sphere(center0, center1, radius, material): the centre goes from center0 to center1 over the shutter time of a sample
struct moving_sphere {
    point3 center0, center1;
    float radius;
    material_ptr mat;
    moving_sphere(point3 c0, point3 c1, float r, material_ptr m) : center0(c0), center1(c1), radius(r), mat(std::move(m)) {}
};

// ---- hittables (object.cuh) ------------------------------------------------------------------
struct hittable {
    int type = RT_PRIM_SPHERE;
    float f[6] = {0, 0, 0, 0, 0, 0};
    material_ptr mat;
    // triangle only (taichi-version/hittable.py:95-110): corners and their texture coordinates
    float v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, uv[6] = {0, 0, 0, 0, 0, 0};
    // ... and, for smooth shading, its three vertex normals (rt_scene_add_triangle_normals)
    bool has_normals = false;
    float n[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // cylinder only: rotate (axis, radians) then translate, as cylinder::rotate/translate compose
    bool has_rotate = false, has_translate = false;
    vec3 axis{0, 0, 1}, offset;
    float radians = 0;
    // (quad, box: is_box, and the same pair)
    bool is_box = false;
    void rotate(vec3 a, float rad) {  // object.cuh:225-227
        if ((type != RT_PRIM_CYLINDER && type != RT_PRIM_QUAD) || has_rotate || has_translate)
            throw std::logic_error("rotate: only once, on a cylinder, quad or box, before translate");
        has_rotate = true, axis = a, radians = rad;
    }
    void translate(vec3 o) {  // object.cuh:229-231
        if ((type != RT_PRIM_CYLINDER && type != RT_PRIM_QUAD) || has_translate)
            throw std::logic_error("translate: only once, on a cylinder, quad or box");
        has_translate = true, offset = o;
    }
};
inline hittable sphere(point3 cen, float r, material_ptr m) {  // object.cuh:44-45
    hittable h;
    h.type = RT_PRIM_SPHERE, h.f[0] = cen.x(), h.f[1] = cen.y(), h.f[2] = cen.z(), h.f[3] = r, h.mat = std::move(m);
    return h;
}
inline hittable make_rect(int type, float a0, float a1, float b0, float b1, float k, material_ptr m) {
    hittable h;
    h.type = type, h.f[0] = a0, h.f[1] = a1, h.f[2] = b0, h.f[3] = b1, h.f[4] = k, h.mat = std::move(m);
    return h;
}
inline hittable xy_rect(float x0, float x1, float y0, float y1, float k, material_ptr m) {  // object.cuh:100-103
    return make_rect(RT_PRIM_XY_RECT, x0, x1, y0, y1, k, std::move(m));
}
inline hittable xz_rect(float x0, float x1, float z0, float z1, float k, material_ptr m) {  // object.cuh:138-141
    return make_rect(RT_PRIM_XZ_RECT, x0, x1, z0, z1, k, std::move(m));
}
inline hittable yz_rect(float y0, float y1, float z0, float z1, float k, material_ptr m) {  // object.cuh:170-173
    return make_rect(RT_PRIM_YZ_RECT, y0, y1, z0, z1, k, std::move(m));
}
// Triangle(v1, v2, v3, u1, u2, u3, material), taichi-version/hittable.py:95-110 (u = texture coordinates, 2 each)
inline hittable triangle(point3 v1, point3 v2, point3 v3, material_ptr m, const float *u1 = nullptr, const float *u2 = nullptr,
                         const float *u3 = nullptr) {
    hittable h;
    h.type = RT_PRIM_TRIANGLE, h.mat = std::move(m);
    const point3 *c[3] = {&v1, &v2, &v3};
    const float *u[3] = {u1, u2, u3};
    for (int k = 0; k < 3; ++k) {
        h.v[3 * k] = c[k]->x(), h.v[3 * k + 1] = c[k]->y(), h.v[3 * k + 2] = c[k]->z();
        if (u[k]) h.uv[2 * k] = u[k][0], h.uv[2 * k + 1] = u[k][1];
    }
    return h;
}
// ... with the vertex normals n1, n2, n3 of smooth shading (rt_scene_add_triangle_normals)
inline hittable smooth_triangle(point3 v1, point3 v2, point3 v3, vec3 n1, vec3 n2, vec3 n3, material_ptr m, const float *u1 = nullptr,
                                const float *u2 = nullptr, const float *u3 = nullptr) {
    hittable h = triangle(v1, v2, v3, std::move(m), u1, u2, u3);
    const vec3 *n[3] = {&n1, &n2, &n3};
    h.has_normals = true;
    for (int k = 0; k < 3; ++k) h.n[3 * k] = n[k]->x(), h.n[3 * k + 1] = n[k]->y(), h.n[3 * k + 2] = n[k]->z();
    return h;
}
// quad(Q, u, v, material): the parallelogram Q, Q + u, Q + u + v, Q + v; rotate() / translate() as a cylinder's
inline hittable quad(point3 Q, vec3 u, vec3 v, material_ptr m) {
    hittable h;
    h.type = RT_PRIM_QUAD, h.mat = std::move(m);
    const vec3 *c[3] = {&Q, &u, &v};
    for (int k = 0; k < 3; ++k) h.v[3 * k] = c[k]->x(), h.v[3 * k + 1] = c[k]->y(), h.v[3 * k + 2] = c[k]->z();
    return h;
}
// box(min, max, material): six quads, normals outward; scene::add returns the id of the first
inline hittable box(point3 mn, point3 mx, material_ptr m) {
    hittable h = quad(mn, mx, vec3(), std::move(m));
    h.is_box = true;
    return h;
}
inline hittable cylinder(float radius, float zmin, float zmax, material_ptr m) {  // object.cuh:220-223
    hittable h;
    h.type = RT_PRIM_CYLINDER, h.f[0] = radius, h.f[1] = zmin, h.f[2] = zmax, h.mat = std::move(m);
    return h;
}

struct camera {  // camera.cuh:9-15
    point3 lookfrom, lookat;
    vec3 vup;
    float vfov, aspect_ratio, aperture, focus_dist;
    camera(point3 from, point3 at, vec3 up, float fov, float aspect, float ap, float focus)
        : lookfrom(from), lookat(at), vup(up), vfov(fov), aspect_ratio(aspect), aperture(ap), focus_dist(focus) {}
};

// ---- scene = parser.hpp:16-32 `struct scene` + hittable_list ------------------------------------
class scene {
public:
    scene(int width, int height, int samples_per_pixel, int max_depth)
        : s_(rt_scene_new(width, height, samples_per_pixel, max_depth)) {
        if (!s_) throw error(RT_ERR_ARG, "rt_scene_new");
    }
    explicit scene(const std::string &json_file) : s_(rt_scene_load_json(json_file.c_str())) {  // parse_scene
        if (!s_) throw error(RT_ERR_SCENE, "parse_scene(" + json_file + ")");
    }
    ~scene() { rt_scene_free(s_); }
    scene(const scene &) = delete;
    scene &operator=(const scene &) = delete;

    void set_background(color c, bool sky_gradient, bool defocus_blur = true) {
        check(rt_scene_set_background(s_, c.e, (sky_gradient ? RT_FLAG_SKY_GRADIENT : 0u) |
                                                   (defocus_blur ? RT_FLAG_DEFOCUS_BLUR : 0u)),
              "set_background");
    }
    void set_camera(const camera &c) {
        check(rt_scene_set_camera(s_, c.lookfrom.e, c.lookat.e, c.vup.e, c.vfov, c.aspect_ratio, c.aperture,
                                  c.focus_dist),
              "camera");
    }
    // a medium joins the scene's media list (not the hittable list) -> its id
    int add(const constant_medium &m) {
        const rt_medium &r = m.rec;
        const int id = r.shape == RT_MEDIUM_SPHERE ? rt_scene_add_medium_sphere(s_, r.f, r.f[3], r.density, r.albedo)
                                                   : rt_scene_add_medium_box(s_, r.f, r.f + 3, r.density, r.albedo);
        if (id < 0) throw error(-id, "add(constant_medium)");
        if (m.g != 0.0f) set_medium_phase(id, m.g);
        return id;
    }
    void set_medium_phase(int medium, float g) { check(rt_scene_set_medium_phase(s_, medium, g), "set_medium_phase"); }
    float medium_phase(int medium) const {
        float g = 0.0f;
        const int rc = rt_scene_get_medium_phase(s_, medium, &g);
        if (rc != RT_OK) throw error(rc, "medium_phase");
        return g;
    }
    std::vector<rt_medium> media() const {
        const int n = rt_scene_get_media(s_, nullptr, 0);
        if (n < 0) throw error(-n, "media");
        std::vector<rt_medium> out((size_t)n);
        if (n > 0) rt_scene_get_media(s_, out.data(), n);
        return out;
    }
    void clear_media() { check(rt_scene_clear_media(s_), "clear_media"); }
    // a moving sphere joins the scene's list of movers (not the hittable list) -> its id
    int add(const moving_sphere &m) {
        if (!m.mat) throw std::logic_error("moving_sphere without a material");
        const int id = rt_scene_add_moving_sphere(s_, m.center0.e, m.center1.e, m.radius, material_id(m.mat));
        if (id < 0) throw error(-id, "add(moving_sphere)");
        return id;
    }
    std::vector<rt_moving_sphere> moving_spheres() const {
        const int n = rt_scene_get_moving_spheres(s_, nullptr, 0);
        if (n < 0) throw error(-n, "moving_spheres");
        std::vector<rt_moving_sphere> out((size_t)n);
        if (n > 0) rt_scene_get_moving_spheres(s_, out.data(), n);
        return out;
    }
    void clear_moving_spheres() { check(rt_scene_clear_moving_spheres(s_), "clear_moving_spheres"); }
    // analytic lights (rt_scene_add_point_light ...): lights without geometry, sampled by light sampling alone -> index
    int point_light(point3 position, color intensity) {
        const int id = rt_scene_add_point_light(s_, position.e, intensity.e);
        if (id < 0) throw error(-id, "point_light");
        return id;
    }
    int spot_light(point3 position, vec3 direction, color intensity, float inner_deg, float outer_deg) {
        const int id = rt_scene_add_spot_light(s_, position.e, direction.e, intensity.e, inner_deg, outer_deg);
        if (id < 0) throw error(-id, "spot_light");
        return id;
    }
    int distant_light(vec3 direction_of_travel, color irradiance, float angular_radius_deg = 0.0f) {
        const int id = rt_scene_add_distant_light(s_, direction_of_travel.e, irradiance.e, angular_radius_deg);
        if (id < 0) throw error(-id, "distant_light");
        return id;
    }
    std::vector<rt_analytic_light> analytic_lights() const {
        const int n = rt_scene_get_analytic_lights(s_, nullptr, 0);
        if (n < 0) throw error(-n, "analytic_lights");
        std::vector<rt_analytic_light> out((size_t)n);
        if (n > 0) rt_scene_get_analytic_lights(s_, out.data(), n);
        return out;
    }
    void clear_analytic_lights() { check(rt_scene_clear_analytic_lights(s_), "clear_analytic_lights"); }
    // hittable_list::add
    int add(const hittable &h) {
        if (!h.mat) throw std::logic_error("hittable without a material");
        const int m = material_id(h.mat);
        int id;
        switch (h.type) {
        case RT_PRIM_SPHERE: id = rt_scene_add_sphere(s_, h.f, h.f[3], m); break;
        case RT_PRIM_TRIANGLE:
            id = h.has_normals ? rt_scene_add_triangle_normals(s_, h.v, h.v + 3, h.v + 6, h.n, h.n + 3, h.n + 6, h.uv, h.uv + 2, h.uv + 4, m)
                               : rt_scene_add_triangle(s_, h.v, h.v + 3, h.v + 6, h.uv, h.uv + 2, h.uv + 4, m);
            break;
        case RT_PRIM_QUAD: {
            const float deg = h.radians * 180.0f / 3.14159265358979323846f;
            const float *ax = h.has_rotate ? h.axis.e : nullptr, *off = h.has_translate ? h.offset.e : nullptr;
            id = h.is_box ? rt_scene_add_box(s_, h.v, h.v + 3, m, ax, deg, off) : rt_scene_add_quad(s_, h.v, h.v + 3, h.v + 6, m, ax, deg, off);
            break;
        }
        case RT_PRIM_CYLINDER: {
            const float deg = h.radians * 180.0f / 3.14159265358979323846f;
            id = rt_scene_add_cylinder(s_, h.f[0], h.f[1], h.f[2], m, h.has_rotate ? h.axis.e : nullptr, deg,
                                       h.has_translate ? h.offset.e : nullptr);
            break;
        }
        default: id = rt_scene_add_rect(s_, h.type - RT_PRIM_XY_RECT, h.f[0], h.f[1], h.f[2], h.f[3], h.f[4], m); break;
        }
        if (id < 0) throw error(-id, "add");
        return id;
    }
    // readobj + placement (taichi-version/main.py:23-41, 110-118): triangles added
    int add_obj(const std::string &path, const material_ptr &m, float scale = 1.0f, const float *matrix9 = nullptr,
                const float *translate3 = nullptr) {
        int n = rt_scene_add_obj(s_, path.c_str(), material_id(m), scale, matrix9, translate3);
        if (n < 0) throw error(-n, "add_obj");
        return n;
    }
    // ... with vertex normals (smooth shading): from the file's vn lines, or generated within a crease angle
    int add_obj(const std::string &path, const material_ptr &m, rt_mesh_normals normals, float crease_degrees = 180.0f, float scale = 1.0f,
                const float *matrix9 = nullptr, const float *translate3 = nullptr) {
        int n = rt_scene_add_obj_normals(s_, path.c_str(), material_id(m), scale, matrix9, translate3, normals, crease_degrees);
        if (n < 0) throw error(-n, "add_obj");
        return n;
    }
    void override_size(int w, int h, int spp, int depth) { check(rt_scene_override(s_, w, h, spp, depth), "override"); }

    // camera projections (rt_scene_set_projection): orthographic (p0 = height), panoramic (p0 = hfov, p1 = vfov,
    // degrees), fisheye (p0 = fov); kept by every other camera setter.  projection(): the type, and the parameters if asked for
    void set_projection(rt_projection_type type, float p0 = 0.0f, float p1 = 0.0f) {
        const float p[2] = {p0, p1};
        check(rt_scene_set_projection(s_, type, type == RT_PROJ_PERSPECTIVE ? nullptr : p), "set_projection");
    }
    rt_projection_type projection(float params[2] = nullptr) const {
        int type = 0;
        check(rt_scene_get_projection(s_, &type, params), "projection");
        return (rt_projection_type)type;
    }
    // the ray the kernels start at (s, t) for the lens sample (lx, ly), any projection (rt_camera_ray; no GPU needed); false:
    // no ray there (outside a fisheye's image circle)
    bool camera_ray(float s, float t, rt_ray &out, float lx = 0.0f, float ly = 0.0f) const {
        int valid = 0;
        check(rt_camera_ray(s_, s, t, lx, ly, &out, &valid), "camera_ray");
        return valid != 0;
    }

    // the beam table of the frame (rt_scene_tile_beams): 16 words per 8x8 tile of the whole frame, row-major,
    // {count, ids ...}, count 0xffff = the overflow mark; as the host computes it (no GPU needed), or -- on_device -- as device
    // opts->device builds it for its launches (rt_scene_tile_beams_device).  The two agree word for word
    std::vector<uint16_t> tile_beams(bool on_device = false, const rt_opts *opts = nullptr) const {
        const int n = on_device ? rt_scene_tile_beams_device(s_, opts, nullptr, 0) : rt_scene_tile_beams(s_, nullptr, 0);
        check(n < 0 ? -n : 0, "tile_beams");
        std::vector<uint16_t> out((size_t)n * 16);
        const int m = on_device ? rt_scene_tile_beams_device(s_, opts, out.data(), n) : rt_scene_tile_beams(s_, out.data(), n);
        check(m < 0 ? -m : 0, "tile_beams");
        return out;
    }

    // ray queries (rt_trace_hip): the renderer's closest-hit query for caller-supplied rays, one record per ray (prim -1: a
    // miss, RT_HIT_INVALID: the ray failed rt_ray_valid); occluded(): 1 where the closest-hit query would report a hit
    std::vector<rt_hit> trace(const std::vector<rt_ray> &rays, const rt_opts *opts = nullptr) const {
        std::vector<rt_hit> out(rays.size());
        check(rt_trace_hip(s_, opts, RT_TRACE_CLOSEST, rays.data(), rays.size(), out.data(), nullptr), "trace");
        return out;
    }
    std::vector<uint8_t> occluded(const std::vector<rt_ray> &rays, const rt_opts *opts = nullptr) const {
        std::vector<uint8_t> out(rays.size());
        check(rt_trace_hip(s_, opts, RT_TRACE_OCCLUDED, rays.data(), rays.size(), out.data(), nullptr), "occluded");
        return out;
    }

    rt_scene_info info() const {
        rt_scene_info i;
        check(rt_scene_get_info(s_, &i), "info");
        return i;
    }
    std::string to_json() const {
        std::string out(rt_scene_to_json(s_, nullptr, 0), '\0');
        rt_scene_to_json(s_, &out[0], out.size());
        out.resize(out.size() - 1);
        return out;
    }
    // render<<<>>> + synchronise + copy back, main.cu:505-513: W*H*3 sums, row 0 = bottom
    std::vector<float> render(const rt_opts *opts = nullptr, rt_stats *stats = nullptr) const {
        rt_opts o;
        if (opts) o = *opts;
        else rt_opts_default(&o);
        const rt_scene_info i = info();
        std::vector<float> img((size_t)rt_shard_rows(s_, &o) * i.width * 3);
        check(rt_render_hip(s_, &o, img.data(), stats), "render");
        return img;
    }
    // Russian roulette (4_0_path_tracing.py's p_RR): survival probability per bounce, 0 = off
    void set_russian_roulette(float p) { check(rt_scene_set_russian_roulette(s_, p), "set_russian_roulette"); }
    // light sampling: next-event estimation + MIS at lambertian and fuzzy-metal vertices (rt_scene_set_light_sampling)
    void set_light_sampling(bool on) { check(rt_scene_set_light_sampling(s_, on ? 1 : 0), "set_light_sampling"); }
    // mesh lights: emissive triangles join the emitters that light sampling samples (rt_scene_set_mesh_lights)
    void set_mesh_lights(bool on) { check(rt_scene_set_mesh_lights(s_, on ? 1 : 0), "set_mesh_lights"); }
    bool mesh_lights() const { return rt_scene_get_mesh_lights(s_) > 0; }
    // light sampling in participating media: medium vertices take light samples, shadow rays see the media (rt_scene_set_media_light_sampling)
    void set_media_light_sampling(bool on) { check(rt_scene_set_media_light_sampling(s_, on ? 1 : 0), "set_media_light_sampling"); }
    bool media_light_sampling() const { return rt_scene_get_media_light_sampling(s_) > 0; }
    // nested grid: overfull cells of the candidate grid get a sub-grid of their own (rt_scene_set_nested_grid)
    void set_nested_grid(bool on) { check(rt_scene_set_nested_grid(s_, on ? 1 : 0), "set_nested_grid"); }
    bool nested_grid() const { return rt_scene_get_nested_grid(s_) > 0; }
    // environment map: rows x cols x 3 floats in lat-long layout, or a .hdr / .pfm / .png / .ppm file (rt_scene_set_environment)
    void set_environment(int rows, int cols, const float *rgb, float scale = 1.0f, float rotate_deg = 0.0f) {
        check(rt_scene_set_environment(s_, rows, cols, rgb, scale, rotate_deg), "set_environment");
    }
    void set_environment(const std::string &path, float scale = 1.0f, float rotate_deg = 0.0f) {
        check(rt_scene_set_environment_file(s_, path.c_str(), scale, rotate_deg), "set_environment");
    }
    void clear_environment() { check(rt_scene_set_environment(s_, 0, 0, nullptr, 1.0f, 0.0f), "clear_environment"); }
    bool has_environment() const {
        int rows = 0;
        return rt_scene_get_environment(s_, &rows, nullptr, nullptr, nullptr, nullptr, 0) == RT_OK && rows > 0;
    }
    // progressive rendering: adds samples [first, first + count) to the caller's exact pixel sums
    // (resized and zeroed when empty) and returns the framebuffer of the updated sums
    std::vector<float> accumulate(std::vector<int64_t> &acc, int first, int count, const rt_opts *opts = nullptr,
                                  rt_stats *stats = nullptr) const {
        rt_opts o;
        if (opts) o = *opts;
        else rt_opts_default(&o);
        o.sample_first = first, o.sample_count = count;
        const rt_scene_info i = info();
        const size_t n = (size_t)rt_shard_rows(s_, &o) * i.width * 3;
        if (acc.empty()) acc.assign(n, 0);
        if (acc.size() != n) throw std::runtime_error("rtmi: accumulate: accumulator size does not match the shard");
        std::vector<float> img(n);
        check(rt_render_hip_accumulate(s_, &o, acc.data(), img.data(), stats), "accumulate");
        return img;
    }
    // adaptive sampling (rt_render_hip_adaptive): W*H*3 sums of each pixel's own spp_map[y*W + x] samples, row 0 = bottom
    std::vector<float> render_adaptive(const rt_adaptive &a, std::vector<int32_t> &spp_map, const rt_opts *opts = nullptr,
                                       rt_adaptive_stats *stats = nullptr) const {
        const rt_scene_info i = info();
        std::vector<float> img((size_t)i.width * i.height * 3);
        spp_map.assign((size_t)i.width * i.height, 0);
        check(rt_render_hip_adaptive(s_, opts, &a, img.data(), spp_map.data(), stats), "render_adaptive");
        return img;
    }
    // one first-hit feature pass (rt_render_hip_feature): local_rows*W*3 sums over the samples of `opts`
    std::vector<float> render_feature(rt_feature feature, const rt_opts *opts = nullptr, rt_stats *stats = nullptr) const {
        const rt_scene_info i = info();
        const int rows = opts ? rt_shard_rows(s_, opts) : i.height;
        if (rows < 0) throw error(-rows, "render_feature");
        std::vector<float> sum((size_t)rows * i.width * 3);
        check(rt_render_hip_feature(s_, opts, (int)feature, sum.data(), stats), "render_feature");
        return sum;
    }
    // the edge-avoiding filter on a whole frame of this scene (rt_denoise_hip); spp_map: the per-pixel counts of render_adaptive
    std::vector<float> denoise(const std::vector<float> &rgb_sum, int spp, const std::vector<float> &albedo_sum,
                               const std::vector<float> &normal_sum, const std::vector<float> &depth_sum, int feature_spp,
                               const rt_denoise *params = nullptr, const std::vector<int32_t> *spp_map = nullptr, int device = 0,
                               double *ms = nullptr) const {
        const rt_scene_info i = info();
        const size_t n = (size_t)i.width * i.height * 3;
        if (rgb_sum.size() != n || albedo_sum.size() != n || normal_sum.size() != n || depth_sum.size() != n ||
            (spp_map && spp_map->size() * 3 != n))
            throw error(RT_ERR_ARG, "denoise: buffer sizes");
        std::vector<float> out(n);
        check(rt_denoise_hip(i.width, i.height, rgb_sum.data(), spp, spp_map ? spp_map->data() : nullptr, albedo_sum.data(),
                             normal_sum.data(), depth_sum.data(), feature_spp, params, device, out.data(), ms), "denoise");
        return out;
    }
    // the display stage on a whole frame of this scene (rt_display_hip): exposure, bloom, tone curve -> the quantised bytes, rows
    // top to bottom, and -- if out_rgb != nullptr -- the display-referred linear colour (a sum over one sample)
    std::vector<uint8_t> display(const std::vector<float> &rgb_sum, int spp, const rt_display *params = nullptr,
                                 const std::vector<int32_t> *spp_map = nullptr, int device = 0, std::vector<float> *out_rgb = nullptr,
                                 rt_display_stats *stats = nullptr) const {
        const rt_scene_info i = info();
        const size_t n = (size_t)i.width * i.height * 3;
        if (rgb_sum.size() != n || (spp_map && spp_map->size() * 3 != n)) throw error(RT_ERR_ARG, "display: buffer sizes");
        std::vector<uint8_t> out8(n);
        if (out_rgb) out_rgb->resize(n);
        check(rt_display_hip(i.width, i.height, rgb_sum.data(), spp, spp_map ? spp_map->data() : nullptr, params, device,
                             out_rgb ? out_rgb->data() : nullptr, out8.data(), stats), "display");
        return out8;
    }
    // the metallic-roughness material: pbr() registers one and returns its descriptor; set_pbr_map() gives a
    // registered one another map (null: none); pbr_map() is the texture id of its map, or -1
    material_ptr pbr(std::shared_ptr<mytexture> base, float metallic = 0.0f, float roughness = 0.5f, float ior = 1.5f,
                     std::shared_ptr<mytexture> metallic_roughness = nullptr) {
        material_ptr m = rtmi::pbr(std::move(base), metallic, roughness, ior, std::move(metallic_roughness));
        material_id(m);
        return m;
    }
    void set_pbr_map(const material_ptr &m, std::shared_ptr<mytexture> metallic_roughness) {
        const int id = material_id(m);
        check(rt_scene_set_pbr_map(s_, id, metallic_roughness ? texture_id(metallic_roughness) : -1), "set_pbr_map");
        m->map = std::move(metallic_roughness);
    }
    int pbr_map(const material_ptr &m) {
        int t = -1;
        check(rt_scene_get_pbr_map(s_, material_id(m), &t), "pbr_map");
        return t;
    }
    rt_scene *handle() const { return s_; }

private:
    rt_scene *s_;
    // registered descriptors are kept alive so an address is never reused for another one
    std::vector<std::pair<material_ptr, int>> mats_;
    std::vector<std::pair<std::shared_ptr<mytexture>, int>> texs_;
    static void check(int st, const char *where) {
        if (st != RT_OK) throw error(st, where);
    }
    int add_image(const mytexture &t) {  // (an alpha plane, DESIGN 7v: through the RGBA call)
        if (t.alpha.empty()) return rt_scene_add_image_texture(s_, t.rows, t.cols, t.rgb.data());
        std::vector<uint8_t> rgba(t.alpha.size() * 4);
        for (size_t i = 0; i < t.alpha.size() && 3 * i + 2 < t.rgb.size(); ++i) {
            rgba[4 * i] = t.rgb[3 * i], rgba[4 * i + 1] = t.rgb[3 * i + 1], rgba[4 * i + 2] = t.rgb[3 * i + 2];
            rgba[4 * i + 3] = t.alpha[i];
        }
        return (size_t)t.rows * t.cols == t.alpha.size() ? rt_scene_add_image_texture_rgba(s_, t.rows, t.cols, rgba.data()) : -RT_ERR_ARG;
    }
    int texture_id(const std::shared_ptr<mytexture> &t) {
        for (auto &kv : texs_)
            if (kv.first == t) return kv.second;
        int id = t->type == RT_TEX_CHECKER ? rt_scene_add_checker(s_, t->c0.e, t->c1.e)
                 : t->type == RT_TEX_IMAGE ? add_image(*t)
                 : t->type == RT_TEX_NOISE ? rt_scene_add_noise_texture(s_, t->c0.e, t->c1.e, &t->noise)
                                           : rt_scene_add_solid_color(s_, t->c0.e);
        if (id < 0) throw error(-id, "texture");
        texs_.emplace_back(t, id);
        return id;
    }
    int material_id(const material_ptr &m) {
        for (auto &kv : mats_)
            if (kv.first == m) return kv.second;
        int id;
        switch (m->type) {
        case RT_MAT_LAMBERTIAN: id = rt_scene_add_lambertian(s_, texture_id(m->tex)); break;
        case RT_MAT_METAL: id = rt_scene_add_metal(s_, m->albedo.e, m->fuzz); break;
        case RT_MAT_DIELECTRIC: id = rt_scene_add_dielectric(s_, m->ir); break;
        case RT_MAT_ROUGH_METAL: id = rt_scene_add_rough_metal(s_, m->albedo.e, m->fuzz); break;
        case RT_MAT_PLASTIC: id = rt_scene_add_plastic(s_, texture_id(m->tex), m->ir, m->fuzz); break;
        case RT_MAT_ROUGH_GLASS: id = rt_scene_add_rough_glass(s_, m->ir, m->fuzz, m->albedo.e); break;
        case RT_MAT_PBR: id = rt_scene_add_pbr(s_, texture_id(m->tex), m->albedo.e[0], m->fuzz, m->ir); break;
        default: id = rt_scene_add_diffuse_light(s_, texture_id(m->tex)); break;
        }
        if (id < 0) throw error(-id, "material");
        if (m->bump) check(rt_scene_set_bump(s_, id, texture_id(m->bump), m->bump_strength), "bump");
        if (m->normal_map) check(rt_scene_set_normal_map(s_, id, texture_id(m->normal_map), m->normal_scale), "normal map");
        if (m->alpha) check(rt_scene_set_alpha(s_, id, texture_id(m->alpha), m->alpha_cutoff), "alpha mask");
        if (m->type == RT_MAT_PBR && m->map) check(rt_scene_set_pbr_map(s_, id, texture_id(m->map)), "pbr map");
        mats_.emplace_back(m, id);
        return id;
    }
};

// output_image(image, W, H, spp, filename), main.cu:359-372
inline void output_image(const std::vector<float> &image, const scene &sc, const std::string &filename) {
    const rt_scene_info i = sc.info();
    int st = rt_write_ppm(filename.c_str(), image.data(), i.width, i.height, i.samples_per_pixel);
    if (st != RT_OK) throw error(st, "output_image");
}

}  // namespace rtmi
