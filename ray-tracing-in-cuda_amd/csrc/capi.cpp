// C ABI glue (include/rtmi.h): scene I/O and building, table read-back, PPM output.
// The render entry points live in render_host.hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <new>
#include <sstream>
#include <string>
#include <vector>

#include "philox.h"
#include "rt_camera.h"
#include "rt_env.h"
#include "rt_media.h"
// (rt_phase.h stands on rt_glossy.h, whose square root in a device pass is the kernels' own (render_device.h): the device pass of
//  this file, which holds no kernel, leaves the header and the two bodies that evaluate it out)
#if !(defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__)
#define RT_CAPI_HOST_PASS 1
#include "rt_phase.h"
#endif
#include "rt_motion.h"
#include "rt_trace.h"
#include "scene.hpp"

using namespace rtmi;

namespace {

rt_scene *finish(rt_scene *s, int rc) {
    if (rc != RT_OK) {
        delete s;
        return nullptr;
    }
    return s;
}

bool bad_scene(const rt_scene *s, const char *fn) {
    if (!s) {
        set_error("%s: null scene", fn);
        return true;
    }
    return false;
}

}  // namespace

extern "C" {

int rt_abi_version(void) { return RTMI_ABI_VERSION; }

size_t rt_struct_size(int which) {
    switch (which) {
    case 0: return sizeof(rt_opts);
    case 1: return sizeof(rt_stats);
    case 2: return sizeof(rt_prim);
    case 3: return sizeof(rt_material);
    case 4: return sizeof(rt_texture);
    case 5: return sizeof(rt_camera);
    case 6: return sizeof(rt_scene_info);
    case 7: return sizeof(rt_table_info);
    case 8: return sizeof(rt_adaptive);
    case 9: return sizeof(rt_adaptive_stats);
    case 10: return sizeof(rt_nested_info);
    case 16: return sizeof(rt_denoise);  // (11 .. 15 stay 0: the next structs of the scene / render interface)
    case 17: return sizeof(rt_medium);
    case 18: return sizeof(rt_moving_sphere);
    case 19: return sizeof(rt_display);
    case 20: return sizeof(rt_display_stats);
    case 21: return sizeof(rt_ray);
    case 22: return sizeof(rt_hit);
    case 24: return sizeof(rt_noise);  // (23 stays 0)
    case 25: return sizeof(rt_analytic_light);
    default: return 0;
    }
}

const char *rt_last_error(void) { return get_error(); }

const char *rt_status_string(int status) {
    switch (status) {
    case RT_OK: return "ok";
    case RT_ERR_ARG: return "invalid argument";
    case RT_ERR_IO: return "I/O error";
    case RT_ERR_JSON: return "malformed JSON";
    case RT_ERR_SCENE: return "invalid scene";
    case RT_ERR_HIP: return "HIP runtime or device error";
    case RT_ERR_LIMIT: return "scene exceeds a kernel limit";
    default: return "unknown status";
    }
}

void rt_opts_default(rt_opts *o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->seed = 2023;
    o->tile_rows = 8;
    o->tile_stride = 1;
}

// ---- scene I/O ------------------------------------------------------------------
rt_scene *rt_scene_parse_json(const char *text, size_t len) {
    if (!text) {
        set_error("rt_scene_parse_json: null text");
        return nullptr;
    }
    rt_scene *s = new (std::nothrow) rt_scene();
    if (!s) {
        set_error("out of memory");
        return nullptr;
    }
    return finish(s, scene_from_json(text, len, s->s));
}

rt_scene *rt_scene_load_json(const char *path) {
    if (!path) {
        set_error("rt_scene_load_json: null path");
        return nullptr;
    }
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        set_error("cannot open scene file '%s'", path);
        return nullptr;
    }
    std::stringstream ss;
    ss << f.rdbuf();
    std::string text = ss.str();
    rt_scene *s = new (std::nothrow) rt_scene();
    if (!s) {
        set_error("out of memory");
        return nullptr;
    }
    // "file" entries of image textures and meshes are relative to the scene file
    std::string dir(path);
    const size_t slash = dir.find_last_of('/');
    dir = slash == std::string::npos ? std::string(".") : dir.substr(0, slash);
    return finish(s, scene_from_json(text.data(), text.size(), s->s, dir.c_str()));
}

rt_scene *rt_scene_rtiow(uint32_t seed, int width, int height, int spp, int max_depth) {
    rt_scene *s = new (std::nothrow) rt_scene();
    if (!s) {
        set_error("out of memory");
        return nullptr;
    }
    scene_rtiow(s->s, seed, width, height, spp, max_depth);
    return finish(s, scene_validate(s->s));
}

size_t rt_scene_to_json(const rt_scene *s, char *out, size_t cap) {
    if (bad_scene(s, "rt_scene_to_json")) return 0;
    std::string j = scene_to_json(s->s);
    if (out && cap) {
        size_t n = j.size() < cap - 1 ? j.size() : cap - 1;
        memcpy(out, j.data(), n);
        out[n] = 0;
    }
    return j.size() + 1;
}

void rt_scene_free(rt_scene *s) { delete s; }

// ---- building -------------------------------------------------------------------
rt_scene *rt_scene_new(int width, int height, int spp, int max_depth) {
    rt_scene *s = new (std::nothrow) rt_scene();
    if (!s) {
        set_error("out of memory");
        return nullptr;
    }
    s->s.width = width, s->s.height = height, s->s.spp = spp, s->s.max_depth = max_depth;
    s->s.flags = RT_FLAG_SKY_GRADIENT | RT_FLAG_DEFOCUS_BLUR;  // cmake-cpu-version semantics
    return s;
}

int rt_scene_set_light_sampling(rt_scene *s, int on) {
    if (bad_scene(s, "rt_scene_set_light_sampling")) return RT_ERR_ARG;
    s->s.light_sampling = on != 0;
    s->s.touch();
    return RT_OK;
}

int rt_scene_get_light_sampling(const rt_scene *s) {
    if (bad_scene(s, "rt_scene_get_light_sampling")) return -RT_ERR_ARG;
    return s->s.light_sampling ? 1 : 0;
}

int rt_scene_set_mesh_lights(rt_scene *s, int on) {
    if (bad_scene(s, "rt_scene_set_mesh_lights")) return RT_ERR_ARG;
    s->s.mesh_lights = on != 0;
    s->s.touch();
    return RT_OK;
}

int rt_scene_get_mesh_lights(const rt_scene *s) {
    if (bad_scene(s, "rt_scene_get_mesh_lights")) return -RT_ERR_ARG;
    return s->s.mesh_lights ? 1 : 0;
}

int rt_scene_set_media_light_sampling(rt_scene *s, int on) {
    if (bad_scene(s, "rt_scene_set_media_light_sampling")) return RT_ERR_ARG;
    s->s.media_light_sampling = on != 0;
    s->s.touch();
    return RT_OK;
}

int rt_scene_get_media_light_sampling(const rt_scene *s) {
    if (bad_scene(s, "rt_scene_get_media_light_sampling")) return -RT_ERR_ARG;
    return s->s.media_light_sampling ? 1 : 0;
}

int rt_scene_set_nested_grid(rt_scene *s, int on) {
    if (bad_scene(s, "rt_scene_set_nested_grid")) return RT_ERR_ARG;
    s->s.nested_grid = on != 0;
    s->s.touch();
    return RT_OK;
}

int rt_scene_get_nested_grid(const rt_scene *s) {
    if (bad_scene(s, "rt_scene_get_nested_grid")) return -RT_ERR_ARG;
    return s->s.nested_grid ? 1 : 0;
}

int rt_scene_get_lights(const rt_scene *s, rt_light *out, int cap) {
    if (bad_scene(s, "rt_scene_get_lights")) return -RT_ERR_ARG;
    const std::vector<SceneLight> lights = scene_lights(s->s);
    for (int i = 0; out && i < cap && i < (int)lights.size(); ++i) {
        const SceneLight &l = lights[(size_t)i];
        rt_light &o = out[i];
        o.prim = l.prim, o.shape = l.type, o.probability = (float)l.prob, o.area = (float)l.area;
        for (int c = 0; c < 3; ++c) o.emission[c] = l.even[c], o.emission_odd[c] = l.odd[c];
    }
    return (int)lights.size();
}

int rt_scene_set_russian_roulette(rt_scene *s, float p) {
    if (bad_scene(s, "rt_scene_set_russian_roulette")) return RT_ERR_ARG;
    if (!(p >= 0.0f && p <= 1.0f)) {
        set_error("rt_scene_set_russian_roulette: p = %g is not a probability", (double)p);
        return RT_ERR_ARG;
    }
    s->s.rr_p = p;
    s->s.touch();
    return RT_OK;
}

int rt_scene_set_background(rt_scene *s, const float rgb[3], uint32_t flags) {
    if (bad_scene(s, "rt_scene_set_background")) return RT_ERR_ARG;
    if (rgb) memcpy(s->s.background, rgb, 3 * sizeof(float));
    s->s.flags = flags & (RT_FLAG_SKY_GRADIENT | RT_FLAG_DEFOCUS_BLUR);
    s->s.touch();
    return RT_OK;
}

int rt_scene_set_camera(rt_scene *s, const float lookfrom[3], const float lookat[3], const float vup[3], float vfov,
                        float aspect, float aperture, float focus_dist) {
    if (bad_scene(s, "rt_scene_set_camera")) return RT_ERR_ARG;
    if (!lookfrom || !lookat || !vup) {
        set_error("rt_scene_set_camera: null vector");
        return RT_ERR_ARG;
    }
    CameraParams &c = s->s.cam;
    for (int i = 0; i < 3; ++i) c.lookfrom[i] = lookfrom[i], c.lookat[i] = lookat[i], c.vup[i] = vup[i];
    c.vfov = vfov;
    c.aspect = aspect > 0 ? (double)aspect : 0.0;
    c.aperture = aperture;
    c.focus_dist = focus_dist > 0 ? (double)focus_dist : 0.0;
    s->s.touch();
    return RT_OK;
}

// the projection: checked as a whole, stored beside the camera's parameters, which no other setter of them touches
int rt_scene_set_projection(rt_scene *s, int type, const float params[2]) {
    if (bad_scene(s, "rt_scene_set_projection")) return RT_ERR_ARG;
    double p[2] = {0.0, 0.0};
    if (params) p[0] = params[0], p[1] = params[1];
    else if (type == RT_PROJ_PANORAMIC) p[0] = 360.0, p[1] = 180.0;
    else if (type == RT_PROJ_FISHEYE) p[0] = 180.0;
    else if (type == RT_PROJ_ORTHOGRAPHIC) {
        set_error("rt_scene_set_projection: an orthographic projection needs params[0], its height");
        return RT_ERR_ARG;
    }
    if (!projection_ok(type, p, "rt_scene_set_projection")) return RT_ERR_ARG;
    CameraParams &c = s->s.cam;
    c.projection = type;
    c.proj[0] = type == RT_PROJ_PERSPECTIVE ? 0.0 : p[0];
    c.proj[1] = type == RT_PROJ_PANORAMIC ? p[1] : 0.0;
    s->s.touch();
    return RT_OK;
}

int rt_scene_get_projection(const rt_scene *s, int *type, float params[2]) {
    if (bad_scene(s, "rt_scene_get_projection")) return RT_ERR_ARG;
    if (type) *type = s->s.cam.projection;
    if (params) params[0] = (float)s->s.cam.proj[0], params[1] = (float)s->s.cam.proj[1];
    return RT_OK;
}

// the camera's ray on the host: the records the packer writes, through the text the kernels compile
int rt_camera_ray(const rt_scene *s, float sx, float t, float lx, float ly, rt_ray *out, int *valid) {
    if (bad_scene(s, "rt_camera_ray")) return RT_ERR_ARG;
    if (!out) {
        set_error("rt_camera_ray: null ray");
        return RT_ERR_ARG;
    }
    int rc = scene_validate(s->s);
    if (rc) return rc;
    struct V4 { float x, y, z, w; };
    float rec[6][3], lens_radius;
    camera_records(s->s, rec, &lens_radius);
    V4 c[6];
    for (int k = 0; k < 6; ++k) c[k] = V4{rec[k][0], rec[k][1], rec[k][2], 0.0f};
    float offx = 0.0f, offy = 0.0f, offz = 0.0f;
    if (s->s.flags & RT_FLAG_DEFOCUS_BLUR) camera_lens_offset(lens_radius, c[4], c[5], lx, ly, offx, offy, offz);
    bool seen = true;
    const int model = s->s.cam.projection;
    if (model == RT_PROJ_PERSPECTIVE)
        camera_ray_perspective(c[0], c[1], c[2], c[3], sx, t, offx, offy, offz, out->origin[0], out->origin[1], out->origin[2], out->dir[0],
                               out->dir[1], out->dir[2]);
    else
        seen = camera_ray(model, c[0], c[1], c[2], c[3], c[4], c[5], sx, t, offx, offy, offz, out->origin[0], out->origin[1], out->origin[2],
                          out->dir[0], out->dir[1], out->dir[2]);
    out->t_max = INFINITY, out->reserved = 0.0f;
    if (valid) *valid = seen ? 1 : 0;
    return RT_OK;
}

static int add_texture(rt_scene *s, int type, const float a[3], const float b[3]) {
    if (bad_scene(s, "rt_scene_add_texture")) return -RT_ERR_ARG;
    if (!a || !b) {
        set_error("texture colour is null");
        return -RT_ERR_ARG;
    }
    rt_texture t;
    memset(&t, 0, sizeof t);
    t.type = type;
    memcpy(t.c0, a, sizeof t.c0);
    memcpy(t.c1, b, sizeof t.c1);
    s->s.texs.push_back(t);
    s->s.touch();
    return (int)s->s.texs.size() - 1;
}
int rt_scene_add_solid_color(rt_scene *s, const float rgb[3]) { return add_texture(s, RT_TEX_SOLID, rgb, rgb); }
int rt_scene_add_checker(rt_scene *s, const float even[3], const float odd[3]) {
    return add_texture(s, RT_TEX_CHECKER, even, odd);
}

// a noise texture: the two colours in the texture record, the parameters beside the table
int rt_scene_add_noise_texture(rt_scene *s, const float c0[3], const float c1[3], const rt_noise *noise) {
    if (bad_scene(s, "rt_scene_add_noise_texture")) return -RT_ERR_ARG;
    if (!noise) {
        set_error("rt_scene_add_noise_texture: null parameters");
        return -RT_ERR_ARG;
    }
    return add_noise_texture(s->s, c0, c1, *noise, "rt_scene_add_noise_texture");
}

int rt_scene_get_noise(const rt_scene *s, int texture, rt_noise *out) {
    if (bad_scene(s, "rt_scene_get_noise")) return RT_ERR_ARG;
    if (!out) {
        set_error("rt_scene_get_noise: null output");
        return RT_ERR_ARG;
    }
    if (texture < 0 || texture >= (int)s->s.texs.size() || s->s.texs[texture].type != RT_TEX_NOISE || (size_t)texture >= s->s.noise.size()) {
        set_error("texture %d is not a noise texture", texture);
        return RT_ERR_ARG;
    }
    *out = s->s.noise[texture];
    return RT_OK;
}

static int add_material(rt_scene *s, int type, int tex, const float *albedo, float fuzz, float ir) {
    if (bad_scene(s, "rt_scene_add_material")) return -RT_ERR_ARG;
    if ((type == RT_MAT_LAMBERTIAN || type == RT_MAT_DIFFUSE_LIGHT) && (tex < 0 || tex >= (int)s->s.texs.size())) {
        set_error("material references texture %d (have %zu)", tex, s->s.texs.size());
        return -RT_ERR_SCENE;
    }
    rt_material m;
    memset(&m, 0, sizeof m);
    m.type = type;
    m.texture = tex;
    if (albedo) memcpy(m.albedo, albedo, sizeof m.albedo);
    m.fuzz = fuzz < 1 ? fuzz : 1;  // material.cuh:61
    m.ir = ir;
    s->s.mats.push_back(m);
    s->s.touch();
    return (int)s->s.mats.size() - 1;
}
int rt_scene_add_lambertian(rt_scene *s, int texture) { return add_material(s, RT_MAT_LAMBERTIAN, texture, nullptr, 0, 0); }
int rt_scene_add_metal(rt_scene *s, const float albedo[3], float fuzz) {
    if (!albedo) {
        set_error("metal albedo is null");
        return -RT_ERR_ARG;
    }
    return add_material(s, RT_MAT_METAL, -1, albedo, fuzz, 0);
}
// glossy materials: the record's fuzz holds the roughness, albedo is F0, ir the coat's index
static int add_glossy(rt_scene *s, const rt_material &m, const char *where) {
    if (bad_scene(s, where)) return -RT_ERR_ARG;
    if (!glossy_material_ok(m, s->s.texs.size(), where)) return -RT_ERR_ARG;
    s->s.mats.push_back(m);
    s->s.touch();
    return (int)s->s.mats.size() - 1;
}
int rt_scene_add_rough_metal(rt_scene *s, const float albedo[3], float roughness) {
    if (!albedo) {
        set_error("rt_scene_add_rough_metal: albedo is null");
        return -RT_ERR_ARG;
    }
    rt_material m;
    memset(&m, 0, sizeof m);
    m.type = RT_MAT_ROUGH_METAL, m.texture = -1, m.fuzz = roughness;
    memcpy(m.albedo, albedo, sizeof m.albedo);
    return add_glossy(s, m, "rt_scene_add_rough_metal");
}
int rt_scene_add_plastic(rt_scene *s, int texture, float ior, float roughness) {
    rt_material m;
    memset(&m, 0, sizeof m);
    m.type = RT_MAT_PLASTIC, m.texture = texture, m.ir = ior, m.fuzz = roughness;
    return add_glossy(s, m, "rt_scene_add_plastic");
}
// rough glass: ir the index, fuzz the roughness, albedo the absorption coefficient (NULL: clear)
int rt_scene_add_rough_glass(rt_scene *s, float ir, float roughness, const float absorption[3]) {
    rt_material m;
    memset(&m, 0, sizeof m);
    m.type = RT_MAT_ROUGH_GLASS, m.texture = -1, m.ir = ir, m.fuzz = roughness;
    if (absorption) memcpy(m.albedo, absorption, sizeof m.albedo);
    return add_glossy(s, m, "rt_scene_add_rough_glass");
}
// the metallic-roughness material: texture the base colour, albedo[0] the metallic factor, fuzz the roughness
// factor, ir the coat's index; its map lives beside the material table, as the bumps do
int rt_scene_add_pbr(rt_scene *s, int base_texture, float metallic, float roughness, float ior) {
    rt_material m;
    memset(&m, 0, sizeof m);
    m.type = RT_MAT_PBR, m.texture = base_texture, m.albedo[0] = metallic, m.fuzz = roughness, m.ir = ior;
    return add_glossy(s, m, "rt_scene_add_pbr");
}
int rt_scene_set_pbr_map(rt_scene *s, int material, int texture) {
    if (bad_scene(s, "rt_scene_set_pbr_map")) return RT_ERR_ARG;
    return set_pbr_map(s->s, material, texture, "rt_scene_set_pbr_map") ? RT_OK : RT_ERR_ARG;
}
int rt_scene_get_pbr_map(const rt_scene *s, int material, int *texture) {
    if (bad_scene(s, "rt_scene_get_pbr_map")) return RT_ERR_ARG;
    if (material < 0 || material >= (int)s->s.mats.size() || s->s.mats[(size_t)material].type != RT_MAT_PBR) {
        set_error("rt_scene_get_pbr_map: material %d is not a pbr material (have %zu materials)", material, s->s.mats.size());
        return RT_ERR_ARG;
    }
    if (texture) *texture = scene_pbr_map(s->s, material);
    return RT_OK;
}
int rt_scene_add_dielectric(rt_scene *s, float ir) { return add_material(s, RT_MAT_DIELECTRIC, -1, nullptr, 0, ir); }
int rt_scene_add_diffuse_light(rt_scene *s, int texture) {
    return add_material(s, RT_MAT_DIFFUSE_LIGHT, texture, nullptr, 0, 0);
}

// bump mapping: a side table beside the materials, as rt_noise is beside the textures
int rt_scene_set_bump(rt_scene *s, int material, int texture, float strength) {
    if (bad_scene(s, "rt_scene_set_bump")) return RT_ERR_ARG;
    return set_bump(s->s, material, texture, strength, "rt_scene_set_bump") ? RT_OK : RT_ERR_ARG;
}

int rt_scene_get_bump(const rt_scene *s, int material, int *texture, float *strength) {
    if (bad_scene(s, "rt_scene_get_bump")) return RT_ERR_ARG;
    if (material < 0 || material >= (int)s->s.mats.size()) {
        set_error("rt_scene_get_bump: unknown material %d (have %zu)", material, s->s.mats.size());
        return RT_ERR_ARG;
    }
    const SceneBump *b = scene_bump(s->s, material);
    if (texture) *texture = b ? b->texture : -1;
    if (strength) *strength = b ? b->strength : 0.0f;
    return RT_OK;
}

// normal maps: a side table beside the materials, as the bumps are
int rt_scene_set_normal_map(rt_scene *s, int material, int texture, float scale) {
    if (bad_scene(s, "rt_scene_set_normal_map")) return RT_ERR_ARG;
    return set_normal_map(s->s, material, texture, scale, "rt_scene_set_normal_map") ? RT_OK : RT_ERR_ARG;
}

int rt_scene_get_normal_map(const rt_scene *s, int material, int *texture, float *scale) {
    if (bad_scene(s, "rt_scene_get_normal_map")) return RT_ERR_ARG;
    if (material < 0 || material >= (int)s->s.mats.size()) {
        set_error("rt_scene_get_normal_map: unknown material %d (have %zu)", material, s->s.mats.size());
        return RT_ERR_ARG;
    }
    const SceneNormalMap *b = scene_normal_map(s->s, material);
    if (texture) *texture = b ? b->texture : -1;
    if (scale) *scale = b ? b->scale : 0.0f;
    return RT_OK;
}

// alpha masks: a side table beside the materials, as the bumps are
int rt_scene_set_alpha(rt_scene *s, int material, int texture, float cutoff) {
    if (bad_scene(s, "rt_scene_set_alpha")) return RT_ERR_ARG;
    return set_alpha(s->s, material, texture, cutoff, "rt_scene_set_alpha") ? RT_OK : RT_ERR_ARG;
}

int rt_scene_get_alpha(const rt_scene *s, int material, int *texture, float *cutoff) {
    if (bad_scene(s, "rt_scene_get_alpha")) return RT_ERR_ARG;
    if (material < 0 || material >= (int)s->s.mats.size()) {
        set_error("rt_scene_get_alpha: unknown material %d (have %zu)", material, s->s.mats.size());
        return RT_ERR_ARG;
    }
    const SceneAlpha *b = scene_alpha(s->s, material);
    if (texture) *texture = b ? b->texture : -1;
    if (cutoff) *cutoff = b ? b->cutoff : 0.0f;
    return RT_OK;
}

static bool bad_material(rt_scene *s, int material) {
    if (material < 0 || material >= (int)s->s.mats.size()) {
        set_error("object references material %d (have %zu)", material, s->s.mats.size());
        return true;
    }
    return false;
}

int rt_scene_add_sphere(rt_scene *s, const float center[3], float radius, int material) {
    if (bad_scene(s, "rt_scene_add_sphere")) return -RT_ERR_ARG;
    if (!center) {
        set_error("sphere center is null");
        return -RT_ERR_ARG;
    }
    if (bad_material(s, material)) return -RT_ERR_SCENE;
    if (radius == 0.0f) {
        set_error("sphere radius is zero");
        return -RT_ERR_SCENE;
    }
    rt_prim p;
    memset(&p, 0, sizeof p);
    p.type = RT_PRIM_SPHERE, p.material = material;
    p.f[0] = center[0], p.f[1] = center[1], p.f[2] = center[2], p.f[3] = radius;
    s->s.prims.push_back(p);
    s->s.xforms.emplace_back();
    s->s.touch();
    return (int)s->s.prims.size() - 1;
}

int rt_scene_add_image_texture(rt_scene *s, int rows, int cols, const uint8_t *rgb) {
    if (bad_scene(s, "rt_scene_add_image_texture")) return -RT_ERR_ARG;
    return add_image_texture(s->s, rows, cols, rgb, "");
}

// an image with an alpha plane: rows x cols x 4 bytes R G B A
int rt_scene_add_image_texture_rgba(rt_scene *s, int rows, int cols, const uint8_t *rgba) {
    if (bad_scene(s, "rt_scene_add_image_texture_rgba")) return -RT_ERR_ARG;
    if (rows < 1 || cols < 1 || rows > 16384 || cols > 16384 || !rgba) {
        set_error("image texture: rows and cols must be in 1..16384 and the pixels not null (got %d x %d)", rows, cols);
        return -RT_ERR_ARG;
    }
    const size_t n = (size_t)rows * cols;
    std::vector<uint8_t> rgb(n * 3), alpha(n);
    for (size_t i = 0; i < n; ++i) {
        rgb[3 * i] = rgba[4 * i], rgb[3 * i + 1] = rgba[4 * i + 1], rgb[3 * i + 2] = rgba[4 * i + 2];
        alpha[i] = rgba[4 * i + 3];
    }
    return add_image_texture(s->s, rows, cols, rgb.data(), "", alpha.data());
}

int rt_scene_add_image_texture_file(rt_scene *s, const char *path) {
    if (bad_scene(s, "rt_scene_add_image_texture_file")) return -RT_ERR_ARG;
    if (!path) {
        set_error("rt_scene_add_image_texture_file: null path");
        return -RT_ERR_ARG;
    }
    return add_image_texture_file(s->s, path);
}

int rt_scene_get_image(const rt_scene *s, int texture, int *rows, int *cols, uint8_t *out, size_t cap) {
    if (bad_scene(s, "rt_scene_get_image")) return -RT_ERR_ARG;
    if (texture < 0 || texture >= (int)s->s.texs.size() || s->s.texs[texture].type != RT_TEX_IMAGE) {
        set_error("texture %d is not an image texture", texture);
        return -RT_ERR_ARG;
    }
    const SceneImage &im = s->s.images[(size_t)s->s.texs[texture].c0[0]];
    if (rows) *rows = im.rows;
    if (cols) *cols = im.cols;
    if (out) {
        if (cap < im.rgb.size()) {
            set_error("rt_scene_get_image: buffer of %zu bytes, image needs %zu", cap, im.rgb.size());
            return -RT_ERR_ARG;
        }
        memcpy(out, im.rgb.data(), im.rgb.size());
    }
    return RT_OK;
}

int rt_scene_get_image_alpha(const rt_scene *s, int texture, int *rows, int *cols, uint8_t *out, size_t cap) {
    if (bad_scene(s, "rt_scene_get_image_alpha")) return -RT_ERR_ARG;
    if (texture < 0 || texture >= (int)s->s.texs.size() || s->s.texs[texture].type != RT_TEX_IMAGE) {
        set_error("texture %d is not an image texture", texture);
        return -RT_ERR_ARG;
    }
    const SceneImage &im = s->s.images[(size_t)s->s.texs[texture].c0[0]];
    if (rows) *rows = im.rows;
    if (cols) *cols = im.cols;
    if (out && !im.alpha.empty()) {
        if (cap < im.alpha.size()) {
            set_error("rt_scene_get_image_alpha: buffer of %zu bytes, the plane needs %zu", cap, im.alpha.size());
            return -RT_ERR_ARG;
        }
        memcpy(out, im.alpha.data(), im.alpha.size());
    }
    return im.alpha.empty() ? 0 : 1;
}

int rt_scene_add_triangle(rt_scene *s, const float v1[3], const float v2[3], const float v3[3], const float uv1[2],
                          const float uv2[2], const float uv3[2], int material) {
    if (bad_scene(s, "rt_scene_add_triangle")) return -RT_ERR_ARG;
    if (!v1 || !v2 || !v3) {
        set_error("triangle vertex is null");
        return -RT_ERR_ARG;
    }
    if (bad_material(s, material)) return -RT_ERR_SCENE;
    return add_triangle(s->s, v1, v2, v3, uv1, uv2, uv3, material);
}

int rt_scene_add_obj(rt_scene *s, const char *path, int material, float scale, const float matrix[9],
                     const float translate[3]) {
    if (bad_scene(s, "rt_scene_add_obj")) return -RT_ERR_ARG;
    if (!path) {
        set_error("rt_scene_add_obj: null path");
        return -RT_ERR_ARG;
    }
    if (bad_material(s, material)) return -RT_ERR_SCENE;
    return add_obj(s->s, path, material, scale, matrix, translate);
}

int rt_scene_add_triangle_normals(rt_scene *s, const float v1[3], const float v2[3], const float v3[3], const float n1[3],
                                  const float n2[3], const float n3[3], const float uv1[2], const float uv2[2], const float uv3[2],
                                  int material) {
    if (bad_scene(s, "rt_scene_add_triangle_normals")) return -RT_ERR_ARG;
    if (!v1 || !v2 || !v3) {
        set_error("triangle vertex is null");
        return -RT_ERR_ARG;
    }
    if (!n1 || !n2 || !n3) {
        set_error("triangle vertex normal is null");
        return -RT_ERR_ARG;
    }
    if (bad_material(s, material)) return -RT_ERR_SCENE;
    return add_triangle_normals(s->s, v1, v2, v3, n1, n2, n3, uv1, uv2, uv3, material);
}

int rt_scene_add_obj_normals(rt_scene *s, const char *path, int material, float scale, const float matrix[9],
                             const float translate[3], int mode, float crease_degrees) {
    if (bad_scene(s, "rt_scene_add_obj_normals")) return -RT_ERR_ARG;
    if (!path) {
        set_error("rt_scene_add_obj_normals: null path");
        return -RT_ERR_ARG;
    }
    if (bad_material(s, material)) return -RT_ERR_SCENE;
    return add_obj_normals(s->s, path, material, scale, matrix, translate, mode, crease_degrees);
}

void rt_set_mesh_normals_override(int mode, float crease_degrees) { set_mesh_normals_override(mode, crease_degrees); }

int rt_scene_add_rect(rt_scene *s, int axis, float a0, float a1, float b0, float b1, float k, int material) {
    if (bad_scene(s, "rt_scene_add_rect")) return -RT_ERR_ARG;
    if (axis < 0 || axis > 2) {
        set_error("rect axis must be 0 (xy), 1 (xz) or 2 (yz)");
        return -RT_ERR_ARG;
    }
    if (bad_material(s, material)) return -RT_ERR_SCENE;
    rt_prim p;
    memset(&p, 0, sizeof p);
    p.type = RT_PRIM_XY_RECT + axis, p.material = material;
    p.f[0] = a0, p.f[1] = a1, p.f[2] = b0, p.f[3] = b1, p.f[4] = k;
    s->s.prims.push_back(p);
    s->s.xforms.emplace_back();
    s->s.touch();
    return (int)s->s.prims.size() - 1;
}

int rt_scene_add_cylinder(rt_scene *s, float radius, float zmin, float zmax, int material, const float rot_axis[3],
                          float rot_degrees, const float translate[3]) {
    if (bad_scene(s, "rt_scene_add_cylinder")) return -RT_ERR_ARG;
    if (bad_material(s, material)) return -RT_ERR_SCENE;
    double ax[3], off[3];
    if (rot_axis)
        for (int i = 0; i < 3; ++i) ax[i] = rot_axis[i];
    if (translate)
        for (int i = 0; i < 3; ++i) off[i] = translate[i];
    return add_cylinder(s->s, radius, zmin, zmax, material, rot_axis ? ax : nullptr, rot_degrees,
                        translate ? off : nullptr);
}

int rt_scene_add_quad(rt_scene *s, const float q[3], const float u[3], const float v[3], int material, const float rot_axis[3],
                      float rot_degrees, const float translate[3]) {
    if (bad_scene(s, "rt_scene_add_quad")) return -RT_ERR_ARG;
    if (!q || !u || !v) {
        set_error("quad corner or edge is null");
        return -RT_ERR_ARG;
    }
    if (bad_material(s, material)) return -RT_ERR_SCENE;
    double ax[3], off[3];
    if (rot_axis)
        for (int i = 0; i < 3; ++i) ax[i] = rot_axis[i];
    if (translate)
        for (int i = 0; i < 3; ++i) off[i] = translate[i];
    return add_quad(s->s, q, u, v, material, rot_axis ? ax : nullptr, rot_degrees, translate ? off : nullptr);
}

int rt_scene_add_box(rt_scene *s, const float min[3], const float max[3], int material, const float rot_axis[3], float rot_degrees,
                     const float translate[3]) {
    if (bad_scene(s, "rt_scene_add_box")) return -RT_ERR_ARG;
    if (!min || !max) {
        set_error("box min or max is null");
        return -RT_ERR_ARG;
    }
    if (bad_material(s, material)) return -RT_ERR_SCENE;
    double ax[3], off[3];
    if (rot_axis)
        for (int i = 0; i < 3; ++i) ax[i] = rot_axis[i];
    if (translate)
        for (int i = 0; i < 3; ++i) off[i] = translate[i];
    return add_box(s->s, min, max, material, rot_axis ? ax : nullptr, rot_degrees, translate ? off : nullptr);
}

// ---- animation ---------------------------------------------------------------------------
rt_scene *rt_scene_clone(const rt_scene *src) {
    if (bad_scene(src, "rt_scene_clone")) return nullptr;
    rt_scene *s = new (std::nothrow) rt_scene();
    if (!s) {
        set_error("out of memory");
        return nullptr;
    }
    s->s = src->s;
    s->s.dev.reset();  // device residency is per scene object
    s->s.touch();
    return s;
}

int rt_scene_set_output_file(rt_scene *s, const char *path) {
    if (bad_scene(s, "rt_scene_set_output_file") || !path) return RT_ERR_ARG;
    s->s.output_file = path;
    return RT_OK;
}

int rt_scene_rotate_cylinders(rt_scene *s, double degrees) {
    if (bad_scene(s, "rt_scene_rotate_cylinders")) return -RT_ERR_ARG;
    Scene &sc = s->s;
    int changed = 0;
    for (size_t i = 0; i < sc.prims.size(); ++i) {
        if (sc.prims[i].type != RT_PRIM_CYLINDER || !sc.xforms[i].has_rotate) continue;
        CylinderXform xf = sc.xforms[i];
        xf.degrees += degrees;
        // rebuild through the same path the parser uses (parser.hpp:423-440)
        Scene tmp;
        tmp.mats.resize(sc.mats.size());
        int rc = add_cylinder(tmp, sc.prims[i].f[0], sc.prims[i].f[1], sc.prims[i].f[2], sc.prims[i].material, xf.axis,
                              xf.degrees, xf.has_translate ? xf.offset : nullptr);
        if (rc < 0) return rc;
        sc.prims[i] = tmp.prims[0];
        sc.xforms[i] = tmp.xforms[0];
        ++changed;
    }
    sc.touch();
    return changed;
}

rt_scene *rt_scene_dna(const rt_scene *base, double angle) {
    rt_scene *s = new (std::nothrow) rt_scene();
    if (!s) {
        set_error("out of memory");
        return nullptr;
    }
    Scene &sc = s->s;
    if (base) {
        sc = base->s;
        sc.dev.reset();
        sc.prims.clear(), sc.xforms.clear(), sc.mats.clear(), sc.texs.clear(), sc.noise.clear(), sc.bumps.clear(), sc.pbr_maps.clear(), sc.normal_maps.clear(), sc.alphas.clear();
    } else {  // gpu-version/basic_scene.json
        sc.width = 1600, sc.height = 900, sc.spp = 100, sc.max_depth = 50;
        sc.background[0] = 0.0005f, sc.background[1] = 0.0007f, sc.background[2] = 0.00099f;
        sc.flags = 0;  // constant background, no lens sampling: what gpu-version renders from that file
        sc.cam = CameraParams();
        sc.cam.lookfrom[0] = 0, sc.cam.lookfrom[1] = 0, sc.cam.lookfrom[2] = -20;
        sc.cam.vfov = 23, sc.cam.aperture = 0.1;
    }
    const double pi = std::acos(-1.0);
    const int num_object = 5;
    const double space = 5;
    // dna.py:29-53: three solid colours and three diffuse_light materials per i in range(-15, 15)
    for (int i = 0; i < num_object * 6; ++i) {
        const double cols[3][3] = {{232 / 256.0, 209 / 256.0, 209 / 256.0},
                                   {232 / 256.0, 209 / 256.0, 209 / 256.0},
                                   {202 / 256.0, 202 / 256.0, 224 / 256.0}};
        for (int k = 0; k < 3; ++k) {
            rt_texture t;
            memset(&t, 0, sizeof t);
            t.type = RT_TEX_SOLID;
            for (int c = 0; c < 3; ++c) t.c0[c] = t.c1[c] = (float)cols[k][c];
            sc.texs.push_back(t);
        }
        for (int k = 0; k < 3; ++k) {
            rt_material m;
            memset(&m, 0, sizeof m);
            m.type = RT_MAT_DIFFUSE_LIGHT;
            m.texture = i * 3 + k;
            sc.mats.push_back(m);
        }
    }
    // dna.py:55-84
    for (int offset = 0; offset < 3; ++offset) {
        for (int i = 0; i < 2 * num_object; ++i) {
            const int id = i - num_object;
            const double theta = (36.0 * (id + num_object) + angle) / 180.0 * pi;
            const double xoffset = offset * space - space;
            const double zoffset = std::fabs(offset - 1.0) * -20 + 20;
            auto add_sphere = [&](double th, int mat) {
                rt_prim p;
                memset(&p, 0, sizeof p);
                p.type = RT_PRIM_SPHERE, p.material = mat;
                p.f[0] = (float)(2.5 * std::cos(th) + xoffset), p.f[1] = (float)id;
                p.f[2] = (float)(2.5 * std::sin(th) + zoffset), p.f[3] = 0.5f;
                sc.prims.push_back(p);
                sc.xforms.emplace_back();
            };
            add_sphere(theta, i * 3 + 0);
            add_sphere(theta + pi, i * 3 + 1);
            const double axis[3] = {0, 1, 0}, off[3] = {xoffset, (double)id, zoffset};
            int rc = add_cylinder(sc, 0.3f, -2.18f, 2.18f, i * 3 + 2, axis, 36.0 * -(id + num_object) + 90 + angle, off);
            if (rc < 0) return finish(s, RT_ERR_SCENE);
        }
    }
    sc.touch();
    return finish(s, scene_validate(sc));
}

int rt_scene_override(rt_scene *s, int width, int height, int spp, int max_depth) {
    if (bad_scene(s, "rt_scene_override")) return RT_ERR_ARG;
    int w = s->s.width, h = s->s.height, p = s->s.spp, d = s->s.max_depth;
    if (width > 0) s->s.width = width;
    if (height > 0) s->s.height = height;
    if (spp > 0) s->s.spp = spp;
    if (max_depth > 0) s->s.max_depth = max_depth;
    int rc = scene_validate(s->s);
    if (rc != RT_OK) s->s.width = w, s->s.height = h, s->s.spp = p, s->s.max_depth = d;
    s->s.touch();
    return rc;
}

// ---- read-back --------------------------------------------------------------------
int rt_scene_get_info(const rt_scene *s, rt_scene_info *out) {
    if (bad_scene(s, "rt_scene_get_info") || !out) return RT_ERR_ARG;
    out->width = s->s.width, out->height = s->s.height;
    out->samples_per_pixel = s->s.spp, out->max_depth = s->s.max_depth;
    out->num_prims = (int)s->s.prims.size();
    out->num_materials = (int)s->s.mats.size();
    out->num_textures = (int)s->s.texs.size();
    out->flags = s->s.flags;
    memcpy(out->background, s->s.background, sizeof out->background);
    out->russian_roulette = s->s.rr_p;
    return RT_OK;
}

int rt_scene_get_camera(const rt_scene *s, rt_camera *out) {
    if (bad_scene(s, "rt_scene_get_camera") || !out) return RT_ERR_ARG;
    derive_camera(s->s, out);
    return RT_OK;
}

int rt_scene_get_prims(const rt_scene *s, rt_prim *out, int cap) {
    if (bad_scene(s, "rt_scene_get_prims")) return -RT_ERR_ARG;
    int n = (int)s->s.prims.size();
    if (out)
        for (int i = 0; i < n && i < cap; ++i) out[i] = s->s.prims[i];
    return n;
}
int rt_scene_get_materials(const rt_scene *s, rt_material *out, int cap) {
    if (bad_scene(s, "rt_scene_get_materials")) return -RT_ERR_ARG;
    int n = (int)s->s.mats.size();
    if (out)
        for (int i = 0; i < n && i < cap; ++i) out[i] = s->s.mats[i];
    return n;
}
int rt_scene_get_textures(const rt_scene *s, rt_texture *out, int cap) {
    if (bad_scene(s, "rt_scene_get_textures")) return -RT_ERR_ARG;
    int n = (int)s->s.texs.size();
    if (out)
        for (int i = 0; i < n && i < cap; ++i) out[i] = s->s.texs[i];
    return n;
}

const char *rt_scene_output_file(const rt_scene *s) { return s ? s->s.output_file.c_str() : ""; }

// ---- output -------------------------------------------------------------------------
// write_color(FILE*, color, spp), gpu-version/color.cuh:70-95: fp32 throughout
static inline int quantize(float sum, int spp, int gamma) {
    float v;
    if (gamma) {
        float scale = 1.0f / (float)spp;
        v = std::sqrt(sum * scale);
    } else {
        v = sum / (float)spp;  // write_image, color.cuh:24-26
    }
    if (!(v == v)) return 0;  // NaN: the reference's cast is undefined; write black
    if (v < 0.0f) v = 0.0f;
    if (v > 0.999f) v = 0.999f;
    return (int)(256.0f * v);
}

void rt_acc_to_rgb(const int64_t *acc, float *rgb_sum, size_t n_values) {
    if (!acc || !rgb_sum) return;
    // same expression as the device's finalize step (render_kernel.hip): exact in double, one rounding to float
    for (size_t i = 0; i < n_values; ++i) rgb_sum[i] = (float)((double)acc[i] * (1.0 / 16777216.0));
}

int rt_quantize_rgb8(const float *rgb_sum, int width, int height, int spp, int gamma, uint8_t *out) {
    if (!rgb_sum || !out || width <= 0 || height <= 0 || spp <= 0) {
        set_error("rt_quantize_rgb8: bad argument");
        return RT_ERR_ARG;
    }
    size_t k = 0;
    for (int j = height - 1; j >= 0; --j)
        for (int i = 0; i < width; ++i)
            for (int c = 0; c < 3; ++c) out[k++] = (uint8_t)quantize(rgb_sum[((size_t)j * width + i) * 3 + c], spp, gamma);
    return RT_OK;
}

// the P3 text of bytes that are already quantised, rows top to bottom
int rt_write_ppm_rgb8(const char *path, const uint8_t *rgb8, int width, int height) {
    if (!path || !rgb8 || width <= 0 || height <= 0) {
        set_error("rt_write_ppm_rgb8: bad argument");
        return RT_ERR_ARG;
    }
    FILE *fp = fopen(path, "w");
    if (!fp) {
        set_error("cannot open '%s' for writing", path);
        return RT_ERR_IO;
    }
    std::string buf;
    buf.reserve((size_t)width * 12 + 64);
    fprintf(fp, "P3\n%d %d\n255\n", width, height);  // main.cu:363
    char line[48];
    for (int j = 0; j < height; ++j) {
        buf.clear();
        for (int i = 0; i < width; ++i) {
            const uint8_t *p = rgb8 + ((size_t)j * width + i) * 3;
            int n = snprintf(line, sizeof line, "%d %d %d\n", p[0], p[1], p[2]);
            buf.append(line, (size_t)n);
        }
        if (fwrite(buf.data(), 1, buf.size(), fp) != buf.size()) {
            fclose(fp);
            set_error("short write to '%s'", path);
            return RT_ERR_IO;
        }
    }
    if (fclose(fp) != 0) {
        set_error("error closing '%s'", path);
        return RT_ERR_IO;
    }
    return RT_OK;
}

int rt_write_ppm(const char *path, const float *rgb_sum, int width, int height, int spp) {
    if (!path || !rgb_sum || width <= 0 || height <= 0 || spp <= 0) {
        set_error("rt_write_ppm: bad argument");
        return RT_ERR_ARG;
    }
    std::vector<uint8_t> rgb8((size_t)width * height * 3);
    rt_quantize_rgb8(rgb_sum, width, height, spp, 1, rgb8.data());
    return rt_write_ppm_rgb8(path, rgb8.data(), width, height);
}

// write_image(), gpu-version/color.cuh:15-35: 8-bit RGB PNG of the LINEAR means (no gamma), rows top
// to bottom.  The reference encodes with stb_image_write; here a minimal encoder (zlib "stored"
// blocks, no compression) keeps the library dependency-free.  gamma != 0 applies write_color's sqrt.
namespace {
uint32_t crc32_update(uint32_t crc, const uint8_t *p, size_t n) {
    static uint32_t table[256];
    static bool init = false;
    if (!init) {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
        init = true;
    }
    for (size_t i = 0; i < n; ++i) crc = table[(crc ^ p[i]) & 0xFF] ^ (crc >> 8);
    return crc;
}
void put_be32(std::string &o, uint32_t v) {
    o.push_back((char)(v >> 24)), o.push_back((char)(v >> 16)), o.push_back((char)(v >> 8)), o.push_back((char)v);
}
void put_chunk(std::string &png, const char type[4], const std::string &data) {
    put_be32(png, (uint32_t)data.size());
    std::string body(type, 4);
    body += data;
    png += body;
    put_be32(png, crc32_update(0xFFFFFFFFu, (const uint8_t *)body.data(), body.size()) ^ 0xFFFFFFFFu);
}
}  // namespace

int rt_write_png(const char *path, const float *rgb_sum, int width, int height, int spp, int gamma) {
    if (!path || !rgb_sum || width <= 0 || height <= 0 || spp <= 0) {
        set_error("rt_write_png: bad argument");
        return RT_ERR_ARG;
    }
    std::vector<uint8_t> rgb8((size_t)width * height * 3);
    rt_quantize_rgb8(rgb_sum, width, height, spp, gamma, rgb8.data());
    return rt_write_png_rgb8(path, rgb8.data(), width, height);
}

// the encoder: bytes that are already quantised, rows top to bottom
int rt_write_png_rgb8(const char *path, const uint8_t *rgb8, int width, int height) {
    if (!path || !rgb8 || width <= 0 || height <= 0) {
        set_error("rt_write_png_rgb8: bad argument");
        return RT_ERR_ARG;
    }
    // raw scanlines: filter byte 0 + RGB bytes, top row first
    std::string raw;
    raw.reserve((size_t)height * ((size_t)width * 3 + 1));
    for (int j = 0; j < height; ++j) {
        raw.push_back(0);
        raw.append((const char *)rgb8 + (size_t)j * width * 3, (size_t)width * 3);
    }
    std::string z;
    z.push_back(0x78), z.push_back(0x01);  // zlib header, no preset dictionary
    uint32_t a = 1, b = 0;                 // adler32
    for (unsigned char ch : raw) a = (a + ch) % 65521u, b = (b + a) % 65521u;
    size_t pos = 0;
    do {
        size_t n = raw.size() - pos < 65535 ? raw.size() - pos : 65535;
        z.push_back(pos + n == raw.size() ? 1 : 0);  // BFINAL, BTYPE = 00 (stored)
        z.push_back((char)(n & 0xFF)), z.push_back((char)(n >> 8));
        z.push_back((char)(~n & 0xFF)), z.push_back((char)((~n >> 8) & 0xFF));
        z.append(raw, pos, n);
        pos += n;
    } while (pos < raw.size());
    put_be32(z, (b << 16) | a);
    std::string png("\x89PNG\r\n\x1a\n", 8);
    std::string ihdr;
    put_be32(ihdr, (uint32_t)width), put_be32(ihdr, (uint32_t)height);
    ihdr.push_back(8), ihdr.push_back(2), ihdr.push_back(0), ihdr.push_back(0), ihdr.push_back(0);  // 8-bit RGB
    put_chunk(png, "IHDR", ihdr);
    put_chunk(png, "IDAT", z);
    put_chunk(png, "IEND", std::string());
    FILE *fp = fopen(path, "wb");
    if (!fp) {
        set_error("cannot open '%s' for writing", path);
        return RT_ERR_IO;
    }
    bool ok = fwrite(png.data(), 1, png.size(), fp) == png.size();
    ok = (fclose(fp) == 0) && ok;
    if (!ok) {
        set_error("short write to '%s'", path);
        return RT_ERR_IO;
    }
    return RT_OK;
}

// ---- float image files of the mean image (scene-referred: what the environment readers of env_read.hpp take back) ----
static int write_file(const char *path, const std::string &data) {
    FILE *fp = fopen(path, "wb");
    if (!fp) {
        set_error("cannot open '%s' for writing", path);
        return RT_ERR_IO;
    }
    bool ok = fwrite(data.data(), 1, data.size(), fp) == data.size();
    ok = (fclose(fp) == 0) && ok;
    if (!ok) {
        set_error("short write to '%s'", path);
        return RT_ERR_IO;
    }
    return RT_OK;
}

// Radiance RGBE (Ward, "Real Pixels", Graphics Gems II): the exponent of the largest channel, mantissas truncated
int rt_write_hdr(const char *path, const float *rgb_sum, int width, int height, int spp) {
    if (!path || !rgb_sum || width <= 0 || height <= 0 || spp <= 0) {
        set_error("rt_write_hdr: bad argument");
        return RT_ERR_ARG;
    }
    char head[96];
    const int hn = snprintf(head, sizeof head, "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n", height, width);
    std::string out(head, (size_t)hn);
    out.reserve(out.size() + (size_t)width * height * 4 + (size_t)height * 8);
    std::string row;
    const float n = (float)spp;
    for (int j = height - 1; j >= 0; --j) {  // top row first
        row.clear();
        for (int i = 0; i < width; ++i) {
            const float *p = rgb_sum + ((size_t)j * width + i) * 3;
            double c[3];
            for (int k = 0; k < 3; ++k) {
                const float v = p[k] / n;
                c[k] = v > 0.0f ? (double)v : 0.0;  // (negative and NaN: 0)
            }
            const double m = std::max(c[0], std::max(c[1], c[2]));
            unsigned char q[4] = {0, 0, 0, 0};
            if (m >= 1e-32) {
                int e = 0;
                if (std::isfinite(m)) (void)std::frexp(m, &e);  // m = f 2^e, f in [0.5, 1)
                else e = 128;
                if (e > 127) {  // beyond the format: its largest value
                    q[0] = c[0] >= m ? 255 : 0, q[1] = c[1] >= m ? 255 : 0, q[2] = c[2] >= m ? 255 : 0, q[3] = 255;
                } else {
                    for (int k = 0; k < 3; ++k) q[k] = (unsigned char)(int)std::ldexp(c[k], 8 - e);  // exact, then truncated
                    q[3] = (unsigned char)(e + 128);
                }
            }
            row.append((const char *)q, 4);
        }
        // (the largest channel's mantissa is >= 128, so no scanline begins with the 2, 2 of a run-length coded one)
        out += row;
    }
    return write_file(path, out);
}

int rt_write_pfm(const char *path, const float *rgb_sum, int width, int height, int spp) {
    if (!path || !rgb_sum || width <= 0 || height <= 0 || spp <= 0) {
        set_error("rt_write_pfm: bad argument");
        return RT_ERR_ARG;
    }
    char head[64];
    const int hn = snprintf(head, sizeof head, "PF\n%d %d\n-1.0\n", width, height);
    std::string out(head, (size_t)hn);
    const size_t count = (size_t)width * height * 3;
    out.reserve(out.size() + count * 4);
    const float n = (float)spp;
    for (size_t i = 0; i < count; ++i) {  // rows bottom to top: the framebuffer's order
        const float v = rgb_sum[i] / n;
        uint32_t u;
        memcpy(&u, &v, 4);
        const char b[4] = {(char)(u & 255), (char)((u >> 8) & 255), (char)((u >> 16) & 255), (char)(u >> 24)};
        out.append(b, 4);
    }
    return write_file(path, out);
}

// ---- misc ----------------------------------------------------------------------------
void rt_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    Philox4 p = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    for (int i = 0; i < 4; ++i) out[i] = p.v[i];
}

// first n raw words of the stream of one (pixel, sample): known-answer tests
void rt_sample_stream(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t *out, int n) {
    Xor128 g = xor128_seed(pixel, sample, (uint32_t)seed, (uint32_t)(seed >> 32));
    for (int i = 0; i < n; ++i) out[i] = xor128_next(g);
}

// aabb::hit, gpu-version/aabb.hpp:15-29
int rt_aabb_hit(const float bmin[3], const float bmax[3], const float orig[3], const float dir[3], float t_min_f,
                float t_max_f) {
    double t_min = t_min_f, t_max = t_max_f;
    for (int a = 0; a < 3; ++a) {
        float invD = 1.0f / dir[a];
        float t0 = (bmin[a] - orig[a]) * invD;
        float t1 = (bmax[a] - orig[a]) * invD;
        if (invD < 0.0f) {
            float tmp = t0;
            t0 = t1;
            t1 = tmp;
        }
        t_min = t0 > t_min ? t0 : t_min;
        t_max = t1 < t_max ? t1 : t_max;
        if (t_max <= t_min) return 0;
    }
    return 1;
}

// ---- homogeneous media: the scene interface and the host evaluation of the device's interval (rt_media.h)
int rt_scene_add_medium_sphere(rt_scene *s, const float center[3], float radius, float density, const float albedo[3]) {
    if (!s || !center || !albedo) {
        set_error("rt_scene_add_medium_sphere: null argument");
        return -RT_ERR_ARG;
    }
    rt_medium m;
    memset(&m, 0, sizeof m);
    m.shape = RT_MEDIUM_SPHERE;
    for (int k = 0; k < 3; ++k) m.f[k] = center[k], m.albedo[k] = albedo[k];
    m.f[3] = radius, m.density = density;
    return add_medium(s->s, m);
}

int rt_scene_add_medium_box(rt_scene *s, const float bmin[3], const float bmax[3], float density, const float albedo[3]) {
    if (!s || !bmin || !bmax || !albedo) {
        set_error("rt_scene_add_medium_box: null argument");
        return -RT_ERR_ARG;
    }
    rt_medium m;
    memset(&m, 0, sizeof m);
    m.shape = RT_MEDIUM_BOX;
    for (int k = 0; k < 3; ++k) m.f[k] = bmin[k], m.f[3 + k] = bmax[k], m.albedo[k] = albedo[k];
    m.density = density;
    return add_medium(s->s, m);
}

int rt_scene_get_media(const rt_scene *s, rt_medium *out, int cap) {
    if (bad_scene(s, "rt_scene_get_media")) return -RT_ERR_ARG;
    for (int i = 0; out && i < cap && i < (int)s->s.media.size(); ++i) out[i] = s->s.media[(size_t)i];
    return (int)s->s.media.size();
}

int rt_scene_clear_media(rt_scene *s) {
    if (bad_scene(s, "rt_scene_clear_media")) return RT_ERR_ARG;
    if (!s->s.media.empty()) {  // (a scene without media stays the scene it was: same version, same tables)
        s->s.media.clear();
        s->s.media_g.clear();
        s->s.touch();
    }
    return RT_OK;
}

int rt_medium_interval(const rt_medium *m, const float orig[3], const float dir[3], float t_max, float *t_in, float *t_out) {
    if (!m || !orig || !dir) {
        set_error("rt_medium_interval: null argument");
        return -RT_ERR_ARG;
    }
    if (m->shape != RT_MEDIUM_SPHERE && m->shape != RT_MEDIUM_BOX) {
        set_error("rt_medium_interval: shape %d (0 sphere, 1 box)", m->shape);
        return -RT_ERR_ARG;
    }
    float a, b;
    const bool hit = medium_interval(m->shape, m->f[0], m->f[1], m->f[2], m->f[3], m->f[4], m->f[5], orig[0], orig[1], orig[2], dir[0],
                                     dir[1], dir[2], t_max, a, b);
    if (t_in) *t_in = a;
    if (t_out) *t_out = b;
    return hit ? 1 : 0;
}

// a shadow ray's transmittance through the scene's media: the media walk of a lane in its shadow phase, from the
// device's own functions (rt_media.h) -- len = sqrt(d.d) as the kernels form it, the media in list order
int rt_media_transmittance(const rt_scene *s, const float orig[3], const float dir[3], float t_max, float *T) {
    if (bad_scene(s, "rt_media_transmittance")) return RT_ERR_ARG;
    if (!orig || !dir || !T) {
        set_error("rt_media_transmittance: null argument");
        return RT_ERR_ARG;
    }
    const float ra = fmaf(dir[0], dir[0], fmaf(dir[1], dir[1], dir[2] * dir[2]));
    const float len = sqrtf(ra);
    float tau = 0.0f;
    for (const rt_medium &m : s->s.media) {
        float a, b;
        if (m.density > 0.0f && medium_interval(m.shape, m.f[0], m.f[1], m.f[2], m.f[3], m.f[4], m.f[5], orig[0], orig[1], orig[2], dir[0],
                                                dir[1], dir[2], t_max, a, b))
            tau = medium_tau_add(m.density, a, b, len, tau);
    }
    *T = media_transmittance(tau);
    return RT_OK;
}

// ---- anisotropic media: a medium's asymmetry and the host evaluations of the device's phase function (rt_phase.h)
int rt_scene_set_medium_phase(rt_scene *s, int medium, float g) {
    if (bad_scene(s, "rt_scene_set_medium_phase")) return RT_ERR_ARG;
    return set_medium_phase(s->s, medium, g);
}

int rt_scene_get_medium_phase(const rt_scene *s, int medium, float *g) {
    if (bad_scene(s, "rt_scene_get_medium_phase")) return RT_ERR_ARG;
    if (!g) {
        set_error("rt_scene_get_medium_phase: null argument");
        return RT_ERR_ARG;
    }
    if (medium < 0 || (size_t)medium >= s->s.media.size()) {
        set_error("rt_scene_get_medium_phase: medium %d out of range (the scene has %zu)", medium, s->s.media.size());
        return RT_ERR_ARG;
    }
    *g = s->s.media_g[(size_t)medium];
    return RT_OK;
}

int rt_phase_hg_sample(float g, const float dir[3], float u1, float u2, float out[3]) {
    if (!dir || !out) {
        set_error("rt_phase_hg_sample: null argument");
        return RT_ERR_ARG;
    }
    if (!(std::isfinite(g) && std::fabs(g) <= RT_PHASE_G_MAX && g != 0.0f)) {
        set_error("rt_phase_hg_sample: g %g must be non-zero and within [-%g, %g] (g = 0 is the rejection loop's vertex)", (double)g,
                  (double)RT_PHASE_G_MAX, (double)RT_PHASE_G_MAX);
        return RT_ERR_ARG;
    }
#ifdef RT_CAPI_HOST_PASS
    // the kernels' 1 / |d| of a query: ra = d.d, inv_len = 1 / sqrt(ra)
    const float ra = fmaf(dir[0], dir[0], fmaf(dir[1], dir[1], dir[2] * dir[2]));
    const float inv_len = 1.0f / sqrtf(ra);
    phase_hg_sample(g, inv_len * dir[0], inv_len * dir[1], inv_len * dir[2], u1, u2, out[0], out[1], out[2]);
#endif
    return RT_OK;
}

float rt_phase_hg_eval(float g, float cos_theta) {
#ifdef RT_CAPI_HOST_PASS
    return phase_hg_eval(g, cos_theta);
#else
    return 0.0f;
#endif
}

// ---- moving spheres: the scene interface and the host evaluations of the device's functions (rt_motion.h)
int rt_scene_add_moving_sphere(rt_scene *s, const float center0[3], const float center1[3], float radius, int material) {
    if (!s || !center0 || !center1) {
        set_error("rt_scene_add_moving_sphere: null argument");
        return -RT_ERR_ARG;
    }
    rt_moving_sphere m;
    memset(&m, 0, sizeof m);
    for (int k = 0; k < 3; ++k) m.center0[k] = center0[k], m.center1[k] = center1[k];
    m.radius = radius, m.material = material;
    return add_moving_sphere(s->s, m);
}

int rt_scene_moving_sphere_count(const rt_scene *s) {
    if (bad_scene(s, "rt_scene_moving_sphere_count")) return -RT_ERR_ARG;
    return (int)s->s.movers.size();
}

int rt_scene_get_moving_spheres(const rt_scene *s, rt_moving_sphere *out, int cap) {
    if (bad_scene(s, "rt_scene_get_moving_spheres")) return -RT_ERR_ARG;
    for (int i = 0; out && i < cap && i < (int)s->s.movers.size(); ++i) out[i] = s->s.movers[(size_t)i];
    return (int)s->s.movers.size();
}

int rt_scene_clear_moving_spheres(rt_scene *s) {
    if (bad_scene(s, "rt_scene_clear_moving_spheres")) return RT_ERR_ARG;
    if (!s->s.movers.empty()) {  // (a scene without movers stays the scene it was: same version, same tables)
        s->s.movers.clear();
        s->s.touch();
    }
    return RT_OK;
}

// ---- analytic lights: a list of its own, as given; scene_lights() derives what the tables hold
static int add_analytic_light(rt_scene *s, const char *fn, int type, const float *position, const float *direction, const float *color,
                              float a0, float a1) {
    if (!s || !color || (type != RT_LIGHT_DISTANT && !position) || (type != RT_LIGHT_POINT && !direction)) {
        set_error("%s: null argument", fn);
        return -RT_ERR_ARG;
    }
    rt_analytic_light l;
    memset(&l, 0, sizeof l);
    l.type = type;
    for (int k = 0; k < 3; ++k) {
        if (position) l.position[k] = position[k];
        if (direction) l.direction[k] = direction[k];
        l.color[k] = color[k];
    }
    l.angle[0] = a0, l.angle[1] = a1;
    if (!analytic_light_ok(l, fn)) return -RT_ERR_ARG;
    s->s.alights.push_back(l);
    s->s.touch();
    return (int)s->s.alights.size() - 1;
}

int rt_scene_add_point_light(rt_scene *s, const float position[3], const float intensity[3]) {
    return add_analytic_light(s, "rt_scene_add_point_light", RT_LIGHT_POINT, position, nullptr, intensity, 0.0f, 0.0f);
}

int rt_scene_add_spot_light(rt_scene *s, const float position[3], const float direction[3], const float intensity[3], float inner_deg,
                            float outer_deg) {
    return add_analytic_light(s, "rt_scene_add_spot_light", RT_LIGHT_SPOT, position, direction, intensity, inner_deg, outer_deg);
}

int rt_scene_add_distant_light(rt_scene *s, const float direction_of_travel[3], const float irradiance[3], float angular_radius_deg) {
    return add_analytic_light(s, "rt_scene_add_distant_light", RT_LIGHT_DISTANT, nullptr, direction_of_travel, irradiance,
                              angular_radius_deg, 0.0f);
}

int rt_scene_get_analytic_lights(const rt_scene *s, rt_analytic_light *out, int cap) {
    if (bad_scene(s, "rt_scene_get_analytic_lights")) return -RT_ERR_ARG;
    for (int i = 0; out && i < cap && i < (int)s->s.alights.size(); ++i) out[i] = s->s.alights[(size_t)i];
    return (int)s->s.alights.size();
}

int rt_scene_clear_analytic_lights(rt_scene *s) {
    if (bad_scene(s, "rt_scene_clear_analytic_lights")) return RT_ERR_ARG;
    if (!s->s.alights.empty()) {  // (a scene without them stays the scene it was: same version, same tables)
        s->s.alights.clear();
        s->s.touch();
    }
    return RT_OK;
}

int rt_moving_sphere_hit(const rt_moving_sphere *m, float s, const float orig[3], const float dir[3], float t_max, float *t) {
    if (!m || !orig || !dir) {
        set_error("rt_moving_sphere_hit: null argument");
        return -RT_ERR_ARG;
    }
    // the ray's A = d.d and 1 / A as the kernel carries them (render_body.h: ra, rinv_a), v as the packer writes it
    const float A = fmaf(dir[0], dir[0], fmaf(dir[1], dir[1], dir[2] * dir[2])), inv_a = 1.0f / A;
    float root = 0.0f;
    const bool hit = moving_sphere_hit(m->center0[0], m->center0[1], m->center0[2], m->radius, m->center1[0] - m->center0[0],
                                       m->center1[1] - m->center0[1], m->center1[2] - m->center0[2], s, orig[0], orig[1], orig[2], dir[0],
                                       dir[1], dir[2], A, inv_a, t_max, root);
    if (hit && t) *t = root;
    return hit ? 1 : 0;
}

// ---- ray queries: the host evaluation of the kernel's guard (rt_trace.h)
static_assert(sizeof(rt_ray) == 32 && sizeof(rt_hit) == 48, "two and three 16-byte records");
int rt_ray_valid(const rt_ray *r) {
    if (!r) return 0;
    return ray_valid(r->origin[0], r->origin[1], r->origin[2], r->t_max, r->dir[0], r->dir[1], r->dir[2]) ? 1 : 0;
}

float rt_shutter_time(uint64_t seed, uint32_t pixel, uint32_t sample) {
    return shutter_time(pixel, sample, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// ---- environment map: the scene interface and the host evaluations of the device functions of rt_env.h (no GPU needed)
static EnvView env_host_view(const Scene &s) {
    const SceneEnvironment &e = *s.env;
    return EnvView{e.rgb.data(), e.marg.data(), e.cond.data(), e.band.data(), e.ct.data(), e.rows, e.cols, s.env_scale, env_uoff(s.env_rotate)};
}

int rt_scene_set_environment(rt_scene *s, int rows, int cols, const float *rgb, float scale, float rotate_deg) {
    if (!s) {
        set_error("rt_scene_set_environment: null scene");
        return RT_ERR_ARG;
    }
    return set_environment(s->s, rows, cols, rgb, scale, rotate_deg, "");
}

int rt_scene_set_environment_file(rt_scene *s, const char *path, float scale, float rotate_deg) {
    if (!s || !path) {
        set_error("rt_scene_set_environment_file: null scene or path");
        return RT_ERR_ARG;
    }
    return set_environment_file(s->s, path, scale, rotate_deg);
}

int rt_scene_get_environment(const rt_scene *s, int *rows, int *cols, float *scale, float *rotate_deg, float *rgb, size_t cap_floats) {
    if (!s) {
        set_error("rt_scene_get_environment: null scene");
        return RT_ERR_ARG;
    }
    const SceneEnvironment *e = s->s.env.get();
    if (rows) *rows = e ? e->rows : 0;
    if (cols) *cols = e ? e->cols : 0;
    if (scale) *scale = s->s.env_scale;
    if (rotate_deg) *rotate_deg = s->s.env_rotate;
    if (e && rgb) {
        if (cap_floats < e->rgb.size()) {
            set_error("rt_scene_get_environment: buffer of %zu floats, the map needs %zu", cap_floats, e->rgb.size());
            return RT_ERR_ARG;
        }
        memcpy(rgb, e->rgb.data(), e->rgb.size() * sizeof(float));
    }
    return RT_OK;
}

int rt_environment_eval(const rt_scene *s, const float dir[3], float rgb[3], float *pdf) {
    if (!s || !dir || !s->s.env) {
        set_error("rt_environment_eval: null argument, or a scene without an environment");
        return RT_ERR_ARG;
    }
    const double len = std::sqrt((double)dir[0] * dir[0] + (double)dir[1] * dir[1] + (double)dir[2] * dir[2]);
    if (!(len > 0.0) || !std::isfinite(len)) {
        set_error("rt_environment_eval: direction of length %g", len);
        return RT_ERR_ARG;
    }
    const EnvView E = env_host_view(s->s);
    float r, g, b, p;
    env_eval(E, (float)(dir[0] / len), (float)(dir[1] / len), (float)(dir[2] / len), r, g, b, p);
    if (rgb) rgb[0] = r, rgb[1] = g, rgb[2] = b;
    if (pdf) *pdf = p;
    return RT_OK;
}

int rt_environment_sample(const rt_scene *s, float u1, float u2, float dir[3], float rgb[3], float *pdf) {
    if (!s || !dir || !s->s.env) {
        set_error("rt_environment_sample: null argument, or a scene without an environment");
        return RT_ERR_ARG;
    }
    if (!(u1 >= 0.0f && u1 < 1.0f && u2 >= 0.0f && u2 < 1.0f)) {
        set_error("rt_environment_sample: u1, u2 must lie in [0, 1)");
        return RT_ERR_ARG;
    }
    const EnvView E = env_host_view(s->s);
    float r = 0, g = 0, b = 0, p = 0;
    dir[0] = 0, dir[1] = 1, dir[2] = 0;
    if (s->s.env->flux > 0.0) {  // (an all-zero map has nothing to draw: pdf 0)
        env_sample(E, u1, u2, dir[0], dir[1], dir[2]);
        env_eval(E, dir[0], dir[1], dir[2], r, g, b, p);
    }
    if (rgb) rgb[0] = r, rgb[1] = g, rgb[2] = b;
    if (pdf) *pdf = p;
    return RT_OK;
}

}  // extern "C"
