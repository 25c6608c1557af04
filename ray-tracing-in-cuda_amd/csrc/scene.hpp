// Host scene model: the reference's object graph (gpu-version/parser.hpp:16-32
// `struct scene` + the hittable/material/mytexture class hierarchy) flattened to
// POD tables that one hipMemcpy can upload.  The reference instead re-`new`s every
// object on the device from a <<<1,1>>> kernel to get device vtables
// (gpu-version/main.cu:374-446); there are no virtual calls here, so that step is
// designed away.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "../../include/rtmi.h"

namespace rtmi {

struct CameraParams {
    double lookfrom[3] = {0, 0, 1}, lookat[3] = {0, 0, 0}, vup[3] = {0, 1, 0};
    double vfov = 40.0;
    double aspect = 0.0;      // <= 0: width / height
    double aperture = 0.0;
    double focus_dist = 0.0;  // <= 0: |lookfrom - lookat|
    // the projection (rt_projection_type) and its parameters: orthographic {height}, panoramic {hfov, vfov} in
    // degrees, fisheye {fov} in degrees; unused ones are 0.  Kept by every setter of the fields above
    int projection = RT_PROJ_PERSPECTIVE;
    double proj[2] = {0.0, 0.0};
};

// how a cylinder's transform was specified (kept for JSON serialisation)
struct CylinderXform {
    bool has_rotate = false, has_translate = false;
    double axis[3] = {0, 0, 1};
    double degrees = 0.0;
    double offset[3] = {0, 0, 0};
};

// pixels of an image texture (taichi-version/material.py:96-110): rows x cols texels, R G B bytes
struct SceneImage {
    int rows = 0, cols = 0;
    std::vector<uint8_t> rgb;
    std::vector<uint8_t> alpha;  // rows x cols alpha bytes; empty: no plane, every texel is 255
    std::string file;  // where it was read from ("" = given inline), for serialisation
};

// An environment map: rows x cols fp32 RGB texels in lat-long layout (row 0 = the zenith, +y) and the sampling
// tables built from them (csrc/rt_env.h says what they hold).  Immutable once built: clones share it.
struct SceneEnvironment {
    int rows = 0, cols = 0;
    std::vector<float> rgb;
    std::vector<float> marg, cond, band, ct;
    double flux = 0.0;  // sum over texels of luminance x solid angle (scale 1); 0: nothing to sample
    std::string file;   // where it was read from ("" = given inline), for serialisation
};

struct DeviceSceneCache;  // owned by the render module

// a material's bump: the height field is the scalar s of noise texture `texture`, scaled by `strength`
struct SceneBump {
    int texture = -1;
    float strength = 0.0f;
};

// a material's normal map: image texture `texture` read in the surface's tangent frame, its tangential part x `scale`
struct SceneNormalMap {
    int texture = -1;
    float scale = 0.0f;
};

// a material's alpha mask: the alpha byte of image texture `texture` at the hit's (u, v) against c8 =
// alpha_cutoff_byte(cutoff) (rt_alpha.h); a8 < c8: the hit is transparent
struct SceneAlpha {
    int texture = -1;
    float cutoff = 0.0f;
};

struct Scene {
    int width = 400, height = 225, spp = 100, max_depth = 50;
    float background[3] = {0, 0, 0};
    uint32_t flags = 0;
    float rr_p = 0.0f;  // Russian-roulette survival probability per bounce, 0 = off
    bool light_sampling = false;  // next-event estimation + MIS (rt_scene_set_light_sampling)
    bool mesh_lights = false;     // scene_lights() also lists emissive triangles (rt_scene_set_mesh_lights)
    bool media_light_sampling = false;  // light samples at medium vertices and through media (rt_scene_set_media_light_sampling)
    bool nested_grid = false;     // overfull grid cells get a sub-grid (rt_scene_set_nested_grid)
    std::string output_file = "main.png";  // parser.hpp:566-567 default
    CameraParams cam;
    std::vector<rt_prim> prims;
    std::vector<CylinderXform> xforms;  // parallel to prims (meaningful for cylinders)
    std::vector<rt_material> mats;
    std::vector<rt_texture> texs;
    std::vector<SceneImage> images;  // referenced by RT_TEX_IMAGE textures (c0[0] = index)
    std::vector<rt_noise> noise;     // noise[i]: the parameters of texture i where it is an RT_TEX_NOISE; beside the
                                     // texture table as the images are, as long as the last noise texture's id + 1
    std::vector<SceneBump> bumps;    // bumps[m]: the bump of material m, texture < 0: none; beside the material table
                                     // as `noise` is beside the textures, at most as long as the last bumped material's id + 1
    std::vector<int> pbr_maps;       // pbr_maps[m]: the metallic-roughness map of pbr material m, -1: none; beside the
                                     // material table as the bumps are, at most as long as the last mapped material's id + 1
    std::vector<SceneNormalMap> normal_maps;  // normal_maps[m]: the normal map of material m, texture < 0: none; beside
                                     // the material table as the bumps are, at most as long as the last mapped material's id + 1
    std::vector<SceneAlpha> alphas;  // alphas[m]: the alpha mask of material m, texture < 0: none; beside the material
                                     // table as the bumps are, at most as long as the last masked material's id + 1
    std::shared_ptr<const SceneEnvironment> env;  // null: no environment (a miss gives the background / the sky)
    float env_scale = 1.0f, env_rotate = 0.0f;    // radiance = scale x texel; degrees about +y
    std::vector<rt_medium> media;  // homogeneous participating media, a list of its own: at most RT_MAX_MEDIA
    std::vector<float> media_g;    // media_g[i]: the Henyey-Greenstein asymmetry of medium i as stored (0: isotropic),
                                   // beside `media` and always as long
    std::vector<rt_moving_sphere> movers;  // moving spheres, a list of its own: at most RT_MAX_MOVING_SPHERES
    std::vector<rt_analytic_light> alights;  // point, spot and distant lights, a list of its own, as given
    uint64_t version = 1;  // bumped on every mutation; invalidates device caches
    std::shared_ptr<DeviceSceneCache> dev;

    void touch() { ++version; }
};

// the emitters that light sampling samples (spheres, axis-aligned rects and rigid cylinder tubes -- with Scene::mesh_lights,
// triangles too, one light each -- whose material is a diffuse_light with a solid or checker texture and nonzero power), in
// list order, with their selection probabilities (proportional to area x mean emission luminance)
struct SceneLight {
    int prim = 0, type = 0;  // list index, rt_prim_type; the environment (always last): -1, RT_LIGHT_ENVIRONMENT
    double area = 0.0, prob = 0.0;
    float even[3] = {0, 0, 0}, odd[3] = {0, 0, 0};
    bool checker = false;
    int analytic = -1;  // an analytic light: its index in Scene::alights; prim = -1, type = RT_LIGHT_POINT / SPOT / DISTANT
};
std::vector<SceneLight> scene_lights(const Scene &s);

// analytic lights.  What the light record and the selection weight hold, derived in fp64 from the fp32 record:
// `dir` the unit axis of a spot / the unit direction TOWARDS a distant light; `color` rounded once (a distant light's with the
// fold 2 / (1 + cos alpha)); `measure` x lum(color as given) / pi is the selection weight
struct AnalyticRecord {
    double dir[3] = {0, 0, 0};
    float color[3] = {0, 0, 0};
    float cos_o = 0.0f, inv = 0.0f;  // spot: cos(outer), min(1 / (cos_i - cos_o), FLT_MAX)
    float omc = 0.0f, dist = 0.0f;   // distant: 1 - cos alpha, D = 4 r
    double measure = 0.0, weight = 0.0;
};
AnalyticRecord analytic_record(const rt_analytic_light &l, double bound_radius);
// is the record within the argument rules (false: the message is set, prefixed with `where`)
bool analytic_light_ok(const rt_analytic_light &l, const char *where);

// derive the camera frame (camera.cuh:9-29) in fp64, round once to fp32
void derive_camera(const Scene &s, rt_camera *out);
// the six camera records of the hot table (xyz each) and the lens radius, for any projection (csrc/rt_camera.h says what they
// hold): derived in fp64, rounded once.  The perspective ones are derive_camera's {origin, lower_left, horizontal, vertical, u, v}
void camera_records(const Scene &s, float rec[6][3], float *lens_radius);
// are a projection's parameters within the argument rules (false: the message is set, prefixed with `where`); p: two values,
// of which the type's unused ones are ignored
bool projection_ok(int type, const double p[2], const char *where);
const char *projection_name(int type);  // "perspective", ... ; null: no such type

// all return RT_OK or an rt_status, message via set_error()
// base_dir: directory that relative "file" entries (image textures, meshes) are resolved against (NULL: the cwd)
int scene_from_json(const char *text, size_t len, Scene &out, const char *base_dir = nullptr);
std::string scene_to_json(const Scene &s);
void scene_rtiow(Scene &out, uint32_t seed, int width, int height, int spp, int max_depth);
int scene_validate(const Scene &s);

int add_cylinder(Scene &s, float radius, float zmin, float zmax, int material, const double *axis,
                 double degrees, const double *offset);

// -> texture id / triangles added / prim id, or -rt_status
// alpha: rows x cols alpha bytes, or null: the image has no alpha plane
int add_image_texture(Scene &s, int rows, int cols, const uint8_t *rgb, const std::string &file, const uint8_t *alpha = nullptr);
int add_image_texture_file(Scene &s, const char *path);
// an 8-bit image file (PNG by signature, else PPM) -> RT_OK or an rt_status
int read_image_file(const char *path, int &rows, int &cols, std::vector<uint8_t> &rgb, std::vector<uint8_t> *alpha = nullptr);

// the environment map (scene.cpp).  set_environment: rows = 0 clears; file: what to_json writes in place of the texels ("" = inline)
constexpr long long kEnvMaxTexels = 1LL << 25;
int set_environment(Scene &s, int rows, int cols, const float *rgb, float scale, float rotate_deg, const std::string &file);
int set_environment_file(Scene &s, const char *path, float scale, float rotate_deg);
float env_uoff(float rotate_deg);           // the rotation as the lookup's offset of u, in [0, 1)
double scene_bound_radius(const Scene &s);  // radius of the bounding sphere of the primitives (of their boxes' union)
// quads and boxes: rotate (axis, degrees) then translate, either may be null -- applied on the host, in fp64.
// add_box -> the index of the first of its six quads
int add_quad(Scene &s, const float q[3], const float u[3], const float v[3], int material, const double *axis, double degrees,
             const double *offset);
int add_box(Scene &s, const float mn[3], const float mx[3], int material, const double *axis, double degrees, const double *offset);
int add_triangle(Scene &s, const float v1[3], const float v2[3], const float v3[3], const float uv1[2], const float uv2[2],
                 const float uv3[2], int material);
int add_obj(Scene &s, const char *path, int material, float scale, const float matrix[9], const float translate[3]);
// smooth shading: a triangle with vertex normals; a mesh whose normals come from `mode` (rt_mesh_normals)
int add_triangle_normals(Scene &s, const float v1[3], const float v2[3], const float v3[3], const float n1[3], const float n2[3],
                         const float n3[3], const float uv1[2], const float uv2[2], const float uv3[2], int material);
int add_obj_normals(Scene &s, const char *path, int material, float scale, const float matrix[9], const float translate[3], int mode,
                    float crease_degrees);
void set_mesh_normals_override(int mode, float crease_degrees);
// does triangle p carry vertex normals (any of the nine words non-zero)?
inline bool tri_has_normals(const rt_prim &p) {
    for (int k = 0; k < 6; ++k)
        if (p.f[k] != 0.0f) return true;
    return p.m_inv[6] != 0.0f || p.m_inv[7] != 0.0f || p.m_inv[8] != 0.0f;
}

// glossy materials: does the material table hold one (such a scene runs the general kernels over the wide tables);
// is a rough_metal / plastic record within its argument rules (false: the message is set, prefixed with `where`)
// (rough_glass, DESIGN 7r, is the third of them)
// (pbr, DESIGN 7t, becomes a rough_metal or a plastic at every vertex: fuzz = the roughness factor, albedo[0] = the metallic factor)
inline bool is_glossy(const rt_material &m) {
    return m.type == RT_MAT_ROUGH_METAL || m.type == RT_MAT_PLASTIC || m.type == RT_MAT_ROUGH_GLASS || m.type == RT_MAT_PBR;
}
inline bool scene_has_glossy(const Scene &s) {
    for (const rt_material &m : s.mats)
        if (is_glossy(m)) return true;
    return false;
}
bool glossy_material_ok(const rt_material &m, size_t textures, const char *where);

// noise textures: does the texture table hold one (such a scene runs the general kernels over the wide tables, as
// one with an image texture does); are two colours and a parameter record within the argument rules (false: the message is
// set, prefixed with `where`); checks and appends -> texture id, or -RT_ERR_ARG.  A style other than marble has neither axis
// nor distortion: the stored record keeps zeros there, whatever the caller's held.
inline bool scene_has_noise(const Scene &s) {
    for (const rt_texture &t : s.texs)
        if (t.type == RT_TEX_NOISE) return true;
    return false;
}
bool noise_texture_ok(const float c0[3], const float c1[3], const rt_noise &n, const char *where);
int add_noise_texture(Scene &s, const float c0[3], const float c1[3], const rt_noise &n, const char *where);

// bump mapping: the bump of material m, or null; does any material carry one (such a scene runs the general
// kernels over the wide tables); set_bump checks (false: the message is set, prefixed with `where`) and stores -- texture -1
// or strength 0 removes
inline const SceneBump *scene_bump(const Scene &s, int m) {
    return (m >= 0 && (size_t)m < s.bumps.size() && s.bumps[(size_t)m].texture >= 0) ? &s.bumps[(size_t)m] : nullptr;
}
inline bool scene_has_bump(const Scene &s) {
    for (const SceneBump &b : s.bumps)
        if (b.texture >= 0) return true;
    return false;
}
bool set_bump(Scene &s, int material, int texture, float strength, const char *where);

// the metallic-roughness map of pbr material m, or -1; set_pbr_map checks (false: the message is set, prefixed
// with `where`) and stores -- texture -1 removes
inline int scene_pbr_map(const Scene &s, int m) { return (m >= 0 && (size_t)m < s.pbr_maps.size()) ? s.pbr_maps[(size_t)m] : -1; }
bool set_pbr_map(Scene &s, int material, int texture, const char *where);

// normal maps: the map of material m, or null; does any material carry one (such a scene runs the general kernels
// over the wide tables, as one with a bump); set_normal_map checks (false: the message is set, prefixed with `where`) and
// stores -- texture -1 or scale 0 removes.  A material carries a bump or a map, not both: either setter refuses the second
inline const SceneNormalMap *scene_normal_map(const Scene &s, int m) {
    return (m >= 0 && (size_t)m < s.normal_maps.size() && s.normal_maps[(size_t)m].texture >= 0) ? &s.normal_maps[(size_t)m] : nullptr;
}
inline bool scene_has_normal_map(const Scene &s) {
    for (const SceneNormalMap &b : s.normal_maps)
        if (b.texture >= 0) return true;
    return false;
}
bool set_normal_map(Scene &s, int material, int texture, float scale, const char *where);

// alpha masks: the mask of material m, or null; does any material carry one (such a scene runs the general kernels
// over the wide tables: its texture is an image); set_alpha checks (false: the message is set, prefixed with `where`) and
// stores -- texture -1 removes
inline const SceneAlpha *scene_alpha(const Scene &s, int m) {
    return (m >= 0 && (size_t)m < s.alphas.size() && s.alphas[(size_t)m].texture >= 0) ? &s.alphas[(size_t)m] : nullptr;
}
inline bool scene_has_alpha(const Scene &s) {
    for (const SceneAlpha &b : s.alphas)
        if (b.texture >= 0) return true;
    return false;
}
bool set_alpha(Scene &s, int material, int texture, float cutoff, const char *where);

// a medium (scene.cpp): checks the record and appends it -> medium id, or -rt_status
int add_medium(Scene &s, const rt_medium &m);
// the asymmetry g of a medium's phase function: checks it and stores it (|g| < 1e-3 as 0) -> RT_OK or an rt_status
int set_medium_phase(Scene &s, int medium, float g);
// a moving sphere (scene.cpp): checks the record and appends it -> mover id, or -rt_status
int add_moving_sphere(Scene &s, const rt_moving_sphere &m);

void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
const char *get_error();

}  // namespace rtmi

struct rt_scene {
    rtmi::Scene s;
};
