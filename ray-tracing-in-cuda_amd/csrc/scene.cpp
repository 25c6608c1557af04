// Scene construction: JSON -> tables, RTIOW generator, camera derivation, JSON out.
#include "scene.hpp"

#include <algorithm>
#include <array>
#include <cctype>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>

#include "env_read.hpp"
#include "json.hpp"
#include "png_read.hpp"
#include "philox.h"
#include "rt_media.h"

namespace rtmi {

// ---------------------------------------------------------------- errors
static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
const char *get_error() { return g_err; }

// ---------------------------------------------------------------- camera
// camera::camera, gpu-version/camera.cuh:9-29 / cmake-cpu-version/camera.h:9-31.
// Evaluated in fp64 from the stored parameters and rounded to fp32 once, so the
// kernel, the fp32 checker and the fp64 reference build all start from one frame.
static inline void v3sub(const double *a, const double *b, double *o) {
    o[0] = a[0] - b[0], o[1] = a[1] - b[1], o[2] = a[2] - b[2];
}
static inline void v3cross(const double *a, const double *b, double *o) {
    double x = a[1] * b[2] - a[2] * b[1];
    double y = a[2] * b[0] - a[0] * b[2];
    double z = a[0] * b[1] - a[1] * b[0];
    o[0] = x, o[1] = y, o[2] = z;
}
static inline double v3len(const double *a) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
static inline void v3unit(double *a) {
    double inv = 1.0 / v3len(a);
    a[0] *= inv, a[1] *= inv, a[2] *= inv;
}

void derive_camera(const Scene &s, rt_camera *out) {
    const CameraParams &c = s.cam;
    const double pi = std::acos(-1.0);
    double aspect = c.aspect > 0 ? c.aspect : (double)s.width / (double)s.height;
    double d[3];
    v3sub(c.lookfrom, c.lookat, d);
    double focus = c.focus_dist > 0 ? c.focus_dist : v3len(d);

    double theta = c.vfov * pi / 180.0;
    double h = std::tan(theta / 2);
    double vh = 2.0 * h, vw = aspect * vh;
    double w[3] = {d[0], d[1], d[2]}, u[3], v[3];
    v3unit(w);
    v3cross(c.vup, w, u);
    v3unit(u);
    v3cross(w, u, v);
    for (int i = 0; i < 3; ++i) {
        double hor = focus * vw * u[i];
        double ver = focus * vh * v[i];
        double llc = c.lookfrom[i] - hor / 2 - ver / 2 - focus * w[i];
        out->lookfrom[i] = (float)c.lookfrom[i];
        out->lookat[i] = (float)c.lookat[i];
        out->vup[i] = (float)c.vup[i];
        out->origin[i] = (float)c.lookfrom[i];
        out->horizontal[i] = (float)hor;
        out->vertical[i] = (float)ver;
        out->lower_left[i] = (float)llc;
        out->u[i] = (float)u[i];
        out->v[i] = (float)v[i];
        out->w[i] = (float)w[i];
    }
    out->vfov = (float)c.vfov;
    out->aspect = (float)aspect;
    out->aperture = (float)c.aperture;
    out->focus_dist = (float)focus;
    out->lens_radius = (float)(c.aperture / 2);
}

// the camera records of any projection (rt_camera.h has the table)
void camera_records(const Scene &s, float rec[6][3], float *lens_radius) {
    rt_camera cam;
    derive_camera(s, &cam);
    const float *src[6] = {cam.origin, cam.lower_left, cam.horizontal, cam.vertical, cam.u, cam.v};
    for (int k = 0; k < 6; ++k)
        for (int i = 0; i < 3; ++i) rec[k][i] = src[k][i];
    *lens_radius = cam.lens_radius;
    const CameraParams &c = s.cam;
    if (c.projection == RT_PROJ_PERSPECTIVE) return;
    // the frame again in fp64, as derive_camera forms it
    const double pi = std::acos(-1.0);
    const double aspect = c.aspect > 0 ? c.aspect : (double)s.width / (double)s.height;
    double d[3];
    v3sub(c.lookfrom, c.lookat, d);
    const double focus = c.focus_dist > 0 ? c.focus_dist : v3len(d);
    double w[3] = {d[0], d[1], d[2]}, u[3], v[3];
    v3unit(w);
    v3cross(c.vup, w, u);
    v3unit(u);
    v3cross(w, u, v);
    if (c.projection == RT_PROJ_ORTHOGRAPHIC) {
        const double h = c.proj[0];
        for (int i = 0; i < 3; ++i) {
            const double hor = h * aspect * u[i], ver = h * v[i];
            rec[0][i] = (float)(-focus * w[i]);  // D = fd f
            rec[1][i] = (float)(c.lookfrom[i] - hor / 2 - ver / 2);
            rec[2][i] = (float)hor;
            rec[3][i] = (float)ver;
        }
        return;
    }
    for (int i = 0; i < 3; ++i) rec[2][i] = 0.0f, rec[3][i] = (float)(-w[i]);
    rec[2][0] = (float)focus;
    if (c.projection == RT_PROJ_PANORAMIC) {
        rec[1][0] = (float)(c.proj[0] * pi / 180.0), rec[1][1] = (float)(c.proj[1] * pi / 180.0), rec[1][2] = 0.0f;
    } else {  // fisheye: the half angle, and the image circle inscribed in the shorter side
        rec[1][0] = (float)(c.proj[0] * pi / 360.0);
        rec[1][1] = (float)std::max(aspect, 1.0), rec[1][2] = (float)std::max(1.0 / aspect, 1.0);
    }
}

const char *projection_name(int type) {
    static const char *const names[] = {"perspective", "orthographic", "panoramic", "fisheye"};
    return type >= 0 && type < 4 ? names[type] : nullptr;
}

bool projection_ok(int type, const double p[2], const char *where) {
    auto in = [](double x, double hi) { return std::isfinite(x) && x > 0 && x <= hi; };
    switch (type) {
    case RT_PROJ_PERSPECTIVE: return true;
    case RT_PROJ_ORTHOGRAPHIC:
        // (the records are fp32: a height whose fp32 value is 0 or inf is out of range too)
        if (!(std::isfinite(p[0]) && (float)p[0] > 0.0f && std::isfinite((float)p[0]))) {
            set_error("%s: an orthographic projection's \"height\" must be a positive finite number", where);
            return false;
        }
        return true;
    case RT_PROJ_PANORAMIC:
        if (!in(p[0], 360.0) || !in(p[1], 180.0)) {
            set_error("%s: a panoramic projection's \"hfov\" must be in (0, 360] and its \"vfov\" in (0, 180] degrees", where);
            return false;
        }
        return true;
    case RT_PROJ_FISHEYE:
        if (!in(p[0], 360.0)) {
            set_error("%s: a fisheye projection's \"fov\" must be in (0, 360] degrees", where);
            return false;
        }
        return true;
    }
    set_error("%s: unknown projection type %d (0 perspective, 1 orthographic, 2 panoramic, 3 fisheye)", where, type);
    return false;
}

// ---------------------------------------------------------------- cylinders
// cylinder::rotate/translate (object.cuh:225-231) with rotate() = Rodrigues form of
// vec3.cuh:396-418 and translate() of vec3.cuh:384-394, composed as the parser
// does (parser.hpp:423-440: rotate first, then translate => o2w = T * R).
// m = [R | t], m_inv = [R^T | -R^T t]; built in fp64, rounded once.
int add_cylinder(Scene &s, float radius, float zmin, float zmax, int material, const double *axis,
                 double degrees, const double *offset) {
    rt_prim p;
    memset(&p, 0, sizeof p);
    p.type = RT_PRIM_CYLINDER;
    p.material = material;
    p.f[0] = radius, p.f[1] = zmin, p.f[2] = zmax;
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    double t[3] = {0, 0, 0};
    CylinderXform xf;
    if (axis) {
        double a[3] = {axis[0], axis[1], axis[2]};
        double len = v3len(a);
        if (!(len > 0)) {
            set_error("cylinder rotate.axis has zero length");
            return -RT_ERR_SCENE;
        }
        v3unit(a);
        const double pi = std::acos(-1.0);
        double th = degrees / 180.0 * pi;
        double sn = std::sin(th), cs = std::cos(th);
        R[0][0] = a[0] * a[0] + (1 - a[0] * a[0]) * cs;
        R[0][1] = a[0] * a[1] * (1 - cs) - a[2] * sn;
        R[0][2] = a[0] * a[2] * (1 - cs) + a[1] * sn;
        R[1][0] = a[0] * a[1] * (1 - cs) + a[2] * sn;
        R[1][1] = a[1] * a[1] + (1 - a[1] * a[1]) * cs;
        R[1][2] = a[1] * a[2] * (1 - cs) - a[0] * sn;
        R[2][0] = a[0] * a[2] * (1 - cs) - a[1] * sn;
        R[2][1] = a[1] * a[2] * (1 - cs) + a[0] * sn;
        R[2][2] = a[2] * a[2] + (1 - a[2] * a[2]) * cs;
        xf.has_rotate = true;
        xf.axis[0] = axis[0], xf.axis[1] = axis[1], xf.axis[2] = axis[2];
        xf.degrees = degrees;
    }
    if (offset) {
        t[0] = offset[0], t[1] = offset[1], t[2] = offset[2];
        xf.has_translate = true;
        xf.offset[0] = t[0], xf.offset[1] = t[1], xf.offset[2] = t[2];
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            p.m[i * 4 + j] = (float)R[i][j];
            p.m_inv[i * 4 + j] = (float)R[j][i];
        }
        p.m[i * 4 + 3] = (float)t[i];
        p.m_inv[i * 4 + 3] = (float)(-(R[0][i] * t[0] + R[1][i] * t[1] + R[2][i] * t[2]));
    }
    s.prims.push_back(p);
    s.xforms.push_back(xf);
    s.touch();
    return (int)s.prims.size() - 1;
}

// ---------------------------------------------------------------- quads and boxes
// The cylinder's pair and order: rotate about `axis` by `degrees` (the Rodrigues form above), then translate by `offset`; either
// may be null.  False: the axis has zero length or something is not finite.
static bool rigid_transform(const double *axis, double degrees, const double *offset, double R[3][3], double t[3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = i == j ? 1.0 : 0.0;
    t[0] = t[1] = t[2] = 0.0;
    if (axis) {
        double a[3] = {axis[0], axis[1], axis[2]};
        const double len = v3len(a);
        if (!(len > 0) || !std::isfinite(len) || !std::isfinite(degrees)) return false;
        v3unit(a);
        const double pi = std::acos(-1.0);
        const double th = degrees / 180.0 * pi;
        const double sn = std::sin(th), cs = std::cos(th);
        R[0][0] = a[0] * a[0] + (1 - a[0] * a[0]) * cs;
        R[0][1] = a[0] * a[1] * (1 - cs) - a[2] * sn;
        R[0][2] = a[0] * a[2] * (1 - cs) + a[1] * sn;
        R[1][0] = a[0] * a[1] * (1 - cs) + a[2] * sn;
        R[1][1] = a[1] * a[1] + (1 - a[1] * a[1]) * cs;
        R[1][2] = a[1] * a[2] * (1 - cs) - a[0] * sn;
        R[2][0] = a[0] * a[2] * (1 - cs) - a[1] * sn;
        R[2][1] = a[1] * a[2] * (1 - cs) + a[0] * sn;
        R[2][2] = a[2] * a[2] + (1 - a[2] * a[2]) * cs;
    }
    if (offset) {
        for (int i = 0; i < 3; ++i) t[i] = offset[i];
        if (!std::isfinite(t[0]) || !std::isfinite(t[1]) || !std::isfinite(t[2])) return false;
    }
    return true;
}

// The record of the quad with corner Q and edges u, v (fp64 in, rounded once to the fp32 the record holds), and what the hit
// test reads, derived in fp64 from THOSE fp32 values and rounded once: c = u x v, n = c / |c|, w = c / (c.c), A = v x w,
// B = w x u (include/rtmi.h, RT_PRIM_QUAD).  False: |c|^2 is not finite or not positive, or a word is not finite.
static bool quad_record(const double Q[3], const double u[3], const double v[3], int material, rt_prim &p) {
    memset(&p, 0, sizeof p);
    p.type = RT_PRIM_QUAD;
    p.material = material;
    double q[3], a[3], b[3], c[3], w[3], A[3], B[3];
    for (int k = 0; k < 3; ++k) {
        p.m[k] = (float)Q[k], p.m[3 + k] = (float)u[k], p.m[6 + k] = (float)v[k];
        q[k] = p.m[k], a[k] = p.m[3 + k], b[k] = p.m[6 + k];
        if (!std::isfinite(p.m[k]) || !std::isfinite(p.m[3 + k]) || !std::isfinite(p.m[6 + k])) return false;
    }
    v3cross(a, b, c);
    const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
    if (!std::isfinite(cc) || !(cc > 0)) return false;
    const double len = std::sqrt(cc);
    for (int k = 0; k < 3; ++k) w[k] = c[k] / cc;
    v3cross(b, w, A);
    v3cross(w, a, B);
    for (int k = 0; k < 3; ++k) {
        p.m[9 + k] = (float)(c[k] / len);
        p.m_inv[k] = (float)A[k], p.m_inv[3 + k] = (float)B[k];
        if (!std::isfinite(p.m[9 + k]) || !std::isfinite(p.m_inv[k]) || !std::isfinite(p.m_inv[3 + k])) return false;
    }
    // (the fp32 record must still name a plane and an area: the light record holds 1 / |c| in fp32)
    if (!((float)len > 0.0f) || !std::isfinite((float)(1.0 / len)) || !std::isfinite((float)len)) return false;
    return true;
}

static void apply_rigid(const double R[3][3], const double *t, const double x[3], double out[3]) {
    for (int i = 0; i < 3; ++i) out[i] = R[i][0] * x[0] + R[i][1] * x[1] + R[i][2] * x[2] + (t ? t[i] : 0.0);
}

int add_quad(Scene &s, const float q[3], const float u[3], const float v[3], int material, const double *axis, double degrees,
             const double *offset) {
    double R[3][3], t[3];
    if (!rigid_transform(axis, degrees, offset, R, t)) {
        set_error("quad: rotate.axis has zero length, or the transform is not finite");
        return -RT_ERR_SCENE;
    }
    double Q[3] = {q[0], q[1], q[2]}, U[3] = {u[0], u[1], u[2]}, V[3] = {v[0], v[1], v[2]};
    if (axis || offset) {  // (no transform: the values as given, not through a multiplication by one)
        double Q2[3], U2[3], V2[3];
        apply_rigid(R, t, Q, Q2), apply_rigid(R, nullptr, U, U2), apply_rigid(R, nullptr, V, V2);
        for (int k = 0; k < 3; ++k) Q[k] = Q2[k], U[k] = U2[k], V[k] = V2[k];
    }
    rt_prim p;
    if (!quad_record(Q, U, V, material, p)) {
        set_error("quad with zero area (|u x v|^2 not positive or not finite), or non-finite corner or edges");
        return -RT_ERR_SCENE;
    }
    s.prims.push_back(p);
    s.xforms.emplace_back();
    s.touch();
    return (int)s.prims.size() - 1;
}

// box(min, max): six quads, every u x v pointing outward (so that `front` is the outside: a dielectric box refracts as a solid),
// in the order +z, -z, +x, -x, +y, -y; all six or none
int add_box(Scene &s, const float mn[3], const float mx[3], int material, const double *axis, double degrees, const double *offset) {
    double R[3][3], t[3];
    if (!rigid_transform(axis, degrees, offset, R, t)) {
        set_error("box: rotate.axis has zero length, or the transform is not finite");
        return -RT_ERR_SCENE;
    }
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(mn[k]) || !std::isfinite(mx[k]) || !(mn[k] < mx[k])) {
            set_error("box: min %g must be finite and below max %g on axis %d", (double)mn[k], (double)mx[k], k);
            return -RT_ERR_SCENE;
        }
    const double x0 = mn[0], y0 = mn[1], z0 = mn[2], x1 = mx[0], y1 = mx[1], z1 = mx[2];
    const double dx = x1 - x0, dy = y1 - y0, dz = z1 - z0;
    const double face[6][9] = {{x0, y0, z1, dx, 0, 0, 0, dy, 0},   // +z
                               {x0, y0, z0, 0, dy, 0, dx, 0, 0},   // -z
                               {x1, y0, z0, 0, dy, 0, 0, 0, dz},   // +x
                               {x0, y0, z0, 0, 0, dz, 0, dy, 0},   // -x
                               {x0, y1, z0, 0, 0, dz, dx, 0, 0},   // +y
                               {x0, y0, z0, dx, 0, 0, 0, 0, dz}};  // -y
    rt_prim rec[6];
    for (int f = 0; f < 6; ++f) {
        double Q[3], U[3], V[3];
        if (axis || offset) apply_rigid(R, t, face[f], Q), apply_rigid(R, nullptr, face[f] + 3, U), apply_rigid(R, nullptr, face[f] + 6, V);
        else
            for (int k = 0; k < 3; ++k) Q[k] = face[f][k], U[k] = face[f][3 + k], V[k] = face[f][6 + k];
        if (!quad_record(Q, U, V, material, rec[f])) {
            set_error("box: a face has no area in fp32, or is not finite");
            return -RT_ERR_SCENE;
        }
    }
    for (int f = 0; f < 6; ++f) s.prims.push_back(rec[f]), s.xforms.emplace_back();
    s.touch();
    return (int)s.prims.size() - 6;
}

// ---------------------------------------------------------------- validation
bool glossy_material_ok(const rt_material &m, size_t textures, const char *where) {
    if (!(m.fuzz >= 0.0f && m.fuzz <= 1.0f)) {  // (a NaN fails the comparison)
        set_error("%s: roughness must be finite and in [0, 1] (got %g)", where, (double)m.fuzz);
        return false;
    }
    if (m.type == RT_MAT_ROUGH_METAL) {
        for (int k = 0; k < 3; ++k)
            if (!(m.albedo[k] >= 0.0f && m.albedo[k] <= 1.0f)) {
                set_error("%s: rough_metal albedo (F0) components must be finite and in [0, 1] (got %g)", where, (double)m.albedo[k]);
                return false;
            }
    } else if (m.type == RT_MAT_ROUGH_GLASS) {  // albedo holds the absorption coefficient
        if (!(m.ir > 1.0f && m.ir < INFINITY)) {
            set_error("%s: rough_glass ir must be finite and > 1 (got %g)", where, (double)m.ir);
            return false;
        }
        for (int k = 0; k < 3; ++k)
            if (!(m.albedo[k] >= 0.0f && m.albedo[k] < INFINITY)) {
                set_error("%s: rough_glass absorption components must be finite and >= 0 (got %g)", where, (double)m.albedo[k]);
                return false;
            }
        if (m.texture != -1) {
            set_error("%s: rough_glass takes no texture (got %d)", where, m.texture);
            return false;
        }
    } else {
        if (m.type == RT_MAT_PBR) {  // albedo[0] holds the metallic factor, the rest of albedo nothing
            if (!(m.albedo[0] >= 0.0f && m.albedo[0] <= 1.0f)) {
                set_error("%s: pbr metallic factor must be finite and in [0, 1] (got %g)", where, (double)m.albedo[0]);
                return false;
            }
            if (m.albedo[1] != 0.0f || m.albedo[2] != 0.0f) {
                set_error("%s: pbr albedo[1..2] must be 0 (got %g, %g)", where, (double)m.albedo[1], (double)m.albedo[2]);
                return false;
            }
        }
        if (!(m.ir > 1.0f && m.ir < INFINITY)) {
            set_error("%s: %s ior must be finite and > 1 (got %g)", where, m.type == RT_MAT_PBR ? "pbr" : "plastic", (double)m.ir);
            return false;
        }
        if (m.texture < 0 || (size_t)m.texture >= textures) {
            set_error("%s references texture %d (have %zu)", where, m.texture, textures);
            return false;
        }
    }
    return true;
}

bool noise_texture_ok(const float c0[3], const float c1[3], const rt_noise &n, const char *where) {
    for (int k = 0; k < 3; ++k)
        if (!(c0[k] >= 0.0f && c0[k] < INFINITY && c1[k] >= 0.0f && c1[k] < INFINITY)) {  // (a NaN fails the comparison)
            set_error("%s: noise texture colours must be finite and >= 0 (got %g, %g)", where, (double)c0[k], (double)c1[k]);
            return false;
        }
    if (n.style < RT_NOISE_STYLE_FBM || n.style > RT_NOISE_STYLE_MARBLE) {
        set_error("%s: noise style must be 0 (fbm), 1 (turbulence) or 2 (marble) (got %d)", where, n.style);
        return false;
    }
    if (!(n.scale > 0.0f && n.scale < INFINITY)) {
        set_error("%s: noise scale must be finite and > 0 (got %g)", where, (double)n.scale);
        return false;
    }
    if (n.octaves < 1 || n.octaves > 8) {
        set_error("%s: noise octaves must be in 1..8 (got %d)", where, n.octaves);
        return false;
    }
    if (n.style == RT_NOISE_STYLE_MARBLE) {
        if (n.axis < 0 || n.axis > 2) {
            set_error("%s: marble axis must be 0 (x), 1 (y) or 2 (z) (got %d)", where, n.axis);
            return false;
        }
        if (!(std::fabs(n.distortion) < INFINITY)) {
            set_error("%s: marble distortion must be finite (got %g)", where, (double)n.distortion);
            return false;
        }
    }
    return true;
}

int add_noise_texture(Scene &s, const float c0[3], const float c1[3], const rt_noise &n, const char *where) {
    if (!c0 || !c1) {
        set_error("%s: noise texture colour is null", where);
        return -RT_ERR_ARG;
    }
    if (!noise_texture_ok(c0, c1, n, where)) return -RT_ERR_ARG;
    rt_texture t;
    memset(&t, 0, sizeof t);
    t.type = RT_TEX_NOISE;
    memcpy(t.c0, c0, sizeof t.c0);
    memcpy(t.c1, c1, sizeof t.c1);
    rt_noise rec = n;
    if (rec.style != RT_NOISE_STYLE_MARBLE) rec.axis = 0, rec.distortion = 0.0f;  // (fields of marble alone)
    s.texs.push_back(t);
    rt_noise none;
    memset(&none, 0, sizeof none);
    s.noise.resize(s.texs.size(), none);
    s.noise.back() = rec;
    s.touch();
    return (int)s.texs.size() - 1;
}

// bump mapping: the argument rules of a bump, shared by the C call, the JSON reader and scene_validate.
// none_ok: texture -1 (no bump) passes
static bool bump_ok(const Scene &s, int material, int texture, float strength, bool none_ok, const char *where) {
    if (material < 0 || material >= (int)s.mats.size()) {
        set_error("%s: unknown material %d (have %zu)", where, material, s.mats.size());
        return false;
    }
    if (s.mats[(size_t)material].type == RT_MAT_DIFFUSE_LIGHT) {
        set_error("%s: material %d is a diffuse_light, which takes no bump", where, material);
        return false;
    }
    if (!(std::fabs(strength) < INFINITY)) {  // (a NaN fails the comparison)
        set_error("%s: bump strength must be finite (got %g)", where, (double)strength);
        return false;
    }
    if (none_ok && texture == -1) return true;
    if (texture < 0 || texture >= (int)s.texs.size() || s.texs[(size_t)texture].type != RT_TEX_NOISE) {
        set_error("%s: bump texture %d is not a noise texture", where, texture);
        return false;
    }
    return true;
}

bool set_bump(Scene &s, int material, int texture, float strength, const char *where) {
    if (!bump_ok(s, material, texture, strength, true, where)) return false;
    if (texture != -1 && strength != 0.0f && scene_normal_map(s, material)) {  // (one of the two)
        set_error("%s: material %d carries a normal map; a material takes a bump or a normal map, not both", where, material);
        return false;
    }
    if (texture == -1 || strength == 0.0f) {  // removes; the table ends at the last bumped material
        if ((size_t)material < s.bumps.size()) s.bumps[(size_t)material] = SceneBump();
        while (!s.bumps.empty() && s.bumps.back().texture < 0) s.bumps.pop_back();
    } else {
        if (s.bumps.size() <= (size_t)material) s.bumps.resize((size_t)material + 1);
        s.bumps[(size_t)material].texture = texture, s.bumps[(size_t)material].strength = strength;
    }
    s.touch();
    return true;
}

// normal maps: the argument rules of a map, shared by the C call, the JSON reader and scene_validate.
// none_ok: texture -1 (no map) passes
static bool normal_map_ok(const Scene &s, int material, int texture, float scale, bool none_ok, const char *where) {
    if (material < 0 || material >= (int)s.mats.size()) {
        set_error("%s: unknown material %d (have %zu)", where, material, s.mats.size());
        return false;
    }
    if (s.mats[(size_t)material].type == RT_MAT_DIFFUSE_LIGHT) {
        set_error("%s: material %d is a diffuse_light, which takes no normal map", where, material);
        return false;
    }
    if (!(std::fabs(scale) < INFINITY)) {  // (a NaN fails the comparison)
        set_error("%s: normal map scale must be finite (got %g)", where, (double)scale);
        return false;
    }
    if (none_ok && texture == -1) return true;
    if (texture < 0 || texture >= (int)s.texs.size() || s.texs[(size_t)texture].type != RT_TEX_IMAGE) {
        set_error("%s: normal map texture %d is not an image texture", where, texture);
        return false;
    }
    if (scale != 0.0f && scene_bump(s, material)) {  // (scale 0 removes, as set_bump's strength 0: removing is always allowed)
        set_error("%s: material %d carries a bump; a material takes a bump or a normal map, not both", where, material);
        return false;
    }
    return true;
}

bool set_normal_map(Scene &s, int material, int texture, float scale, const char *where) {
    if (!normal_map_ok(s, material, texture, scale, true, where)) return false;
    if (texture == -1 || scale == 0.0f) {  // removes; the table ends at the last mapped material
        if ((size_t)material < s.normal_maps.size()) s.normal_maps[(size_t)material] = SceneNormalMap();
        while (!s.normal_maps.empty() && s.normal_maps.back().texture < 0) s.normal_maps.pop_back();
    } else {
        if (s.normal_maps.size() <= (size_t)material) s.normal_maps.resize((size_t)material + 1);
        s.normal_maps[(size_t)material].texture = texture, s.normal_maps[(size_t)material].scale = scale;
    }
    s.touch();
    return true;
}

// alpha masks: the argument rules of a mask, shared by the C call, the JSON reader and scene_validate.
// none_ok: texture -1 (no mask) passes
static bool alpha_ok(const Scene &s, int material, int texture, float cutoff, bool none_ok, const char *where) {
    if (material < 0 || material >= (int)s.mats.size()) {
        set_error("%s: unknown material %d (have %zu)", where, material, s.mats.size());
        return false;
    }
    if (none_ok && texture == -1) return true;
    if (s.mats[(size_t)material].type == RT_MAT_DIFFUSE_LIGHT) {
        set_error("%s: material %d is a diffuse_light, which takes no alpha mask (the light sampler would not know its holes)", where, material);
        return false;
    }
    if (texture < 0 || texture >= (int)s.texs.size() || s.texs[(size_t)texture].type != RT_TEX_IMAGE) {
        set_error("%s: alpha texture %d is not an image texture", where, texture);
        return false;
    }
    const int im = (int)s.texs[(size_t)texture].c0[0];
    if (im < 0 || im >= (int)s.images.size() || s.images[(size_t)im].alpha.empty()) {
        set_error("%s: alpha texture %d has no alpha plane", where, texture);
        return false;
    }
    if (!(cutoff > 0.0f && cutoff <= 1.0f)) {  // (a NaN fails the comparison)
        set_error("%s: alpha cutoff must lie in (0, 1] (got %g)", where, (double)cutoff);
        return false;
    }
    return true;
}

bool set_alpha(Scene &s, int material, int texture, float cutoff, const char *where) {
    if (!alpha_ok(s, material, texture, cutoff, true, where)) return false;
    if (texture == -1) {  // removes; the table ends at the last masked material
        if ((size_t)material < s.alphas.size()) s.alphas[(size_t)material] = SceneAlpha();
        while (!s.alphas.empty() && s.alphas.back().texture < 0) s.alphas.pop_back();
    } else {
        if (s.alphas.size() <= (size_t)material) s.alphas.resize((size_t)material + 1);
        s.alphas[(size_t)material].texture = texture, s.alphas[(size_t)material].cutoff = cutoff;
    }
    s.touch();
    return true;
}

// the metallic-roughness map of a pbr material: the argument rules, shared by the C call, the JSON reader and
// scene_validate.  none_ok: texture -1 (no map) passes
static bool pbr_map_ok(const Scene &s, int material, int texture, bool none_ok, const char *where) {
    if (material < 0 || material >= (int)s.mats.size()) {
        set_error("%s: unknown material %d (have %zu)", where, material, s.mats.size());
        return false;
    }
    if (s.mats[(size_t)material].type != RT_MAT_PBR) {
        set_error("%s: material %d is not a pbr material, which alone takes a metallic-roughness map", where, material);
        return false;
    }
    if (none_ok && texture == -1) return true;
    if (texture < 0 || texture >= (int)s.texs.size()) {
        set_error("%s: metallic-roughness map references texture %d (have %zu)", where, texture, s.texs.size());
        return false;
    }
    return true;
}

bool set_pbr_map(Scene &s, int material, int texture, const char *where) {
    if (!pbr_map_ok(s, material, texture, true, where)) return false;
    if (texture == -1) {  // removes; the table ends at the last mapped material
        if ((size_t)material < s.pbr_maps.size()) s.pbr_maps[(size_t)material] = -1;
        while (!s.pbr_maps.empty() && s.pbr_maps.back() < 0) s.pbr_maps.pop_back();
    } else {
        if (s.pbr_maps.size() <= (size_t)material) s.pbr_maps.resize((size_t)material + 1, -1);
        s.pbr_maps[(size_t)material] = texture;
    }
    s.touch();
    return true;
}

int scene_validate(const Scene &s) {
    if (s.width < 2 || s.height < 2) {
        // u = (x + xi) / (W - 1), main.cu:97-98: W = 1 divides by zero
        set_error("width and height must be >= 2 (got %dx%d)", s.width, s.height);
        return RT_ERR_SCENE;
    }
    // (THIS is the check the kernels rely on for a sample's pixel id: row x width + column is one 24-bit multiply-add there,
    //  which takes both factors below 2^24 -- render_body.h, the refill.  Every entry point validates the scene before it
    //  packs or renders it; the launch path's own width check in render_host.hip guards the tile index it packs, nothing else.
    //  An image this size is a malformed scene rather than a kernel limit, hence RT_ERR_SCENE as before.)
    if (s.width > 65536 || s.height > 65536) {
        set_error("image larger than 65536 on a side (%dx%d)", s.width, s.height);
        return RT_ERR_SCENE;
    }
    // (likewise: a material record's byte offset, 48 x its index, is a 24-bit multiply in the scatter step)
    if (s.mats.size() >= ((size_t)1 << 24)) {
        set_error("%zu materials exceed the kernels' 24-bit material index", s.mats.size());
        return RT_ERR_LIMIT;
    }
    if (s.spp < 1 || s.max_depth < 0) {
        set_error("samples_per_pixel must be >= 1 and max_depth >= 0 (got %d, %d)", s.spp, s.max_depth);
        return RT_ERR_SCENE;
    }
    for (size_t i = 0; i < s.mats.size(); ++i) {
        const rt_material &m = s.mats[i];
        if (m.type == RT_MAT_LAMBERTIAN || m.type == RT_MAT_DIFFUSE_LIGHT) {
            if (m.texture < 0 || m.texture >= (int)s.texs.size()) {
                set_error("material %zu references texture %d (have %zu)", i, m.texture, s.texs.size());
                return RT_ERR_SCENE;
            }
        } else if (is_glossy(m)) {
            char where[32];
            snprintf(where, sizeof where, "material %zu", i);
            if (!glossy_material_ok(m, s.texs.size(), where)) return RT_ERR_SCENE;
        }
    }
    for (size_t i = 0; i < s.bumps.size(); ++i) {
        if (s.bumps[i].texture < 0) continue;
        char where[32];
        snprintf(where, sizeof where, "material %zu", i);
        if (!bump_ok(s, (int)i, s.bumps[i].texture, s.bumps[i].strength, false, where)) return RT_ERR_SCENE;
    }
    for (size_t i = 0; i < s.normal_maps.size(); ++i) {
        if (s.normal_maps[i].texture < 0) continue;
        char where[32];
        snprintf(where, sizeof where, "material %zu", i);
        if (!normal_map_ok(s, (int)i, s.normal_maps[i].texture, s.normal_maps[i].scale, false, where)) return RT_ERR_SCENE;
    }
    for (size_t i = 0; i < s.alphas.size(); ++i) {
        if (s.alphas[i].texture < 0) continue;
        char where[32];
        snprintf(where, sizeof where, "material %zu", i);
        if (!alpha_ok(s, (int)i, s.alphas[i].texture, s.alphas[i].cutoff, false, where)) return RT_ERR_SCENE;
    }
    for (size_t i = 0; i < s.pbr_maps.size(); ++i) {
        if (s.pbr_maps[i] < 0) continue;
        char where[32];
        snprintf(where, sizeof where, "material %zu", i);
        if (!pbr_map_ok(s, (int)i, s.pbr_maps[i], false, where)) return RT_ERR_SCENE;
    }
    for (size_t i = 0; i < s.texs.size(); ++i) {
        const rt_texture &t = s.texs[i];
        if (t.type == RT_TEX_IMAGE) {
            const int im = (int)t.c0[0];
            if (im < 0 || im >= (int)s.images.size() || s.images[im].rows != (int)t.c0[1] || s.images[im].cols != (int)t.c0[2] ||
                s.images[im].rgb.size() != (size_t)s.images[im].rows * s.images[im].cols * 3 ||
                (!s.images[im].alpha.empty() && s.images[im].alpha.size() != (size_t)s.images[im].rows * s.images[im].cols)) {
                set_error("texture %zu references image %d, which is missing or has another size", i, im);
                return RT_ERR_SCENE;
            }
        } else if (t.type == RT_TEX_NOISE) {
            char where[32];
            snprintf(where, sizeof where, "texture %zu", i);
            if (i >= s.noise.size()) {
                set_error("texture %zu is a noise texture without parameters", i);
                return RT_ERR_SCENE;
            }
            if (!noise_texture_ok(t.c0, t.c1, s.noise[i], where)) return RT_ERR_SCENE;
        } else if (t.type != RT_TEX_SOLID && t.type != RT_TEX_CHECKER) {
            set_error("texture %zu has unknown type %d", i, t.type);
            return RT_ERR_SCENE;
        }
    }
    for (size_t i = 0; i < s.prims.size(); ++i) {
        const rt_prim &p = s.prims[i];
        if (p.type < RT_PRIM_SPHERE || p.type > RT_PRIM_QUAD) {
            set_error("object %zu has unknown type %d", i, p.type);
            return RT_ERR_SCENE;
        }
        if (p.material < 0 || p.material >= (int)s.mats.size()) {
            set_error("object %zu references material %d (have %zu)", i, p.material, s.mats.size());
            return RT_ERR_SCENE;
        }
        if (p.type == RT_PRIM_SPHERE && p.f[3] == 0.0f) {
            set_error("object %zu: sphere radius is zero", i);
            return RT_ERR_SCENE;
        }
    }
    for (size_t i = 0; i < s.movers.size(); ++i)
        if (s.movers[i].material < 0 || s.movers[i].material >= (int)s.mats.size()) {
            set_error("moving sphere %zu references material %d (have %zu)", i, s.movers[i].material, s.mats.size());
            return RT_ERR_SCENE;
        }
    double d[3];
    v3sub(s.cam.lookfrom, s.cam.lookat, d);
    if (!(v3len(d) > 0)) {
        set_error("camera lookfrom equals lookat");
        return RT_ERR_SCENE;
    }
    return RT_OK;
}

// ---------------------------------------------------------------- image textures, triangles, meshes
int add_image_texture(Scene &s, int rows, int cols, const uint8_t *rgb, const std::string &file, const uint8_t *alpha) {
    if (rows < 1 || cols < 1 || rows > 16384 || cols > 16384 || !rgb) {
        set_error("image texture: rows and cols must be in 1..16384 and the pixels not null (got %d x %d)", rows, cols);
        return -RT_ERR_ARG;
    }
    SceneImage im;
    im.rows = rows, im.cols = cols, im.file = file;
    im.rgb.assign(rgb, rgb + (size_t)rows * cols * 3);
    if (alpha) im.alpha.assign(alpha, alpha + (size_t)rows * cols);
    s.images.push_back(std::move(im));
    rt_texture t;
    memset(&t, 0, sizeof t);
    t.type = RT_TEX_IMAGE;
    t.c0[0] = (float)(s.images.size() - 1), t.c0[1] = (float)rows, t.c0[2] = (float)cols;
    s.texs.push_back(t);
    s.touch();
    return (int)s.texs.size() - 1;
}

// P6 (binary) or P3 (text) PPM with maxval 255; '#' comments allowed in the header
static int read_ppm(const char *path, int &rows, int &cols, std::vector<uint8_t> &rgb) {
    FILE *fp = fopen(path, "rb");
    if (!fp) {
        set_error("cannot open %s", path);
        return RT_ERR_IO;
    }
    std::vector<unsigned char> buf;
    unsigned char chunk[65536];
    size_t n;
    while ((n = fread(chunk, 1, sizeof chunk, fp)) > 0) buf.insert(buf.end(), chunk, chunk + n);
    fclose(fp);
    size_t pos = 0;
    auto token = [&](long &out) -> bool {  // next unsigned integer of the header / a P3 body
        for (;;) {
            while (pos < buf.size() && isspace(buf[pos])) ++pos;
            if (pos < buf.size() && buf[pos] == '#') {
                while (pos < buf.size() && buf[pos] != '\n') ++pos;
                continue;
            }
            break;
        }
        if (pos >= buf.size() || !isdigit(buf[pos])) return false;
        long v = 0;
        while (pos < buf.size() && isdigit(buf[pos])) {
            v = v * 10 + (buf[pos++] - '0');
            if (v > 100000000) return false;
        }
        out = v;
        return true;
    };
    if (buf.size() < 2 || buf[0] != 'P' || (buf[1] != '6' && buf[1] != '3')) {
        set_error("%s is not a PPM file (P6 or P3)", path);
        return RT_ERR_IO;
    }
    const bool binary = buf[1] == '6';
    pos = 2;
    long w = 0, h = 0, mx = 0;
    if (!token(w) || !token(h) || !token(mx) || w < 1 || h < 1 || w > 16384 || h > 16384 || mx != 255) {
        set_error("%s: unsupported PPM header (need width, height <= 16384 and maxval 255)", path);
        return RT_ERR_IO;
    }
    rows = (int)h, cols = (int)w;
    const size_t need = (size_t)w * h * 3;
    rgb.resize(need);
    if (binary) {
        ++pos;  // the single whitespace byte after maxval
        if (buf.size() - pos < need) {
            set_error("%s is truncated", path);
            return RT_ERR_IO;
        }
        memcpy(rgb.data(), buf.data() + pos, need);
    } else {
        for (size_t i = 0; i < need; ++i) {
            long v = 0;
            if (!token(v) || v > 255) {
                set_error("%s: bad or missing sample %zu", path, i);
                return RT_ERR_IO;
            }
            rgb[i] = (uint8_t)v;
        }
    }
    return RT_OK;
}

int read_image_file(const char *path, int &rows, int &cols, std::vector<uint8_t> &rgb, std::vector<uint8_t> *alpha) {
    if (alpha) alpha->clear();
    // PNG by signature (8-bit, non-interlaced), else PPM
    bool is_png = false;
    if (FILE *fp = fopen(path, "rb")) {
        unsigned char sig[8] = {0};
        is_png = fread(sig, 1, 8, fp) == 8 && sig[0] == 137 && sig[1] == 'P' && sig[2] == 'N' && sig[3] == 'G';
        std::vector<uint8_t> file;
        if (is_png) {
            fseek(fp, 0, SEEK_SET);
            unsigned char chunk[65536];
            size_t n;
            while ((n = fread(chunk, 1, sizeof chunk, fp)) > 0) file.insert(file.end(), chunk, chunk + n);
        }
        fclose(fp);
        if (is_png) {
            std::string err;
            if (!png::read(file, rows, cols, rgb, err, alpha)) {
                set_error("%s: %s", path, err.c_str());
                return RT_ERR_IO;
            }
            return RT_OK;
        }
    }
    return read_ppm(path, rows, cols, rgb);
}

int add_image_texture_file(Scene &s, const char *path) {
    int rows = 0, cols = 0;
    std::vector<uint8_t> rgb, alpha;
    int rc = read_image_file(path, rows, cols, rgb, &alpha);
    if (rc) return -rc;
    return add_image_texture(s, rows, cols, rgb.data(), path, alpha.empty() ? nullptr : alpha.data());
}

// Triangle.__init__, taichi-version/hittable.py:95-110: the unit normal (v2 - v1) x (v3 - v1) / |..| is a
// constructor value there too; derived in fp64 from the fp32 vertices and rounded once
int add_triangle(Scene &s, const float v1[3], const float v2[3], const float v3[3], const float uv1[2], const float uv2[2],
                 const float uv3[2], int material) {
    double a[3], b[3], n[3];
    for (int k = 0; k < 3; ++k) a[k] = (double)v2[k] - (double)v1[k], b[k] = (double)v3[k] - (double)v1[k];
    v3cross(a, b, n);
    const double len = v3len(n);
    if (!(len > 0) || !std::isfinite(len)) {
        set_error("triangle with zero area (or non-finite vertices)");
        return -RT_ERR_SCENE;
    }
    rt_prim p;
    memset(&p, 0, sizeof p);
    p.type = RT_PRIM_TRIANGLE;
    p.material = material;
    for (int k = 0; k < 3; ++k) {
        p.m[k] = v1[k], p.m[3 + k] = v2[k], p.m[6 + k] = v3[k];
        p.m[9 + k] = (float)(n[k] / len);
    }
    const float *uv[3] = {uv1, uv2, uv3};
    for (int c = 0; c < 3; ++c)
        if (uv[c]) p.m_inv[2 * c] = uv[c][0], p.m_inv[2 * c + 1] = uv[c][1];
    s.prims.push_back(p);
    s.xforms.emplace_back();
    s.touch();
    return (int)s.prims.size() - 1;
}

// Smooth shading: the three vertex normals of triangle p, normalised in fp64 and rounded once, into the words
// a triangle leaves unused (include/rtmi.h, RT_PRIM_TRIANGLE).  False: a normal is zero or not finite.
static bool store_tri_normals(rt_prim &p, const double n[3][3]) {
    float *dst[3] = {p.f, p.f + 3, p.m_inv + 6};
    for (int c = 0; c < 3; ++c) {
        const double len = v3len(n[c]);
        if (!(len > 0) || !std::isfinite(len)) return false;
        // (a vector within fp32 rounding of unit length -- sqrt(3) x 2^-24 -- is one that was stored before: kept bit for bit,
        //  so that a scene written to JSON and read back has the same normals)
        const double div = std::fabs(len - 1.0) <= 1.5e-7 ? 1.0 : len;
        for (int k = 0; k < 3; ++k) dst[c][k] = (float)(n[c][k] / div);
    }
    return true;
}

int add_triangle_normals(Scene &s, const float v1[3], const float v2[3], const float v3[3], const float n1[3], const float n2[3],
                         const float n3[3], const float uv1[2], const float uv2[2], const float uv3[2], int material) {
    const float *nn[3] = {n1, n2, n3};
    double n[3][3];
    rt_prim probe;
    memset(&probe, 0, sizeof probe);
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 3; ++k) n[c][k] = (double)nn[c][k];
    if (!store_tri_normals(probe, n)) {
        set_error("triangle vertex normal is zero or not finite");
        return -RT_ERR_ARG;
    }
    const int id = add_triangle(s, v1, v2, v3, uv1, uv2, uv3, material);
    if (id < 0) return id;
    store_tri_normals(s.prims[(size_t)id], n);
    return id;
}

static thread_local int g_mesh_normals_mode = -1;
static thread_local float g_mesh_normals_crease = 180.0f;
void set_mesh_normals_override(int mode, float crease_degrees) { g_mesh_normals_mode = mode, g_mesh_normals_crease = crease_degrees; }

int add_obj(Scene &s, const char *path, int material, float scale, const float matrix[9], const float translate[3]) {
    return add_obj_normals(s, path, material, scale, matrix, translate, RT_MESH_NORMALS_FLAT, 0.0f);
}

// readobj(), taichi-version/main.py:23-41, and the placement of main.py:110-118 (scale * Rot @ x + dis); the vertex
// normals of smooth shading by `mode` (rt_mesh_normals, include/rtmi.h)
int add_obj_normals(Scene &s, const char *path, int material, float scale, const float matrix[9], const float translate[3], int mode,
                    float crease_degrees) {
    if (mode < RT_MESH_NORMALS_FLAT || mode > RT_MESH_NORMALS_SMOOTH) {
        set_error("mesh normals mode %d (0 flat, 1 file, 2 smooth)", mode);
        return -RT_ERR_ARG;
    }
    if (mode == RT_MESH_NORMALS_SMOOTH && !(crease_degrees >= 0.0f && crease_degrees <= 180.0f)) {
        set_error("mesh crease angle %g outside [0, 180] degrees", (double)crease_degrees);
        return -RT_ERR_ARG;
    }
    FILE *fp = fopen(path, "r");
    if (!fp) {
        set_error("cannot open %s", path);
        return -RT_ERR_IO;
    }
    std::vector<std::array<float, 3>> pts;
    std::vector<std::array<float, 2>> vts;
    std::vector<std::array<double, 3>> vns;
    struct Corner {
        long v, t, n;
    };
    std::vector<std::array<Corner, 3>> faces;
    char line[1024];
    int lineno = 0;
    bool bad = false;
    while (fgets(line, sizeof line, fp)) {
        ++lineno;
        char *p = line;
        while (*p == ' ' || *p == '\t') ++p;
        if (p[0] == 'v' && (p[1] == ' ' || p[1] == '\t')) {
            double x, y, z;
            if (sscanf(p + 1, "%lf %lf %lf", &x, &y, &z) != 3) bad = true;
            else pts.push_back({(float)x, (float)y, (float)z});
        } else if (p[0] == 'v' && p[1] == 't' && (p[2] == ' ' || p[2] == '\t')) {
            double u, v;
            if (sscanf(p + 2, "%lf %lf", &u, &v) != 2) bad = true;
            else vts.push_back({(float)u, (float)v});
        } else if (mode == RT_MESH_NORMALS_FILE && p[0] == 'v' && p[1] == 'n' && (p[2] == ' ' || p[2] == '\t')) {
            double x, y, z;
            if (sscanf(p + 2, "%lf %lf %lf", &x, &y, &z) != 3) bad = true;
            else vns.push_back({x, y, z});
        } else if (p[0] == 'f' && (p[1] == ' ' || p[1] == '\t')) {
            std::array<Corner, 3> f;
            char *q = p + 1;
            int got = 0;
            for (; got < 3; ++got) {
                while (*q == ' ' || *q == '\t') ++q;
                char *e;
                long vi = strtol(q, &e, 10), ti = 0, ni = 0;
                if (e == q) break;
                q = e;
                if (*q == '/') {  // a/t or a/t/n or a//n
                    ++q;
                    ti = strtol(q, &e, 10);
                    q = e;
                    if (*q == '/') {
                        ++q;
                        ni = strtol(q, &e, 10);
                        if (e != q && ni == 0) ni = -1;  // "0" is written but names nothing: out of range below
                        q = e;
                    }
                }
                f[got] = {vi, ti ? ti : vi, ni};  // without vt indices the reference takes texids[face corner]
            }
            if (got != 3) bad = true;
            else faces.push_back(f);
        }
        if (bad) break;
    }
    fclose(fp);
    if (bad) {
        set_error("%s:%d: cannot parse this line", path, lineno);
        return -RT_ERR_IO;
    }
    // the placed corners of every face, then its unit normal and corner angles in fp64 (what add_triangle derives too)
    struct Face {
        float v[3][3], uv[3][2];
        double n[3], angle[3];
    };
    std::vector<Face> placed(faces.size());
    for (size_t i = 0; i < faces.size(); ++i) {
        Face &F = placed[i];
        for (int c = 0; c < 3; ++c) {
            const long vi = faces[i][c].v, ti = faces[i][c].t;
            if (vi < 1 || vi > (long)pts.size()) {
                set_error("%s: face refers to vertex %ld (have %zu)", path, vi, pts.size());
                return -RT_ERR_SCENE;
            }
            const auto &x = pts[vi - 1];
            for (int r = 0; r < 3; ++r) {
                double m = matrix ? (double)matrix[3 * r] * x[0] + (double)matrix[3 * r + 1] * x[1] + (double)matrix[3 * r + 2] * x[2]
                                  : (double)x[r];
                F.v[c][r] = (float)((double)scale * m + (translate ? (double)translate[r] : 0.0));
            }
            F.uv[c][0] = F.uv[c][1] = 0.0f;
            if (ti >= 1 && ti <= (long)vts.size()) F.uv[c][0] = vts[ti - 1][0], F.uv[c][1] = vts[ti - 1][1];
        }
        if (mode == RT_MESH_NORMALS_FLAT) continue;
        double e[3][3];  // e[c]: from corner c to corner c + 1
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 3; ++k) e[c][k] = (double)F.v[(c + 1) % 3][k] - (double)F.v[c][k];
        const double back[3] = {-e[2][0], -e[2][1], -e[2][2]};  // v3 - v1
        v3cross(e[0], back, F.n);
        const double len = v3len(F.n);
        if (!(len > 0) || !std::isfinite(len)) {
            set_error("%s: face %zu has zero area (or non-finite vertices)", path, i + 1);
            return -RT_ERR_SCENE;
        }
        for (int k = 0; k < 3; ++k) F.n[k] /= len;
        for (int c = 0; c < 3; ++c) {  // the angle at corner c, between the edges that leave it
            const double *a = e[c], *b = e[(c + 2) % 3];
            double x[3];
            v3cross(a, b, x);
            F.angle[c] = std::atan2(v3len(x), -(a[0] * b[0] + a[1] * b[1] + a[2] * b[2]));
        }
    }
    // FILE: n -> (scale M)^-T n, up to a positive factor cof(M) n x sign(scale det M)
    double cof[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, flip = scale < 0.0f ? -1.0 : 1.0;
    if (matrix) {
        const float *m = matrix;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                cof[3 * r + c] = (double)m[3 * r1 + c1] * m[3 * r2 + c2] - (double)m[3 * r1 + c2] * m[3 * r2 + c1];
            }
        const double det = m[0] * cof[0] + m[1] * cof[1] + m[2] * cof[2];
        if (det < 0) flip = -flip;
    }
    // SMOOTH: the corners that share a placed position
    std::map<std::array<float, 3>, std::vector<std::pair<int, int>>> at;
    if (mode == RT_MESH_NORMALS_SMOOTH)
        for (size_t i = 0; i < placed.size(); ++i)
            for (int c = 0; c < 3; ++c) at[{placed[i].v[c][0], placed[i].v[c][1], placed[i].v[c][2]}].push_back({(int)i, c});
    const double cos_crease = std::cos((double)crease_degrees * std::acos(-1.0) / 180.0) - 1e-12;
    int added = 0;
    for (size_t i = 0; i < placed.size(); ++i) {
        const Face &F = placed[i];
        int rc;
        if (mode == RT_MESH_NORMALS_FLAT) {
            rc = add_triangle(s, F.v[0], F.v[1], F.v[2], F.uv[0], F.uv[1], F.uv[2], material);
        } else {
            double n[3][3];
            for (int c = 0; c < 3; ++c) {
                double *o = n[c];
                o[0] = F.n[0], o[1] = F.n[1], o[2] = F.n[2];  // a corner without a normal of its own: the face's
                if (mode == RT_MESH_NORMALS_FILE) {
                    const long ni = faces[i][c].n;
                    if (ni == 0) continue;
                    if (ni < 1 || ni > (long)vns.size()) {
                        set_error("%s: face refers to normal %ld (have %zu)", path, ni, vns.size());
                        return -RT_ERR_SCENE;
                    }
                    const auto &x = vns[ni - 1];
                    double t[3];
                    for (int r = 0; r < 3; ++r) t[r] = flip * (cof[3 * r] * x[0] + cof[3 * r + 1] * x[1] + cof[3 * r + 2] * x[2]);
                    const double len = v3len(t);
                    if (len > 0 && std::isfinite(len)) o[0] = t[0] / len, o[1] = t[1] / len, o[2] = t[2] / len;
                } else {
                    double sum[3] = {0, 0, 0};
                    for (const auto &fc : at[{F.v[c][0], F.v[c][1], F.v[c][2]}]) {
                        const Face &G = placed[(size_t)fc.first];
                        if (G.n[0] * F.n[0] + G.n[1] * F.n[1] + G.n[2] * F.n[2] < cos_crease) continue;
                        for (int k = 0; k < 3; ++k) sum[k] += G.angle[fc.second] * G.n[k];
                    }
                    const double len = v3len(sum);
                    if (len > 0 && std::isfinite(len)) o[0] = sum[0] / len, o[1] = sum[1] / len, o[2] = sum[2] / len;
                }
            }
            const float nf[3][3] = {{(float)n[0][0], (float)n[0][1], (float)n[0][2]},
                                    {(float)n[1][0], (float)n[1][1], (float)n[1][2]},
                                    {(float)n[2][0], (float)n[2][1], (float)n[2][2]}};
            rc = add_triangle_normals(s, F.v[0], F.v[1], F.v[2], nf[0], nf[1], nf[2], F.uv[0], F.uv[1], F.uv[2], material);
        }
        if (rc < 0) return rc;
        ++added;
    }
    return added;
}

// ---------------------------------------------------------------- JSON in
namespace {

struct Reader {
    bool ok = true;
    void fail(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
        if (!ok) return;
        ok = false;
        char buf[400];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        set_error("%s", buf);
    }
    double num(const JsonValue &o, const char *key, const char *where) {
        const JsonValue *v = o.find(key);
        if (!v || !v->is_number()) {
            fail("%s: missing or non-numeric \"%s\"", where, key);
            return 0;
        }
        return v->num;
    }
    int integer(const JsonValue &o, const char *key, const char *where) {
        double d = num(o, key, where);
        if (ok && (d != std::floor(d) || std::fabs(d) > 1e9)) fail("%s: \"%s\" must be an integer", where, key);
        return (int)d;
    }
    void vec3(const JsonValue &o, const char *key, const char *where, double out[3]) {
        const JsonValue *v = o.find(key);
        if (!v || !v->is_array() || v->arr.size() != 3 || !v->arr[0].is_number() || !v->arr[1].is_number() ||
            !v->arr[2].is_number()) {
            fail("%s: \"%s\" must be an array of 3 numbers", where, key);
            out[0] = out[1] = out[2] = 0;
            return;
        }
        for (int i = 0; i < 3; ++i) out[i] = v->arr[i].num;
    }
    const JsonValue *data_array(const JsonValue &root, const char *key) {
        // {"object": {"data": [...]}} (parser.hpp:519-521)
        const JsonValue *o = root.find(key);
        if (!o || !o->is_object()) {
            fail("top level: missing object \"%s\"", key);
            return nullptr;
        }
        const JsonValue *d = o->find("data");
        if (!d || !d->is_array()) {
            fail("\"%s\": missing array \"data\"", key);
            return nullptr;
        }
        return d;
    }
};

}  // namespace

int scene_from_json(const char *text, size_t len, Scene &s, const char *base_dir) {
    auto resolve = [&](const std::string &file) {  // relative "file" entries: next to the scene file
        if (file.empty() || file[0] == '/' || !base_dir || !*base_dir) return file;
        return std::string(base_dir) + "/" + file;
    };
    JsonValue root;
    std::string perr;
    JsonParser parser(text, len);
    if (!parser.parse(root, perr)) {
        set_error("%s", perr.c_str());
        return RT_ERR_JSON;
    }
    if (!root.is_object()) {
        set_error("top level of a scene file must be an object");
        return RT_ERR_SCENE;
    }
    Reader r;
    char where[96];

    // scalars, parser.hpp:512-517
    double bg[3];
    r.vec3(root, "background", "top level", bg);
    s.background[0] = (float)bg[0], s.background[1] = (float)bg[1], s.background[2] = (float)bg[2];
    s.max_depth = r.integer(root, "max_depth", "top level");
    s.spp = r.integer(root, "samples_per_pixel", "top level");
    s.width = r.integer(root, "width", "top level");
    s.height = r.integer(root, "height", "top level");
    if (const JsonValue *of = root.find("output_file")) {
        if (!of->is_string()) r.fail("top level: \"output_file\" must be a string");
        else s.output_file = of->str;
    }
    // The JSON interface is gpu-version's, whose camera::get_ray has the lens sample commented out
    // (camera.cuh:33-34: rd = 0, no draws): a scene file that does not say otherwise renders without defocus
    // blur, like `parallel_compute -f scene.json`.  "defocus_blur": true selects cmake-cpu-version/camera.h:34.
    s.flags = 0;
    if (const JsonValue *f = root.find("sky_gradient")) {
        if (f->kind != JsonValue::Bool) r.fail("top level: \"sky_gradient\" must be a boolean");
        else if (f->b) s.flags |= RT_FLAG_SKY_GRADIENT;
    }
    if (const JsonValue *f = root.find("defocus_blur")) {
        if (f->kind != JsonValue::Bool) r.fail("top level: \"defocus_blur\" must be a boolean");
        else if (f->b) s.flags |= RT_FLAG_DEFOCUS_BLUR;
    }
    if (root.find("russian_roulette")) {
        const double p = r.num(root, "russian_roulette", "top level");
        if (!(p >= 0.0 && p <= 1.0)) r.fail("top level: \"russian_roulette\" must be a probability in [0, 1]");
        else s.rr_p = (float)p;
    }
    if (const JsonValue *f = root.find("light_sampling")) {
        if (f->kind != JsonValue::Bool) r.fail("top level: \"light_sampling\" must be a boolean");
        else s.light_sampling = f->b;
    }
    if (const JsonValue *f = root.find("media_light_sampling")) {
        if (f->kind != JsonValue::Bool) r.fail("top level: \"media_light_sampling\" must be a boolean");
        else s.media_light_sampling = f->b;
    }
    if (const JsonValue *f = root.find("mesh_lights")) {
        if (f->kind != JsonValue::Bool) r.fail("top level: \"mesh_lights\" must be a boolean");
        else s.mesh_lights = f->b;
    }
    if (const JsonValue *f = root.find("nested_grid")) {
        if (f->kind != JsonValue::Bool) r.fail("top level: \"nested_grid\" must be a boolean");
        else s.nested_grid = f->b;
    }
    // "environment": {"file": path} or {"rows", "cols", "data": [rows x cols x 3 numbers]}, with optional "scale", "rotate"
    int env_rc = RT_OK;
    if (const JsonValue *e = root.find("environment")) {
        if (!e->is_object()) r.fail("top level: \"environment\" must be an object");
        else {
            const double scale = e->find("scale") ? r.num(*e, "scale", "environment") : 1.0;
            const double rotate = e->find("rotate") ? r.num(*e, "rotate", "environment") : 0.0;
            const JsonValue *f = e->find("file");
            if (f && !f->is_string()) r.fail("environment: \"file\" must be a string");
            else if (r.ok && f) {
                env_rc = set_environment_file(s, resolve(f->str).c_str(), (float)scale, (float)rotate);
                if (env_rc == RT_OK) {  // (written back as given)
                    auto named = std::make_shared<SceneEnvironment>(*s.env);
                    named->file = f->str;
                    s.env = named;
                }
            } else if (r.ok) {
                const int rows = r.integer(*e, "rows", "environment"), cols = r.integer(*e, "cols", "environment");
                const JsonValue *d = e->find("data");
                if (r.ok && (rows < 1 || cols < 1)) r.fail("environment: \"rows\" and \"cols\" must be positive");
                if (r.ok && (long long)rows * cols > kEnvMaxTexels) {
                    set_error("environment map of %d x %d texels exceeds the limit of %lld", rows, cols, kEnvMaxTexels);
                    return RT_ERR_LIMIT;
                }
                if (r.ok && (!d || !d->is_array() || d->arr.size() != (size_t)rows * (size_t)cols * 3))
                    r.fail("environment: \"data\" must be an array of rows x cols x 3 numbers");
                if (r.ok) {
                    std::vector<float> rgb(d->arr.size());
                    for (size_t i = 0; i < rgb.size() && r.ok; ++i) {
                        if (!d->arr[i].is_number()) r.fail("environment: \"data\" entry %zu is not a number", i);
                        else rgb[i] = (float)d->arr[i].num;
                    }
                    if (r.ok) env_rc = set_environment(s, rows, cols, rgb.data(), (float)scale, (float)rotate, "");
                }
            }
        }
    }
    if (r.ok && env_rc != RT_OK) return env_rc == RT_ERR_ARG ? RT_ERR_SCENE : env_rc;
    // "media": {"data": [{"type": "sphere", "center", "radius", "density", "albedo"}, {"type": "box", "min", "max", "density", "albedo"}]}
    // and on either, optionally, "g": the asymmetry of the phase function
    s.media.clear();
    s.media_g.clear();
    if (root.find("media")) {
        if (const JsonValue *arr = r.data_array(root, "media")) {
            for (size_t i = 0; i < arr->arr.size() && r.ok; ++i) {
                const JsonValue &t = arr->arr[i];
                snprintf(where, sizeof where, "medium %zu", i);
                const JsonValue *ty = t.find("type");
                if (!t.is_object() || !ty || !ty->is_string()) {
                    r.fail("%s: missing string \"type\"", where);
                    break;
                }
                rt_medium m;
                memset(&m, 0, sizeof m);
                double v[3], w[3];
                if (ty->str == "sphere") {
                    m.shape = RT_MEDIUM_SPHERE;
                    r.vec3(t, "center", where, v);
                    for (int k = 0; k < 3; ++k) m.f[k] = (float)v[k];
                    m.f[3] = (float)r.num(t, "radius", where);
                } else if (ty->str == "box") {
                    m.shape = RT_MEDIUM_BOX;
                    r.vec3(t, "min", where, v);
                    r.vec3(t, "max", where, w);
                    for (int k = 0; k < 3; ++k) m.f[k] = (float)v[k], m.f[3 + k] = (float)w[k];
                } else {
                    r.fail("%s: unknown type \"%s\" (sphere, box)", where, ty->str.c_str());
                    break;
                }
                m.density = (float)r.num(t, "density", where);
                r.vec3(t, "albedo", where, v);
                for (int k = 0; k < 3; ++k) m.albedo[k] = (float)v[k];
                const float g = t.find("g") ? (float)r.num(t, "g", where) : 0.0f;
                if (!r.ok) break;
                int rc = add_medium(s, m);
                if (rc >= 0) rc = -set_medium_phase(s, rc, g);
                if (rc < 0) {  // (the record's own message, with its place in the file)
                    const std::string why = get_error();
                    set_error("%s: %s", where, why.c_str());
                    return -rc;
                }
            }
        }
    }
    // "lights": [{"type": "point" | "spot" | "distant", ...}]; without a "light_sampling" key they switch it on
    s.alights.clear();
    if (const JsonValue *arr = root.find("lights")) {
        if (!arr->is_array()) r.fail("top level: \"lights\" must be an array");
        for (size_t i = 0; r.ok && i < arr->arr.size(); ++i) {
            const JsonValue &t = arr->arr[i];
            snprintf(where, sizeof where, "light %zu", i);
            const JsonValue *ty = t.find("type");
            if (!t.is_object() || !ty || !ty->is_string()) {
                r.fail("%s: missing string \"type\"", where);
                break;
            }
            auto only_keys = [&](std::initializer_list<const char *> known) {  // (a field the type does not have is an error)
                for (const auto &kv : t.obj) {
                    bool found = false;
                    for (const char *k : known) found = found || kv.first == k;
                    if (!found && r.ok) r.fail("%s: a %s light has no field \"%s\"", where, ty->str.c_str(), kv.first.c_str());
                }
            };
            rt_analytic_light l;
            memset(&l, 0, sizeof l);
            double v[3] = {0, 0, 0}, w[3] = {0, 0, 0};
            if (ty->str == "point") {
                only_keys({"type", "position", "intensity"});
                l.type = RT_LIGHT_POINT;
                r.vec3(t, "position", where, v);
                for (int k = 0; k < 3; ++k) l.position[k] = (float)v[k];
                r.vec3(t, "intensity", where, v);
            } else if (ty->str == "spot") {
                only_keys({"type", "position", "direction", "target", "intensity", "inner_angle", "outer_angle"});
                l.type = RT_LIGHT_SPOT;
                r.vec3(t, "position", where, v);
                for (int k = 0; k < 3; ++k) l.position[k] = (float)v[k];
                const bool has_dir = t.find("direction") != nullptr, has_target = t.find("target") != nullptr;
                if (r.ok && has_dir == has_target) r.fail("%s: a spot light takes one of \"direction\" and \"target\"", where);
                if (r.ok) {
                    r.vec3(t, has_dir ? "direction" : "target", where, w);
                    for (int k = 0; k < 3; ++k) l.direction[k] = (float)(has_dir ? w[k] : w[k] - v[k]);
                }
                l.angle[0] = (float)r.num(t, "inner_angle", where);
                l.angle[1] = (float)r.num(t, "outer_angle", where);
                r.vec3(t, "intensity", where, v);
            } else if (ty->str == "distant") {
                only_keys({"type", "direction", "irradiance", "angular_radius"});
                l.type = RT_LIGHT_DISTANT;
                r.vec3(t, "direction", where, w);
                for (int k = 0; k < 3; ++k) l.direction[k] = (float)w[k];
                if (t.find("angular_radius")) l.angle[0] = (float)r.num(t, "angular_radius", where);
                r.vec3(t, "irradiance", where, v);
            } else {
                r.fail("%s: unknown type \"%s\" (point, spot, distant)", where, ty->str.c_str());
                break;
            }
            for (int k = 0; k < 3; ++k) l.color[k] = (float)v[k];
            if (!r.ok) break;
            if (!analytic_light_ok(l, where)) return RT_ERR_SCENE;
            s.alights.push_back(l);
        }
        if (r.ok && !root.find("light_sampling")) s.light_sampling = true;
    }

    // camera, parser.hpp:113-141
    const JsonValue *cam = root.find("camera");
    if (!cam || !cam->is_object()) r.fail("top level: missing object \"camera\"");
    else {
        r.vec3(*cam, "lookfrom", "camera", s.cam.lookfrom);
        r.vec3(*cam, "lookat", "camera", s.cam.lookat);
        r.vec3(*cam, "vup", "camera", s.cam.vup);
        s.cam.vfov = r.num(*cam, "vfov", "camera");
        s.cam.aperture = r.num(*cam, "aperture", "camera");
        s.cam.aspect = 0.0;      // width / height (parser.hpp:122)
        s.cam.focus_dist = 0.0;  // |lookfrom - lookat| (parser.hpp:124)
        if (const JsonValue *fd = cam->find("focus_dist")) {
            if (fd->is_number() && fd->num > 0) s.cam.focus_dist = fd->num;
            else r.fail("camera: \"focus_dist\" must be a positive number");
        }
        // "projection": {"type": ..., parameters}; absent: perspective
        s.cam.projection = RT_PROJ_PERSPECTIVE, s.cam.proj[0] = s.cam.proj[1] = 0.0;
        if (const JsonValue *pj = cam->find("projection")) {
            const JsonValue *ty = pj->is_object() ? pj->find("type") : nullptr;
            if (!ty || !ty->is_string()) r.fail("camera: \"projection\" must be an object with a string \"type\"");
            else {
                int type = -1;
                for (int k = 0; k < 4; ++k)
                    if (ty->str == projection_name(k)) type = k;
                // the fields of each type, the first two in the order of CameraParams::proj; {default, or 0: required}
                static const char *const fields[4][2] = {{nullptr, nullptr}, {"height", nullptr}, {"hfov", "vfov"}, {"fov", nullptr}};
                static const double defaults[4][2] = {{0, 0}, {0, 0}, {360, 180}, {180, 0}};
                if (type < 0) r.fail("camera: projection: unknown type \"%s\" (perspective, orthographic, panoramic, fisheye)", ty->str.c_str());
                else {
                    for (const auto &kv : pj->obj) {
                        bool known = kv.first == "type";
                        for (int k = 0; k < 2; ++k) known = known || (fields[type][k] && kv.first == fields[type][k]);
                        if (!known) r.fail("camera: projection: unknown field \"%s\" of type \"%s\"", kv.first.c_str(), ty->str.c_str());
                    }
                    double p[2] = {0, 0};
                    for (int k = 0; k < 2 && r.ok; ++k) {
                        if (!fields[type][k]) continue;
                        const JsonValue *f = pj->find(fields[type][k]);
                        if (f && !f->is_number()) r.fail("camera: projection: \"%s\" must be a number", fields[type][k]);
                        else if (f) p[k] = f->num;
                        else if (defaults[type][k] > 0) p[k] = defaults[type][k];
                        else r.fail("camera: projection: missing number \"%s\"", fields[type][k]);
                    }
                    if (r.ok) {
                        if (!projection_ok(type, p, "camera: projection")) return RT_ERR_SCENE;
                        s.cam.projection = type, s.cam.proj[0] = p[0], s.cam.proj[1] = p[1];
                    }
                }
            }
        }
    }
    if (!r.ok) return RT_ERR_SCENE;

    // textures, parser.hpp:143-184 (+ checker, texture.cuh:33-57)
    if (const JsonValue *arr = r.data_array(root, "texture")) {
        for (size_t i = 0; i < arr->arr.size() && r.ok; ++i) {
            const JsonValue &t = arr->arr[i];
            snprintf(where, sizeof where, "texture %zu", i);
            const JsonValue *ty = t.find("type");
            if (!t.is_object() || !ty || !ty->is_string()) {
                r.fail("%s: missing string \"type\"", where);
                break;
            }
            rt_texture rec;
            memset(&rec, 0, sizeof rec);
            double c[3];
            if (ty->str == "solid_color") {
                rec.type = RT_TEX_SOLID;
                r.vec3(t, "color", where, c);
                for (int k = 0; k < 3; ++k) rec.c0[k] = rec.c1[k] = (float)c[k];
            } else if (ty->str == "checker") {
                rec.type = RT_TEX_CHECKER;
                r.vec3(t, "even", where, c);
                for (int k = 0; k < 3; ++k) rec.c0[k] = (float)c[k];
                r.vec3(t, "odd", where, c);
                for (int k = 0; k < 3; ++k) rec.c1[k] = (float)c[k];
            } else if (ty->str == "image") {
                // taichi-version/material.py:137-144 (one 100 x 100 image there, read with cv2 at hittable.py:165-172)
                int id = -1;
                if (const JsonValue *f = t.find("file")) {
                    if (!f->is_string()) r.fail("%s: \"file\" must be a string", where);
                    else {
                        id = add_image_texture_file(s, resolve(f->str).c_str());
                        if (id >= 0) s.images.back().file = f->str;  // serialised as given
                        if (t.find("alpha")) r.fail("%s: \"alpha\" goes with inline \"data\" (a file brings its own)", where);
                    }
                } else {
                    const int rows = r.integer(t, "rows", where), cols = r.integer(t, "cols", where);
                    const JsonValue *d = t.find("data");
                    if (r.ok && (!d || !d->is_array() || rows < 1 || cols < 1 || d->arr.size() != (size_t)rows * cols * 3))
                        r.fail("%s: \"data\" must be an array of rows * cols * 3 bytes", where);
                    if (r.ok) {
                        std::vector<uint8_t> px(d->arr.size());
                        for (size_t k = 0; k < px.size() && r.ok; ++k) {
                            const JsonValue &v = d->arr[k];
                            if (!v.is_number() || v.num < 0 || v.num > 255 || v.num != std::floor(v.num))
                                r.fail("%s: \"data\"[%zu] is not a byte", where, k);
                            else px[k] = (uint8_t)v.num;
                        }
                        // an alpha plane: rows * cols bytes beside the pixels
                        std::vector<uint8_t> al;
                        if (const JsonValue *a = t.find("alpha")) {
                            if (!a->is_array() || a->arr.size() != (size_t)rows * cols) r.fail("%s: \"alpha\" must be an array of rows * cols bytes", where);
                            else {
                                al.resize(a->arr.size());
                                for (size_t k = 0; k < al.size() && r.ok; ++k) {
                                    const JsonValue &v = a->arr[k];
                                    if (!v.is_number() || v.num < 0 || v.num > 255 || v.num != std::floor(v.num))
                                        r.fail("%s: \"alpha\"[%zu] is not a byte", where, k);
                                    else al[k] = (uint8_t)v.num;
                                }
                            }
                        }
                        if (r.ok) id = add_image_texture(s, rows, cols, px.data(), "", al.empty() ? nullptr : al.data());
                    }
                }
                if (r.ok && id < 0) return -id;
                continue;  // add_image_texture appended the texture record
            } else if (ty->str == "noise") {  // DESIGN 7o; a field the style does not have is an error, as for the glossy materials
                rt_noise n;
                memset(&n, 0, sizeof n);
                const JsonValue *st = t.find("style");
                if (!st || !st->is_string()) r.fail("%s: missing string \"style\"", where);
                else if (st->str == "fbm") n.style = RT_NOISE_STYLE_FBM;
                else if (st->str == "turbulence") n.style = RT_NOISE_STYLE_TURBULENCE;
                else if (st->str == "marble") n.style = RT_NOISE_STYLE_MARBLE;
                else r.fail("%s: unknown style \"%s\" (fbm, turbulence, marble)", where, st->str.c_str());
                const bool marble = n.style == RT_NOISE_STYLE_MARBLE;
                for (const auto &kv : t.obj) {
                    bool found = false;
                    for (const char *k : {"type", "style", "color0", "color1", "scale", "octaves", "seed"}) found = found || kv.first == k;
                    if (marble) found = found || kv.first == "axis" || kv.first == "distortion";
                    if (!found) r.fail("%s: unknown field \"%s\"", where, kv.first.c_str());
                }
                double c1[3];
                r.vec3(t, "color0", where, c);
                r.vec3(t, "color1", where, c1);
                n.scale = (float)r.num(t, "scale", where);
                n.octaves = r.integer(t, "octaves", where);
                const double seed = r.num(t, "seed", where);
                if (!(seed >= 0 && seed <= 4294967295.0 && seed == std::floor(seed))) r.fail("%s: \"seed\" must be an integer in 0..2^32 - 1", where);
                else n.seed = (uint32_t)seed;
                if (marble) {
                    const JsonValue *ax = t.find("axis");
                    if (!ax || !ax->is_string() || ax->str.size() != 1 || ax->str[0] < 'x' || ax->str[0] > 'z')
                        r.fail("%s: \"axis\" must be \"x\", \"y\" or \"z\"", where);
                    else n.axis = ax->str[0] - 'x';
                    n.distortion = (float)r.num(t, "distortion", where);
                }
                if (!r.ok) break;
                const float f0[3] = {(float)c[0], (float)c[1], (float)c[2]}, f1[3] = {(float)c1[0], (float)c1[1], (float)c1[2]};
                if (add_noise_texture(s, f0, f1, n, where) < 0) return RT_ERR_SCENE;
                continue;  // add_noise_texture appended the texture record
            } else {
                r.fail("%s: unknown type \"%s\"", where, ty->str.c_str());
            }
            s.texs.push_back(rec);
        }
    }
    if (!r.ok) return RT_ERR_SCENE;

    // materials, parser.hpp:186-281
    if (const JsonValue *arr = r.data_array(root, "material")) {
        for (size_t i = 0; i < arr->arr.size() && r.ok; ++i) {
            const JsonValue &m = arr->arr[i];
            snprintf(where, sizeof where, "material %zu", i);
            const JsonValue *ty = m.find("type");
            if (!m.is_object() || !ty || !ty->is_string()) {
                r.fail("%s: missing string \"type\"", where);
                break;
            }
            rt_material rec;
            memset(&rec, 0, sizeof rec);
            rec.texture = -1;
            auto only_keys = [&](const JsonValue &o, std::initializer_list<const char *> known) {  // (the glossy materials: a misspelt field is an error)
                for (const auto &kv : o.obj) {
                    bool found = false;
                    for (const char *k : known) found = found || kv.first == k;
                    if (!found) r.fail("%s: unknown field \"%s\"", where, kv.first.c_str());
                }
            };
            // a bump on any material but an emitter: {"texture": <noise texture>, "strength": <number>}
            const JsonValue *bump = m.find("bump");
            int pbr_map = -1;  // (a pbr material's "metallic_roughness")
            bool has_pbr_map = false;
            int bump_tex = -1;
            float bump_k = 0.0f;
            if (bump) {
                if (!bump->is_object()) r.fail("%s: \"bump\" must be an object", where);
                else {
                    char bw[128];
                    snprintf(bw, sizeof bw, "%s: bump", where);
                    for (const auto &kv : bump->obj)
                        if (kv.first != "texture" && kv.first != "strength") r.fail("%s: unknown field \"%s\"", bw, kv.first.c_str());
                    bump_tex = r.integer(*bump, "texture", bw);
                    bump_k = (float)r.num(*bump, "strength", bw);
                }
            }
            // a normal map on any material but an emitter: {"texture": <image texture>, "scale": <number, default 1>}
            const JsonValue *nmap = m.find("normal_map");
            int nmap_tex = -1;
            float nmap_s = 1.0f;
            if (nmap) {
                if (!nmap->is_object()) r.fail("%s: \"normal_map\" must be an object", where);
                else {
                    char bw[128];
                    snprintf(bw, sizeof bw, "%s: normal_map", where);
                    for (const auto &kv : nmap->obj)
                        if (kv.first != "texture" && kv.first != "scale") r.fail("%s: unknown field \"%s\"", bw, kv.first.c_str());
                    nmap_tex = r.integer(*nmap, "texture", bw);
                    if (nmap->find("scale")) nmap_s = (float)r.num(*nmap, "scale", bw);
                }
            }
            // an alpha mask on any material but an emitter: {"texture": <image texture with alpha>, "cutoff": <number, default 0.5>}
            const JsonValue *amask = m.find("alpha");
            int amask_tex = -1;
            float amask_c = 0.5f;
            if (amask) {
                if (!amask->is_object()) r.fail("%s: \"alpha\" must be an object", where);
                else {
                    char bw[128];
                    snprintf(bw, sizeof bw, "%s: alpha", where);
                    for (const auto &kv : amask->obj)
                        if (kv.first != "texture" && kv.first != "cutoff") r.fail("%s: unknown field \"%s\"", bw, kv.first.c_str());
                    amask_tex = r.integer(*amask, "texture", bw);
                    if (amask->find("cutoff")) amask_c = (float)r.num(*amask, "cutoff", bw);
                    if (r.ok && amask_tex < 0) r.fail("%s: \"texture\" must be an image texture", bw);
                }
            }
            if (ty->str == "lambertian") {
                rec.type = RT_MAT_LAMBERTIAN;
                rec.texture = r.integer(m, "texture", where);
            } else if (ty->str == "metal") {
                rec.type = RT_MAT_METAL;
                double c[3];
                r.vec3(m, "albedo", where, c);
                for (int k = 0; k < 3; ++k) rec.albedo[k] = (float)c[k];
                float f = (float)r.num(m, "fuzz", where);
                rec.fuzz = f < 1 ? f : 1;  // material.cuh:61
            } else if (ty->str == "rough_metal") {  // albedo is F0, fuzz holds the roughness
                rec.type = RT_MAT_ROUGH_METAL;
                only_keys(m, {"type", "albedo", "roughness", "bump", "normal_map", "alpha"});
                double c[3];
                r.vec3(m, "albedo", where, c);
                for (int k = 0; k < 3; ++k) rec.albedo[k] = (float)c[k];
                rec.fuzz = (float)r.num(m, "roughness", where);
                if (r.ok && !glossy_material_ok(rec, s.texs.size(), where)) r.ok = false;
            } else if (ty->str == "plastic") {  // texture is the body colour, fuzz the roughness, ir the coat's index
                rec.type = RT_MAT_PLASTIC;
                only_keys(m, {"type", "texture", "ior", "roughness", "bump", "normal_map", "alpha"});
                rec.texture = r.integer(m, "texture", where);
                rec.ir = (float)r.num(m, "ior", where);
                rec.fuzz = (float)r.num(m, "roughness", where);
                if (r.ok && !glossy_material_ok(rec, s.texs.size(), where)) r.ok = false;
            } else if (ty->str == "pbr") {  // fuzz holds the roughness factor, albedo[0] the metallic factor
                rec.type = RT_MAT_PBR;
                only_keys(m, {"type", "texture", "metallic", "roughness", "ior", "metallic_roughness", "bump", "normal_map", "alpha"});
                rec.texture = r.integer(m, "texture", where);
                rec.albedo[0] = (float)r.num(m, "metallic", where);
                rec.fuzz = (float)r.num(m, "roughness", where);
                rec.ir = m.find("ior") ? (float)r.num(m, "ior", where) : 1.5f;
                if (m.find("metallic_roughness")) pbr_map = r.integer(m, "metallic_roughness", where), has_pbr_map = true;
                if (r.ok && !glossy_material_ok(rec, s.texs.size(), where)) r.ok = false;
            } else if (ty->str == "rough_glass") {  // fuzz holds the roughness, albedo the absorption coefficient
                rec.type = RT_MAT_ROUGH_GLASS;
                only_keys(m, {"type", "ir", "roughness", "absorption", "tint", "tint_distance", "bump", "normal_map", "alpha"});
                rec.ir = (float)r.num(m, "ir", where);
                rec.fuzz = (float)r.num(m, "roughness", where);
                const bool has_tint = m.find("tint") || m.find("tint_distance");
                if (m.find("absorption") && has_tint) r.fail("%s: \"absorption\" and \"tint\" / \"tint_distance\" exclude each other", where);
                else if (m.find("absorption")) {
                    double c[3];
                    r.vec3(m, "absorption", where, c);
                    for (int k = 0; k < 3; ++k) rec.albedo[k] = (float)c[k];
                } else if (has_tint) {  // sigma = -ln(tint) / tint_distance, in fp64, rounded once
                    double c[3] = {1, 1, 1};
                    r.vec3(m, "tint", where, c);
                    const double d = r.num(m, "tint_distance", where);
                    if (r.ok && !(d > 0.0 && d < (double)INFINITY)) r.fail("%s: tint_distance must be finite and > 0 (got %g)", where, d);
                    for (int k = 0; k < 3 && r.ok; ++k) {
                        if (!(c[k] > 0.0 && c[k] <= 1.0)) r.fail("%s: tint components must be in (0, 1] (got %g)", where, c[k]);
                        else rec.albedo[k] = (float)(-std::log(c[k]) / d + 0.0);
                    }
                }
                if (r.ok && !glossy_material_ok(rec, s.texs.size(), where)) r.ok = false;
            } else if (ty->str == "dielectric") {
                rec.type = RT_MAT_DIELECTRIC;
                rec.ir = (float)r.num(m, "index_of_refraction", where);
            } else if (ty->str == "diffuse_light") {
                rec.type = RT_MAT_DIFFUSE_LIGHT;
                rec.texture = r.integer(m, "texture", where);
            } else {
                r.fail("%s: unknown type \"%s\"", where, ty->str.c_str());
            }
            s.mats.push_back(rec);
            if (r.ok && bump && !set_bump(s, (int)s.mats.size() - 1, bump_tex, bump_k, where)) r.ok = false;
            if (r.ok && nmap && !set_normal_map(s, (int)s.mats.size() - 1, nmap_tex, nmap_s, where)) r.ok = false;
            if (r.ok && amask && !set_alpha(s, (int)s.mats.size() - 1, amask_tex, amask_c, where)) r.ok = false;
            if (r.ok && has_pbr_map && !set_pbr_map(s, (int)s.mats.size() - 1, pbr_map, where)) r.ok = false;  // (-1: no map)
        }
    }
    if (!r.ok) return RT_ERR_SCENE;

    // objects, parser.hpp:283-478 (a "moving_sphere" -- a sphere with "center0" and "center1" -- joins the movers' list)
    s.movers.clear();
    if (const JsonValue *arr = r.data_array(root, "object")) {
        for (size_t i = 0; i < arr->arr.size() && r.ok; ++i) {
            const JsonValue &o = arr->arr[i];
            snprintf(where, sizeof where, "object %zu", i);
            const JsonValue *ty = o.find("type");
            if (!o.is_object() || !ty || !ty->is_string()) {
                r.fail("%s: missing string \"type\"", where);
                break;
            }
            rt_prim rec;
            memset(&rec, 0, sizeof rec);
            const std::string &t = ty->str;
            if (t == "sphere") {
                rec.type = RT_PRIM_SPHERE;
                double c[3];
                r.vec3(o, "center", where, c);
                rec.f[0] = (float)c[0], rec.f[1] = (float)c[1], rec.f[2] = (float)c[2];
                rec.f[3] = (float)r.num(o, "radius", where);
                rec.material = r.integer(o, "material", where);
                s.prims.push_back(rec);
                s.xforms.emplace_back();
            } else if (t == "moving_sphere") {
                rt_moving_sphere m;
                memset(&m, 0, sizeof m);
                double c0[3], c1[3];
                r.vec3(o, "center0", where, c0);
                r.vec3(o, "center1", where, c1);
                for (int k = 0; k < 3; ++k) m.center0[k] = (float)c0[k], m.center1[k] = (float)c1[k];
                m.radius = (float)r.num(o, "radius", where);
                m.material = r.integer(o, "material", where);
                if (!r.ok) break;
                const int rc = add_moving_sphere(s, m);
                if (rc < 0) {  // (the record's own message, with its place in the file)
                    const std::string why = get_error();
                    set_error("%s: %s", where, why.c_str());
                    return -rc;
                }
            } else if (t == "xy_rect" || t == "xz_rect" || t == "yz_rect") {
                const char *k0, *k1, *k2, *k3;
                if (t == "xy_rect") rec.type = RT_PRIM_XY_RECT, k0 = "x0", k1 = "x1", k2 = "y0", k3 = "y1";
                else if (t == "xz_rect") rec.type = RT_PRIM_XZ_RECT, k0 = "x0", k1 = "x1", k2 = "z0", k3 = "z1";
                else rec.type = RT_PRIM_YZ_RECT, k0 = "y0", k1 = "y1", k2 = "z0", k3 = "z1";
                rec.f[0] = (float)r.num(o, k0, where);
                rec.f[1] = (float)r.num(o, k1, where);
                rec.f[2] = (float)r.num(o, k2, where);
                rec.f[3] = (float)r.num(o, k3, where);
                rec.f[4] = (float)r.num(o, "k", where);
                rec.material = r.integer(o, "material", where);
                s.prims.push_back(rec);
                s.xforms.emplace_back();
            } else if (t == "cylinder") {
                float radius = (float)r.num(o, "radius", where);
                float zmin = (float)r.num(o, "zmin", where);
                float zmax = (float)r.num(o, "zmax", where);
                int mat = r.integer(o, "material", where);
                double axis[3], off[3], deg = 0;
                const double *pa = nullptr, *po = nullptr;
                if (const JsonValue *rot = o.find("rotate")) {
                    if (!rot->is_object()) r.fail("%s: \"rotate\" must be an object", where);
                    else {
                        r.vec3(*rot, "axis", where, axis);
                        deg = r.num(*rot, "angle", where);
                        pa = axis;
                    }
                }
                if (o.find("translate")) {
                    r.vec3(o, "translate", where, off);
                    po = off;
                }
                if (r.ok) {
                    int rc = add_cylinder(s, radius, zmin, zmax, mat, pa, deg, po);
                    if (rc < 0) return RT_ERR_SCENE;
                }
            } else if (t == "triangle") {  // taichi-version/hittable.py:95-110
                double v[3][3], u[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
                r.vec3(o, "v1", where, v[0]), r.vec3(o, "v2", where, v[1]), r.vec3(o, "v3", where, v[2]);
                const char *uk[3] = {"u1", "u2", "u3"};
                for (int c = 0; c < 3; ++c)
                    if (const JsonValue *uv = o.find(uk[c])) {
                        if (!uv->is_array() || uv->arr.size() < 2 || !uv->arr[0].is_number() || !uv->arr[1].is_number())
                            r.fail("%s: \"%s\" must be an array of 2 numbers", where, uk[c]);
                        else u[c][0] = uv->arr[0].num, u[c][1] = uv->arr[1].num;
                    }
                // vertex normals: all three or none
                double n[3][3];
                const char *nk[3] = {"n1", "n2", "n3"};
                const int have_n = (o.find("n1") != nullptr) + (o.find("n2") != nullptr) + (o.find("n3") != nullptr);
                if (have_n == 3) r.vec3(o, "n1", where, n[0]), r.vec3(o, "n2", where, n[1]), r.vec3(o, "n3", where, n[2]);
                else if (have_n != 0) r.fail("%s: \"%s\", \"%s\" and \"%s\" come together", where, nk[0], nk[1], nk[2]);
                const int mat = r.integer(o, "material", where);
                if (r.ok) {
                    float vf[3][3], uf[3][2], nf[3][3];
                    for (int c = 0; c < 3; ++c) {
                        for (int k = 0; k < 3; ++k) vf[c][k] = (float)v[c][k], nf[c][k] = have_n ? (float)n[c][k] : 0.0f;
                        uf[c][0] = (float)u[c][0], uf[c][1] = (float)u[c][1];
                    }
                    const int rc = have_n ? add_triangle_normals(s, vf[0], vf[1], vf[2], nf[0], nf[1], nf[2], uf[0], uf[1], uf[2], mat)
                                          : add_triangle(s, vf[0], vf[1], vf[2], uf[0], uf[1], uf[2], mat);
                    if (rc < 0) return RT_ERR_SCENE;
                }
            } else if (t == "quad" || t == "box") {  // a parallelogram; six of them over [min, max]
                const bool is_box = t == "box";
                for (const auto &kv : o.obj) {  // (a field the type does not have is an error, as for the glossy materials)
                    const std::string &k = kv.first;
                    const bool known = k == "type" || k == "material" || k == "rotate" || k == "translate" ||
                                       (is_box ? (k == "min" || k == "max") : (k == "q" || k == "u" || k == "v"));
                    if (!known) r.fail("%s: unknown field \"%s\"", where, k.c_str());
                }
                double a3[3][3];
                if (is_box) r.vec3(o, "min", where, a3[0]), r.vec3(o, "max", where, a3[1]);
                else r.vec3(o, "q", where, a3[0]), r.vec3(o, "u", where, a3[1]), r.vec3(o, "v", where, a3[2]);
                const int mat = r.integer(o, "material", where);
                double axis[3], off[3], deg = 0;
                const double *pa = nullptr, *po = nullptr;
                if (const JsonValue *rot = o.find("rotate")) {
                    if (!rot->is_object()) r.fail("%s: \"rotate\" must be an object", where);
                    else {
                        for (const auto &kv : rot->obj)
                            if (kv.first != "axis" && kv.first != "angle") r.fail("%s: rotate: unknown field \"%s\"", where, kv.first.c_str());
                        r.vec3(*rot, "axis", where, axis);
                        deg = r.num(*rot, "angle", where);
                        pa = axis;
                    }
                }
                if (o.find("translate")) {
                    r.vec3(o, "translate", where, off);
                    po = off;
                }
                if (r.ok) {
                    float f3[3][3];
                    for (int c = 0; c < 3; ++c)
                        for (int k = 0; k < 3; ++k) f3[c][k] = (float)a3[c][k];
                    const int rc = is_box ? add_box(s, f3[0], f3[1], mat, pa, deg, po) : add_quad(s, f3[0], f3[1], f3[2], mat, pa, deg, po);
                    if (rc < 0) {
                        const std::string why = get_error();
                        set_error("%s: %s", where, why.c_str());
                        return RT_ERR_SCENE;
                    }
                }
            } else if (t == "mesh") {  // readobj + placement, taichi-version/main.py:23-41, 110-118
                const JsonValue *f = o.find("file");
                if (!f || !f->is_string()) r.fail("%s: missing string \"file\"", where);
                const int mat = r.integer(o, "material", where);
                float scale = 1.0f, M[9], T[3];
                const float *pm = nullptr, *pt = nullptr;
                if (o.find("scale")) scale = (float)r.num(o, "scale", where);
                if (const JsonValue *m = o.find("matrix")) {
                    if (!m->is_array() || m->arr.size() != 9) r.fail("%s: \"matrix\" must be an array of 9 numbers", where);
                    else {
                        for (int k = 0; k < 9; ++k) {
                            if (!m->arr[k].is_number()) r.fail("%s: \"matrix\" must be an array of 9 numbers", where);
                            M[k] = (float)m->arr[k].num;
                        }
                        pm = M;
                    }
                }
                if (o.find("translate")) {
                    double d[3];
                    r.vec3(o, "translate", where, d);
                    T[0] = (float)d[0], T[1] = (float)d[1], T[2] = (float)d[2];
                    pt = T;
                }
                // "normals": "flat" (default) | "file" | "smooth", "crease_angle" in degrees
                int mode = RT_MESH_NORMALS_FLAT;
                float crease = 180.0f;
                if (const JsonValue *nv = o.find("normals")) {
                    if (nv->is_string() && nv->str == "flat") mode = RT_MESH_NORMALS_FLAT;
                    else if (nv->is_string() && nv->str == "file") mode = RT_MESH_NORMALS_FILE;
                    else if (nv->is_string() && nv->str == "smooth") mode = RT_MESH_NORMALS_SMOOTH;
                    else r.fail("%s: \"normals\" must be \"flat\", \"file\" or \"smooth\"", where);
                }
                if (o.find("crease_angle")) crease = (float)r.num(o, "crease_angle", where);
                if (g_mesh_normals_mode >= 0) mode = g_mesh_normals_mode, crease = g_mesh_normals_crease;
                if (r.ok) {
                    const int rc = add_obj_normals(s, resolve(f->str).c_str(), mat, scale, pm, pt, mode, crease);
                    if (rc < 0) return -rc;
                }
            } else {
                r.fail("%s: unknown type \"%s\"", where, t.c_str());
            }
        }
    }
    if (!r.ok) return RT_ERR_SCENE;
    s.touch();
    return scene_validate(s);
}

// ---------------------------------------------------------------- JSON out
static void put_vec3(std::string &o, const float *v) {
    o += "[" + json_float(v[0]) + ", " + json_float(v[1]) + ", " + json_float(v[2]) + "]";
}
static std::string json_double(double d) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.17g", d);
    return buf;
}
static void put_vec3d(std::string &o, const double *v) {
    o += "[" + json_double(v[0]) + ", " + json_double(v[1]) + ", " + json_double(v[2]) + "]";
}

std::string scene_to_json(const Scene &s) {
    std::string o = "{\n";
    o += "  \"output_file\": " + json_escape(s.output_file) + ",\n";
    o += "  \"background\": ";
    put_vec3(o, s.background);
    o += ",\n";
    o += "  \"max_depth\": " + std::to_string(s.max_depth) + ",\n";
    o += "  \"samples_per_pixel\": " + std::to_string(s.spp) + ",\n";
    o += "  \"width\": " + std::to_string(s.width) + ",\n";
    o += "  \"height\": " + std::to_string(s.height) + ",\n";
    o += std::string("  \"sky_gradient\": ") + ((s.flags & RT_FLAG_SKY_GRADIENT) ? "true" : "false") + ",\n";
    o += std::string("  \"defocus_blur\": ") + ((s.flags & RT_FLAG_DEFOCUS_BLUR) ? "true" : "false") + ",\n";
    if (s.rr_p > 0.0f) o += "  \"russian_roulette\": " + json_double((double)s.rr_p) + ",\n";
    if (s.light_sampling) o += "  \"light_sampling\": true,\n";
    else if (!s.alights.empty()) o += "  \"light_sampling\": false,\n";  // ("lights" alone would switch it on)
    if (!s.alights.empty()) {  // analytic lights, as given
        o += "  \"lights\": [";
        for (size_t i = 0; i < s.alights.size(); ++i) {
            const rt_analytic_light &l = s.alights[i];
            o += i ? ",\n    " : "\n    ";
            if (l.type == RT_LIGHT_DISTANT) {
                o += "{\"type\": \"distant\", \"direction\": ";
                put_vec3(o, l.direction);
                o += ", \"irradiance\": ";
                put_vec3(o, l.color);
                o += ", \"angular_radius\": " + json_float(l.angle[0]) + "}";
                continue;
            }
            o += l.type == RT_LIGHT_SPOT ? "{\"type\": \"spot\", \"position\": " : "{\"type\": \"point\", \"position\": ";
            put_vec3(o, l.position);
            if (l.type == RT_LIGHT_SPOT) {
                o += ", \"direction\": ";
                put_vec3(o, l.direction);
                o += ", \"inner_angle\": " + json_float(l.angle[0]) + ", \"outer_angle\": " + json_float(l.angle[1]);
            }
            o += ", \"intensity\": ";
            put_vec3(o, l.color);
            o += "}";
        }
        o += "\n  ],\n";
    }
    if (s.mesh_lights) o += "  \"mesh_lights\": true,\n";
    if (s.media_light_sampling) o += "  \"media_light_sampling\": true,\n";
    if (s.nested_grid) o += "  \"nested_grid\": true,\n";
    if (s.env) {
        o += "  \"environment\": {";
        if (!s.env->file.empty()) o += "\"file\": " + json_escape(s.env->file);
        else {
            o += "\"rows\": " + std::to_string(s.env->rows) + ", \"cols\": " + std::to_string(s.env->cols) + ", \"data\": [";
            for (size_t i = 0; i < s.env->rgb.size(); ++i) o += (i ? ", " : "") + json_float(s.env->rgb[i]);
            o += "]";
        }
        o += ", \"scale\": " + json_float(s.env_scale) + ", \"rotate\": " + json_float(s.env_rotate) + "},\n";
    }
    if (!s.media.empty()) {
        o += "  \"media\": {\"data\": [";
        for (size_t i = 0; i < s.media.size(); ++i) {
            const rt_medium &m = s.media[i];
            o += i ? ",\n    " : "\n    ";
            if (m.shape == RT_MEDIUM_SPHERE) {
                o += "{\"type\": \"sphere\", \"center\": ";
                put_vec3(o, m.f);
                o += ", \"radius\": " + json_float(m.f[3]);
            } else {
                o += "{\"type\": \"box\", \"min\": ";
                put_vec3(o, m.f);
                o += ", \"max\": ";
                put_vec3(o, m.f + 3);
            }
            o += ", \"density\": " + json_float(m.density) + ", \"albedo\": ";
            put_vec3(o, m.albedo);
            if (s.media_g[i] != 0.0f) o += ", \"g\": " + json_float(s.media_g[i]);
            o += "}";
        }
        o += "\n  ]},\n";
    }
    o += "  \"camera\": {\"lookfrom\": ";
    put_vec3d(o, s.cam.lookfrom);
    o += ", \"lookat\": ";
    put_vec3d(o, s.cam.lookat);
    o += ", \"vup\": ";
    put_vec3d(o, s.cam.vup);
    o += ", \"vfov\": " + json_double(s.cam.vfov) + ", \"aperture\": " + json_double(s.cam.aperture);
    if (s.cam.focus_dist > 0) o += ", \"focus_dist\": " + json_double(s.cam.focus_dist);
    if (s.cam.projection != RT_PROJ_PERSPECTIVE) {  // (a perspective scene is written as it always was)
        o += std::string(", \"projection\": {\"type\": \"") + projection_name(s.cam.projection) + "\"";
        if (s.cam.projection == RT_PROJ_ORTHOGRAPHIC) o += ", \"height\": " + json_double(s.cam.proj[0]);
        if (s.cam.projection == RT_PROJ_PANORAMIC) o += ", \"hfov\": " + json_double(s.cam.proj[0]) + ", \"vfov\": " + json_double(s.cam.proj[1]);
        if (s.cam.projection == RT_PROJ_FISHEYE) o += ", \"fov\": " + json_double(s.cam.proj[0]);
        o += "}";
    }
    o += "},\n";

    o += "  \"object\": {\"data\": [";
    for (size_t i = 0; i < s.prims.size(); ++i) {
        const rt_prim &p = s.prims[i];
        o += i ? ",\n    " : "\n    ";
        switch (p.type) {
        case RT_PRIM_SPHERE:
            o += "{\"type\": \"sphere\", \"center\": ";
            put_vec3(o, p.f);
            o += ", \"radius\": " + json_float(p.f[3]);
            break;
        case RT_PRIM_XY_RECT:
        case RT_PRIM_XZ_RECT:
        case RT_PRIM_YZ_RECT: {
            const char *names[3][5] = {{"xy_rect", "x0", "x1", "y0", "y1"},
                                       {"xz_rect", "x0", "x1", "z0", "z1"},
                                       {"yz_rect", "y0", "y1", "z0", "z1"}};
            const char **n = names[p.type - RT_PRIM_XY_RECT];
            o += std::string("{\"type\": \"") + n[0] + "\"";
            for (int k = 0; k < 4; ++k) o += std::string(", \"") + n[k + 1] + "\": " + json_float(p.f[k]);
            o += ", \"k\": " + json_float(p.f[4]);
            break;
        }
        case RT_PRIM_CYLINDER: {
            const CylinderXform &xf = s.xforms[i];
            o += "{\"type\": \"cylinder\", \"radius\": " + json_float(p.f[0]) + ", \"zmin\": " + json_float(p.f[1]) +
                 ", \"zmax\": " + json_float(p.f[2]);
            if (xf.has_rotate) {
                o += ", \"rotate\": {\"axis\": ";
                put_vec3d(o, xf.axis);
                o += ", \"angle\": " + json_double(xf.degrees) + "}";
            }
            if (xf.has_translate) {
                o += ", \"translate\": ";
                put_vec3d(o, xf.offset);
            }
            break;
        }
        case RT_PRIM_TRIANGLE: {
            o += "{\"type\": \"triangle\"";
            const char *vk[3] = {"v1", "v2", "v3"}, *uk[3] = {"u1", "u2", "u3"};
            for (int c = 0; c < 3; ++c) {
                o += std::string(", \"") + vk[c] + "\": ";
                put_vec3(o, p.m + 3 * c);
            }
            for (int c = 0; c < 3; ++c)
                o += std::string(", \"") + uk[c] + "\": [" + json_float(p.m_inv[2 * c]) + ", " + json_float(p.m_inv[2 * c + 1]) + "]";
            if (tri_has_normals(p)) {  // smooth shading
                const char *nk[3] = {"n1", "n2", "n3"};
                const float *nv[3] = {p.f, p.f + 3, p.m_inv + 6};
                for (int c = 0; c < 3; ++c) {
                    o += std::string(", \"") + nk[c] + "\": ";
                    put_vec3(o, nv[c]);
                }
            }
            break;
        }
        case RT_PRIM_QUAD: {  // (as stored: a rotated quad, or a box's face, comes out as the quad it became)
            o += "{\"type\": \"quad\"";
            const char *qk[3] = {"q", "u", "v"};
            for (int c = 0; c < 3; ++c) {
                o += std::string(", \"") + qk[c] + "\": ";
                put_vec3(o, p.m + 3 * c);
            }
            break;
        }
        default: break;
        }
        o += ", \"material\": " + std::to_string(p.material) + "}";
    }
    for (size_t i = 0; i < s.movers.size(); ++i) {  // the moving spheres, behind the primitives
        const rt_moving_sphere &m = s.movers[i];
        o += (i || !s.prims.empty()) ? ",\n    " : "\n    ";
        o += "{\"type\": \"moving_sphere\", \"center0\": ";
        put_vec3(o, m.center0);
        o += ", \"center1\": ";
        put_vec3(o, m.center1);
        o += ", \"radius\": " + json_float(m.radius) + ", \"material\": " + std::to_string(m.material) + "}";
    }
    o += "\n  ]},\n";

    o += "  \"material\": {\"data\": [";
    for (size_t i = 0; i < s.mats.size(); ++i) {
        const rt_material &m = s.mats[i];
        o += i ? ",\n    " : "\n    ";
        switch (m.type) {
        case RT_MAT_LAMBERTIAN: o += "{\"type\": \"lambertian\", \"texture\": " + std::to_string(m.texture) + "}"; break;
        case RT_MAT_METAL:
            o += "{\"type\": \"metal\", \"albedo\": ";
            put_vec3(o, m.albedo);
            o += ", \"fuzz\": " + json_float(m.fuzz) + "}";
            break;
        case RT_MAT_DIELECTRIC:
            o += "{\"type\": \"dielectric\", \"index_of_refraction\": " + json_float(m.ir) + "}";
            break;
        case RT_MAT_DIFFUSE_LIGHT:
            o += "{\"type\": \"diffuse_light\", \"texture\": " + std::to_string(m.texture) + "}";
            break;
        case RT_MAT_ROUGH_METAL:
            o += "{\"type\": \"rough_metal\", \"albedo\": ";
            put_vec3(o, m.albedo);
            o += ", \"roughness\": " + json_float(m.fuzz) + "}";
            break;
        case RT_MAT_PLASTIC:
            o += "{\"type\": \"plastic\", \"texture\": " + std::to_string(m.texture) + ", \"ior\": " + json_float(m.ir) +
                 ", \"roughness\": " + json_float(m.fuzz) + "}";
            break;
        case RT_MAT_PBR:
            o += "{\"type\": \"pbr\", \"texture\": " + std::to_string(m.texture) + ", \"metallic\": " + json_float(m.albedo[0]) +
                 ", \"roughness\": " + json_float(m.fuzz) + ", \"ior\": " + json_float(m.ir);
            if (scene_pbr_map(s, (int)i) >= 0) o += ", \"metallic_roughness\": " + std::to_string(scene_pbr_map(s, (int)i));
            o += "}";
            break;
        case RT_MAT_ROUGH_GLASS:  // (a tint comes back as the absorption it was converted to)
            o += "{\"type\": \"rough_glass\", \"ir\": " + json_float(m.ir) + ", \"roughness\": " + json_float(m.fuzz) + ", \"absorption\": ";
            put_vec3(o, m.albedo);
            o += "}";
            break;
        default: break;
        }
        if (const SceneBump *b = scene_bump(s, (int)i)) {  // (inside the material's object: before its closing brace)
            o.pop_back();
            o += ", \"bump\": {\"texture\": " + std::to_string(b->texture) + ", \"strength\": " + json_float(b->strength) + "}}";
        }
        if (const SceneNormalMap *b = scene_normal_map(s, (int)i)) {
            o.pop_back();
            o += ", \"normal_map\": {\"texture\": " + std::to_string(b->texture) + ", \"scale\": " + json_float(b->scale) + "}}";
        }
        if (const SceneAlpha *b = scene_alpha(s, (int)i)) {
            o.pop_back();
            o += ", \"alpha\": {\"texture\": " + std::to_string(b->texture) + ", \"cutoff\": " + json_float(b->cutoff) + "}}";
        }
    }
    o += "\n  ]},\n";

    o += "  \"texture\": {\"data\": [";
    for (size_t i = 0; i < s.texs.size(); ++i) {
        const rt_texture &t = s.texs[i];
        o += i ? ",\n    " : "\n    ";
        if (t.type == RT_TEX_SOLID) {
            o += "{\"type\": \"solid_color\", \"color\": ";
            put_vec3(o, t.c0);
            o += "}";
        } else if (t.type == RT_TEX_IMAGE) {
            const SceneImage &im = s.images[(size_t)t.c0[0]];
            if (!im.file.empty()) {
                o += "{\"type\": \"image\", \"file\": " + json_escape(im.file) + "}";
            } else {
                o += "{\"type\": \"image\", \"rows\": " + std::to_string(im.rows) + ", \"cols\": " + std::to_string(im.cols) +
                     ", \"data\": [";
                for (size_t k = 0; k < im.rgb.size(); ++k) o += (k ? "," : "") + std::to_string((int)im.rgb[k]);
                o += "]";
                if (!im.alpha.empty()) {
                    o += ", \"alpha\": [";
                    for (size_t k = 0; k < im.alpha.size(); ++k) o += (k ? "," : "") + std::to_string((int)im.alpha[k]);
                    o += "]";
                }
                o += "}";
            }
        } else if (t.type == RT_TEX_NOISE) {
            const rt_noise &n = s.noise[i];
            static const char *const styles[3] = {"fbm", "turbulence", "marble"};
            o += std::string("{\"type\": \"noise\", \"style\": \"") + styles[n.style] + "\", \"color0\": ";
            put_vec3(o, t.c0);
            o += ", \"color1\": ";
            put_vec3(o, t.c1);
            o += ", \"scale\": " + json_float(n.scale) + ", \"octaves\": " + std::to_string(n.octaves) + ", \"seed\": " + std::to_string(n.seed);
            if (n.style == RT_NOISE_STYLE_MARBLE)
                o += std::string(", \"axis\": \"") + (char)('x' + n.axis) + "\", \"distortion\": " + json_float(n.distortion);
            o += "}";
        } else {
            o += "{\"type\": \"checker\", \"even\": ";
            put_vec3(o, t.c0);
            o += ", \"odd\": ";
            put_vec3(o, t.c1);
            o += "}";
        }
    }
    o += "\n  ]}\n}\n";
    return o;
}

// ---------------------------------------------------------------- RTIOW scene
// random_scene(), cmake-cpu-version/main.cpp:125-172 with the camera of :89-94.
// The reference draws from rand() seeded by srand(7) in an order that depends on
// the compiler (argument evaluation order is unspecified); here
// the draws come from Philox keyed by `seed` in a fixed order: choose_mat,
// center.x, center.z, then the material's draws, x before y before z.
namespace {
struct SceneRng {
    uint32_t k0, k1, block = 0, pos = 4;
    Philox4 buf;
    explicit SceneRng(uint32_t seed) : k0(seed), k1(0x52544957u /* "RTIW" */) {}
    double next() {  // [0,1), 24 bits
        if (pos == 4) {
            buf = philox4x32_10(block++, 0, 0, 0, k0, k1);
            pos = 0;
        }
        return (double)(buf.v[pos++] >> 8) * (1.0 / 16777216.0);
    }
    double range(double lo, double hi) { return lo + (hi - lo) * next(); }
};
}  // namespace

void scene_rtiow(Scene &s, uint32_t seed, int width, int height, int spp, int max_depth) {
    s = Scene();
    s.width = width, s.height = height, s.spp = spp, s.max_depth = max_depth;
    s.flags = RT_FLAG_SKY_GRADIENT | RT_FLAG_DEFOCUS_BLUR;
    s.background[0] = 0.5f, s.background[1] = 0.7f, s.background[2] = 1.0f;
    s.output_file = "rtiow.png";
    // camera, main.cpp:89-94
    s.cam.lookfrom[0] = 13, s.cam.lookfrom[1] = 2, s.cam.lookfrom[2] = 3;
    s.cam.lookat[0] = s.cam.lookat[1] = s.cam.lookat[2] = 0;
    s.cam.vup[0] = 0, s.cam.vup[1] = 1, s.cam.vup[2] = 0;
    s.cam.vfov = 20;
    s.cam.aperture = 0.1;
    s.cam.aspect = 0;
    s.cam.focus_dist = 0;

    auto add_tex_solid = [&](double r, double g, double b) {
        rt_texture t;
        memset(&t, 0, sizeof t);
        t.type = RT_TEX_SOLID;
        t.c0[0] = t.c1[0] = (float)r, t.c0[1] = t.c1[1] = (float)g, t.c0[2] = t.c1[2] = (float)b;
        s.texs.push_back(t);
        return (int)s.texs.size() - 1;
    };
    auto add_mat = [&](int type, int tex, double r, double g, double b, double fuzz, double ir) {
        rt_material m;
        memset(&m, 0, sizeof m);
        m.type = type, m.texture = tex;
        m.albedo[0] = (float)r, m.albedo[1] = (float)g, m.albedo[2] = (float)b;
        float f = (float)fuzz;
        m.fuzz = f < 1 ? f : 1;
        m.ir = (float)ir;
        s.mats.push_back(m);
        return (int)s.mats.size() - 1;
    };
    auto add_sphere = [&](double x, double y, double z, double rad, int mat) {
        rt_prim p;
        memset(&p, 0, sizeof p);
        p.type = RT_PRIM_SPHERE, p.material = mat;
        p.f[0] = (float)x, p.f[1] = (float)y, p.f[2] = (float)z, p.f[3] = (float)rad;
        s.prims.push_back(p);
        s.xforms.emplace_back();
    };

    // ground: checker_texture(color(0.2,0.3,0.1), color(0.9,0.9,0.9)), main.cpp:131-132
    {
        rt_texture t;
        memset(&t, 0, sizeof t);
        t.type = RT_TEX_CHECKER;
        t.c0[0] = 0.2f, t.c0[1] = 0.3f, t.c0[2] = 0.1f;  // even
        t.c1[0] = t.c1[1] = t.c1[2] = 0.9f;              // odd
        s.texs.push_back(t);
        add_sphere(0, -1000, 0, 1000, add_mat(RT_MAT_LAMBERTIAN, 0, 0, 0, 0, 0, 0));
    }
    SceneRng rng(seed);
    for (int a = -11; a < 11; ++a) {
        for (int b = -11; b < 11; ++b) {
            double choose = rng.next();
            double cx = a + 0.9 * rng.next();
            double cz = b + 0.9 * rng.next();
            double dx = cx - 4, dy = 0.2 - 0.2, dz = cz - 0;
            if (std::sqrt(dx * dx + dy * dy + dz * dz) > 0.9) {  // main.cpp:139
                if (choose < 0.8) {  // diffuse: albedo = random() * random()
                    double c1[3], c2[3];
                    for (double &c : c1) c = rng.next();
                    for (double &c : c2) c = rng.next();
                    int tex = add_tex_solid(c1[0] * c2[0], c1[1] * c2[1], c1[2] * c2[2]);
                    add_sphere(cx, 0.2, cz, 0.2, add_mat(RT_MAT_LAMBERTIAN, tex, 0, 0, 0, 0, 0));
                } else if (choose < 0.95) {  // metal: albedo = random(0.5,1), fuzz = random(0,0.5)
                    double c[3];
                    for (double &v : c) v = rng.range(0.5, 1);
                    double fuzz = rng.range(0, 0.5);
                    add_sphere(cx, 0.2, cz, 0.2, add_mat(RT_MAT_METAL, -1, c[0], c[1], c[2], fuzz, 0));
                } else {  // glass
                    add_sphere(cx, 0.2, cz, 0.2, add_mat(RT_MAT_DIELECTRIC, -1, 0, 0, 0, 0, 1.5));
                }
            }
        }
    }
    add_sphere(0, 1, 0, 1.0, add_mat(RT_MAT_DIELECTRIC, -1, 0, 0, 0, 0, 1.5));
    add_sphere(-4, 1, 0, 1.0, add_mat(RT_MAT_LAMBERTIAN, add_tex_solid(0.4, 0.2, 0.1), 0, 0, 0, 0, 0));
    add_sphere(4, 1, 0, 1.0, add_mat(RT_MAT_METAL, -1, 0.7, 0.6, 0.5, 0.0, 0));
    s.touch();
}

}  // namespace rtmi

namespace rtmi {

std::vector<SceneLight> scene_lights(const Scene &s) {
    std::vector<SceneLight> out;
    const double pi = std::acos(-1.0);
    auto luminance = [](const float *c) { return 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2]; };
    for (size_t i = 0; i < s.prims.size(); ++i) {
        const rt_prim &p = s.prims[i];
        if (p.material < 0 || p.material >= (int)s.mats.size()) continue;
        const rt_material &m = s.mats[(size_t)p.material];
        if (m.type != RT_MAT_DIFFUSE_LIGHT || m.texture < 0 || m.texture >= (int)s.texs.size()) continue;
        const rt_texture &t = s.texs[(size_t)m.texture];
        if (t.type != RT_TEX_SOLID && t.type != RT_TEX_CHECKER) continue;  // image-textured emitters stay BSDF-only
        SceneLight l;
        l.prim = (int)i, l.type = p.type;
        l.checker = t.type == RT_TEX_CHECKER;
        for (int c = 0; c < 3; ++c) l.even[c] = t.c0[c], l.odd[c] = l.checker ? t.c1[c] : t.c0[c];
        switch (p.type) {
        case RT_PRIM_SPHERE: l.area = 4.0 * pi * (double)p.f[3] * (double)p.f[3]; break;
        case RT_PRIM_XY_RECT:
        case RT_PRIM_XZ_RECT:
        case RT_PRIM_YZ_RECT: l.area = ((double)p.f[1] - p.f[0]) * ((double)p.f[3] - p.f[2]); break;
        case RT_PRIM_CYLINDER: {
            // the kernel samples the tube in object space and maps the point through o2w: only a rigid transform keeps the
            // density uniform by area (R R^T = I)
            bool rigid = true;
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    double d = 0.0;
                    for (int k = 0; k < 3; ++k) d += (double)p.m[4 * a + k] * p.m[4 * b + k];
                    if (std::fabs(d - (a == b ? 1.0 : 0.0)) > 1e-4) rigid = false;
                }
            if (!rigid) continue;
            l.area = 2.0 * pi * std::fabs((double)p.f[0]) * ((double)p.f[2] - p.f[1]);
            break;
        }
        case RT_PRIM_TRIANGLE: {
            // mesh lights, opt-in: one light per triangle, |e1 x e2| / 2 in fp64 from the stored vertices.  A
            // degenerate triangle -- no area, or a sliver whose area or 1 / area the light record's fp32 words cannot hold --
            // is skipped: it stays a BSDF-only emitter
            if (!s.mesh_lights) continue;
            double a[3], b[3], n[3];
            for (int k = 0; k < 3; ++k) a[k] = (double)p.m[3 + k] - (double)p.m[k], b[k] = (double)p.m[6 + k] - (double)p.m[k];
            v3cross(a, b, n);
            l.area = 0.5 * v3len(n);
            if (!((float)l.area > 0.0f) || !std::isfinite((float)(1.0 / l.area))) continue;
            break;
        }
        case RT_PRIM_QUAD: {
            // quads always join, as rects do: |u x v| in fp64 from the stored edges
            double a[3] = {p.m[3], p.m[4], p.m[5]}, b[3] = {p.m[6], p.m[7], p.m[8]}, n[3];
            v3cross(a, b, n);
            l.area = v3len(n);
            if (!((float)l.area > 0.0f) || !std::isfinite((float)(1.0 / l.area))) continue;
            break;
        }
        default: continue;
        }
        const double power = l.area * 0.5 * (luminance(l.even) + luminance(l.odd));
        if (!(l.area > 0.0) || !(power > 0.0) || !std::isfinite(power)) continue;
        l.prob = power;
        out.push_back(l);
    }
    // analytic lights, behind the area emitters: measure x luminance / pi in the same units -- 4 lum(I), 2 (1 - (cos_i
    // + cos_o) / 2) lum(I), r^2 lum(E)
    if (!s.alights.empty()) {
        const double r = scene_bound_radius(s);
        for (size_t i = 0; i < s.alights.size(); ++i) {
            const AnalyticRecord a = analytic_record(s.alights[i], r);
            if (!(a.weight > 0.0) || !std::isfinite(a.weight)) continue;
            SceneLight l;
            l.prim = -1, l.type = s.alights[i].type, l.analytic = (int)i;
            l.area = a.measure, l.prob = a.weight;
            for (int c = 0; c < 3; ++c) l.even[c] = l.odd[c] = a.color[c];
            out.push_back(l);
        }
    }
    // the environment, last: r^2 x scale x sum of luminance x solid angle, r the radius of the primitives' bounding sphere --
    // the flux through that sphere's cross-section up to pi, as area x luminance is an area emitter's up to pi
    if (s.env && s.env->flux > 0.0 && s.env_scale > 0.0f) {
        const double r = scene_bound_radius(s);
        const double power = r * r * (double)s.env_scale * s.env->flux;
        if (power > 0.0 && std::isfinite(power)) {
            SceneLight l;
            l.prim = -1, l.type = RT_LIGHT_ENVIRONMENT;
            l.area = 4.0 * pi;
            l.prob = power;
            // (reported emission: the mean radiance over the sphere)
            double mean[3] = {0, 0, 0};
            for (int i = 0; i < s.env->rows; ++i)
                for (int j = 0; j < s.env->cols; ++j)
                    for (int c = 0; c < 3; ++c) mean[c] += (double)s.env->rgb[3 * ((size_t)i * s.env->cols + j) + c] * s.env->band[(size_t)i];
            for (int c = 0; c < 3; ++c) l.even[c] = l.odd[c] = (float)((double)s.env_scale * mean[c] / (4.0 * pi));
            out.push_back(l);
        }
    }
    double total = 0.0;
    for (const SceneLight &l : out) total += l.prob;
    for (SceneLight &l : out) l.prob /= total;
    return out;
}

}  // namespace rtmi

// ---------------------------------------------------------------- environment map: validation, the sampling
// tables (rt_env.h says what they hold) and the file formats
namespace rtmi {

float env_uoff(float rotate_deg) {
    double t = (double)rotate_deg / 360.0;
    t -= std::floor(t);
    const float f = (float)t;
    return f < 1.0f ? f : 0.0f;
}

static bool env_args(float scale, float rotate_deg) {
    if (!(scale >= 0.0f) || !std::isfinite(scale)) {
        set_error("environment: scale %g must be finite and >= 0", (double)scale);
        return false;
    }
    if (!std::isfinite(rotate_deg)) {
        set_error("environment: rotate must be finite");
        return false;
    }
    return true;
}

// takes the texels over (rgb is moved from)
static int install_environment(Scene &s, int rows, int cols, std::vector<float> &&rgb, float scale, float rotate_deg,
                               const std::string &file) {
    for (size_t i = 0; i < rgb.size(); ++i)
        if (!(rgb[i] >= 0.0f) || !std::isfinite(rgb[i])) {
            set_error("environment: texel value %zu (%g) is negative or not finite", i, (double)rgb[i]);
            return RT_ERR_SCENE;
        }
    auto e = std::make_shared<SceneEnvironment>();
    e->rows = rows, e->cols = cols, e->file = file;
    e->rgb = std::move(rgb);
    // the tables, in fp64, stored as fp32: weight of a texel = luminance x the exact solid angle of its row band / cols
    const double pi = std::acos(-1.0);
    e->ct.resize((size_t)rows + 1);
    std::vector<double> ctd((size_t)rows + 1);
    for (int i = 0; i <= rows; ++i) ctd[(size_t)i] = i == 0 ? 1.0 : (i == rows ? -1.0 : std::cos(pi * (double)i / (double)rows));
    for (int i = 0; i <= rows; ++i) e->ct[(size_t)i] = (float)ctd[(size_t)i];
    e->band.resize((size_t)rows);
    std::vector<double> bandd((size_t)rows), row_sum((size_t)rows, 0.0);
    for (int i = 0; i < rows; ++i) {
        bandd[(size_t)i] = (2.0 * pi / (double)cols) * (ctd[(size_t)i] - ctd[(size_t)i + 1]);
        e->band[(size_t)i] = (float)bandd[(size_t)i];
    }
    auto lum = [&](size_t texel) {
        const float *t = e->rgb.data() + 3 * texel;
        return 0.2126 * t[0] + 0.7152 * t[1] + 0.0722 * t[2];
    };
    double total = 0.0;
    for (int i = 0; i < rows; ++i) {
        double acc = 0.0;
        for (int j = 0; j < cols; ++j) acc += lum((size_t)i * cols + j);
        row_sum[(size_t)i] = acc * bandd[(size_t)i];
        total += row_sum[(size_t)i];
    }
    if (!std::isfinite(total)) {
        set_error("environment: the texels' total is not finite");
        return RT_ERR_SCENE;
    }
    e->flux = total;
    e->marg.assign((size_t)rows + 1, 0.0f);
    e->cond.assign((size_t)rows * ((size_t)cols + 1), 0.0f);
    if (total > 0.0) {
        double cum = 0.0;
        for (int i = 0; i < rows; ++i) {
            cum += row_sum[(size_t)i];
            e->marg[(size_t)i + 1] = (float)std::fmin(cum / total, 1.0);
            if (!(row_sum[(size_t)i] > 0.0)) continue;
            float *c = e->cond.data() + (size_t)i * ((size_t)cols + 1);
            const double rs = row_sum[(size_t)i] / bandd[(size_t)i];
            double cc = 0.0;
            for (int j = 0; j < cols; ++j) {
                cc += lum((size_t)i * cols + j);
                c[j + 1] = (float)std::fmin(cc / rs, 1.0);
            }
            c[cols] = 1.0f;
        }
        e->marg[(size_t)rows] = 1.0f;
    }
    s.env = std::move(e);
    s.env_scale = scale, s.env_rotate = rotate_deg;
    s.touch();
    return RT_OK;
}

static int env_size(long long rows, long long cols) {
    if (rows < 1 || cols < 1) {
        set_error("environment: %lld x %lld texels", rows, cols);
        return RT_ERR_ARG;
    }
    if (rows > kEnvMaxTexels || cols > kEnvMaxTexels || rows * cols > kEnvMaxTexels) {
        set_error("environment map of %lld x %lld texels exceeds the limit of %lld", rows, cols, kEnvMaxTexels);
        return RT_ERR_LIMIT;
    }
    return RT_OK;
}

int set_environment(Scene &s, int rows, int cols, const float *rgb, float scale, float rotate_deg, const std::string &file) {
    if (rows == 0) {
        s.env.reset();
        s.env_scale = 1.0f, s.env_rotate = 0.0f;
        s.touch();
        return RT_OK;
    }
    int rc = env_size(rows, cols);
    if (rc) return rc;
    if (!rgb) {
        set_error("environment: null texels");
        return RT_ERR_ARG;
    }
    if (!env_args(scale, rotate_deg)) return RT_ERR_ARG;
    std::vector<float> copy(rgb, rgb + (size_t)rows * (size_t)cols * 3);
    return install_environment(s, rows, cols, std::move(copy), scale, rotate_deg, file);
}

int set_environment_file(Scene &s, const char *path, float scale, float rotate_deg) {
    if (!env_args(scale, rotate_deg)) return RT_ERR_ARG;
    std::vector<uint8_t> file;
    FILE *fp = fopen(path, "rb");
    if (!fp) {
        set_error("cannot open environment map '%s'", path);
        return RT_ERR_IO;
    }
    unsigned char head[4] = {0, 0, 0, 0};
    const size_t got = fread(head, 1, 4, fp);
    const std::vector<uint8_t> magic(head, head + got);
    const bool hdr = envfile::is_hdr(magic), pfm = envfile::is_pfm(magic);
    if (hdr || pfm) {
        file.assign(head, head + got);
        unsigned char chunk[65536];
        size_t n;
        while ((n = fread(chunk, 1, sizeof chunk, fp)) > 0) file.insert(file.end(), chunk, chunk + n);
    }
    fclose(fp);
    int rows = 0, cols = 0;
    std::vector<float> rgb;
    if (hdr || pfm) {
        std::string err;
        const int rc = hdr ? envfile::read_hdr(file, kEnvMaxTexels, rows, cols, rgb, err) : envfile::read_pfm(file, kEnvMaxTexels, rows, cols, rgb, err);
        if (rc) {
            set_error("%s: %s", path, err.c_str());
            return rc;
        }
    } else {  // an 8-bit image (PNG / PPM) as an LDR map: byte / 255, as image textures read their texels
        std::vector<uint8_t> bytes;
        int rc = read_image_file(path, rows, cols, bytes);
        if (rc) return rc;
        rc = env_size(rows, cols);
        if (rc) return rc;
        rgb.resize(bytes.size());
        for (size_t i = 0; i < bytes.size(); ++i) rgb[i] = (float)bytes[i] / 255.0f;
    }
    return install_environment(s, rows, cols, std::move(rgb), scale, rotate_deg, path);
}

double scene_bound_radius(const Scene &s) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    auto add = [&](double x, double y, double z) {
        const double p[3] = {x, y, z};
        for (int a = 0; a < 3; ++a) lo[a] = std::fmin(lo[a], p[a]), hi[a] = std::fmax(hi[a], p[a]);
    };
    for (const rt_prim &p : s.prims) {
        switch (p.type) {
        case RT_PRIM_SPHERE: {
            const double r = std::fabs((double)p.f[3]);
            add(p.f[0] - r, p.f[1] - r, p.f[2] - r), add(p.f[0] + r, p.f[1] + r, p.f[2] + r);
            break;
        }
        case RT_PRIM_XY_RECT: add(p.f[0], p.f[2], p.f[4]), add(p.f[1], p.f[3], p.f[4]); break;
        case RT_PRIM_XZ_RECT: add(p.f[0], p.f[4], p.f[2]), add(p.f[1], p.f[4], p.f[3]); break;
        case RT_PRIM_YZ_RECT: add(p.f[4], p.f[0], p.f[2]), add(p.f[4], p.f[1], p.f[3]); break;
        case RT_PRIM_CYLINDER: {
            const double r = std::fabs((double)p.f[0]);
            for (int k = 0; k < 8; ++k) {
                const double q[3] = {(k & 1) ? r : -r, (k & 2) ? r : -r, (k & 4) ? (double)p.f[2] : (double)p.f[1]};
                double w[3];
                for (int a = 0; a < 3; ++a) w[a] = p.m[4 * a] * q[0] + p.m[4 * a + 1] * q[1] + p.m[4 * a + 2] * q[2] + p.m[4 * a + 3];
                add(w[0], w[1], w[2]);
            }
            break;
        }
        case RT_PRIM_TRIANGLE:
            for (int k = 0; k < 3; ++k) add(p.m[3 * k], p.m[3 * k + 1], p.m[3 * k + 2]);
            break;
        case RT_PRIM_QUAD:
            for (int k = 0; k < 4; ++k) {
                const double fu = (k == 1 || k == 2) ? 1.0 : 0.0, fv = k >= 2 ? 1.0 : 0.0;
                add(p.m[0] + fu * p.m[3] + fv * p.m[6], p.m[1] + fu * p.m[4] + fv * p.m[7], p.m[2] + fu * p.m[5] + fv * p.m[8]);
            }
            break;
        default: break;
        }
    }
    if (!(hi[0] >= lo[0])) return 0.0;
    double d2 = 0.0;
    for (int a = 0; a < 3; ++a) d2 += (hi[a] - lo[a]) * (hi[a] - lo[a]);
    return 0.5 * std::sqrt(d2);
}

// ---------------------------------------------------------------- homogeneous media
int add_medium(Scene &s, const rt_medium &m) {
    if (m.shape != RT_MEDIUM_SPHERE && m.shape != RT_MEDIUM_BOX) {
        set_error("medium: shape %d (0 sphere, 1 box)", m.shape);
        return -RT_ERR_SCENE;
    }
    if (!(std::isfinite(m.density) && m.density >= 0.0f)) {
        set_error("medium: density %g must be finite and >= 0", (double)m.density);
        return -RT_ERR_SCENE;
    }
    for (int c = 0; c < 3; ++c)
        if (!(m.albedo[c] >= 0.0f && m.albedo[c] <= 1.0f)) {
            set_error("medium: albedo component %d (%g) outside [0, 1]", c, (double)m.albedo[c]);
            return -RT_ERR_SCENE;
        }
    const int nf = m.shape == RT_MEDIUM_SPHERE ? 4 : 6;
    for (int k = 0; k < nf; ++k)
        if (!std::isfinite(m.f[k])) {
            set_error("medium: a bound is not finite");
            return -RT_ERR_SCENE;
        }
    if (m.shape == RT_MEDIUM_SPHERE) {
        if (!(m.f[3] > 0.0f)) {
            set_error("medium sphere: radius %g must be > 0", (double)m.f[3]);
            return -RT_ERR_SCENE;
        }
    } else {
        for (int k = 0; k < 3; ++k)
            if (!(m.f[k] < m.f[3 + k])) {
                set_error("medium box: min %g >= max %g on axis %d", (double)m.f[k], (double)m.f[3 + k], k);
                return -RT_ERR_SCENE;
            }
    }
    if (s.media.size() >= (size_t)RT_MAX_MEDIA) {
        set_error("a scene holds at most %d media", RT_MAX_MEDIA);
        return -RT_ERR_LIMIT;
    }
    rt_medium rec = m;
    if (rec.shape == RT_MEDIUM_SPHERE) rec.f[4] = rec.f[5] = 0.0f;
    s.media.push_back(rec);
    s.media_g.push_back(0.0f);
    s.touch();
    return (int)s.media.size() - 1;
}

// ---------------------------------------------------------------- anisotropic media
int set_medium_phase(Scene &s, int medium, float g) {
    if (medium < 0 || (size_t)medium >= s.media.size()) {
        set_error("medium phase: medium %d out of range (the scene has %zu)", medium, s.media.size());
        return RT_ERR_ARG;
    }
    if (!(std::isfinite(g) && std::fabs(g) <= RT_PHASE_G_MAX)) {
        set_error("medium phase: g %g must be finite and within [-%g, %g]", (double)g, (double)RT_PHASE_G_MAX, (double)RT_PHASE_G_MAX);
        return RT_ERR_SCENE;
    }
    const float stored = std::fabs(g) < RT_PHASE_G_SNAP ? 0.0f : g;  // (the isotropic medium, instruction for instruction)
    if (s.media_g[(size_t)medium] != stored) {  // (a scene set to what it holds stays the scene it was: same version, same tables)
        s.media_g[(size_t)medium] = stored;
        s.touch();
    }
    return RT_OK;
}

// ---------------------------------------------------------------- moving spheres
int add_moving_sphere(Scene &s, const rt_moving_sphere &m) {
    if (!(std::isfinite(m.radius) && m.radius > 0.0f)) {
        set_error("moving sphere: radius %g must be finite and > 0", (double)m.radius);
        return -RT_ERR_SCENE;
    }
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(m.center0[k]) || !std::isfinite(m.center1[k]) || !std::isfinite(m.center1[k] - m.center0[k])) {
            set_error("moving sphere: a centre is not finite");
            return -RT_ERR_SCENE;
        }
    if (m.material < 0 || m.material >= (int)s.mats.size()) {
        set_error("moving sphere: unknown material %d (have %zu)", m.material, s.mats.size());
        return -RT_ERR_SCENE;
    }
    if (s.movers.size() >= (size_t)RT_MAX_MOVING_SPHERES) {
        set_error("a scene holds at most %d moving spheres", RT_MAX_MOVING_SPHERES);
        return -RT_ERR_LIMIT;
    }
    s.movers.push_back(m);
    s.touch();
    return (int)s.movers.size() - 1;
}

// ---------------------------------------------------------------- analytic lights
bool analytic_light_ok(const rt_analytic_light &l, const char *where) {
    if (l.type != RT_LIGHT_POINT && l.type != RT_LIGHT_SPOT && l.type != RT_LIGHT_DISTANT) {
        set_error("%s: unknown light type %d", where, l.type);
        return false;
    }
    const char *colour = l.type == RT_LIGHT_DISTANT ? "irradiance" : "intensity";
    bool any = false;
    for (int c = 0; c < 3; ++c) {
        if (!(std::isfinite(l.color[c]) && l.color[c] >= 0.0f)) {
            set_error("%s: %s component %d (%g) must be finite and >= 0", where, colour, c, (double)l.color[c]);
            return false;
        }
        any = any || l.color[c] > 0.0f;
    }
    if (!any) {
        set_error("%s: the %s is all zero", where, colour);
        return false;
    }
    if (l.type != RT_LIGHT_DISTANT)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(l.position[k])) {
                set_error("%s: the position is not finite", where);
                return false;
            }
    if (l.type != RT_LIGHT_POINT) {
        double n2 = 0.0;
        for (int k = 0; k < 3; ++k) n2 += (double)l.direction[k] * (double)l.direction[k];
        if (!(std::isfinite(n2) && n2 > 0.0)) {
            set_error("%s: the direction must be finite and non-zero", where);
            return false;
        }
    }
    if (l.type == RT_LIGHT_SPOT && !(l.angle[0] >= 0.0f && l.angle[0] <= l.angle[1] && l.angle[1] > 0.0f && l.angle[1] <= 179.0f)) {
        set_error("%s: the angles (inner %g, outer %g) must satisfy 0 <= inner <= outer, 0 < outer <= 179 degrees", where,
                  (double)l.angle[0], (double)l.angle[1]);
        return false;
    }
    if (l.type == RT_LIGHT_DISTANT && !(l.angle[0] >= 0.0f && l.angle[0] <= 45.0f)) {
        set_error("%s: the angular radius (%g) must lie in [0, 45] degrees", where, (double)l.angle[0]);
        return false;
    }
    return true;
}

AnalyticRecord analytic_record(const rt_analytic_light &l, double bound_radius) {
    AnalyticRecord a;
    const double pi = std::acos(-1.0), rad = pi / 180.0;
    const double lum = 0.2126 * (double)l.color[0] + 0.7152 * (double)l.color[1] + 0.0722 * (double)l.color[2];
    double fold = 1.0;
    if (l.type != RT_LIGHT_POINT) {
        double n2 = 0.0;
        for (int k = 0; k < 3; ++k) n2 += (double)l.direction[k] * (double)l.direction[k];
        const double inv_len = (l.type == RT_LIGHT_DISTANT ? -1.0 : 1.0) / std::sqrt(n2);  // (the record: TOWARDS a distant light)
        for (int k = 0; k < 3; ++k) a.dir[k] = (double)l.direction[k] * inv_len + 0.0;  // (+ 0.0: no negative zero in the record)
    }
    if (l.type == RT_LIGHT_POINT) {
        a.measure = 4.0 * pi;
    } else if (l.type == RT_LIGHT_SPOT) {
        const double ci = std::cos((double)l.angle[0] * rad), co = std::cos((double)l.angle[1] * rad);
        a.cos_o = (float)co;
        a.inv = (float)std::min(1.0 / (ci - co), (double)FLT_MAX);
        a.measure = 2.0 * pi * (1.0 - 0.5 * (ci + co));
    } else {
        const double ca = std::cos((double)l.angle[0] * rad);
        a.omc = (float)(1.0 - ca);
        a.dist = (float)(4.0 * bound_radius);
        fold = 2.0 / (1.0 + ca);
        a.measure = pi * bound_radius * bound_radius;
    }
    for (int c = 0; c < 3; ++c) a.color[c] = (float)((double)l.color[c] * fold);
    a.weight = a.measure * lum / pi;
    // (what the record's fp32 words cannot hold is left out, as a sliver triangle is)
    if (!std::isfinite(a.color[0]) || !std::isfinite(a.color[1]) || !std::isfinite(a.color[2]) || !((float)a.measure > 0.0f) ||
        !std::isfinite((float)(1.0 / a.measure)) || !std::isfinite(a.dist))
        a.weight = 0.0;
    return a;
}

}  // namespace rtmi
