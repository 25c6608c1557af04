// Camera projections: the map (s, t, lens sample) -> ray of the orthographic, panoramic and fisheye cameras.  fp32
// with a FIXED operation sequence, every fused multiply-add explicit, sincosf from the math library of either side: the
// kernels of camera_kernel.h (render_body.h, section 6b) and the host evaluation (rt_camera_ray, capi.cpp) compile this text.
// These kernels are held per sample to an fp64 statement (tests/ref64_camera.py), not bit for bit to a restatement.
//
// Every projection defines a pinhole ray (o, D) with |D| = fd, the focus distance; the lens rule is the perspective camera's:
// off = lens_radius (lx u + ly v), ray = (o + off, D - off), so that every lens ray of a sample passes through o + D.
//
// The six camera records of the hot table (device_scene.h: off_cam), xyz each -- record 0's w stays the lens radius, the w of
// records 1 to 5 belong to other parts.  What the host derives in fp64 and rounds once (scene.cpp, camera_records):
//                   0          1                                   2            3            4   5
//   perspective     lookfrom   lower_left                          horizontal   vertical     u   v     (untouched: camera.h:9-31)
//   orthographic    D = fd f   lower_left = lookfrom - hor/2       horizontal   vertical     u   v     hor = h a u, ver = h v
//                                                  - ver/2                                             o = ll + s hor + t ver
//   panoramic       lookfrom   {hfov, vfov, 0} in radians          {fd, 0, 0}   f            u   v
//   fisheye         lookfrom   {fov / 2 in radians, max(a, 1),     {fd, 0, 0}   f            u   v
//                               max(1 / a, 1)}
// f = -w is the unit forward direction, a the aspect ratio.  The model number travels in RenderParams::flags (RT_PFLAG_PROJ_*).
#pragma once
#include <math.h>

#ifndef RTMI_HD
#ifdef __HIPCC__
#define RTMI_HD __host__ __device__ inline
#else
#define RTMI_HD inline
#endif
#endif

namespace rtmi {

// the model numbers: rt_projection_type of include/rtmi.h
enum CameraModel : int { CAM_PERSPECTIVE = 0, CAM_ORTHOGRAPHIC = 1, CAM_PANORAMIC = 2, CAM_FISHEYE = 3 };

// The ray of (s, t) through the lens point of offset off = lens_radius (lx u + ly v) (zeros: the pinhole ray), for the three
// models above; V: a four-vector with x, y, z (float4 on the device).  false: no ray -- a fisheye sample outside the image
// circle (r > 1); o and d are then zeros.
template <class V>
RTMI_HD bool camera_ray(int model, const V &c0, const V &c1, const V &c2, const V &c3, const V &c_u, const V &c_v, float s, float t,
                        float offx, float offy, float offz, float &ox, float &oy, float &oz, float &dx, float &dy, float &dz) {
    float px, py, pz;  // o
    float Dx, Dy, Dz;  // D
    if (model == CAM_ORTHOGRAPHIC) {
        px = fmaf(t, c3.x, fmaf(s, c2.x, c1.x));
        py = fmaf(t, c3.y, fmaf(s, c2.y, c1.y));
        pz = fmaf(t, c3.z, fmaf(s, c2.z, c1.z));
        Dx = c0.x, Dy = c0.y, Dz = c0.z;
    } else {
        float kf, ku, kv;  // d^ = kf f + ku u + kv v
        if (model == CAM_PANORAMIC) {
            const float phi = (s - 0.5f) * c1.x, psi = (t - 0.5f) * c1.y;
            float sp, cp, ss, cs;
            sincosf(phi, &sp, &cp);
            sincosf(psi, &ss, &cs);
            kf = cs * cp, ku = cs * sp, kv = ss;
        } else {  // equidistant fisheye: theta = r fov / 2 from f, the image circle inscribed in the shorter side
            const float qx = fmaf(2.0f, s, -1.0f) * c1.y, qy = fmaf(2.0f, t, -1.0f) * c1.z;
            const float r = sqrtf(fmaf(qx, qx, qy * qy));
            if (r > 1.0f) {
                ox = oy = oz = dx = dy = dz = 0.0f;
                return false;
            }
            float st, ct;
            sincosf(r * c1.x, &st, &ct);
            const float k = r > 0.0f ? st / r : 0.0f;  // (r = 0: qx = qy = 0 and d^ = f)
            kf = ct, ku = k * qx, kv = k * qy;
        }
        const float fd = c2.x;
        Dx = fd * fmaf(kv, c_v.x, fmaf(ku, c_u.x, kf * c3.x));
        Dy = fd * fmaf(kv, c_v.y, fmaf(ku, c_u.y, kf * c3.y));
        Dz = fd * fmaf(kv, c_v.z, fmaf(ku, c_u.z, kf * c3.z));
        px = c0.x, py = c0.y, pz = c0.z;
    }
    dx = Dx - offx, dy = Dy - offy, dz = Dz - offz;
    ox = px + offx, oy = py + offy, oz = pz + offz;
    return true;
}

// the perspective camera's ray as the kernels form it (render_body.h 6b; camera::get_ray, camera.h:32-39), for the host
// evaluation: c0 = origin, c1 = lower_left, c2 = horizontal, c3 = vertical
template <class V>
RTMI_HD void camera_ray_perspective(const V &c0, const V &c1, const V &c2, const V &c3, float s, float t, float offx, float offy, float offz,
                                    float &ox, float &oy, float &oz, float &dx, float &dy, float &dz) {
    dx = fmaf(t, c3.x, fmaf(s, c2.x, c1.x));
    dy = fmaf(t, c3.y, fmaf(s, c2.y, c1.y));
    dz = fmaf(t, c3.z, fmaf(s, c2.z, c1.z));
    dx = (dx - c0.x) - offx;
    dy = (dy - c0.y) - offy;
    dz = (dz - c0.z) - offz;
    ox = c0.x + offx;
    oy = c0.y + offy;
    oz = c0.z + offz;
}

// the lens offset of the sample (lx, ly) of the unit disk: lens_radius (lx u + ly v), as render_body.h 6b forms it
template <class V>
RTMI_HD void camera_lens_offset(float lens_radius, const V &c_u, const V &c_v, float lx, float ly, float &offx, float &offy, float &offz) {
    const float rdx = lens_radius * lx, rdy = lens_radius * ly;
    offx = fmaf(c_u.x, rdx, c_v.x * rdy);
    offy = fmaf(c_u.y, rdx, c_v.y * rdy);
    offz = fmaf(c_u.z, rdx, c_v.z * rdy);
}

}  // namespace rtmi
