"""rtmi -- Python host mirror of the reference's scene-JSON -> render -> PPM interface.

Thin ctypes binding over the C ABI of ``librtmi.so`` (``include/rtmi.h``).  Names
follow the reference (``gpu-version/parser.hpp:504`` ``parse_scene``,
``gpu-version/main.cu:359`` ``output_image``, the ``camera`` / ``sphere`` /
``xy_rect`` / ``cylinder`` / ``lambertian`` / ``metal`` / ``dielectric`` /
``diffuse_light`` / ``solid_color`` / ``checker_texture`` constructors).

There is NO CPU rendering path in this package: if ``librtmi.so`` is missing the
import fails, and if no gfx950 device is usable every ``render*`` call raises
``RtmiError``.

The directory name (``ray-tracing-in-cuda_amd``) is not a valid Python identifier;
load the package with ``__graft_entry__.load_package()`` (module name ``rtmi``).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

try:  # torch first, so that one HIP runtime (torch's bundled one) serves both
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the binding itself
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
# RTMI_LIB: alternative build of the same library (kernel tuning A/B); default is the in-tree one
_LIB_PATH = os.environ.get("RTMI_LIB") or os.path.join(_HERE, "librtmi.so")
if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `make -C {_HERE}` (or __graft_entry__.build()); "
        "this package has no fallback implementation"
    )
_lib = C.CDLL(_LIB_PATH)

RT_OK = 0
FLAG_SKY_GRADIENT = 1
FLAG_DEFOCUS_BLUR = 2
PRIM_SPHERE, PRIM_XY_RECT, PRIM_XZ_RECT, PRIM_YZ_RECT, PRIM_CYLINDER, PRIM_TRIANGLE, PRIM_QUAD = range(7)
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_DIFFUSE_LIGHT = range(4)
TEX_SOLID, TEX_CHECKER, TEX_IMAGE = range(3)

# numpy views of the table records (layouts of include/rtmi.h)
MESH_NORMALS = {"flat": 0, "file": 1, "smooth": 2}  # rt_mesh_normals
PRIM_DTYPE = np.dtype(
    [("type", "<i4"), ("material", "<i4"), ("f", "<f4", (6,)), ("m", "<f4", (12,)), ("m_inv", "<f4", (12,))]
)
MATERIAL_DTYPE = np.dtype(
    [("type", "<i4"), ("texture", "<i4"), ("albedo", "<f4", (3,)), ("fuzz", "<f4"), ("ir", "<f4")]
)
TEXTURE_DTYPE = np.dtype([("type", "<i4"), ("c0", "<f4", (3,)), ("c1", "<f4", (3,))])
LIGHT_ENVIRONMENT = 100  # rt_light.shape of the environment map (RT_LIGHT_ENVIRONMENT)
MEDIUM_SPHERE, MEDIUM_BOX = 0, 1  # rt_medium.shape
MEDIUM_DTYPE = np.dtype(  # rt_medium: sphere f = {cx, cy, cz, r}; box f = {min.xyz, max.xyz}
    [("shape", "<i4"), ("f", "<f4", (6,)), ("density", "<f4"), ("albedo", "<f4", (3,))]
)
MAX_MOVING_SPHERES = 64
MOVING_SPHERE_DTYPE = np.dtype(  # rt_moving_sphere: the centre at shutter time 0 and at 1
    [("center0", "<f4", (3,)), ("center1", "<f4", (3,)), ("radius", "<f4"), ("material", "<i4")]
)
# ray queries (rt_trace_hip): rt_ray is two 16-byte records, rt_hit three
RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("t_max", "<f4"), ("dir", "<f4", (3,)), ("reserved", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("prim", "<i4"), ("material", "<i4"), ("front", "<i4"), ("normal", "<f4", (3,)), ("u", "<f4"),
                      ("point", "<f4", (3,)), ("v", "<f4")])
HIT_INVALID = -2     # rt_hit.prim of a ray that failed the guard (RT_HIT_INVALID)
TRACE_CLOSEST, TRACE_OCCLUDED = 0, 1
PROJECTIONS = ("perspective", "orthographic", "panoramic", "fisheye")  # rt_projection_type, by number
TRACE_ITEM = 64      # rays per work item of the query kernels (RT_TRACE_ITEM): scheduling only
TRACE_LAYOUT = 8192  # Stats.kernel_variant of a ray query: the layout | 8192
LIGHT_POINT, LIGHT_SPOT, LIGHT_DISTANT = 101, 102, 103  # rt_analytic_light.type, and rt_light.shape of such a light
ANALYTIC_LIGHT_DTYPE = np.dtype(  # rt_analytic_light; angle: degrees -- spot: inner, outer; distant: angular radius, 0
    [("type", "<i4"), ("position", "<f4", (3,)), ("direction", "<f4", (3,)), ("color", "<f4", (3,)), ("angle", "<f4", (2,))]
)
LIGHT_DTYPE = np.dtype(
    [("prim", "<i4"), ("shape", "<i4"), ("probability", "<f4"), ("area", "<f4"), ("emission", "<f4", (3,)),
     ("emission_odd", "<f4", (3,))]
)


class RtmiError(RuntimeError):
    def __init__(self, status: int, where: str):
        self.status = status
        msg = _lib.rt_last_error().decode(errors="replace")
        kind = _lib.rt_status_string(status).decode()
        super().__init__(f"{where}: {kind} ({status}): {msg}")


class _Camera(C.Structure):
    _fields_ = [
        ("lookfrom", C.c_float * 3), ("lookat", C.c_float * 3), ("vup", C.c_float * 3),
        ("vfov", C.c_float), ("aspect", C.c_float), ("aperture", C.c_float), ("focus_dist", C.c_float),
        ("origin", C.c_float * 3), ("lower_left", C.c_float * 3), ("horizontal", C.c_float * 3),
        ("vertical", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3), ("w", C.c_float * 3),
        ("lens_radius", C.c_float),
    ]


class _Info(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("samples_per_pixel", C.c_int32), ("max_depth", C.c_int32),
        ("num_prims", C.c_int32), ("num_materials", C.c_int32), ("num_textures", C.c_int32),
        ("flags", C.c_uint32), ("background", C.c_float * 3), ("russian_roulette", C.c_float),
    ]


class Opts(C.Structure):
    """rt_opts (include/rtmi.h)."""
    _fields_ = [
        ("seed", C.c_uint64), ("device", C.c_int32), ("tile_rows", C.c_int32), ("tile_first", C.c_int32),
        ("tile_stride", C.c_int32), ("tile_rotate", C.c_int32), ("spp_chunk", C.c_int32), ("sample_first", C.c_int32),
        ("sample_count", C.c_int32), ("variant", C.c_uint32),
    ]

    def __init__(self, **kw):
        super().__init__()
        _lib.rt_opts_default(C.byref(self))
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError(f"rt_opts has no field {k!r}")
            setattr(self, k, v)


class Stats(C.Structure):
    """rt_stats (include/rtmi.h)."""
    _fields_ = [
        ("kernel_ms", C.c_double), ("upload_ms", C.c_double), ("launches", C.c_int32), ("local_rows", C.c_int32),
        ("samples", C.c_uint64), ("queries", C.c_uint64), ("prim_tests", C.c_uint64), ("hits", C.c_uint64),
        ("misses", C.c_uint64), ("scatter", C.c_uint64 * 4), ("rng_draws", C.c_uint64),
        ("cand_lanes", C.c_uint64), ("cand_waves", C.c_uint64), ("clusters_visited", C.c_uint64),
        ("wave_queries", C.c_uint64), ("groups_visited", C.c_uint64), ("lane_clusters", C.c_uint64),
        ("lane_groups", C.c_uint64), ("group_maxpop", C.c_uint64), ("query_maxpop", C.c_uint64), ("cycles", C.c_uint64 * 6),
        ("cull_prefix", C.c_int32),
        ("cull_clusters", C.c_int32), ("cull_groups", C.c_int32), ("cull_cluster_size", C.c_int32),
        ("wave_start_spread_us", C.c_double), ("wave_end_spread_us", C.c_double), ("wave_span_us", C.c_double),
        ("lane_cands", C.c_uint64), ("cull_mode", C.c_int32), ("cull_windows", C.c_int32), ("gather_ms", C.c_double), ("devices_used", C.c_int32), ("grid_sheet", C.c_int32),
        ("kernel_variant", C.c_int32), ("walk_resumed", C.c_int32),
    ]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in ("scatter", "cycles")}
        d["scatter"] = list(self.scatter)
        d["cycles"] = list(self.cycles)
        return d


class TableInfo(C.Structure):
    """rt_table_info (include/rtmi.h): the device tables the host builds for a scene."""
    _fields_ = [
        ("image_floats", C.c_int32), ("grid_wide", C.c_int32), ("grid_sheet", C.c_int32), ("grid_cells", C.c_int32),
        ("grid_n", C.c_int32 * 3), ("grid_min", C.c_float * 3), ("grid_size", C.c_float * 3),
        ("ob_near2", C.c_float), ("ob_far2", C.c_float),
        ("ns", C.c_int32), ("np", C.c_int32), ("ncl", C.c_int32), ("nr", C.c_int32), ("nc", C.c_int32), ("nt", C.c_int32),
        ("nr_a", C.c_int32), ("nc_a", C.c_int32), ("nt_a", C.c_int32),
        ("off_grid_cells", C.c_int32), ("off_grid_items", C.c_int32),
        ("off_sph_cold", C.c_int32), ("off_rect_cold", C.c_int32), ("off_cyl_cold", C.c_int32), ("off_tri_cold", C.c_int32),
        ("off_rect_hot", C.c_int32), ("off_cyl_hot", C.c_int32), ("off_tri_hot", C.c_int32),
        ("hot_bytes_grid", C.c_int32), ("kernel_variant", C.c_int32),
    ]


class NestedInfo(C.Structure):
    """rt_nested_info (include/rtmi.h): the nested cells of a scene's tables; all zero while they are flat."""
    _fields_ = [
        ("cells", C.c_int32), ("sub_cells", C.c_int32), ("sub_items", C.c_int64),
        ("off_sub_grids", C.c_int32), ("off_sub_cells", C.c_int32), ("first_sub_cell", C.c_int32),
        ("threshold", C.c_int32), ("axis_cap", C.c_int32), ("longest", C.c_int32),
    ]


class Adaptive(C.Structure):
    """rt_adaptive (include/rtmi.h): the noise target of an adaptive render."""
    _fields_ = [("min_spp", C.c_int32), ("max_spp", C.c_int32), ("threshold", C.c_float)]


class AdaptiveStats(C.Structure):
    """rt_adaptive_stats (include/rtmi.h): the schedule an adaptive render ran."""
    _fields_ = [
        ("passes", C.c_int32), ("tiles", C.c_int32), ("spp_after", C.c_int32 * 32), ("active", C.c_int32 * 32),
        ("samples", C.c_uint64), ("kernel_ms", C.c_double),
    ]

    def as_dict(self):
        n = self.passes
        return {"passes": n, "tiles": self.tiles, "spp_after": list(self.spp_after[:n]), "active": list(self.active[:n]),
                "samples": self.samples, "kernel_ms": self.kernel_ms}


class Denoise(C.Structure):
    """rt_denoise (include/rtmi.h): the filter's parameters; a sigma of 0 is its default, iterations -1 the default count."""
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


class Display(C.Structure):
    """rt_display (include/rtmi.h): the display stage's parameters; exposure, white and bloom_levels 0 are their defaults."""
    _fields_ = [("tonemap", C.c_int32), ("exposure", C.c_float), ("auto_key", C.c_float), ("white", C.c_float),
                ("bloom_strength", C.c_float), ("bloom_threshold", C.c_float), ("bloom_levels", C.c_int32)]


class DisplayStats(C.Structure):
    """rt_display_stats (include/rtmi.h)."""
    _fields_ = [("log_sum", C.c_int64), ("exposure_used", C.c_float), ("ms", C.c_double)]


TONEMAP_CLAMP, TONEMAP_REINHARD, TONEMAP_ACES = 0, 1, 2
TONEMAPS = {"clamp": TONEMAP_CLAMP, "reinhard": TONEMAP_REINHARD, "aces": TONEMAP_ACES}
FEATURE_ALBEDO, FEATURE_NORMAL, FEATURE_DEPTH = 0, 1, 2
DENOISE_DEFAULT_ITERATIONS = -1


def _sig(name, restype, *argtypes):
    fn = getattr(_lib, name)
    fn.restype = restype
    fn.argtypes = list(argtypes)
    return fn


_p = C.c_void_p
_f3 = C.POINTER(C.c_float)
_sig("rt_last_error", C.c_char_p)
_sig("rt_status_string", C.c_char_p, C.c_int)
_sig("rt_abi_version", C.c_int)
_sig("rt_has_ablations", C.c_int)
_sig("rt_variant_workgroup", C.c_int, C.c_uint, C.POINTER(C.c_int32))
_sig("rt_device_count", C.c_int)
_sig("rt_struct_size", C.c_size_t, C.c_int)
_sig("rt_opts_default", None, C.POINTER(Opts))
_sig("rt_scene_load_json", _p, C.c_char_p)
_sig("rt_scene_parse_json", _p, C.c_char_p, C.c_size_t)
_sig("rt_scene_rtiow", _p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int)
_sig("rt_scene_to_json", C.c_size_t, _p, C.c_char_p, C.c_size_t)
_sig("rt_scene_free", None, _p)
_sig("rt_scene_new", _p, C.c_int, C.c_int, C.c_int, C.c_int)
_sig("rt_scene_set_background", C.c_int, _p, _f3, C.c_uint32)
_sig("rt_scene_set_camera", C.c_int, _p, _f3, _f3, _f3, C.c_float, C.c_float, C.c_float, C.c_float)
_sig("rt_scene_add_solid_color", C.c_int, _p, _f3)
_sig("rt_scene_add_checker", C.c_int, _p, _f3, _f3)
_sig("rt_scene_add_lambertian", C.c_int, _p, C.c_int)
_sig("rt_scene_add_metal", C.c_int, _p, _f3, C.c_float)
_sig("rt_scene_add_dielectric", C.c_int, _p, C.c_float)
_sig("rt_scene_add_rough_metal", C.c_int, _p, _f3, C.c_float)
_sig("rt_scene_add_plastic", C.c_int, _p, C.c_int, C.c_float, C.c_float)
_sig("rt_scene_add_rough_glass", C.c_int, _p, C.c_float, C.c_float, _f3)
_sig("rt_scene_add_pbr", C.c_int, _p, C.c_int, C.c_float, C.c_float, C.c_float)
_sig("rt_scene_set_pbr_map", C.c_int, _p, C.c_int, C.c_int)
_sig("rt_scene_get_pbr_map", C.c_int, _p, C.c_int, C.POINTER(C.c_int))
_sig("rt_scene_add_diffuse_light", C.c_int, _p, C.c_int)
_sig("rt_scene_add_sphere", C.c_int, _p, _f3, C.c_float, C.c_int)
_sig("rt_scene_add_rect", C.c_int, _p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int)
_sig("rt_scene_add_cylinder", C.c_int, _p, C.c_float, C.c_float, C.c_float, C.c_int, _f3, C.c_float, _f3)
_sig("rt_scene_add_image_texture", C.c_int, _p, C.c_int, C.c_int, _p)
_sig("rt_scene_add_image_texture_file", C.c_int, _p, C.c_char_p)
_sig("rt_scene_get_image", C.c_int, _p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _p, C.c_size_t)


class Noise(C.Structure):  # rt_noise
    _fields_ = [("style", C.c_int32), ("octaves", C.c_int32), ("seed", C.c_uint32), ("axis", C.c_int32), ("scale", C.c_float),
                ("distortion", C.c_float)]


NOISE_STYLES = {"fbm": 0, "turbulence": 1, "marble": 2}
NOISE_AXES = {"x": 0, "y": 1, "z": 2}
_sig("rt_scene_add_noise_texture", C.c_int, _p, _f3, _f3, C.POINTER(Noise))
_sig("rt_scene_get_noise", C.c_int, _p, C.c_int, C.POINTER(Noise))
_sig("rt_scene_set_bump", C.c_int, _p, C.c_int, C.c_int, C.c_float)
_sig("rt_scene_get_bump", C.c_int, _p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float))
_sig("rt_scene_set_normal_map", C.c_int, _p, C.c_int, C.c_int, C.c_float)
_sig("rt_scene_get_normal_map", C.c_int, _p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float))
_sig("rt_scene_add_image_texture_rgba", C.c_int, _p, C.c_int, C.c_int, _p)
_sig("rt_scene_get_image_alpha", C.c_int, _p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _p, C.c_size_t)
_sig("rt_scene_set_alpha", C.c_int, _p, C.c_int, C.c_int, C.c_float)
_sig("rt_scene_get_alpha", C.c_int, _p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float))
assert _lib.rt_struct_size(24) == C.sizeof(Noise) == 24
_sig("rt_scene_add_triangle", C.c_int, _p, _f3, _f3, _f3, _f3, _f3, _f3, C.c_int)
_sig("rt_scene_add_quad", C.c_int, _p, _f3, _f3, _f3, C.c_int, _f3, C.c_float, _f3)
_sig("rt_scene_add_box", C.c_int, _p, _f3, _f3, C.c_int, _f3, C.c_float, _f3)
_sig("rt_scene_add_obj", C.c_int, _p, C.c_char_p, C.c_int, C.c_float, _f3, _f3)
_sig("rt_scene_add_triangle_normals", C.c_int, _p, _f3, _f3, _f3, _f3, _f3, _f3, _f3, _f3, _f3, C.c_int)
_sig("rt_scene_add_obj_normals", C.c_int, _p, C.c_char_p, C.c_int, C.c_float, _f3, _f3, C.c_int, C.c_float)
_sig("rt_set_mesh_normals_override", None, C.c_int, C.c_float)
_sig("rt_scene_override", C.c_int, _p, C.c_int, C.c_int, C.c_int, C.c_int)
_sig("rt_scene_rotate_cylinders", C.c_int, _p, C.c_double)
_sig("rt_scene_set_output_file", C.c_int, _p, C.c_char_p)
_sig("rt_scene_dna", _p, _p, C.c_double)
_sig("rt_scene_clone", _p, _p)
_sig("rt_scene_get_info", C.c_int, _p, C.POINTER(_Info))
_sig("rt_scene_get_camera", C.c_int, _p, C.POINTER(_Camera))
_sig("rt_scene_get_prims", C.c_int, _p, _p, C.c_int)
_sig("rt_scene_get_materials", C.c_int, _p, _p, C.c_int)
_sig("rt_scene_get_textures", C.c_int, _p, _p, C.c_int)
_sig("rt_shard_rows", C.c_int, _p, C.POINTER(Opts))
_sig("rt_shard_global_row", C.c_int, _p, C.POINTER(Opts), C.c_int)
_sig("rt_shard_deal", C.c_int, _p, C.POINTER(Opts), C.c_int)
_sig("rt_render_hip_device", C.c_int, _p, C.POINTER(Opts), _p, _p, C.POINTER(Stats))
_sig("rt_render_hip", C.c_int, _p, C.POINTER(Opts), _p, C.POINTER(Stats))
_sig("rt_render_hip_tiles", C.c_int, _p, C.POINTER(Opts), C.POINTER(C.c_int), C.c_int, _p, C.POINTER(Stats))
_sig("rt_tiles_shutdown", None)
_sig("rt_shard_place_rows_device", C.c_int, _p, C.POINTER(Opts), C.c_int, C.c_int, _p, _p, _p)
_sig("rt_scene_set_russian_roulette", C.c_int, _p, C.c_float)
_sig("rt_scene_set_light_sampling", C.c_int, _p, C.c_int)
_sig("rt_scene_get_light_sampling", C.c_int, _p)
_sig("rt_scene_get_lights", C.c_int, _p, _p, C.c_int)
_sig("rt_scene_set_mesh_lights", C.c_int, _p, C.c_int)
_sig("rt_scene_get_mesh_lights", C.c_int, _p)
_sig("rt_scene_set_media_light_sampling", C.c_int, _p, C.c_int)
_sig("rt_scene_get_media_light_sampling", C.c_int, _p)
_sig("rt_scene_set_environment", C.c_int, _p, C.c_int, C.c_int, _p, C.c_float, C.c_float)
_sig("rt_scene_set_environment_file", C.c_int, _p, C.c_char_p, C.c_float, C.c_float)
_sig("rt_scene_get_environment", C.c_int, _p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float), _p,
     C.c_size_t)
_sig("rt_environment_eval", C.c_int, _p, _f3, _f3, C.POINTER(C.c_float))
_sig("rt_environment_sample", C.c_int, _p, C.c_float, C.c_float, _f3, _f3, C.POINTER(C.c_float))
_sig("rt_scene_add_medium_sphere", C.c_int, _p, _f3, C.c_float, C.c_float, _f3)
_sig("rt_scene_add_medium_box", C.c_int, _p, _f3, _f3, C.c_float, _f3)
_sig("rt_scene_get_media", C.c_int, _p, _p, C.c_int)
_sig("rt_scene_clear_media", C.c_int, _p)
_sig("rt_medium_interval", C.c_int, _p, _f3, _f3, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float))
_sig("rt_scene_set_medium_phase", C.c_int, _p, C.c_int, C.c_float)
_sig("rt_scene_get_medium_phase", C.c_int, _p, C.c_int, C.POINTER(C.c_float))
_sig("rt_phase_hg_sample", C.c_int, C.c_float, _f3, C.c_float, C.c_float, _f3)
_sig("rt_phase_hg_eval", C.c_float, C.c_float, C.c_float)
_sig("rt_media_transmittance", C.c_int, _p, _f3, _f3, C.c_float, C.POINTER(C.c_float))
_sig("rt_scene_add_moving_sphere", C.c_int, _p, _f3, _f3, C.c_float, C.c_int)
_sig("rt_scene_moving_sphere_count", C.c_int, _p)
_sig("rt_scene_get_moving_spheres", C.c_int, _p, _p, C.c_int)
_sig("rt_scene_clear_moving_spheres", C.c_int, _p)
_sig("rt_moving_sphere_hit", C.c_int, _p, C.c_float, _f3, _f3, C.c_float, C.POINTER(C.c_float))
_sig("rt_shutter_time", C.c_float, C.c_uint64, C.c_uint32, C.c_uint32)
_sig("rt_scene_add_point_light", C.c_int, _p, _f3, _f3)
_sig("rt_scene_add_spot_light", C.c_int, _p, _f3, _f3, _f3, C.c_float, C.c_float)
_sig("rt_scene_add_distant_light", C.c_int, _p, _f3, _f3, C.c_float)
_sig("rt_scene_get_analytic_lights", C.c_int, _p, _p, C.c_int)
_sig("rt_scene_clear_analytic_lights", C.c_int, _p)
assert _lib.rt_struct_size(25) == ANALYTIC_LIGHT_DTYPE.itemsize == 48
_sig("rt_scene_set_nested_grid", C.c_int, _p, C.c_int)
_sig("rt_scene_get_nested_grid", C.c_int, _p)
_sig("rt_scene_nested_info", C.c_int, _p, C.POINTER(NestedInfo))
_sig("rt_scene_quad_counts", C.c_int, _p, C.POINTER(C.c_int32), C.POINTER(C.c_int32))
_sig("rt_render_hip_count", C.c_int, _p, C.POINTER(Opts), _p, C.POINTER(Stats))
_sig("rt_scene_table_info", C.c_int, _p, C.POINTER(TableInfo))
_sig("rt_scene_table_image", C.c_int, _p, _p, C.c_int)
_sig("rt_scene_tile_beams", C.c_int, _p, _p, C.c_int)
_sig("rt_scene_tile_beams_device", C.c_int, _p, C.POINTER(Opts), _p, C.c_int)
_sig("rt_scene_tile_beams_capacity", C.c_int)
_sig("rt_render_hip_accumulate", C.c_int, _p, C.POINTER(Opts), _p, _p, C.POINTER(Stats))
_sig("rt_acc_to_rgb", None, _p, _p, C.c_size_t)
_sig("rt_render_hip_adaptive", C.c_int, _p, C.POINTER(Opts), C.POINTER(Adaptive), _p, _p, C.POINTER(AdaptiveStats))
_sig("rt_render_hip_adaptive_device", C.c_int, _p, C.POINTER(Opts), C.POINTER(Adaptive), _p, _p, _p, C.POINTER(AdaptiveStats))
_sig("rt_shard_scatter_rows", C.c_int, _p, C.POINTER(Opts), _p, _p)
_sig("rt_write_ppm", C.c_int, C.c_char_p, _p, C.c_int, C.c_int, C.c_int)
_sig("rt_quantize_rgb8", C.c_int, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p)
_sig("rt_write_png", C.c_int, C.c_char_p, _p, C.c_int, C.c_int, C.c_int, C.c_int)
_sig("rt_scene_output_file", C.c_char_p, _p)
_sig("rt_philox4x32_10", None, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))
_sig("rt_aabb_hit", C.c_int, _f3, _f3, _f3, _f3, C.c_float, C.c_float)
_sig("rt_sample_stream", None, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_int)
_sig("rt_render_hip_feature", C.c_int, _p, C.POINTER(Opts), C.c_int, _p, C.POINTER(Stats))
_sig("rt_render_hip_feature_device", C.c_int, _p, C.POINTER(Opts), C.c_int, _p, _p, C.POINTER(Stats))
_sig("rt_trace_hip", C.c_int, _p, C.POINTER(Opts), C.c_int, _p, C.c_size_t, _p, C.POINTER(Stats))
_sig("rt_trace_hip_device", C.c_int, _p, C.POINTER(Opts), C.c_int, _p, C.c_size_t, _p, _p, C.POINTER(Stats))
_sig("rt_ray_valid", C.c_int, _p)
_sig("rt_scene_set_projection", C.c_int, _p, C.c_int, C.POINTER(C.c_float))
_sig("rt_scene_get_projection", C.c_int, _p, C.POINTER(C.c_int), C.POINTER(C.c_float))
_sig("rt_camera_ray", C.c_int, _p, C.c_float, C.c_float, C.c_float, C.c_float, _p, C.POINTER(C.c_int))
assert _lib.rt_struct_size(21) == RAY_DTYPE.itemsize == 32 and _lib.rt_struct_size(22) == HIT_DTYPE.itemsize == 48
_sig("rt_denoise_hip", C.c_int, C.c_int, C.c_int, _p, C.c_int, _p, _p, _p, _p, C.c_int, C.POINTER(Denoise), C.c_int, _p,
     C.POINTER(C.c_double))
_sig("rt_denoise_hip_device", C.c_int, C.c_int, C.c_int, _p, C.c_int, _p, _p, _p, _p, C.c_int, C.POINTER(Denoise), C.c_int, _p, _p,
     C.POINTER(C.c_double))
_sig("rt_display_hip", C.c_int, C.c_int, C.c_int, _p, C.c_int, _p, C.POINTER(Display), C.c_int, _p, _p, C.POINTER(DisplayStats))
_sig("rt_display_hip_device", C.c_int, C.c_int, C.c_int, _p, C.c_int, _p, C.POINTER(Display), C.c_int, _p, _p, _p,
     C.POINTER(DisplayStats))
_sig("rt_display_timing", C.c_int, C.POINTER(C.c_double), C.c_int)
_sig("rt_write_ppm_rgb8", C.c_int, C.c_char_p, _p, C.c_int, C.c_int)
_sig("rt_write_png_rgb8", C.c_int, C.c_char_p, _p, C.c_int, C.c_int)
_sig("rt_write_hdr", C.c_int, C.c_char_p, _p, C.c_int, C.c_int, C.c_int)
_sig("rt_write_pfm", C.c_int, C.c_char_p, _p, C.c_int, C.c_int, C.c_int)

C_SYMBOLS = [
    "rt_last_error", "rt_status_string", "rt_abi_version", "rt_struct_size", "rt_device_count", "rt_has_ablations", "rt_opts_default",
    "rt_scene_table_info", "rt_scene_table_image", "rt_variant_workgroup",
    "rt_scene_tile_beams", "rt_scene_tile_beams_device", "rt_scene_tile_beams_capacity",
    "rt_scene_load_json", "rt_scene_parse_json", "rt_scene_rtiow", "rt_scene_to_json", "rt_scene_free",
    "rt_scene_new", "rt_scene_set_background", "rt_scene_set_camera", "rt_scene_add_solid_color",
    "rt_scene_add_checker", "rt_scene_add_lambertian", "rt_scene_add_metal", "rt_scene_add_dielectric",
    "rt_scene_add_rough_metal", "rt_scene_add_plastic", "rt_scene_add_rough_glass", "rt_scene_add_noise_texture", "rt_scene_get_noise",
    "rt_scene_set_bump", "rt_scene_get_bump", "rt_scene_set_normal_map", "rt_scene_get_normal_map",
    "rt_scene_add_image_texture_rgba", "rt_scene_get_image_alpha", "rt_scene_set_alpha", "rt_scene_get_alpha", "rt_scene_add_pbr", "rt_scene_set_pbr_map", "rt_scene_get_pbr_map",
    "rt_scene_add_diffuse_light", "rt_scene_add_sphere", "rt_scene_add_rect", "rt_scene_add_cylinder",
    "rt_scene_add_image_texture", "rt_scene_add_image_texture_file", "rt_scene_get_image", "rt_scene_add_triangle",
    "rt_scene_add_quad", "rt_scene_add_box", "rt_scene_add_obj", "rt_scene_add_triangle_normals", "rt_scene_add_obj_normals", "rt_set_mesh_normals_override",
    "rt_scene_override", "rt_scene_get_info", "rt_scene_get_camera", "rt_scene_get_prims",
    "rt_scene_get_materials", "rt_scene_get_textures", "rt_shard_rows", "rt_shard_global_row", "rt_shard_deal",
    "rt_render_hip_device", "rt_render_hip", "rt_render_hip_tiles", "rt_tiles_shutdown", "rt_shard_place_rows_device", "rt_render_hip_count", "rt_render_hip_accumulate", "rt_scene_set_russian_roulette",
    "rt_acc_to_rgb", "rt_shard_scatter_rows", "rt_write_ppm",
    "rt_quantize_rgb8", "rt_philox4x32_10", "rt_aabb_hit", "rt_sample_stream", "rt_write_png",
    "rt_scene_output_file", "rt_scene_rotate_cylinders", "rt_scene_set_output_file", "rt_scene_dna", "rt_scene_clone",
    "rt_scene_set_light_sampling", "rt_scene_get_light_sampling", "rt_scene_get_lights",
    "rt_scene_set_mesh_lights", "rt_scene_get_mesh_lights",
    "rt_scene_set_media_light_sampling", "rt_scene_get_media_light_sampling", "rt_media_transmittance",
    "rt_render_hip_adaptive", "rt_render_hip_adaptive_device",
    "rt_scene_set_nested_grid", "rt_scene_get_nested_grid", "rt_scene_nested_info", "rt_scene_quad_counts",
    "rt_scene_set_environment", "rt_scene_set_environment_file", "rt_scene_get_environment", "rt_environment_eval",
    "rt_environment_sample",
    "rt_scene_add_medium_sphere", "rt_scene_add_medium_box", "rt_scene_get_media", "rt_scene_clear_media", "rt_medium_interval",
    "rt_scene_set_medium_phase", "rt_scene_get_medium_phase", "rt_phase_hg_sample", "rt_phase_hg_eval",
    "rt_scene_add_moving_sphere", "rt_scene_moving_sphere_count", "rt_scene_get_moving_spheres", "rt_scene_clear_moving_spheres",
    "rt_moving_sphere_hit", "rt_shutter_time",
    "rt_scene_add_point_light", "rt_scene_add_spot_light", "rt_scene_add_distant_light", "rt_scene_get_analytic_lights",
    "rt_scene_clear_analytic_lights",
    "rt_trace_hip", "rt_trace_hip_device", "rt_ray_valid",
    "rt_scene_set_projection", "rt_scene_get_projection", "rt_camera_ray",
    "rt_render_hip_feature", "rt_render_hip_feature_device", "rt_denoise_hip", "rt_denoise_hip_device",
    "rt_display_hip", "rt_display_hip_device", "rt_display_timing", "rt_write_hdr", "rt_write_pfm",
    "rt_write_ppm_rgb8", "rt_write_png_rgb8",
]


def _v3(v):
    a = (C.c_float * 3)(*[float(x) for x in v])
    return a


def _check(status: int, where: str):
    if status != RT_OK:
        raise RtmiError(status, where)


def _check_id(rc: int, where: str) -> int:
    if rc < 0:
        raise RtmiError(-rc, where)
    return rc


class Scene:
    """gpu-version/parser.hpp:16-32 ``struct scene``: the flattened scene tables."""

    def __init__(self, handle):
        if not handle:
            raise RtmiError(4, "scene")
        self._h = C.c_void_p(handle)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:  # (module globals are already cleared when the interpreter shuts down)
            _lib.rt_scene_free(h)
            self._h = None

    # ---- construction ------------------------------------------------------
    @classmethod
    def load(cls, path: str) -> "Scene":
        h = _lib.rt_scene_load_json(os.fsencode(path))
        if not h:
            raise RtmiError(_guess_status(), f"parse_scene({path!r})")
        return cls(h)

    @classmethod
    def parse(cls, text: str) -> "Scene":
        b = text.encode()
        h = _lib.rt_scene_parse_json(b, len(b))
        if not h:
            raise RtmiError(_guess_status(), "parse_scene(<text>)")
        return cls(h)

    @classmethod
    def rtiow(cls, seed=7, width=400, height=225, spp=100, max_depth=50) -> "Scene":
        """random_scene() + camera of cmake-cpu-version/main.cpp:89-94, 125-172."""
        h = _lib.rt_scene_rtiow(seed, width, height, spp, max_depth)
        if not h:
            raise RtmiError(_guess_status(), "rt_scene_rtiow")
        return cls(h)

    @classmethod
    def new(cls, width, height, spp, max_depth=50) -> "Scene":
        return cls(_lib.rt_scene_new(width, height, spp, max_depth))

    # ---- builders (reference constructor argument lists) --------------------
    def set_background(self, rgb=(0, 0, 0), sky_gradient=False, defocus_blur=True):
        flags = (FLAG_SKY_GRADIENT if sky_gradient else 0) | (FLAG_DEFOCUS_BLUR if defocus_blur else 0)
        _check(_lib.rt_scene_set_background(self._h, _v3(rgb), flags), "set_background")

    def set_russian_roulette(self, p: float):
        """Survival probability per bounce (4_0_path_tracing.py's p_RR); 0 switches it off."""
        _check(_lib.rt_scene_set_russian_roulette(self._h, float(p)), "set_russian_roulette")

    def set_light_sampling(self, on: bool = True):
        """Next-event estimation with MIS (include/rtmi.h, rt_scene_set_light_sampling); False switches it off."""
        _check(_lib.rt_scene_set_light_sampling(self._h, 1 if on else 0), "set_light_sampling")

    @property
    def light_sampling(self) -> bool:
        return _check_id(_lib.rt_scene_get_light_sampling(self._h), "get_light_sampling") != 0

    def set_mesh_lights(self, on: bool = True):
        """Emissive triangles (OBJ meshes: one light per triangle) join the emitters light sampling samples (include/rtmi.h,
        rt_scene_set_mesh_lights); False, the default, leaves them to the BSDF sample."""
        _check(_lib.rt_scene_set_mesh_lights(self._h, 1 if on else 0), "set_mesh_lights")

    @property
    def mesh_lights(self) -> bool:
        return _check_id(_lib.rt_scene_get_mesh_lights(self._h), "get_mesh_lights") != 0

    def set_media_light_sampling(self, on: bool = True):
        """Light sampling in participating media (include/rtmi.h, rt_scene_set_media_light_sampling): with media and light
        sampling that has something to sample, medium vertices take light samples and shadow rays are attenuated by the
        media they cross; False, the default, leaves that combination refused."""
        _check(_lib.rt_scene_set_media_light_sampling(self._h, 1 if on else 0), "set_media_light_sampling")

    @property
    def media_light_sampling(self) -> bool:
        return _check_id(_lib.rt_scene_get_media_light_sampling(self._h), "get_media_light_sampling") != 0

    def media_transmittance(self, orig, direction, t_max=0.999):
        """Host evaluation of a shadow ray's transmittance through the scene's media (rt_media_transmittance): exp(-tau) over
        orig + t direction, t in [0.001, t_max], as the device text sums tau; exactly 1.0 when the ray stays in no medium."""
        T = C.c_float()
        _check(_lib.rt_media_transmittance(self._h, _v3(orig), _v3(direction), float(t_max), C.byref(T)), "media_transmittance")
        return T.value

    def set_environment(self, rgb=None, scale: float = 1.0, rotate: float = 0.0, file: str = None):
        """Environment map (include/rtmi.h, rt_scene_set_environment): ``rgb`` is a rows x cols x 3 float array in lat-long
        layout (row 0 = +y), or ``file`` names a .hdr / .pfm / .png / .ppm; neither clears the environment."""
        if file is not None:
            _check(_lib.rt_scene_set_environment_file(self._h, os.fsencode(file), float(scale), float(rotate)), "set_environment")
            return
        if rgb is None:
            _check(_lib.rt_scene_set_environment(self._h, 0, 0, None, 1.0, 0.0), "set_environment")
            return
        a = np.ascontiguousarray(rgb, dtype=np.float32)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("environment: a rows x cols x 3 array")
        _check(_lib.rt_scene_set_environment(self._h, a.shape[0], a.shape[1], a.ctypes.data_as(C.c_void_p), float(scale), float(rotate)),
               "set_environment")

    def add_medium_sphere(self, center, radius: float, density: float, albedo=(1.0, 1.0, 1.0), g: float = 0.0) -> int:
        """A homogeneous medium inside a sphere (include/rtmi.h, participating media): density per unit length, scattering
        with the given albedo and Henyey-Greenstein asymmetry ``g`` (0: isotropic).  Returns the medium's id.  The medium is
        added, then its phase set: a refused ``g`` raises and leaves the medium in the scene, isotropic."""
        mid = _check_id(_lib.rt_scene_add_medium_sphere(self._h, _v3(center), float(radius), float(density), _v3(albedo)), "add_medium_sphere")
        if g != 0.0:
            self.set_medium_phase(mid, g)
        return mid

    def add_medium_box(self, bmin, bmax, density: float, albedo=(1.0, 1.0, 1.0), g: float = 0.0) -> int:
        """A homogeneous medium inside an axis-aligned box."""
        mid = _check_id(_lib.rt_scene_add_medium_box(self._h, _v3(bmin), _v3(bmax), float(density), _v3(albedo)), "add_medium_box")
        if g != 0.0:
            self.set_medium_phase(mid, g)
        return mid

    def set_medium_phase(self, medium: int, g: float):
        """The asymmetry g in [-0.99, 0.99] of a medium's Henyey-Greenstein phase function: > 0 scatters forward, < 0
        backward; |g| < 1e-3 is stored as 0, the isotropic medium."""
        _check(_lib.rt_scene_set_medium_phase(self._h, int(medium), float(g)), "set_medium_phase")

    def medium_phase(self, medium: int) -> float:
        """The asymmetry a medium holds (the stored value)."""
        g = C.c_float()
        _check(_lib.rt_scene_get_medium_phase(self._h, int(medium), C.byref(g)), "medium_phase")
        return g.value

    def media(self) -> np.ndarray:
        """The scene's media in list order (MEDIUM_DTYPE records)."""
        return self._table(_lib.rt_scene_get_media, MEDIUM_DTYPE)

    def clear_media(self):
        _check(_lib.rt_scene_clear_media(self._h), "clear_media")

    def add_moving_sphere(self, center0, center1, radius: float, material: int) -> int:
        """A sphere whose centre moves from center0 (shutter time 0) to center1 (shutter time 1) within every sample
        (include/rtmi.h, motion blur).  Returns the mover's id."""
        return _check_id(_lib.rt_scene_add_moving_sphere(self._h, _v3(center0), _v3(center1), float(radius), int(material)),
                         "add_moving_sphere")

    def moving_spheres(self) -> np.ndarray:
        """The scene's moving spheres in list order (MOVING_SPHERE_DTYPE records)."""
        return self._table(_lib.rt_scene_get_moving_spheres, MOVING_SPHERE_DTYPE)

    def clear_moving_spheres(self):
        _check(_lib.rt_scene_clear_moving_spheres(self._h), "clear_moving_spheres")

    def point_light(self, position, intensity) -> int:
        """A point light (include/rtmi.h, rt_scene_add_point_light): ``intensity`` is RGB per steradian.  Analytic
        lights act through light sampling alone (set_light_sampling)."""
        return _check_id(_lib.rt_scene_add_point_light(self._h, _v3(position), _v3(intensity)), "point_light")

    def spot_light(self, position, direction, intensity, inner_angle: float, outer_angle: float) -> int:
        """A spot light pointing along ``direction``: full intensity inside ``inner_angle``, a smoothstep of the cosine down
        to nothing at ``outer_angle`` (degrees from the axis)."""
        return _check_id(_lib.rt_scene_add_spot_light(self._h, _v3(position), _v3(direction), _v3(intensity), float(inner_angle),
                                                      float(outer_angle)), "spot_light")

    def distant_light(self, direction, irradiance, angular_radius: float = 0.0) -> int:
        """A distant light (a sun) whose light travels along ``direction``: ``irradiance`` is what a surface facing it
        receives, ``angular_radius`` (degrees, at most 45) the half-angle of its disc."""
        return _check_id(_lib.rt_scene_add_distant_light(self._h, _v3(direction), _v3(irradiance), float(angular_radius)), "distant_light")

    def analytic_lights(self) -> np.ndarray:
        """The scene's point, spot and distant lights in list order, as given (ANALYTIC_LIGHT_DTYPE records)."""
        return self._table(_lib.rt_scene_get_analytic_lights, ANALYTIC_LIGHT_DTYPE)

    def clear_analytic_lights(self):
        _check(_lib.rt_scene_clear_analytic_lights(self._h), "clear_analytic_lights")

    @property
    def environment(self):
        """(texels as a rows x cols x 3 float32 array, scale, rotate), or None."""
        rows, cols, scale, rot = C.c_int(), C.c_int(), C.c_float(), C.c_float()
        _check(_lib.rt_scene_get_environment(self._h, C.byref(rows), C.byref(cols), C.byref(scale), C.byref(rot), None, 0), "get_environment")
        if rows.value == 0:
            return None
        a = np.empty((rows.value, cols.value, 3), np.float32)
        _check(_lib.rt_scene_get_environment(self._h, None, None, None, None, a.ctypes.data_as(C.c_void_p), a.size), "get_environment")
        return a, scale.value, rot.value

    def environment_eval(self, direction):
        """Host evaluation of the device lookup: (rgb, pdf) of a direction."""
        rgb, pdf = (C.c_float * 3)(), C.c_float()
        _check(_lib.rt_environment_eval(self._h, _v3(direction), rgb, C.byref(pdf)), "environment_eval")
        return np.array(rgb[:], np.float32), np.float32(pdf.value)

    def environment_sample(self, u1: float, u2: float):
        """Host evaluation of the device sampler: (direction, rgb, pdf) for two uniforms in [0, 1)."""
        d, rgb, pdf = (C.c_float * 3)(), (C.c_float * 3)(), C.c_float()
        _check(_lib.rt_environment_sample(self._h, float(u1), float(u2), d, rgb, C.byref(pdf)), "environment_sample")
        return np.array(d[:], np.float32), np.array(rgb[:], np.float32), np.float32(pdf.value)

    def set_nested_grid(self, on: bool = True):
        """A second grid level for clustered geometry (include/rtmi.h, rt_scene_set_nested_grid); False switches it off."""
        _check(_lib.rt_scene_set_nested_grid(self._h, 1 if on else 0), "set_nested_grid")

    @property
    def nested_grid(self) -> bool:
        return _check_id(_lib.rt_scene_get_nested_grid(self._h), "get_nested_grid") != 0

    def nested_info(self) -> NestedInfo:
        """The nested cells of this scene's tables (no GPU needed); all zero while the tables are flat."""
        t = NestedInfo()
        _check(_lib.rt_scene_nested_info(self._h, C.byref(t)), "rt_scene_nested_info")
        return t

    def camera(self, lookfrom, lookat, vup, vfov, aspect_ratio=0.0, aperture=0.0, focus_dist=0.0):
        _check(_lib.rt_scene_set_camera(self._h, _v3(lookfrom), _v3(lookat), _v3(vup), vfov, aspect_ratio,
                                        aperture, focus_dist), "camera")

    def set_projection(self, type, *params) -> None:
        """The camera's projection (rt_scene_set_projection): "perspective" (the default), "orthographic" (height),
        "panoramic" (hfov = 360, vfov = 180) or "fisheye" (fov = 180), by name or number; angles in degrees.  Kept by camera()
        and override()."""
        t = PROJECTIONS.index(type) if isinstance(type, str) and type in PROJECTIONS else type
        if isinstance(t, str) or len(params) > 2:
            raise ValueError(f"set_projection: no projection {type!r} with {len(params)} parameters ({', '.join(PROJECTIONS)})")
        p = (C.c_float * 2)(*[float(x) for x in params]) if params else None
        if p is not None and int(t) == 2 and len(params) == 1:
            p[1] = 180.0
        _check(_lib.rt_scene_set_projection(self._h, int(t), p), "rt_scene_set_projection")

    @property
    def projection(self):
        """(name, parameters): ("perspective", ()), ("orthographic", (height,)), ("panoramic", (hfov, vfov)), ("fisheye", (fov,))"""
        t = C.c_int(0)
        p = (C.c_float * 2)()
        _check(_lib.rt_scene_get_projection(self._h, C.byref(t), p), "rt_scene_get_projection")
        return PROJECTIONS[t.value], tuple(float(x) for x in p[: (0, 1, 2, 1)[t.value]])

    def camera_ray(self, s, t, lx=0.0, ly=0.0):
        """The ray the kernels start at (s, t) for the lens sample (lx, ly), any projection (rt_camera_ray; no GPU needed):
        -> (origin[3], direction[3], valid) as float32 arrays; valid is False outside a fisheye's image circle (zeros)."""
        ray = np.zeros(1, dtype=RAY_DTYPE)
        ok = C.c_int(0)
        _check(_lib.rt_camera_ray(self._h, float(s), float(t), float(lx), float(ly), ray.ctypes.data_as(C.c_void_p), C.byref(ok)), "rt_camera_ray")
        return ray["origin"][0].copy(), ray["dir"][0].copy(), bool(ok.value)

    def solid_color(self, rgb) -> int:
        return _check_id(_lib.rt_scene_add_solid_color(self._h, _v3(rgb)), "solid_color")

    def checker_texture(self, even, odd) -> int:
        return _check_id(_lib.rt_scene_add_checker(self._h, _v3(even), _v3(odd)), "checker_texture")

    def image_texture(self, pixels, alpha=None) -> int:
        """Image texture (taichi-version/material.py:137-144) from a (rows, cols, 3) uint8 array or a PPM / PNG file.
        alpha: a (rows, cols) uint8 alpha plane (a (rows, cols, 4) array brings its own, as a PNG file with alpha does):
        colour lookups ignore it, set_alpha() makes it a material's mask."""
        if isinstance(pixels, (str, bytes, os.PathLike)):
            if alpha is not None:
                raise ValueError("an image file brings its own alpha")
            return _check_id(_lib.rt_scene_add_image_texture_file(self._h, os.fsencode(pixels)), "image_texture")
        px = np.ascontiguousarray(pixels, dtype=np.uint8)
        if px.ndim == 3 and px.shape[2] == 4 and alpha is None:
            px, alpha = np.ascontiguousarray(px[:, :, :3]), px[:, :, 3]
        if alpha is not None:
            al = np.ascontiguousarray(alpha, dtype=np.uint8)
            if px.ndim != 3 or px.shape[2] != 3 or al.shape != px.shape[:2]:
                raise ValueError("image texture pixels must have shape (rows, cols, 3) and alpha (rows, cols)")
            rgba = np.ascontiguousarray(np.concatenate([px, al[:, :, None]], axis=2))
            return _check_id(_lib.rt_scene_add_image_texture_rgba(self._h, px.shape[0], px.shape[1], rgba.ctypes.data_as(C.c_void_p)),
                             "image_texture")
        if px.ndim != 3 or px.shape[2] != 3:
            raise ValueError("image texture pixels must have shape (rows, cols, 3)")
        return _check_id(_lib.rt_scene_add_image_texture(self._h, px.shape[0], px.shape[1], px.ctypes.data_as(C.c_void_p)),
                         "image_texture")

    def noise_texture(self, color0, color1, style="fbm", scale=1.0, octaves=1, seed=0, axis="y", distortion=5.0) -> int:
        """A procedural solid texture: color0 + s (color1 - color0) with s in [0, 1] from lattice noise at the hit
        point.  style: "fbm", "turbulence" or "marble"; axis ("x", "y", "z") and distortion are marble's alone."""
        if style not in NOISE_STYLES:
            raise ValueError('noise_texture style must be "fbm", "turbulence" or "marble"')
        if axis not in NOISE_AXES:
            raise ValueError('noise_texture axis must be "x", "y" or "z"')
        n = Noise(NOISE_STYLES[style], int(octaves), int(seed) & 0xFFFFFFFF, NOISE_AXES[axis], float(scale), float(distortion))
        return _check_id(_lib.rt_scene_add_noise_texture(self._h, _v3(color0), _v3(color1), C.byref(n)), "noise_texture")

    def noise(self, texture: int) -> dict:
        """The parameters of noise texture `texture` as noise_texture() takes them (a style other than marble: axis "x",
        distortion 0 -- it has neither)."""
        n = Noise()
        _check(_lib.rt_scene_get_noise(self._h, texture, C.byref(n)), "rt_scene_get_noise")
        return {"style": [k for k, v in NOISE_STYLES.items() if v == n.style][0], "scale": float(n.scale), "octaves": int(n.octaves),
                "seed": int(n.seed), "axis": "xyz"[n.axis], "distortion": float(n.distortion)}

    def set_bump(self, material: int, texture: int, strength: float) -> None:
        """Bump mapping: the scalar of noise texture `texture` as a height field on `material`; the shading normal
        tilts against its gradient x `strength`.  Any material but a diffuse_light; texture -1 or strength 0 removes it."""
        _check(_lib.rt_scene_set_bump(self._h, int(material), int(texture), float(strength)), "rt_scene_set_bump")

    def bump(self, material: int):
        """(texture, strength) of the material's bump, or None."""
        t, k = C.c_int(), C.c_float()
        _check(_lib.rt_scene_get_bump(self._h, int(material), C.byref(t), C.byref(k)), "rt_scene_get_bump")
        return None if t.value < 0 else (int(t.value), float(k.value))

    def set_normal_map(self, material: int, texture: int, scale: float = 1.0) -> None:
        """Normal mapping: image texture `texture` read at the hit's (u, v) as a direction in the surface's tangent
        frame (R along +dp/du, G along +dp/dv, B along the outward normal) on `material`; the tangential part x `scale`.  Any
        material but a diffuse_light, and not a bumped one; texture -1 or scale 0 removes it."""
        _check(_lib.rt_scene_set_normal_map(self._h, int(material), int(texture), float(scale)), "rt_scene_set_normal_map")

    def normal_map(self, material: int):
        """(texture, scale) of the material's normal map, or None."""
        t, k = C.c_int(), C.c_float()
        _check(_lib.rt_scene_get_normal_map(self._h, int(material), C.byref(t), C.byref(k)), "rt_scene_get_normal_map")
        return None if t.value < 0 else (int(t.value), float(k.value))

    def set_alpha(self, material: int, texture: int, cutoff: float = 0.5) -> None:
        """Alpha cutout: the alpha byte of image texture `texture` at the hit's (u, v) opens a hole in `material`
        where it lies below ceil(255 x cutoff); cutoff in (0, 1].  Any material but a diffuse_light; texture -1 removes it."""
        _check(_lib.rt_scene_set_alpha(self._h, int(material), int(texture), float(cutoff)), "rt_scene_set_alpha")

    def alpha(self, material: int):
        """(texture, cutoff) of the material's alpha mask, or None."""
        t, k = C.c_int(), C.c_float()
        _check(_lib.rt_scene_get_alpha(self._h, int(material), C.byref(t), C.byref(k)), "rt_scene_get_alpha")
        return None if t.value < 0 else (int(t.value), float(k.value))

    def get_image_alpha(self, texture: int):
        """The (rows, cols) uint8 alpha plane of image texture `texture`, or None where it has none."""
        rows, cols = C.c_int(), C.c_int()
        has = _check_id(_lib.rt_scene_get_image_alpha(self._h, texture, C.byref(rows), C.byref(cols), None, 0), "rt_scene_get_image_alpha")
        if not has:
            return None
        out = np.empty((rows.value, cols.value), dtype=np.uint8)
        _check_id(_lib.rt_scene_get_image_alpha(self._h, texture, None, None, out.ctypes.data_as(C.c_void_p), out.nbytes),
                  "rt_scene_get_image_alpha")
        return out

    def get_image(self, texture: int) -> np.ndarray:
        rows, cols = C.c_int(), C.c_int()
        _check_id(_lib.rt_scene_get_image(self._h, texture, C.byref(rows), C.byref(cols), None, 0), "rt_scene_get_image")
        out = np.empty((rows.value, cols.value, 3), dtype=np.uint8)
        _check_id(_lib.rt_scene_get_image(self._h, texture, None, None, out.ctypes.data_as(C.c_void_p), out.nbytes),
                  "rt_scene_get_image")
        return out

    def triangle(self, v1, v2, v3, material, u1=(0, 0), u2=(0, 0), u3=(0, 0), normals=None) -> int:
        """Triangle(v1, v2, v3, u1, u2, u3, material), taichi-version/hittable.py:95-110.  normals: three vertex normals
        (n1, n2, n3) for smooth shading (stored normalised, visible in prims()), None: a flat triangle."""
        uv = [(C.c_float * 3)(float(u[0]), float(u[1]), 0.0) for u in (u1, u2, u3)]
        if normals is not None:
            n = np.asarray(normals, dtype=np.float64)
            if n.shape != (3, 3):
                raise ValueError("triangle normals must be three vectors of 3 numbers")
            return _check_id(_lib.rt_scene_add_triangle_normals(self._h, _v3(v1), _v3(v2), _v3(v3), _v3(n[0]), _v3(n[1]), _v3(n[2]),
                                                                uv[0], uv[1], uv[2], material), "triangle")
        return _check_id(_lib.rt_scene_add_triangle(self._h, _v3(v1), _v3(v2), _v3(v3), uv[0], uv[1], uv[2], material),
                         "triangle")

    def quad(self, q, u, v, material, rotate=None, translate=None) -> int:
        """The parallelogram q, q + u, q + u + v, q + v, its normal along u x v.  rotate: (axis, degrees), then
        translate: an offset -- applied to q, u, v when it is added; prims() shows the quad it became."""
        ax, deg = (_v3(rotate[0]), float(rotate[1])) if rotate is not None else (None, 0.0)
        t = _v3(translate) if translate is not None else None
        return _check_id(_lib.rt_scene_add_quad(self._h, _v3(q), _v3(u), _v3(v), material, ax, deg, t), "quad")

    def box(self, min, max, material, rotate=None, translate=None) -> int:
        """Six quads over [min, max], normals outward, with the same optional rotate (axis, degrees) then translate; returns
        the index of the first of the six (+z, -z, +x, -x, +y, -y)."""
        ax, deg = (_v3(rotate[0]), float(rotate[1])) if rotate is not None else (None, 0.0)
        t = _v3(translate) if translate is not None else None
        return _check_id(_lib.rt_scene_add_box(self._h, _v3(min), _v3(max), material, ax, deg, t), "box")

    def add_obj(self, path, material, scale=1.0, matrix=None, translate=None, normals="flat", crease_angle=180.0) -> int:
        """readobj + placement, taichi-version/main.py:23-41, 110-118; returns the number of triangles added.
        normals: "flat", "file" (the file's vn lines) or "smooth" (generated, angle-weighted, from the faces within
        crease_angle degrees of each other)."""
        m = (C.c_float * 9)(*[float(x) for x in np.asarray(matrix, dtype=np.float64).reshape(9)]) if matrix is not None else None
        t = _v3(translate) if translate is not None else None
        if normals not in MESH_NORMALS:
            raise ValueError('add_obj normals must be "flat", "file" or "smooth"')
        if normals != "flat":
            return _check_id(_lib.rt_scene_add_obj_normals(self._h, os.fsencode(path), material, scale, m, t, MESH_NORMALS[normals],
                                                           float(crease_angle)), "add_obj")
        return _check_id(_lib.rt_scene_add_obj(self._h, os.fsencode(path), material, scale, m, t), "add_obj")

    def lambertian(self, texture_or_color) -> int:
        tex = texture_or_color if isinstance(texture_or_color, int) else self.solid_color(texture_or_color)
        return _check_id(_lib.rt_scene_add_lambertian(self._h, tex), "lambertian")

    def metal(self, albedo, fuzz) -> int:
        return _check_id(_lib.rt_scene_add_metal(self._h, _v3(albedo), fuzz), "metal")

    def rough_metal(self, albedo, roughness) -> int:
        """GGX rough metal: albedo is F0, roughness in [0, 1]; materials() shows it as type 4 with fuzz = roughness."""
        return _check_id(_lib.rt_scene_add_rough_metal(self._h, _v3(albedo), roughness), "rough_metal")

    def plastic(self, texture_or_color, ior=1.5, roughness=0.3) -> int:
        """A diffuse body (a colour or a texture id, as lambertian takes) under a clear GGX coat of index ior > 1;
        materials() shows it as type 5 with fuzz = roughness and ir = ior."""
        tex = texture_or_color if isinstance(texture_or_color, int) else self.solid_color(texture_or_color)
        return _check_id(_lib.rt_scene_add_plastic(self._h, tex, ior, roughness), "plastic")

    def rough_glass(self, ir=1.5, roughness=0.3, absorption=None) -> int:
        """Rough glass: GGX reflection or refraction about a microfacet normal, index ir > 1, roughness in [0, 1];
        absorption: three coefficients >= 0 per unit world length (None: clear) that tint light by the distance travelled inside.
        materials() shows it as type 6 with fuzz = roughness and albedo = absorption."""
        sigma = None if absorption is None else _v3(absorption)
        return _check_id(_lib.rt_scene_add_rough_glass(self._h, ir, roughness, sigma), "rough_glass")

    def pbr(self, texture_or_color, metallic=0.0, roughness=0.5, ior=1.5, metallic_roughness=None) -> int:
        """The metallic-roughness material: a base colour (a texture id of any type, or a colour), a metallic and a
        roughness factor in [0, 1], the coat's index ior > 1, and optionally a metallic-roughness map -- a texture id of any type
        whose G channel scales the roughness and whose B channel scales the metalness (glTF 2.0's convention).  Every vertex is a
        rough_metal (F0 = base colour) with probability metalness, else a plastic.  materials() shows it as type 7 with
        fuzz = roughness factor and albedo[0] = metallic factor."""
        tex = texture_or_color if isinstance(texture_or_color, int) else self.solid_color(texture_or_color)
        m = _check_id(_lib.rt_scene_add_pbr(self._h, tex, metallic, roughness, ior), "pbr")
        if metallic_roughness is not None:
            self.set_pbr_map(m, metallic_roughness)
        return m

    def set_pbr_map(self, material: int, texture: int) -> None:
        """The metallic-roughness map of a pbr material: any texture id; -1 removes it."""
        _check(_lib.rt_scene_set_pbr_map(self._h, int(material), int(texture)), "rt_scene_set_pbr_map")

    def pbr_map(self, material: int):
        """The texture id of a pbr material's metallic-roughness map, or None."""
        t = C.c_int()
        _check(_lib.rt_scene_get_pbr_map(self._h, int(material), C.byref(t)), "rt_scene_get_pbr_map")
        return None if t.value < 0 else int(t.value)

    def dielectric(self, index_of_refraction) -> int:
        return _check_id(_lib.rt_scene_add_dielectric(self._h, index_of_refraction), "dielectric")

    def diffuse_light(self, texture_or_color) -> int:
        tex = texture_or_color if isinstance(texture_or_color, int) else self.solid_color(texture_or_color)
        return _check_id(_lib.rt_scene_add_diffuse_light(self._h, tex), "diffuse_light")

    def sphere(self, center, radius, material) -> int:
        return _check_id(_lib.rt_scene_add_sphere(self._h, _v3(center), radius, material), "sphere")

    def xy_rect(self, x0, x1, y0, y1, k, material) -> int:
        return _check_id(_lib.rt_scene_add_rect(self._h, 0, x0, x1, y0, y1, k, material), "xy_rect")

    def xz_rect(self, x0, x1, z0, z1, k, material) -> int:
        return _check_id(_lib.rt_scene_add_rect(self._h, 1, x0, x1, z0, z1, k, material), "xz_rect")

    def yz_rect(self, y0, y1, z0, z1, k, material) -> int:
        return _check_id(_lib.rt_scene_add_rect(self._h, 2, y0, y1, z0, z1, k, material), "yz_rect")

    def cylinder(self, radius, zmin, zmax, material, rotate=None, translate=None) -> int:
        """rotate = (axis, degrees); applied before translate (parser.hpp:423-440)."""
        axis = _v3(rotate[0]) if rotate else None
        deg = float(rotate[1]) if rotate else 0.0
        off = _v3(translate) if translate is not None else None
        return _check_id(_lib.rt_scene_add_cylinder(self._h, radius, zmin, zmax, material, axis, deg, off), "cylinder")

    # ---- animation (blue.py / blue2.py / dna.py) ---------------------------------------------
    def rotate_cylinders(self, degrees: float) -> int:
        return _check_id(_lib.rt_scene_rotate_cylinders(self._h, degrees), "rotate_cylinders")

    def set_output_file(self, path: str):
        _check(_lib.rt_scene_set_output_file(self._h, os.fsencode(path)), "set_output_file")

    def clone(self) -> "Scene":
        return Scene(_lib.rt_scene_clone(self._h))

    @classmethod
    def dna(cls, angle_degrees: float, base: "Scene | None" = None) -> "Scene":
        """dna.py:17-98: the DNA animation frame at this angle over `base` (default: basic_scene.json)."""
        h = _lib.rt_scene_dna(base._h if base is not None else None, angle_degrees)
        if not h:
            raise RtmiError(_guess_status(), "rt_scene_dna")
        return cls(h)

    def override(self, width=0, height=0, spp=0, max_depth=0):
        _check(_lib.rt_scene_override(self._h, width, height, spp, max_depth), "override")

    # ---- read-back -----------------------------------------------------------
    @property
    def info(self) -> _Info:
        i = _Info()
        _check(_lib.rt_scene_get_info(self._h, C.byref(i)), "get_info")
        return i

    @property
    def width(self):
        return self.info.width

    @property
    def height(self):
        return self.info.height

    @property
    def spp(self):
        return self.info.samples_per_pixel

    @property
    def max_depth(self):
        return self.info.max_depth

    def get_camera(self) -> _Camera:
        c = _Camera()
        _check(_lib.rt_scene_get_camera(self._h, C.byref(c)), "get_camera")
        return c

    def _table(self, fn, dtype):
        n = _check_id(fn(self._h, None, 0), fn.__name__)
        arr = np.zeros(n, dtype=dtype)
        if n:
            fn(self._h, arr.ctypes.data_as(C.c_void_p), n)
        return arr

    def prims(self) -> np.ndarray:
        return self._table(_lib.rt_scene_get_prims, PRIM_DTYPE)

    def materials(self) -> np.ndarray:
        return self._table(_lib.rt_scene_get_materials, MATERIAL_DTYPE)

    def textures(self) -> np.ndarray:
        return self._table(_lib.rt_scene_get_textures, TEXTURE_DTYPE)

    def lights(self) -> np.ndarray:
        """The emitters light sampling samples (LIGHT_DTYPE records), whether or not it is switched on."""
        return self._table(_lib.rt_scene_get_lights, LIGHT_DTYPE)

    @property
    def output_file(self) -> str:
        return _lib.rt_scene_output_file(self._h).decode()

    def to_json(self) -> str:
        n = _lib.rt_scene_to_json(self._h, None, 0)
        buf = C.create_string_buffer(n)
        _lib.rt_scene_to_json(self._h, buf, n)
        return buf.value.decode()

    # ---- shard geometry ---------------------------------------------------------
    def shard_rows(self, opts: Opts | None = None) -> int:
        opts = opts or Opts()
        return _check_id(_lib.rt_shard_rows(self._h, C.byref(opts)), "rt_shard_rows")

    def shard_deal(self, opts: Opts | None, n_ranks: int) -> int:
        """rt_opts.tile_rotate that rt_render_hip_tiles uses to cut this frame into n_ranks shards (rt_shard_deal)."""
        opts = opts or Opts()
        return _check_id(_lib.rt_shard_deal(self._h, C.byref(opts), n_ranks), "rt_shard_deal")

    def shard_global_rows(self, opts: Opts | None = None) -> np.ndarray:
        opts = opts or Opts()
        n = self.shard_rows(opts)
        return np.array([_lib.rt_shard_global_row(self._h, C.byref(opts), r) for r in range(n)], dtype=np.int64)

    # ---- render (HIP only) --------------------------------------------------------
    def render(self, opts: Opts | None = None, stats: Stats | None = None) -> np.ndarray:
        """render<<<>>> + copy back (main.cu:505-513): (local_rows, W, 3) fp32 SUMS, row 0 = bottom."""
        opts = opts or Opts()
        rows = self.shard_rows(opts)
        out = np.empty((rows, self.width, 3), dtype=np.float32)
        st = stats if stats is not None else Stats()
        _check(_lib.rt_render_hip(self._h, C.byref(opts), out.ctypes.data_as(C.c_void_p), C.byref(st)), "rt_render_hip")
        return out

    def render_adaptive(self, threshold: float, min_spp: int = 16, max_spp: int = 0, opts: Opts | None = None):
        """Adaptive sampling (rt_render_hip_adaptive): every 8x8 tile doubles its samples from min_spp until its noise
        estimate is within `threshold` or it reaches max_spp (0: the scene's spp).  Returns (rgb_sum, spp_map, stats): the
        (H, W, 3) fp32 sums of each pixel's own spp_map[y, x] samples [0, n), the (H, W) int32 counts and AdaptiveStats."""
        opts = opts or Opts()
        a = Adaptive(min_spp=int(min_spp), max_spp=int(max_spp), threshold=float(threshold))
        out = np.empty((self.height, self.width, 3), dtype=np.float32)
        spp = np.empty((self.height, self.width), dtype=np.int32)
        st = AdaptiveStats()
        _check(_lib.rt_render_hip_adaptive(self._h, C.byref(opts), C.byref(a), out.ctypes.data_as(C.c_void_p),
                                           spp.ctypes.data_as(C.c_void_p), C.byref(st)), "rt_render_hip_adaptive")
        return out, spp, st

    def render_adaptive_device(self, threshold: float, d_rgb_sum: int, d_spp_map: int, min_spp: int = 16, max_spp: int = 0,
                               stream: int = 0, opts: Opts | None = None) -> AdaptiveStats:
        """The same into DEVICE buffers (rt_render_hip_adaptive_device): d_rgb_sum H x W x 3 float32, d_spp_map H x W int32
        (e.g. torch tensors' data_ptr()), on `stream` (a hipStream_t as an integer).  Returns when the frame is done: the
        schedule reads the active tile count back once per pass."""
        opts = opts or Opts()
        a = Adaptive(min_spp=int(min_spp), max_spp=int(max_spp), threshold=float(threshold))
        st = AdaptiveStats()
        _check(_lib.rt_render_hip_adaptive_device(self._h, C.byref(opts), C.byref(a), C.c_void_p(d_rgb_sum), C.c_void_p(d_spp_map),
                                                  C.c_void_p(stream), C.byref(st)), "rt_render_hip_adaptive_device")
        return st

    def render_feature(self, feature: int, opts: Opts | None = None, stats: Stats | None = None) -> np.ndarray:
        """One first-hit feature pass (rt_render_hip_feature): FEATURE_ALBEDO, FEATURE_NORMAL or FEATURE_DEPTH (t, coverage,
        0).  (local_rows, W, 3) fp32 SUMS over the samples of `opts` (sample_count 0: the scene's spp), rows as render()."""
        opts = opts or Opts()
        rows = self.shard_rows(opts)
        out = np.empty((rows, self.width, 3), dtype=np.float32)
        st = stats if stats is not None else Stats()
        _check(_lib.rt_render_hip_feature(self._h, C.byref(opts), int(feature), out.ctypes.data_as(C.c_void_p), C.byref(st)),
               "rt_render_hip_feature")
        return out

    def render_feature_device(self, feature: int, d_sum: int, stream: int = 0, opts: Opts | None = None, stats: Stats | None = None):
        """The same into a DEVICE buffer (rt_render_hip_feature_device): d_sum shard_rows(opts) x W x 3 float32, on `stream`
        (a hipStream_t as an integer).  Asynchronous when stats is None."""
        opts = opts or Opts()
        _check(_lib.rt_render_hip_feature_device(self._h, C.byref(opts), int(feature), C.c_void_p(d_sum), C.c_void_p(stream),
                                                 C.byref(stats) if stats is not None else None), "rt_render_hip_feature_device")

    # ---- ray queries (HIP only) ---------------------------------------------------
    def trace(self, origins, directions, t_max=float("inf"), occluded: bool = False, opts: Opts | None = None,
              stats: Stats | None = None) -> np.ndarray:
        """Closest hit (rt_trace_hip) of n caller-supplied rays against the scene's static primitives: exactly the renderer's
        closest-hit query over [0.001, t_max], directions not normalised, t in units of the direction.  origins, directions:
        (n, 3); t_max: a scalar or (n,).  Returns n HIT_DTYPE records (prim -1: a miss, HIT_INVALID: the ray failed ray_valid),
        or with occluded=True n bools: would the closest-hit query report a hit.  opts: device and variant (a layout) are read."""
        rays = pack_rays(origins, directions, t_max)
        n = len(rays)
        out = np.zeros(n, dtype=np.uint8) if occluded else np.zeros(n, dtype=HIT_DTYPE)
        opts = opts or Opts()
        _check(_lib.rt_trace_hip(self._h, C.byref(opts), TRACE_OCCLUDED if occluded else TRACE_CLOSEST, rays.ctypes.data_as(C.c_void_p),
                                 n, out.ctypes.data_as(C.c_void_p), C.byref(stats) if stats is not None else None), "rt_trace_hip")
        return out.astype(bool) if occluded else out

    def trace_device(self, d_rays: int, n: int, d_out: int, occluded: bool = False, stream: int = 0, opts: Opts | None = None,
                     stats: Stats | None = None):
        """The same on raw device pointers (rt_trace_hip_device): d_rays n x 32 bytes (RAY_DTYPE; a torch float32 tensor of shape
        (n, 8) passes data_ptr()), d_out n x 48 bytes (HIT_DTYPE; (n, 12) float32) or n bytes with occluded=True, stream e.g.
        torch.cuda.current_stream().cuda_stream.  Asynchronous when stats is None."""
        opts = opts or Opts()
        _check(_lib.rt_trace_hip_device(self._h, C.byref(opts), TRACE_OCCLUDED if occluded else TRACE_CLOSEST, C.c_void_p(d_rays), int(n),
                                        C.c_void_p(d_out), C.c_void_p(stream), C.byref(stats) if stats is not None else None),
               "rt_trace_hip_device")

    def render_tiles(self, devices=None, opts: Opts | None = None, stats: Stats | None = None, n: int | None = None,
                     out: np.ndarray | None = None):
        """One frame over several GPUs of this node: row tiles dealt out to `devices` (ordinals; None =
        0..n-1), one ncclGather to devices[0] (rt_render_hip_tiles).  Returns the (H, W, 3) fp32 sums (in `out` when given:
        a C-contiguous float32 array of that shape)."""
        opts = opts or Opts()
        if devices is None:
            count = int(n if n is not None else 1)
            arr = None
        else:
            count = len(devices)
            arr = (C.c_int * count)(*[int(d) for d in devices])
        if out is None:
            out = np.empty((self.height, self.width, 3), dtype=np.float32)
        elif out.shape != (self.height, self.width, 3) or out.dtype != np.float32 or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("render_tiles: out must be a C-contiguous float32 array of shape (height, width, 3)")
        _check(_lib.rt_render_hip_tiles(self._h, C.byref(opts), arr, count, out.ctypes.data_as(C.c_void_p),
                                        C.byref(stats) if stats is not None else None), "rt_render_hip_tiles")
        return out

    def place_rows_device(self, opts: Opts, n_ranks: int, pad_rows: int, gathered_ptr: int, full_ptr: int, stream: int = 0):
        """Gathered [n_ranks][pad_rows][W][3] device buffer -> full [H][W][3] device buffer (one kernel)."""
        _check(_lib.rt_shard_place_rows_device(self._h, C.byref(opts), n_ranks, pad_rows, C.c_void_p(gathered_ptr),
                                               C.c_void_p(full_ptr), C.c_void_p(stream)), "rt_shard_place_rows_device")

    def render_device(self, opts: Opts, device_ptr: int, stream: int = 0, stats: Stats | None = None):
        """Render into a device buffer (e.g. a torch tensor's data_ptr()) on a HIP stream."""
        _check(_lib.rt_render_hip_device(self._h, C.byref(opts), C.c_void_p(device_ptr), C.c_void_p(stream),
                                         C.byref(stats) if stats is not None else None), "rt_render_hip_device")

    def table_info(self) -> TableInfo:
        """The device tables the host builds for this scene (no GPU needed)."""
        t = TableInfo()
        _check(_lib.rt_scene_table_info(self._h, C.byref(t)), "rt_scene_table_info")
        return t

    def quad_counts(self):
        """(nq, nq_a): the quads of this scene's tables, and how many of them (the leading ones) are tested for every query
        instead of being listed (rt_scene_quad_counts; TableInfo does not count quads; no GPU needed)."""
        nq, nq_a = C.c_int32(), C.c_int32()
        _check(_lib.rt_scene_quad_counts(self._h, C.byref(nq), C.byref(nq_a)), "rt_scene_quad_counts")
        return int(nq.value), int(nq_a.value)

    def table_image(self) -> np.ndarray:
        """The packed device image as float32 records [n][4] (view it as uint32 / uint16 for the index tables)."""
        n = _lib.rt_scene_table_image(self._h, None, 0)
        if n < 0:
            raise RtmiError(-n, "rt_scene_table_image")
        out = np.empty(n, dtype=np.float32)
        _lib.rt_scene_table_image(self._h, out.ctypes.data_as(C.c_void_p), n)
        return out.reshape(-1, 4)

    def tile_beams(self, opts: Opts | None = None, device=False) -> np.ndarray:
        """The beam table of the frame as uint16 records [tiles_y][tiles_x][16]: {count, ids ...} per 8x8 tile of the whole frame,
        the staged spheres a camera ray of the tile can be flagged for; count 0xffff: the overflow mark.  As the host computes
        it (rt_scene_tile_beams; no GPU needed), or with device=True as the device builds it (rt_scene_tile_beams_device)."""
        name = "rt_scene_tile_beams_device" if device else "rt_scene_tile_beams"
        call = (lambda p, n: _lib.rt_scene_tile_beams_device(self._h, C.byref(opts) if opts is not None else None, p, n)) if device else \
               (lambda p, n: _lib.rt_scene_tile_beams(self._h, p, n))
        n = call(None, 0)
        if n < 0:
            raise RtmiError(-n, name)
        out = np.empty((n, 16), dtype=np.uint16)
        n = call(out.ctypes.data_as(C.c_void_p), n)
        if n < 0:
            raise RtmiError(-n, name)
        info = self.info
        return out.reshape((int(info.height) + 7) // 8, (int(info.width) + 7) // 8, 16)

    def tile_beam_list(self, tx: int, ty: int):
        """(ids, overflow) of tile (tx, ty) of the frame's 8x8 tile grid, as the host computes them (no GPU needed)."""
        rec = self.tile_beams()[ty, tx]
        if rec[0] == 0xffff:
            return [], True
        return [int(i) for i in rec[1:1 + int(rec[0])]], False

    def count(self, opts: Opts | None = None, want_image=False):
        """Diagnostic launch with exact event counters (roofline flops accounting)."""
        opts = opts or Opts()
        st = Stats()
        out = None
        ptr = None
        if want_image:
            out = np.empty((self.shard_rows(opts), self.width, 3), dtype=np.float32)
            ptr = out.ctypes.data_as(C.c_void_p)
        _check(_lib.rt_render_hip_count(self._h, C.byref(opts), ptr, C.byref(st)), "rt_render_hip_count")
        return (st, out) if want_image else st

    def accumulate(self, acc: np.ndarray | None = None, opts: Opts | None = None, stats: Stats | None = None,
                   want_image=True):
        """Progressive rendering: add the samples [opts.sample_first, +sample_count) to the exact pixel sums
        `acc` (int64 [local_rows, width, 3], 2^-24 units; None = start from zero).  Returns (acc, image)."""
        opts = opts or Opts()
        rows = self.shard_rows(opts)
        if acc is None:
            acc = np.zeros((rows, self.width, 3), dtype=np.int64)
        if acc.dtype != np.int64 or acc.shape != (rows, self.width, 3) or not acc.flags.c_contiguous:
            raise ValueError(f"acc must be a C-contiguous int64 array of shape {(rows, self.width, 3)}")
        out = np.empty((rows, self.width, 3), dtype=np.float32) if want_image else None
        _check(_lib.rt_render_hip_accumulate(self._h, C.byref(opts), acc.ctypes.data_as(C.c_void_p),
                                             out.ctypes.data_as(C.c_void_p) if want_image else None,
                                             C.byref(stats) if stats is not None else None),
               "rt_render_hip_accumulate")
        return acc, out

    def scatter_rows(self, opts: Opts, local: np.ndarray, full: np.ndarray):
        local = np.ascontiguousarray(local, dtype=np.float32)
        assert full.dtype == np.float32 and full.flags.c_contiguous
        _check(_lib.rt_shard_scatter_rows(self._h, C.byref(opts), local.ctypes.data_as(C.c_void_p),
                                          full.ctypes.data_as(C.c_void_p)), "rt_shard_scatter_rows")


def acc_to_rgb(acc: np.ndarray) -> np.ndarray:
    """fp32 framebuffer values of exact int64 pixel sums (2^-24 units)."""
    acc = np.ascontiguousarray(acc, dtype=np.int64)
    out = np.empty(acc.shape, dtype=np.float32)
    _lib.rt_acc_to_rgb(acc.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), acc.size)
    return out


def denoise(rgb_sum, spp, albedo_sum, normal_sum, depth_sum, feature_spp, *, spp_map=None, iterations=None, sigma_color=0.0,
            sigma_normal=0.0, sigma_depth=0.0, device=0, timing=None):
    """Edge-avoiding a-trous filter (rt_denoise_hip) of an (H, W, 3) frame of SUMS over `spp` samples per pixel -- or over
    spp_map[y, x] samples (an (H, W) int32 array, as render_adaptive returns) -- guided by the three feature passes of
    Scene.render_feature over feature_spp samples.  iterations None: the default; 0: the input bits.  A sigma of 0: its
    default.  Returns the filtered sums, which the writers take unchanged.  timing: a list that receives the kernels' ms."""
    rgb = np.ascontiguousarray(rgb_sum, dtype=np.float32)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("denoise: rgb_sum must have shape (height, width, 3)")
    planes = [np.ascontiguousarray(a, dtype=np.float32) for a in (albedo_sum, normal_sum, depth_sum)]
    for a in planes:
        if a.shape != rgb.shape:
            raise ValueError("denoise: the feature sums must have the frame's shape")
    h, w = rgb.shape[:2]
    m = None
    if spp_map is not None:
        m = np.ascontiguousarray(spp_map, dtype=np.int32)
        if m.shape != (h, w):
            raise ValueError("denoise: spp_map must have shape (height, width)")
    p = Denoise(iterations=DENOISE_DEFAULT_ITERATIONS if iterations is None else int(iterations), sigma_color=float(sigma_color),
                sigma_normal=float(sigma_normal), sigma_depth=float(sigma_depth))
    out = np.empty_like(rgb)
    ms = C.c_double(0.0)
    _check(_lib.rt_denoise_hip(w, h, rgb.ctypes.data_as(C.c_void_p), int(spp), m.ctypes.data_as(C.c_void_p) if m is not None else None,
                               planes[0].ctypes.data_as(C.c_void_p), planes[1].ctypes.data_as(C.c_void_p),
                               planes[2].ctypes.data_as(C.c_void_p), int(feature_spp), C.byref(p), int(device),
                               out.ctypes.data_as(C.c_void_p), C.byref(ms)), "rt_denoise_hip")
    if timing is not None:
        timing.append(ms.value)
    return out


def denoise_device(width, height, d_rgb_sum, spp, d_albedo_sum, d_normal_sum, d_depth_sum, feature_spp, d_out_rgb_sum, stream=0, *,
                   d_spp_map=None, params=None, device=0, timing=None):
    """rt_denoise_hip_device: the filter on DEVICE buffers (addresses as integers; H x W x 3 float32 each, d_spp_map H x W int32
    or None), enqueued on `stream` (a hipStream_t as an integer); params: a Denoise or None (all defaults).  timing: a list that
    receives the kernels' ms -- the call then waits for them; None: asynchronous."""
    ms = C.c_double(0.0) if timing is not None else None
    _check(_lib.rt_denoise_hip_device(int(width), int(height), d_rgb_sum, int(spp), d_spp_map, d_albedo_sum, d_normal_sum, d_depth_sum,
                                      int(feature_spp), C.byref(params) if params is not None else None, int(device), d_out_rgb_sum,
                                      stream or None, C.byref(ms) if ms is not None else None), "rt_denoise_hip_device")
    if timing is not None:
        timing.append(ms.value)


def display(rgb_sum, spp, *, spp_map=None, tonemap=None, exposure=0.0, auto_key=0.0, white=0.0, bloom_strength=0.0,
            bloom_threshold=0.0, bloom_levels=0, device=0, want_rgb=True, want_rgb8=True, stats=None):
    """The display stage (rt_display_hip) on an (H, W, 3) frame of SUMS over `spp` samples per pixel -- or over
    spp_map[y, x] samples.  tonemap: None (a NULL rt_display when every other parameter is at its default too), a name of
    TONEMAPS or its number.  Returns (out_rgb, out_rgb8): display-referred linear colour, (H, W, 3) float32 with row 0 at the
    bottom (the writers take it with spp = 1), and its quantised bytes, (H, W, 3) uint8 with row 0 at the TOP; None for an
    output that was not wanted.  stats: a DisplayStats to fill."""
    rgb = np.ascontiguousarray(rgb_sum, dtype=np.float32)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("display: rgb_sum must have shape (height, width, 3)")
    h, w = rgb.shape[:2]
    m = None
    if spp_map is not None:
        m = np.ascontiguousarray(spp_map, dtype=np.int32)
        if m.shape != (h, w):
            raise ValueError("display: spp_map must have shape (height, width)")
    p = None
    if tonemap is not None or any((exposure, auto_key, white, bloom_strength, bloom_threshold, bloom_levels)):
        t = TONEMAPS[tonemap] if isinstance(tonemap, str) else int(tonemap or 0)
        p = Display(tonemap=t, exposure=float(exposure), auto_key=float(auto_key), white=float(white),
                    bloom_strength=float(bloom_strength), bloom_threshold=float(bloom_threshold), bloom_levels=int(bloom_levels))
    out = np.empty_like(rgb) if want_rgb else None
    out8 = np.empty((h, w, 3), dtype=np.uint8) if want_rgb8 else None
    _check(_lib.rt_display_hip(w, h, rgb.ctypes.data_as(C.c_void_p), int(spp), m.ctypes.data_as(C.c_void_p) if m is not None else None,
                               C.byref(p) if p is not None else None, int(device),
                               out.ctypes.data_as(C.c_void_p) if want_rgb else None,
                               out8.ctypes.data_as(C.c_void_p) if want_rgb8 else None,
                               C.byref(stats) if stats is not None else None), "rt_display_hip")
    return out, out8


def display_device(width, height, d_rgb_sum, spp, d_out_rgb, d_out_rgb8, stream=0, *, d_spp_map=None, params=None, device=0,
                   stats=None):
    """rt_display_hip_device: the display stage on DEVICE buffers (addresses as integers; an output may be None), enqueued on
    `stream` (a hipStream_t as an integer); params: a Display or None (all defaults)."""
    _check(_lib.rt_display_hip_device(int(width), int(height), d_rgb_sum, int(spp), d_spp_map,
                                      C.byref(params) if params is not None else None, int(device), d_out_rgb, d_out_rgb8,
                                      stream or None, C.byref(stats) if stats is not None else None), "rt_display_hip_device")


def display_timing():
    """hipEvent ms of the single kernels of this thread's last display call that had stats, in launch order (rt_display_timing)."""
    buf = (C.c_double * 32)()
    n = _lib.rt_display_timing(buf, 32)
    return list(buf[:n])


def write_hdr(image: np.ndarray, samples_per_pixel: int, filename: str):
    """The mean image as a Radiance RGBE file (rt_write_hdr); rt_scene_set_environment_file reads it back."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    _check(_lib.rt_write_hdr(os.fsencode(filename), img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0], samples_per_pixel),
           "rt_write_hdr")


def write_pfm(image: np.ndarray, samples_per_pixel: int, filename: str):
    """The mean image as a little-endian colour PFM file (rt_write_pfm)."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    _check(_lib.rt_write_pfm(os.fsencode(filename), img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0], samples_per_pixel),
           "rt_write_pfm")


def _guess_status() -> int:
    msg = _lib.rt_last_error().decode(errors="replace")
    if msg.startswith("JSON error"):
        return 3
    if msg.startswith("cannot open"):
        return 2
    return 4


def parse_scene(filename: str) -> Scene:
    """gpu-version/parser.hpp:504 ``parse_scene(filename)``."""
    return Scene.load(filename)


def output_image(image: np.ndarray, samples_per_pixel: int, filename: str = "main.ppm"):
    """gpu-version/main.cu:359-372 ``output_image``: P3 PPM, gamma 2, rows top to bottom."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    h, w = img.shape[0], img.shape[1]
    _check(_lib.rt_write_ppm(os.fsencode(filename), img.ctypes.data_as(C.c_void_p), w, h, samples_per_pixel),
           "rt_write_ppm")


def write_image(image: np.ndarray, samples_per_pixel: int, filename: str = "main.png", gamma: bool = False):
    """gpu-version/color.cuh:15-35 ``write_image``: 8-bit RGB PNG of the linear means."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    h, w = img.shape[0], img.shape[1]
    _check(_lib.rt_write_png(os.fsencode(filename), img.ctypes.data_as(C.c_void_p), w, h, samples_per_pixel, int(gamma)),
           "rt_write_png")


def quantize_rgb8(image: np.ndarray, samples_per_pixel: int, gamma: bool = True) -> np.ndarray:
    img = np.ascontiguousarray(image, dtype=np.float32)
    h, w = img.shape[0], img.shape[1]
    out = np.empty((h, w, 3), dtype=np.uint8)
    _check(_lib.rt_quantize_rgb8(img.ctypes.data_as(C.c_void_p), w, h, samples_per_pixel, int(gamma),
                                 out.ctypes.data_as(C.c_void_p)), "rt_quantize_rgb8")
    return out


def philox4x32_10(ctr, key):
    c = (C.c_uint32 * 4)(*ctr)
    k = (C.c_uint32 * 2)(*key)
    o = (C.c_uint32 * 4)()
    _lib.rt_philox4x32_10(c, k, o)
    return list(o)


def sample_stream(seed, pixel, sample, n):
    out = (C.c_uint32 * n)()
    _lib.rt_sample_stream(seed, pixel, sample, out, n)
    return list(out)


def medium_interval(medium, orig, direction, t_max=float("inf")):
    """Host evaluation of the device's interval formula: the stay of the ray orig + t direction inside the boundary of
    ``medium`` (a MEDIUM_DTYPE record) clipped to [0.001, t_max] -> (non-empty, t_in, t_out)."""
    rec = np.zeros(1, MEDIUM_DTYPE)
    rec[0] = medium
    a, b = C.c_float(), C.c_float()
    rc = _check_id(_lib.rt_medium_interval(rec.ctypes.data_as(C.c_void_p), _v3(orig), _v3(direction), float(t_max), C.byref(a), C.byref(b)),
                   "medium_interval")
    return bool(rc), a.value, b.value


def phase_hg_sample(g, direction, u1, u2):
    """Host evaluation of the device's phase-function sample: the direction a vertex of a medium with asymmetry ``g`` (not 0)
    leaves in, from the direction of travel (any length) and its two draws -> (x, y, z)."""
    out = (C.c_float * 3)()
    _check(_lib.rt_phase_hg_sample(float(g), _v3(direction), float(u1), float(u2), out), "phase_hg_sample")
    return out[0], out[1], out[2]


def phase_hg_eval(g, cos_theta):
    """The Henyey-Greenstein density per steradian as the device text evaluates it."""
    return _lib.rt_phase_hg_eval(float(g), float(cos_theta))


def moving_sphere_hit(mover, s, orig, direction, t_max=float("inf")):
    """Host evaluation of the device's intersection: ``mover`` (a MOVING_SPHERE_DTYPE record) at shutter time ``s`` against
    the ray orig + t direction over [0.001, t_max] -> (hit, t)."""
    rec = np.zeros(1, MOVING_SPHERE_DTYPE)
    rec[0] = mover
    t = C.c_float()
    rc = _check_id(_lib.rt_moving_sphere_hit(rec.ctypes.data_as(C.c_void_p), float(s), _v3(orig), _v3(direction), float(t_max), C.byref(t)),
                   "moving_sphere_hit")
    return bool(rc), t.value


def pack_rays(origins, directions, t_max=float("inf")) -> np.ndarray:
    """(n, 3) origins and directions and a scalar or (n,) t_max as n RAY_DTYPE records"""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    if len(o) != len(d):
        raise ValueError("trace: %d origins for %d directions" % (len(o), len(d)))
    rays = np.zeros(len(o), dtype=RAY_DTYPE)
    rays["origin"], rays["dir"] = o, d
    rays["t_max"] = np.broadcast_to(np.asarray(t_max, dtype=np.float32), (len(o),))
    return rays


def ray_valid(ray) -> bool:
    """May this ray enter the walk (rt_ray_valid, the host evaluation of the kernel's guard)?  ray: one RAY_DTYPE record, or
    (origin, direction) or (origin, direction, t_max)."""
    if not (isinstance(ray, (np.ndarray, np.void)) and ray.dtype == RAY_DTYPE):
        ray = pack_rays([ray[0]], [ray[1]], ray[2] if len(ray) > 2 else float("inf"))
    rec = np.ascontiguousarray(np.asarray(ray, dtype=RAY_DTYPE).reshape(-1)[:1])
    return bool(_lib.rt_ray_valid(rec.ctypes.data_as(C.c_void_p)))


def shutter_time(seed, pixel, sample) -> float:
    """The shutter time in [0, 1) of sample ``sample`` of pixel ``pixel`` (y * width + x): the top 24 bits of word 0 of
    Philox4x32-10(counter = (pixel, sample, 1, 0), key = seed) x 2^-24 -- not a draw of the sample's stream."""
    return float(_lib.rt_shutter_time(int(seed), int(pixel), int(sample)))


def aabb_hit(bmin, bmax, orig, direction, t_min, t_max) -> bool:
    return bool(_lib.rt_aabb_hit(_v3(bmin), _v3(bmax), _v3(orig), _v3(direction), t_min, t_max))


def device_count() -> int:
    return _check_id(_lib.rt_device_count(), "rt_device_count")


def struct_size(which: int) -> int:
    return int(_lib.rt_struct_size(which))


def abi_version() -> int:
    return _lib.rt_abi_version()


def has_ablations() -> bool:
    """Does the loaded library carry the measurement variants and the counting kernels (the default build)?"""
    return bool(_lib.rt_has_ablations())


LIB_PATH = _LIB_PATH


def variant_workgroup(variant: int) -> dict:
    """The workgroup render variant `variant` launches, as the host sizes it (rt_variant_workgroup; no device needed)."""
    out = (C.c_int32 * 5)()
    _check(_lib.rt_variant_workgroup(int(variant), out), "rt_variant_workgroup")
    return dict(zip(("threads", "wave_lds", "max_table_bytes", "max_lds_bytes", "groups_per_cu"), (int(x) for x in out)))
