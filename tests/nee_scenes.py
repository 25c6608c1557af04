"""Scenes and closed forms shared by the light-sampling and environment tests (GPU and CPU): the analytic floor under a
rectangle, the material x light pair scenes, the 200-emitter scene, the floor under a small bright patch of an environment."""
import os

import numpy as np

# ---- the analytic scene: a lambertian floor under a parallel emissive rectangle ---------------------------------------
RHO, LE, H = 0.5, 4.0, 2.0
LX, LZ = (-1.0, 1.0), (-1.0, 1.0)


def analytic_scene(rtmi, w=64, h=36, spp=256):
    sc = rtmi.Scene.new(w, h, spp, 2)  # camera -> floor -> light: the direct term alone
    sc.set_background((0, 0, 0), sky_gradient=False, defocus_blur=False)
    sc.camera((2.5, 1.2, -1.5), (2.5, 0.0, 0.0), (0, 1, 0), 50.0)
    sc.xz_rect(-50, 50, -50, 50, 0.0, sc.lambertian((RHO, RHO, RHO)))
    sc.xz_rect(LX[0], LX[1], LZ[0], LZ[1], H, sc.diffuse_light((LE, LE, LE)))
    return sc


def _ff_corner(a, b, h):
    """form factor from a point to a parallel rectangle [0, a] x [0, b] at height h above it (signed for a, b < 0)"""
    A, B = np.abs(a) / h, np.abs(b) / h
    f = (A / np.sqrt(1 + A * A) * np.arctan(B / np.sqrt(1 + A * A)) + B / np.sqrt(1 + B * B) * np.arctan(A / np.sqrt(1 + B * B)))
    return np.sign(a) * np.sign(b) * f / (2 * np.pi)


def analytic_expected(sc, q=6):
    """rho L F(P) averaged over each pixel's footprint (q x q jitter quadrature); NaN where a ray misses the floor"""
    cam = sc.get_camera()
    org, ll = np.array(cam.origin, np.float64), np.array(cam.lower_left, np.float64)
    hor, ver = np.array(cam.horizontal, np.float64), np.array(cam.vertical, np.float64)
    W, Hh = sc.width, sc.height
    xi = (np.arange(q) + 0.5) / q
    u = (np.arange(W)[None, :, None, None] + xi[None, None, :, None]) / (W - 1)
    v = (np.arange(Hh)[:, None, None, None] + xi[None, None, None, :]) / (Hh - 1)
    d = ll + u[..., None] * hor + v[..., None] * ver - org
    t = -org[1] / d[..., 1]
    px, pz = org[0] + t * d[..., 0], org[2] + t * d[..., 2]
    F = (_ff_corner(LX[1] - px, LZ[1] - pz, H) - _ff_corner(LX[0] - px, LZ[1] - pz, H)
         - _ff_corner(LX[1] - px, LZ[0] - pz, H) + _ff_corner(LX[0] - px, LZ[0] - pz, H))
    val = RHO * LE * F
    val[~(t > 0)] = np.nan
    return val.mean(axis=(2, 3))


def pair_scene(rtmi, mat, light, w=64, h=36, spp=256, depth=6, lift=0.0):
    """`lift` raises the whole scene, camera included: a checker's parity is undefined on the plane y = 0, where the floor lies"""
    Y = lift
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.02, 0.02, 0.03), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5 + Y, 6.0), (0.0, 0.5 + Y, 0.0), (0, 1, 0), 45.0)
    if mat == "lambert":
        m = sc.lambertian((0.6, 0.5, 0.4))
    elif mat == "checker":
        m = sc.lambertian(sc.checker_texture((0.8, 0.8, 0.8), (0.1, 0.3, 0.1)))
    else:
        m = sc.metal((0.8, 0.7, 0.6), float(mat[5:]))
    sc.xz_rect(-20, 20, -20, 20, 0.0 + Y, m)
    sc.sphere((-1.2, 0.6 + Y, 0.5), 0.6, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((1.3, 0.5 + Y, 0.8), 0.5, m)
    e = sc.diffuse_light((6.0, 5.0, 4.0))
    if light == "xy":
        sc.xy_rect(-0.5, 0.5, 1.0 + Y, 2.0 + Y, -1.5, e)
    elif light == "xz":
        sc.xz_rect(-0.6, 0.6, -0.6, 0.6, 2.5 + Y, e)
    elif light == "yz":
        sc.yz_rect(0.5 + Y, 1.5 + Y, -0.5, 0.5, 2.5, e)
    elif light == "sphere":
        sc.sphere((0.3, 2.2 + Y, -0.5), 0.3, e)
    else:
        sc.cylinder(0.15, -0.8, 0.8, e, rotate=((1.0, 0.3, 0.2), 70.0), translate=(0.2, 1.8 + Y, -0.6))
    return sc


def many_lights(rtmi, w=64, h=36, spp=32, floor_y=0.0):
    rng = np.random.default_rng(3)
    sc = rtmi.Scene.new(w, h, spp, 8)
    sc.set_background((0.0, 0.0, 0.0), sky_gradient=False, defocus_blur=False)
    sc.camera((0, 6, 14), (0, 0, 0), (0, 1, 0), 45.0)
    sc.xz_rect(-30, 30, -30, 30, floor_y, sc.lambertian(sc.checker_texture((0.7, 0.7, 0.7), (0.2, 0.2, 0.2))))
    for i in range(200):
        c = (float(rng.uniform(-8, 8)), float(rng.uniform(0.2, 3)), float(rng.uniform(-8, 4)))
        if i % 3 == 0:
            sc.sphere(c, 0.15, sc.diffuse_light(tuple(float(x) for x in rng.uniform(1, 6, 3))))
        elif i % 3 == 1:
            sc.sphere(c, 0.2, sc.lambertian(tuple(float(x) for x in rng.uniform(0.2, 0.9, 3))))
        else:
            sc.xy_rect(c[0], c[0] + 0.3, c[1], c[1] + 0.3, c[2], sc.diffuse_light((3.0, 2.0, 1.0)))
    sc.set_light_sampling(True)
    return sc


# ---- a lambertian floor under a small bright patch of an environment map -----------------------------------------------------
PATCH_ROWS, PATCH_COLS, PATCH_RHO, PATCH_L = 32, 64, 0.5, 50.0


def patch_map():
    env = np.zeros((PATCH_ROWS, PATCH_COLS, 3), np.float32)
    env[4:6, 10:13] = PATCH_L
    return env


def patch_expected(q=64):
    """rho / pi x sum L cos(theta) dOmega by sub-texel quadrature (the floor's normal is +y: cos(theta) = d.y)"""
    rows, cols = PATCH_ROWS, PATCH_COLS
    expected = 0.0
    for i in (4, 5):
        th = np.pi * (i + (np.arange(q) + 0.5) / q) / rows
        expected += 3 * (2 * np.pi / cols) * np.sum(PATCH_L * np.cos(th) * np.sin(th)) * (np.pi / rows / q)
    return expected * PATCH_RHO / np.pi


def patch_scene(rtmi, w=64, h=36, spp=256):
    sc = rtmi.Scene.new(w, h, spp, 2)  # camera -> floor -> environment: the direct term alone
    sc.set_background((0, 0, 0), sky_gradient=False, defocus_blur=False)
    sc.camera((2.5, 1.2, -1.5), (2.5, 0.0, 0.0), (0, 1, 0), 50.0)
    sc.xz_rect(-50, 50, -50, 50, 0.0, sc.lambertian((PATCH_RHO, PATCH_RHO, PATCH_RHO)))
    sc.set_environment(patch_map(), 1.0, 40.0)
    return sc


# ---- the cases of the per-sample comparison with the fp64 reference (test_nee_reference.py, test_gpu_nee_reference.py) -------------
# 48 x 27 pixels x 13 one-sample frames = 16 848 samples per scene, from one fixed seed
REF_W, REF_H, REF_K, REF_SEED = 48, 27, 13, 77
REF_DRAWS = 384  # uniforms requested per sample (a depth-8 path with light samples uses ~60 on average)
LIFT = 0.05      # checker floors are raised off y = 0, where floor(10 y / pi) flips with the last bit of the hit point

PAIR_MATERIALS = ["lambert", "checker", "metal0.05", "metal0.3", "metal1.0"]
PAIR_LIGHTS = ["xy", "xz", "yz", "sphere", "cylinder"]
SCENE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ray-tracing-in-cuda_amd", "scenes")


def _pair(mat, light, **kw):
    return lambda rtmi: pair_scene(rtmi, mat, light, w=REF_W, h=REF_H, spp=1, lift=LIFT if mat == "checker" else 0.0, **kw)


def _glass(rtmi):
    """a dielectric sphere between floor and light: a vertex that takes no light sample, and emitter hits at full weight"""
    sc = rtmi.Scene.new(REF_W, REF_H, 1, 6)
    sc.set_background((0.02, 0.02, 0.03), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.5, 0.4)))
    sc.sphere((-1.2, 0.6, 0.5), 0.6, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((1.3, 0.5, 0.8), 0.5, sc.lambertian((0.6, 0.5, 0.4)))
    sc.xz_rect(-1.5, 1.5, -1.5, 1.5, 2.5, sc.diffuse_light((3.0, 2.5, 2.0)))
    sc.sphere((0.0, 1.4, 0.0), 0.9, sc.dielectric(1.5))  # (large, and close under a wide light: enough of its rays end on it)
    return sc


def _inside(rtmi):
    """Camera, floor and objects inside a large dim emissive sphere, a bright rectangle with them.  Every vertex has c^2 <= r^2 for
    the sphere light: it takes no sample of it when the alias draw picks it (the sphere's area x luminance gives it about two
    picks in three), and a BSDF ray that ends on the sphere keeps full weight.  (Paths end on an emitter, so a vertex inside a
    sphere light only exists where the camera is inside it too.)"""
    sc = rtmi.Scene.new(REF_W, REF_H, 1, 6)
    sc.set_background((0.02, 0.02, 0.03), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.5, 0.4)))
    sc.sphere((-1.2, 0.6, 0.5), 0.6, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((1.3, 0.5, 0.8), 0.5, sc.metal((0.8, 0.7, 0.6), 0.3))
    sc.xz_rect(-0.6, 0.6, -0.6, 0.6, 2.5, sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.sphere((0.0, 1.5, 2.5), 5.0, sc.diffuse_light((0.04, 0.05, 0.07)))
    return sc


def _checker_emitter(rtmi):
    sc = rtmi.Scene.new(REF_W, REF_H, 1, 6)
    sc.set_background((0.02, 0.02, 0.03), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.5, 0.4)))
    sc.sphere((-1.2, 0.6, 0.5), 0.6, sc.metal((0.8, 0.7, 0.6), 0.3))
    sc.xz_rect(-0.9, 0.9, -0.9, 0.9, 2.5, sc.diffuse_light(sc.checker_texture((6.0, 1.0, 0.5), (0.5, 2.0, 6.0))))
    sc.cylinder(0.2, -0.7, 0.7, sc.diffuse_light(sc.checker_texture((3.0, 1.0, 0.5), (0.5, 1.0, 3.0))),
                rotate=((1.0, 0.3, 0.0), 70.0), translate=(1.5, 1.2, 0.3))
    return sc


def _many(rtmi):
    return many_lights(rtmi, w=REF_W, h=REF_H, spp=1, floor_y=LIFT)


def _roulette(rtmi):
    sc = pair_scene(rtmi, "metal1.0", "xz", w=REF_W, h=REF_H, spp=1)
    sc.set_russian_roulette(0.9)
    return sc


def nee_cases():
    """name -> builder of the light-sampling cases (light sampling is switched on by the caller)"""
    cases = {f"{m} x {l}": _pair(m, l) for m in PAIR_MATERIALS for l in PAIR_LIGHTS}
    cases.update({"glass under the light": _glass, "inside the light sphere": _inside, "checker emitters": _checker_emitter,
                  "many lights": _many, "roulette 0.9": _roulette})
    for depth in (1, 2, 3):
        cases[f"max_depth {depth}"] = _pair("lambert", "sphere", depth=depth)
    return cases


# The special vertices a case is there for, by the names of ref64.tally(): the reference must have met each at least
# REQUIRED_EVENTS times among the scene's 16 848 samples, or the case does not test what its name says.  1 % of the samples: an
# estimator wrong by a factor of order one on that many vertices moves the paired mean by 1e-2 of a contribution, four
# orders above the 1e-6 the bias assertion resolves where no branch flips.
REQUIRED_EVENTS = 169
SPECIAL_VERTICES = {
    "inside the light sphere": ("inside_no_sample", "inside_full_weight_hits"),
    "glass under the light": ("dielectric_vertices", "dielectric_full_weight_hits"),
    "many lights": ("alias_picks", "bucket_picks"),
    "roulette 0.9": ("absorbed_metal_light_samples",),
    **{f"metal1.0 x {l}": ("absorbed_metal_light_samples",) for l in PAIR_LIGHTS},
}


def check_special_vertices(name, tally):
    """the case `name` met the vertices it is named for (no case ever samples a light at a dielectric vertex)"""
    assert tally["dielectric_light_samples"] == 0, (name, tally)
    for what in SPECIAL_VERTICES.get(name, ()):
        assert tally[what] >= REQUIRED_EVENTS, (name, what, tally)


def env_geometry(rtmi, emitter=False, depth=6):
    """the objects under the environment maps: every material and primitive type in scope, no checker on y = 0"""
    sc = rtmi.Scene.new(REF_W, REF_H, 1, depth)
    sc.set_background((0.1, 0.2, 0.3), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    sc.xz_rect(-20, 20, -20, 20, LIFT, sc.lambertian(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.4, 0.2))))
    sc.sphere((-1.2, 0.65, 0.5), 0.6, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((1.3, 0.55, 0.8), 0.5, sc.metal((0.8, 0.7, 0.6), 0.3))
    sc.sphere((0.1, 0.5, 1.6), 0.45, sc.dielectric(1.5))
    sc.cylinder(0.2, -0.6, 0.6, sc.metal((0.9, 0.9, 0.9), 0.0), rotate=((1.0, 0.0, 0.0), 90.0), translate=(2.4, 0.65, -0.5))
    if emitter:
        sc.xz_rect(-0.6, 0.6, -0.6, 0.6, 2.5, sc.diffuse_light((6.0, 5.0, 4.0)))
    return sc


def _random_map(rows, cols, seed, zeros=True, sun=None):
    rng = np.random.default_rng(seed)
    env = (rng.random((rows, cols, 3)) * 2 + 0.01).astype(np.float32)
    if zeros:
        env[rows // 3, :] = 0
        env[rows // 2, cols // 4] = 0
        env[rows - 1, cols - 1] = 0
    if sun is not None:
        env[rows // 5, cols // 3] = sun
    return env


def _sun_map():
    import json
    e = json.load(open(os.path.join(SCENE_DIR, "env_sun.json")))["environment"]
    return np.array(e["data"], np.float32).reshape(e["rows"], e["cols"], 3), float(e["scale"]), float(e["rotate"])


def env_cases():
    """name -> (environment texels, scale, rotate, emitter?, roulette) over env_geometry; each runs plain and with light sampling"""
    sun, s_scale, s_rot = _sun_map()
    return {
        "env_sun 8x16": (sun, s_scale, s_rot, False, 0.0),
        "random 7x13, 33.3 deg, x2.5": (_random_map(7, 13, 5), 2.5, 33.3, False, 0.0),
        "1x1": (np.full((1, 1, 3), (0.625, 0.75, 0.875), np.float32), 1.0, 0.0, False, 0.0),
        "64x128": (_random_map(64, 128, 6, sun=(300.0, 280.0, 240.0)), 1.0, 12.0, False, 0.0),
        "37x101": (_random_map(37, 101, 7, sun=(150.0, 150.0, 120.0)), 0.75, 201.5, False, 0.0),
        "area light + 8x16": (sun, s_scale, 25.0, True, 0.0),
        "roulette 0.85": (_random_map(7, 13, 8), 1.0, 0.0, False, 0.85),
    }


def env_scene_of(rtmi, case, with_env=True):
    env, scale, rotate, emitter, rr = case
    sc = env_geometry(rtmi, emitter)
    if rr > 0:
        sc.set_russian_roulette(rr)
    if with_env:
        sc.set_environment(env, scale, rotate)
    return sc
