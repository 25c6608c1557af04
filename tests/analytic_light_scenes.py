"""Scenes of the analytic lights (point, spot and distant lights) shared by test_analytic_lights.py (CPU) and
test_gpu_analytic_lights.py, with their plain twins, the known-answer scenes and the records of the fp32-against-fp64 check.

Every per-sample case uses the frame, sample count, seed and draw budget of nee_scenes.REF_* (48 x 27 pixels x 13 one-sample
frames = 16 848 samples).  A builder called with full=False builds the case's twin geometry (glossy materials as lambertian,
rough glass as a dielectric); the plain twin is that with light sampling off and the environment cleared -- the analytic lights
are then in no table: what the plain kernel renders, the baseline of criterion (b).  The reference of a case is
ref64.reference on its RefScene.

What was fixed, and why: checker floors are lifted off y = 0 (nee_scenes.LIFT); the intensities are chosen so that the alias table
gives every light of a mixed case a share of the picks (the weights are 4 lum(I), 2 (1 - (cos_i + cos_o) / 2) lum(I), r^2 lum(E)
beside area x luminance); the spots' cones cover part of the floor only, so that samples with falloff 0, between 0 and 1 and 1
all occur; under the environment the map keeps scenes/env_sun.json's scale and the distant light's irradiance is set beside it."""
import numpy as np

import feature_scenes as FS
import glass_scenes as GLS
import glossy_scenes as GS
import nee_scenes as NS
import ref64 as R
import ref64_analytic_lights as RA

NEE, ENV, FAMILIES = FS.NEE, FS.ENV, FS.FAMILIES
LIFT = NS.LIFT


class _Mats:
    """the glossy and rough-glass constructors, or their stand-ins in a twin"""

    def __init__(self, sc, full):
        self.g, self.gl = GS._Mats(sc, full), GLS._Mats(sc, full)
        self.rough, self.plastic, self.rough_glass = self.g.rough, self.g.plastic, self.gl.rough_glass


def _frame(rtmi, depth=6, sky=False, background=(0.02, 0.02, 0.03), w=NS.REF_W, h=NS.REF_H, spp=1):
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background(background, sky_gradient=sky, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    return sc


def room(rtmi, full=True, **kw):
    """(i) a room of six quads with one point light and balls of lambertian, fuzz-0.3 metal, plastic, rough glass (r = 0.3)
    and dielectric"""
    sc = _frame(rtmi, **kw)
    m = _Mats(sc, full)
    white, red, green = sc.lambertian((0.7, 0.7, 0.65)), sc.lambertian((0.6, 0.15, 0.1)), sc.lambertian((0.15, 0.5, 0.15))
    x0, x1, y1, z0, z1 = -3.5, 3.5, 4.5, -3.0, 7.0
    sc.quad((x0, 0, z0), (0, 0, z1 - z0), (x1 - x0, 0, 0), white)    # floor (normal +y)
    sc.quad((x0, y1, z0), (x1 - x0, 0, 0), (0, 0, z1 - z0), white)   # ceiling (-y)
    sc.quad((x0, 0, z0), (x1 - x0, 0, 0), (0, y1, 0), white)         # back wall (+z)
    sc.quad((x0, 0, z1), (0, y1, 0), (x1 - x0, 0, 0), white)         # wall behind the camera (-z)
    sc.quad((x0, 0, z0), (0, y1, 0), (0, 0, z1 - z0), red)           # left (+x)
    sc.quad((x1, 0, z0), (0, 0, z1 - z0), (0, y1, 0), green)         # right (-x)
    sc.sphere((-2.4, 0.5, 0.2), 0.5, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((-1.2, 0.5, 0.9), 0.5, sc.metal((0.8, 0.7, 0.6), 0.3))
    sc.sphere((0.0, 0.5, 0.2), 0.5, m.plastic((0.7, 0.15, 0.1), 1.5, 0.15))
    sc.sphere((1.2, 0.5, 0.9), 0.5, m.rough_glass(1.5, 0.3))
    sc.sphere((2.4, 0.5, 0.2), 0.5, sc.dielectric(1.5))
    sc.point_light((0.3, 3.2, 0.8), (30.0, 27.0, 24.0))
    return sc


def spots(rtmi, full=True, **kw):
    """(ii) two spots of different cones and colours beside a quad light and a sphere light: the alias table mixes analytic
    and area lights, and a BSDF ray that ends on an emitter is MIS-weighted with the smaller selection probability"""
    sc = _frame(rtmi, **kw)
    m = _Mats(sc, full)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.5, 0.4)))
    sc.sphere((-1.2, 0.6, 0.5), 0.6, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((1.3, 0.5, 0.8), 0.5, sc.metal((0.8, 0.7, 0.6), 0.3))
    sc.sphere((0.1, 0.45, 1.6), 0.45, m.rough((0.95, 0.64, 0.54), 0.4))
    sc.quad((-0.5, 2.8, -1.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.sphere((2.3, 1.9, -1.0), 0.25, sc.diffuse_light((5.0, 6.0, 7.0)))
    sc.spot_light((-1.5, 3.0, 1.0), (0.5, -3.0, -0.5), (60.0, 20.0, 10.0), 15.0, 25.0)
    sc.spot_light((2.0, 2.5, 2.0), (-1.0, -2.5, -1.5), (5.0, 20.0, 40.0), 0.0, 40.0)
    return sc


def suns(rtmi, full=True, **kw):
    """(iii) a distant light at alpha = 0 and one at 3 degrees over the sky gradient, with a smooth torus (plastic) and a checker
    floor"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0), **kw)
    m = _Mats(sc, full)
    sc.xz_rect(-20, 20, -20, 20, LIFT, sc.lambertian(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.4, 0.2))))
    mat = m.plastic((0.2, 0.35, 0.7), 1.5, 0.3)
    v, n = GLS.torus(segs=8, sides=6, centre=(0.0, 0.8, 0.2))  # (96 triangles)
    for k in range(len(v)):
        sc.triangle(v[k][0], v[k][1], v[k][2], mat, normals=n[k])
    sc.distant_light((-0.4, -1.0, -0.3), (3.0, 2.8, 2.5), 0.0)
    sc.distant_light((0.6, -0.5, 0.2), (0.8, 1.2, 2.2), 3.0)
    return sc


ENV_E = (25.0, 22.0, 18.0)  # (beside the map of scenes/env_sun.json at its scale: about a third of the picks)


def sun_env(rtmi, full=True, **kw):
    """(iv) a distant light beside an environment map: the ENV | NEE family"""
    sc = _frame(rtmi, background=(0.1, 0.2, 0.3), **kw)
    m = _Mats(sc, full)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.6, 0.55)))
    sc.sphere((-1.4, 0.75, 0.2), 0.75, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((0.3, 0.75, -0.2), 0.75, m.rough((0.91, 0.92, 0.92), 0.4))
    sc.sphere((1.8, 0.5, 0.9), 0.5, sc.metal((0.8, 0.7, 0.6), 0.3))
    e, scale, rotate = NS._sun_map()
    sc.set_environment(e, scale, rotate)
    sc.distant_light((0.5, -1.0, -0.4), ENV_E, 1.0)
    return sc


def lone_point(rtmi, full=True, **kw):
    """(v) no emitter but one point light"""
    sc = _frame(rtmi, background=(0.0, 0.0, 0.0), **kw)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.5, 0.4)))
    sc.sphere((-1.2, 0.6, 0.5), 0.6, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((1.3, 0.5, 0.8), 0.5, sc.metal((0.8, 0.7, 0.6), 0.3))
    sc.point_light((0.2, 2.6, 1.0), (12.0, 11.0, 10.0))
    return sc


# name -> (family bits the kernel must report, builder, the keys of the tally that must be nonzero)
_SHADOWS = ("analytic_shadow_occluded", "analytic_shadow_clear")
CASES = {
    "point light in a room": (NEE, room, ("point_picks", "glossy_lit_by_analytic", "dielectric_vertices", "glass_light_samples") + _SHADOWS),
    "two spots + quad + sphere": (NEE, spots, ("spot_picks", "area_picks", "analytic_spot_falloff_zero", "analytic_spot_falloff_partial",
                                               "analytic_spot_falloff_one", "glossy_lit_by_analytic", "emitter_mis_hits") + _SHADOWS),
    "two suns, torus": (NEE, suns, ("distant_picks", "analytic_distant_alpha_zero_samples", "glossy_lit_by_analytic") + _SHADOWS),
    "sun + environment": (ENV | NEE, sun_env, ("distant_picks", "area_picks", "glossy_lit_by_analytic") + _SHADOWS),
    "point light alone": (NEE, lone_point, ("point_picks",) + _SHADOWS),
}
# the case each deliberate mistake is shown on
MISTAKES = (("point light alone", "point_no_inverse_square"), ("two spots + quad + sphere", "spot_linear_falloff"),
            ("distant 20 degrees", "distant_unfolded"), ("point light alone", "delta_power_heuristic"))


def wide_sun(rtmi, full=True, **kw):
    """the case of `distant_unfolded`: one distant light of alpha = 20 degrees (the fold is 2 / (1 + cos 20) = 1.031)"""
    sc = _frame(rtmi, background=(0.0, 0.0, 0.0), **kw)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.5, 0.4)))
    sc.sphere((-1.2, 0.6, 0.5), 0.6, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((1.3, 0.5, 0.8), 0.5, sc.metal((0.8, 0.7, 0.6), 0.3))
    sc.distant_light((-0.3, -1.0, -0.5), (3.0, 2.8, 2.5), 20.0)
    return sc


EXTRA = {"distant 20 degrees": (NEE, wide_sun, ("distant_picks",) + _SHADOWS)}


def _entry(name):
    return CASES[name] if name in CASES else EXTRA[name]


family, seed_of, inputs = FS.bindings(_entry)


def scene(rtmi, name, **kw):
    sc = _entry(name)[1](rtmi, True, **kw)
    sc.set_light_sampling(True)
    return sc


def plain_twin(rtmi, name):
    """made plain, the point, spot and distant lights kept: without light sampling they light nothing"""
    return FS.cleared(_entry(name)[1](rtmi, False), analytic_lights=False)


def check_contents(name, tally):
    """the case holds what it is there for: every count nonzero"""
    for what in _entry(name)[2]:
        assert tally[what] > 0, (name, what, tally[what])


# ------------------------------------------------------------------------------------ known answers: a lambertian floor, one light
RHO = 0.5
POINT_X, POINT_I = (2.5, 2.0, 0.0), (6.0, 5.0, 4.0)
SUN_DIR, SUN_E = (0.3, -1.0, 0.2), (3.0, 2.5, 2.0)       # the direction the light travels
SPOT_X, SPOT_DIR, SPOT_ANGLES = (2.5, 2.0, 0.3), (0.0, -1.0, 0.0), (8.0, 14.0)
BALL = ((2.3, 0.5, 0.1), 0.3)


def floor_scene(rtmi, w=64, h=36, spp=256):
    """nee_scenes.analytic_scene without its rectangle: max_depth 2 (camera -> floor -> light sample), black background"""
    sc = rtmi.Scene.new(w, h, spp, 2)
    sc.set_background((0, 0, 0), sky_gradient=False, defocus_blur=False)
    sc.camera((2.5, 1.2, -1.5), (2.5, 0.0, 0.0), (0, 1, 0), 50.0)
    sc.xz_rect(-50, 50, -50, 50, 0.0, sc.lambertian((RHO, RHO, RHO)))
    sc.set_light_sampling(True)
    return sc


def floor_points(sc, q=6, corners=False):
    """the floor points [H][W][q][q][3] under each pixel's jitter quadrature (corners=True: q = 2 at the footprint's corners),
    and the camera's origin and ray directions"""
    cam = sc.get_camera()
    org, ll = np.array(cam.origin, np.float64), np.array(cam.lower_left, np.float64)
    hor, ver = np.array(cam.horizontal, np.float64), np.array(cam.vertical, np.float64)
    W, H = sc.width, sc.height
    xi = np.array([0.0, 1.0]) if corners else (np.arange(q) + 0.5) / q
    u = (np.arange(W)[None, :, None, None] + xi[None, None, :, None]) / (W - 1)
    v = (np.arange(H)[:, None, None, None] + xi[None, None, None, :]) / (H - 1)
    d = ll + u[..., None] * hor + v[..., None] * ver - org
    t = -org[1] / d[..., 1]
    pts = org + t[..., None] * d
    pts[~(t > 0)] = np.nan
    return pts, org, d


def point_expected(sc, x=POINT_X, intensity=POINT_I):
    """rho I cos(theta) / (pi d^2) per channel, averaged over each pixel's footprint: [H][W][3]"""
    pts, _, _ = floor_points(sc)
    ld = np.asarray(x, np.float64) - pts
    d2 = (ld * ld).sum(axis=-1)
    val = RHO * (ld[..., 1] / np.sqrt(d2)) / (np.pi * d2)
    return val.mean(axis=(2, 3))[..., None] * np.asarray(intensity, np.float64)


def sun_expected(direction=SUN_DIR, irradiance=SUN_E):
    """rho E cos(theta0) / pi per channel: the same at every floor point"""
    d = -np.asarray(direction, np.float64)
    return RHO * np.asarray(irradiance, np.float64) * (d[1] / np.sqrt((d * d).sum())) / np.pi


# ------------------------------------------------------------------------------------ records of the fp32-against-fp64 check
RECORD_WORDS, OUTPUT_WORDS, RECORD_SEED = 16, 8, 5


def records(n=20000, seed=RECORD_SEED):
    """fp32 [3 n][16] records of tests/analytic_light_host_driver.cpp, n per type.  Spots: half the vertices are placed at an
    angle from the axis within 0.5 degrees of the outer or the inner edge, on both sides of it; a tenth have inner == outer
    (inv = FLT_MAX).  Distant: a fifth at alpha = 0, the others in (0, 45] degrees."""
    rng = np.random.default_rng(seed)

    def unit(v):
        return v / np.sqrt((v * v).sum(axis=1))[:, None]
    rec = np.zeros((3, n, RECORD_WORDS), np.float64)
    for k, t in enumerate((RA.POINT, RA.SPOT, RA.DISTANT)):
        rec[k, :, 0] = t
        rec[k, :, 4:6] = rng.uniform(0, 1, (n, 2))
    # point
    rec[0, :, 1:4] = rng.uniform(-5, 5, (n, 3))
    rec[0, :, 6:9] = rng.uniform(-5, 5, (n, 3))
    # spot: the vertex at distance d from x at angle th from the axis
    x, a = rng.uniform(-5, 5, (n, 3)), unit(rng.normal(size=(n, 3)))
    outer = rng.uniform(1, 179, n)
    inner = np.where(rng.uniform(size=n) < 0.1, outer, outer * rng.uniform(0, 1, n))
    th = rng.uniform(0, 180, n)
    edge = rng.uniform(size=n) < 0.5
    th = np.where(edge, np.where(rng.uniform(size=n) < 0.5, outer, inner) + rng.uniform(-0.5, 0.5, n), th)
    b = unit(np.cross(a, rng.normal(size=(n, 3))))
    w = np.cos(np.radians(th))[:, None] * a + np.sin(np.radians(th))[:, None] * b
    rec[1, :, 1:4] = x + rng.uniform(0.1, 8, n)[:, None] * w
    rec[1, :, 6:9], rec[1, :, 9:12] = x, a.astype(np.float32)
    inner, outer = inner.astype(np.float32).astype(np.float64), outer.astype(np.float32).astype(np.float64)
    ci, co = np.cos(np.radians(inner)), np.cos(np.radians(outer))
    with np.errstate(all="ignore"):
        rec[1, :, 12], rec[1, :, 13] = co, np.minimum(1 / (ci - co), RA.FLT_MAX)
    # distant
    alpha = np.where(rng.uniform(size=n) < 0.2, 0.0, rng.uniform(0, 45, n) + 1e-3).clip(0, 45)
    rec[2, :, 1:4] = rng.uniform(-5, 5, (n, 3))
    rec[2, :, 6:9] = unit(rng.normal(size=(n, 3))).astype(np.float32)
    rec[2, :, 14], rec[2, :, 15] = 1 - np.cos(np.radians(alpha)), rng.uniform(1, 400, n)
    return rec.reshape(-1, RECORD_WORDS).astype(np.float32)


def statement(rec, T):
    """what the driver writes for the records, from ref64_analytic_lights at dtype T: [n][8] float64"""
    out = np.zeros((len(rec), OUTPUT_WORDS), np.float64)
    out[:, 4] = 1
    r = rec.astype(T)
    kind = rec[:, 0].astype(int)
    p, u1, u2 = r[:, 1:4], r[:, 4], r[:, 5]
    k = np.flatnonzero(kind != RA.DISTANT)
    ld = r[k, 6:9] - p[k]
    d2 = R._dot(ld, ld)
    fall = np.ones(len(k), T)
    s = np.flatnonzero(kind[k] == RA.SPOT)
    fall[s] = RA.falloff_of(dict(axis=rec[k[s], 9:12], cos_o=rec[k[s], 12], inv=rec[k[s], 13]), ld[s], T)
    with np.errstate(all="ignore"):
        out[k, 0:3], out[k, 3], out[k, 4] = ld, np.where((fall > 0) & (d2 > 0), fall / d2, 0), fall
    k = np.flatnonzero(kind == RA.DISTANT)
    out[k, 0:3] = r[k, 15][:, None] * RA.cone_direction(rec[k, 6:9], rec[k, 14], u1[k], u2[k], T)
    out[k, 3] = 1
    return out


def share(got, ref):
    """(the share of records within 1e-4 max(1, |ref|) in every word, among those on the same branch; the share on another
    branch: a sample made by one and not by the other)"""
    same = (got[:, 3] > 0) == (ref[:, 3] > 0)
    ok = (np.abs(got - ref) <= 1e-4 * np.maximum(1.0, np.abs(ref))).all(axis=1)
    return float(ok[same].mean()), float(1 - same.mean())
