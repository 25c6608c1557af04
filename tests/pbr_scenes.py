"""Scenes of the metallic-roughness material shared by test_pbr.py (CPU) and test_gpu_pbr.py, with their plain
twins, the known-answer scenes and the records of the fp32-against-fp64 check.

Every per-sample case uses the frame, sample count, seed and draw budget of nee_scenes.REF_* (48 x 27 pixels x 13 one-sample
frames = 16 848 samples).  A builder called with full=False builds the case's twin: every pbr material replaced by a lambertian
of its base texture; the plain twin is that with light sampling off, the environment cleared and the analytic lights out of
every table -- what the plain kernel renders, the baseline of criterion (b).  The reference of a case is ref64.reference.

What was fixed, and why: solid colours and factors stay away from the values x with 255 x within 1e-3 of k + 1/2 (0.1, 0.3, 0.7,
0.9 ...), where the byte of an fp32 evaluation and of the fp64 one may differ (0.5 is exact: 128 in both); the image ORM map's G
bytes start at 40 and the noise map's G at 0.3, which keeps those materials' r8 above the light-sample threshold (the reference
once took that decision per material); colours, roughnesses and metalnesses of the maps otherwise run over their whole range.  The
decision is each hit's: the last case holds one material whose checker map carries r8 across the threshold."""
import numpy as np

import feature_scenes as FS
import glass_scenes as GLS
import nee_scenes as NS
import ref64_pbr as RP

NEE, ENV, MEDIA, MOTION, FAMILIES = FS.NEE, FS.ENV, FS.MEDIA, FS.MOTION, FS.FAMILIES
LIFT = NS.LIFT
SMOOTH = (0.02, 0.03)  # roughness factors below the threshold (r8 = 5, 8)


class _Mats:
    """the pbr constructor, or its stand-in in a twin: a lambertian of the base texture"""

    def __init__(self, sc, full):
        self.sc, self.full = sc, full

    def pbr(self, base, metallic=0.0, roughness=0.5, ior=1.5, metallic_roughness=None):
        if self.full:
            return self.sc.pbr(base, metallic, roughness, ior, metallic_roughness)
        return self.sc.lambertian(base)


def _frame(rtmi, depth=6, sky=False, background=(0.02, 0.02, 0.03), w=NS.REF_W, h=NS.REF_H, spp=1):
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background(background, sky_gradient=sky, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    return sc


def images(seed=3, rows=8, cols=8):
    """(base colour image, ORM image) [rows][cols][3] uint8: G (roughness) in 40..255, B (metalness) over 0..255 with a third of the
    texels at 0 and a third at 255; R (occlusion) random, unused"""
    rng = np.random.default_rng(seed)
    base = rng.integers(30, 256, (rows, cols, 3)).astype(np.uint8)
    orm = rng.integers(0, 256, (rows, cols, 3))
    orm[:, :, 1] = rng.integers(40, 256, (rows, cols))
    pick = rng.integers(0, 3, (rows, cols))
    orm[:, :, 2] = np.where(pick == 0, 0, np.where(pick == 1, 255, orm[:, :, 2]))
    return base, orm.astype(np.uint8)


def room(rtmi, full=True, **kw):
    """(1) a room of six quads with balls over m in {0, 0.3, 1} and r8 on both sides of the threshold, one quad light"""
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
    sc.sphere((-2.4, 0.5, 0.2), 0.5, m.pbr((0.31, 0.52, 0.71), 0.0, 0.4))
    sc.sphere((-1.2, 0.5, 0.9), 0.5, m.pbr((0.8, 0.69, 0.31), 0.3, 0.2))
    sc.sphere((0.0, 0.5, 0.2), 0.5, m.pbr((0.95, 0.64, 0.54), 1.0, 0.35))
    sc.sphere((1.2, 0.5, 0.9), 0.5, m.pbr((0.71, 0.2, 0.2), 0.3, SMOOTH[0]))
    sc.sphere((2.4, 0.5, 0.2), 0.5, m.pbr((0.91, 0.91, 0.91), 1.0, SMOOTH[1]))
    sc.sphere((0.0, 1.6, -1.2), 0.6, m.pbr(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.4, 0.2)), 0.5, 0.5, 1.33))
    sc.quad((-0.8, 4.4, -0.5), (1.6, 0.0, 0.0), (0.0, 0.0, 1.6), sc.diffuse_light((14.0, 13.0, 12.0)))
    return sc


def _mapped(sc, m):
    """the mapped materials of cases (2) and (3): image base + image ORM (factors 1: the texels are used exactly), the same
    images under factors below 1, and a turbulence map over a solid colour"""
    base, orm = images()
    tb, to = sc.image_texture(base), sc.image_texture(orm)
    noise = sc.noise_texture((0.0, 0.3, 0.0), (0.0, 1.0, 1.0), style="turbulence", scale=3.0, octaves=3, seed=9)
    return (m.pbr(tb, 1.0, 1.0, 1.5, to), m.pbr(tb, 0.6, 0.8, 1.4, to), m.pbr((0.72, 0.45, 0.2), 1.0, 0.8, 1.5, noise))


def _mapped_objects(sc, mats):
    on_quad, on_sphere, on_torus = mats
    sc.quad((-2.6, 0.02, -0.6), (0.0, 0.0, 2.4), (2.4, 0.0, 0.0), on_quad)  # (a tile on the floor, normal +y)
    sc.sphere((1.6, 0.7, 0.4), 0.7, on_sphere)
    v, n = GLS.torus(R0=0.7, r0=0.3, segs=8, sides=6, centre=(-0.3, 1.5, -0.6))
    for k in range(len(v)):
        sc.triangle(v[k][0], v[k][1], v[k][2], on_torus, normals=n[k])


def maps(rtmi, full=True, **kw):
    """(2) an image base colour and an image ORM map on a quad and on a sphere (u, v), a noise map on a torus mesh; a sphere light
    and a spot light"""
    sc = _frame(rtmi, **kw)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.5, 0.4)))
    _mapped_objects(sc, _mapped(sc, _Mats(sc, full)))
    sc.sphere((2.3, 2.6, -1.0), 0.3, sc.diffuse_light((9.0, 10.0, 12.0)))
    sc.spot_light((-2.0, 3.5, 2.0), (1.0, -3.0, -1.5), (60.0, 50.0, 40.0), 20.0, 40.0)
    return sc


def maps_env(rtmi, full=True, **kw):
    """(3) the same materials under env_sun's map: the ENV | NEE family"""
    sc = _frame(rtmi, background=(0.1, 0.2, 0.3), **kw)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.6, 0.55)))
    _mapped_objects(sc, _mapped(sc, _Mats(sc, full)))
    e, scale, rotate = NS._sun_map()
    sc.set_environment(e, scale, rotate)
    return sc


def plain_bump(rtmi, full=True, **kw):
    """(4) light sampling off, under the sky gradient: the plain EXT family, with a bump on one pbr material"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0), **kw)
    m = _Mats(sc, full)
    sc.xz_rect(-20, 20, -20, 20, LIFT, sc.lambertian(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.4, 0.2))))
    mats = _mapped(sc, m)
    _mapped_objects(sc, mats)
    bumped = m.pbr((0.8, 0.6, 0.2), 0.5, 0.3)
    sc.sphere((0.2, 0.6, 1.6), 0.6, bumped)
    if full:
        sc.set_bump(bumped, sc.noise_texture((0, 0, 0), (1, 1, 1), style="fbm", scale=4.0, octaves=2, seed=4), 0.15)
    sc.sphere((-2.3, 2.2, -1.5), 0.5, sc.diffuse_light((6.0, 5.5, 5.0)))
    return sc


ACROSS = ((0.0, 0.02, 1.0), (0.0, 0.6, 0.0))  # the checker map's two colours: (G, B) = (0.02, 1) and (0.6, 0), r8 = 5 and 153


def across(rtmi, full=True, **kw):
    """(5) one pbr material (m factor 0.5, r factor 1) whose checker map carries r8 from 5 to 153, across the light-sample
    threshold of 13, on a floor tile and two balls under a quad light: its smooth tiles take no light sample, its rough ones do"""
    sc = _frame(rtmi, **kw)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.5, 0.4)))
    mat = _Mats(sc, full).pbr((0.5, 0.5, 0.5), 0.5, 1.0, 1.5, sc.checker_texture(*ACROSS))
    sc.quad((-2.6, LIFT, -1.2), (0.0, 0.0, 3.0), (5.2, 0.0, 0.0), mat)
    sc.sphere((-1.1, 0.75, 0.2), 0.7, mat)
    sc.sphere((1.2, 0.65, 0.6), 0.6, mat)
    sc.quad((-0.8, 3.4, -0.5), (1.6, 0.0, 0.0), (0.0, 0.0, 1.6), sc.diffuse_light((14.0, 13.0, 12.0)))
    return sc


_CHOICES = (("pbr_metal_choices", 500), ("pbr_plastic_choices", 500))
# name -> (family bits the kernel must report, builder, light sampling, (key of the tally, at least))
CASES = {
    "room": (NEE, room, True, _CHOICES + (("pbr_lit", 100), ("pbr_smooth_vertices", 50))),
    "maps": (NEE, maps, True, _CHOICES + (("pbr_lit", 100), ("pbr_image_map_hits", 100), ("pbr_noise_map_hits", 100), ("pbr_image_base_hits", 100))),
    "maps under an environment": (ENV | NEE, maps_env, True, _CHOICES + (("pbr_lit", 100), ("pbr_image_map_hits", 100), ("pbr_noise_map_hits", 100))),
    "plain, bumped": (0, plain_bump, False, _CHOICES + (("pbr_image_map_hits", 100), ("pbr_noise_map_hits", 100))),
    "a map across the threshold": (NEE, across, True, _CHOICES + (("pbr_lit", 100), ("pbr_smooth_vertices", 500), ("pbr_checker_map_hits", 1000))),
}
# the case each deliberate mistake is shown on
MISTAKES = (("half-metal floor", "lobe_draw_not_rescaled"), ("room", "metal_f0_004"), ("maps", "roughness_from_r"), ("maps", "light_step_from_factors"))


def half_metal_floor(rtmi, full=True, **kw):
    """the case of `lobe_draw_not_rescaled`: a floor and two balls at m8 = 128 under a coat of index 2.2, whose plastic vertices
    choose the coat for about a fifth of their draws -- never, if the draw is not rescaled (ul >= m then)"""
    sc = _frame(rtmi, **kw)
    m = _Mats(sc, full)
    sc.quad((-6.0, 0.0, -6.0), (0.0, 0.0, 14.0), (12.0, 0.0, 0.0), m.pbr((0.6, 0.52, 0.4), 0.5, 0.25, 2.2))
    sc.sphere((-1.2, 0.7, 0.4), 0.7, m.pbr((0.31, 0.52, 0.71), 0.5, 0.15, 2.2))
    sc.sphere((1.2, 0.7, 0.4), 0.7, m.pbr((0.8, 0.69, 0.31), 0.5, 0.4, 2.2))
    sc.quad((-0.8, 3.4, -0.5), (1.6, 0.0, 0.0), (0.0, 0.0, 1.6), sc.diffuse_light((14.0, 13.0, 12.0)))
    return sc


EXTRA = {"half-metal floor": (NEE, half_metal_floor, True, _CHOICES + (("pbr_lit", 100),))}


def _entry(name):
    return CASES[name] if name in CASES else EXTRA[name]


family, seed_of, inputs = FS.bindings(_entry)


def scene(rtmi, name, **kw):
    sc = _entry(name)[1](rtmi, True, **kw)
    sc.set_light_sampling(_entry(name)[2])
    return sc


def plain_twin(rtmi, name):
    return FS.cleared(_entry(name)[1](rtmi, False))


def check_contents(name, tally):
    """the case holds the vertices it is about"""
    for what, least in _entry(name)[3]:
        assert tally[what] >= least, (name, what, tally[what], least)


# ----------------------------------------------------------------------------------------- twins and known answers
GRID_C, GRID_R = (102 / 255, 51 / 255, 204 / 255), 77 / 255  # a colour and a roughness on the 8-bit grid


def grid_scene(rtmi, kind, w=NS.REF_W, h=NS.REF_H, spp=1):
    """three balls over a lambertian floor under a rectangle light, with light sampling.  kind "pbr0": pbr(c, m = 0,
    r) with c, r on the 8-bit grid; "plastic": plastic(c, ior, r), its independent twin; "pbr1": pbr(c, m = 1, r);
    "rough_metal": rough_metal(c, r)"""
    sc = _frame(rtmi, w=w, h=h, spp=spp)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.5, 0.4)))
    spec = [(GRID_C, GRID_R, 1.5), ((204 / 255, 204 / 255, 153 / 255), 26 / 255, 1.33), ((51 / 255, 153 / 255, 102 / 255), 10 / 255, 1.5)]
    make = {"pbr0": lambda c, r, ior: sc.pbr(c, 0.0, r, ior), "plastic": lambda c, r, ior: sc.plastic(c, ior, r),
            "pbr1": lambda c, r, ior: sc.pbr(c, 1.0, r, ior), "rough_metal": lambda c, r, ior: sc.rough_metal(c, r)}[kind]
    for k, (c, r, ior) in enumerate(spec):
        sc.sphere((-1.6 + 1.6 * k, 0.6, 0.4), 0.6, make(c, r, ior))
    sc.xz_rect(-0.8, 0.8, -0.5, 1.1, 3.4, sc.diffuse_light((14.0, 13.0, 12.0)))  # (a rect: ref64 samples it without a hook)
    sc.set_light_sampling(True)
    return sc


def linearity_scene(rtmi, m8, w=64, h=36, spp=256):
    """one convex pbr sphere on a black background lit by one quad light: at most one pbr vertex per path"""
    sc = rtmi.Scene.new(w, h, spp, 4)
    sc.set_background((0, 0, 0), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 1.0, 4.0), (0.0, 0.0, 0.0), (0, 1, 0), 35.0)
    sc.sphere((0.0, 0.0, 0.0), 1.0, sc.pbr((0.91, 0.6, 0.31), m8 / 255, 0.35))
    sc.quad((-1.0, 2.5, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), sc.diffuse_light((10.0, 10.0, 10.0)))
    sc.set_light_sampling(True)
    return sc


CHECKER_BYTES = ((255, 0), (26, 255))  # (G, B) of the even and the odd tiles


def checker_map_scene(rtmi, which, w=64, h=36, spp=64):
    """a floor quad under a quad light.  which "map": one pbr material (factors 1) whose checker ORM map alternates the bytes of
    CHECKER_BYTES; "even" / "odd": the constant pbr material of that tile class on the whole quad"""
    sc = rtmi.Scene.new(w, h, spp, 4)
    sc.set_background((0.05, 0.05, 0.05), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0)
    c = (0.8, 0.52, 0.31)
    (ge, be), (go, bo) = CHECKER_BYTES
    if which == "map":
        mat = sc.pbr(c, 1.0, 1.0, 1.5, sc.checker_texture((0.0, ge / 255, be / 255), (0.0, go / 255, bo / 255)))
    else:
        g, b = CHECKER_BYTES[which == "odd"]
        mat = sc.pbr(c, b / 255, g / 255)
    sc.quad((-2.0, LIFT, -2.0), (0.0, 0.0, 4.0), (4.0, 0.0, 0.0), mat)
    sc.quad((-0.7, 2.5, -0.7), (1.4, 0.0, 0.0), (0.0, 0.0, 1.4), sc.diffuse_light((8.0, 8.0, 8.0)))
    sc.set_light_sampling(True)
    return sc


# ------------------------------------------------------------------------------------ records of the fp32-against-fp64 check
RECORD_WORDS, OUTPUT_WORDS, RECORD_SEED = 8, 8, 5


def records(n=20000, seed=RECORD_SEED):
    """fp32 [n][8] records of tests/pbr_host_driver.cpp: base colour (3), G, B, rf, mf, ul.  A quarter of the colours and map
    values lie on the 8-bit grid (an image's texels), a tenth of the map values and of the factors are exactly 0, a tenth exactly 1"""
    rng = np.random.default_rng(seed)
    rec = rng.uniform(0, 1, (n, RECORD_WORDS))
    grid = rng.uniform(size=(n, 5)) < 0.25
    rec[:, 0:5] = np.where(grid, rng.integers(0, 256, (n, 5)) / 255, rec[:, 0:5])
    ends = rng.uniform(size=(n, 4))
    rec[:, 3:7] = np.where(ends < 0.1, 0.0, np.where(ends < 0.2, 1.0, rec[:, 3:7]))
    return rec.astype(np.float32)


def statement(rec, T):
    """what the driver writes for the records, from ref64_pbr at dtype T: [n][8] float64 -- c8 (3), r8, m8, metal, ul', alpha"""
    r = rec.astype(T)
    c8, r8, m8 = RP.byte(r[:, 0:3], T), RP.byte(r[:, 5] * r[:, 3], T), RP.byte(r[:, 6] * r[:, 4], T)
    metal, ulp = RP.choose(m8, r[:, 7], T)
    alpha = RP.alpha_of(RP.unit(r8, T), T)
    return np.column_stack([c8, r8, m8, metal, ulp, alpha]).astype(np.float64)


def excluded(rec):
    """records whose fp64 255 x lies within 1e-4 of a half-integer in any of the five bytes, or whose ul lies within 1e-6 of m"""
    r = rec.astype(np.float64)
    x = np.column_stack([r[:, 0:3], r[:, 5] * r[:, 3], r[:, 6] * r[:, 4]]).clip(0, 1) * 255
    near_half = (np.abs(x - np.floor(x) - 0.5) < 1e-4).any(axis=1)
    m = RP.unit(RP.byte(r[:, 6] * r[:, 4], np.float64), np.float64)
    return near_half | (np.abs(r[:, 7] - m) < 1e-6)
