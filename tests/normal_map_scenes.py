"""Scenes of tangent-space normal maps shared by test_normal_map.py (CPU) and test_gpu_normal_map.py, with their
twins without maps, the seeded points of the frame-against-parametrisation check, and the seeded records of the
fp32-against-fp64 check of csrc/rt_tangent.h.

Every case uses the frame, sample count, seed and draw budget of nee_scenes.REF_* (48 x 27 pixels x 13 one-sample frames =
16 848 samples; the media and motion cases use their families' seed, as bump_scenes.py does).  A builder called with maps=False
builds the case's TWIN: the same primitives, materials AND image textures, in the same order, with no map set -- the baseline of
criterion (b), and the scene whose feature buffers and query records a map must leave alone.  maps="flat" sets every map to a
constant (128, 128, 255) image of the same size: the texel that leaves the normal untouched.

All images are made in memory.  Map content: nearest-texel lookup makes a sample flip where the fp32 and the fp64 (u, v) fall
on different texels, so the maps are coarse and vary gently -- 16 x 16 texels per primitive, one or two waves of a smooth height
field across them, slopes of at most 0.3 (neighbouring texels at most about 15 bytes apart, most a few).

What was adjusted, and why (the fp64 and fp32 numpy references were run on the CPU on every case before it was fixed; a case
stays only if the fp32 reference alone meets criterion (b)):
  * with these maps the fp32 numpy reference alone has 99.82 % (nm_env) to 100.00 % (nm_prims) of the stable samples within
    tolerance, against twins at 99.99 to 100.00 %: (b) holds on every case as first drafted, and no map had to be made gentler.
    A texel flip costs a sample only where the fp32 and fp64 (u, v) straddle one of the 16 texel edges per axis, about one
    sample in 10^5;
  * nm_prims' smooth mesh ball was enlarged (radius 0.6 -> 1.05) and coarsened (6 x 8 -> 4 x 6 facets, so that the interpolated
    normal leaves the facet's by up to 30 degrees) and its maps' scale raised to 2: with the first draft a frame that is not
    re-orthogonalised about n moved 1.8 % of the samples, too few for criterion (d) to see; now 5.4 % (94.7 % agreement);
  * the bumped floor of bump_scenes.py is kept as a bounded mapped panel over a flat far floor, so that a rectangle's map repeats
    nowhere and every mapped point lies within 4 units.
"""
import functools

import numpy as np

import feature_scenes as FS
import media_scenes as MS
import nee_scenes as NS
import ref64_normal_map as NM
import smooth_scenes as SM

NEE, ENV, MEDIA, MOTION, FAMILIES = FS.NEE, FS.ENV, FS.MEDIA, FS.MOTION, FS.FAMILIES
MIN_MAP_SHARE = 0.15  # of a case's samples touch a mapped vertex: a mistake can then pull the agreement below 97 %


def relief(rows=16, cols=16, fu=1.0, fv=1.0, amp=0.3, phase=0.0):
    """[rows][cols][3] uint8: the normal (-h_u, -h_v, 1) / |.| of the height field whose slopes are
    h_u = amp sin(2 pi fu (r + 0.5) / rows + phase), h_v = amp cos(2 pi fv (c + 0.5) / cols + phase), as bytes 128 + 127 x
    (rounded); u indexes rows and v columns, as image_texel reads them"""
    r, c = np.meshgrid(np.arange(rows) + 0.5, np.arange(cols) + 0.5, indexing="ij")
    hu = amp * np.sin(2 * np.pi * fu * r / rows + phase)
    hv = amp * np.cos(2 * np.pi * fv * c / cols + phase)
    n = np.stack([-hu, -hv, np.ones_like(hu)], axis=-1)
    n /= np.sqrt((n * n).sum(axis=-1))[..., None]
    return np.clip(np.rint(128 + 127 * n), 0, 255).astype(np.uint8)


def flat_map(rows=16, cols=16):
    out = np.full((rows, cols, 3), 128, np.uint8)
    out[..., 2] = 255
    return out


M_WAVES = dict(fu=1.0, fv=1.0, amp=0.3)
M_DIMPLES = dict(fu=2.0, fv=2.0, amp=0.25, phase=0.7)
M_RIPPLE = dict(fu=2.0, fv=1.0, amp=0.3, phase=1.9)
M_GENTLE = dict(fu=1.0, fv=2.0, amp=0.15, phase=0.3)


class _Map:
    """puts a normal map on a material; maps=False: makes the image texture and sets nothing (the twin); maps="flat": a constant
    (128, 128, 255) image.  An image texture is made once per parameter set, in the order of first use, in every mode"""

    def __init__(self, sc, maps):
        self.sc, self.maps, self.made = sc, maps, {}

    def __call__(self, material, content, s=1.0):
        key = tuple(sorted(content.items()))
        if key not in self.made:
            self.made[key] = self.sc.image_texture(flat_map() if self.maps == "flat" else relief(**content))
        if self.maps:
            self.sc.set_normal_map(material, self.made[key], s)
        return material


def _frame(rtmi, depth=6, sky=False, background=(0.02, 0.02, 0.03), w=NS.REF_W, h=NS.REF_H, spp=1):
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background(background, sky_gradient=sky, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    return sc


def _floor(sc, b):
    """the far floor (flat) and the mapped floor panel, lifted 0.01 over it"""
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.5, 0.5, 0.45)))
    sc.xz_rect(-3.4, 3.4, -2.4, 2.4, 0.01, b(sc.lambertian((0.7, 0.65, 0.5)), M_WAVES, 1.0))


def uv_of(v, centre):
    """per-corner (u, v) of mesh corners v [n][3][3] from their direction about `centre`: the sphere's own parametrisation (a
    triangle across the seam gets the long way round: any affine (u, v) is a parametrisation)"""
    o = v.astype(np.float64) - np.asarray(centre, np.float64)
    o /= np.sqrt((o * o).sum(axis=-1))[..., None]
    u = (np.arctan2(-o[..., 2], o[..., 0]) + np.pi) / (2 * np.pi)
    w = np.arccos(np.clip(-o[..., 1], -1, 1)) / np.pi
    return np.stack([u, w], axis=-1).astype(np.float32)


def _mesh(sc, centre, radius, rings, segs, mats, smooth=True, every=1):
    v, n = SM.uv_sphere(centre, radius, rings, segs)
    uv = uv_of(v, centre)
    for k in range(len(v)):
        sc.triangle(v[k][0], v[k][1], v[k][2], mats[(k // every) % len(mats)], tuple(uv[k][0]), tuple(uv[k][1]), tuple(uv[k][2]),
                    normals=n[k] if smooth else None)


def _stage(sc, b, rough=0.3):
    """the floor and three mapped balls: rough metal, plastic, lambertian"""
    _floor(sc, b)
    sc.sphere((-1.7, 0.81, 0.2), 0.8, b(sc.rough_metal((0.9, 0.7, 0.4), rough), M_DIMPLES, 1.0))
    sc.sphere((0.0, 0.81, 0.2), 0.8, b(sc.plastic((0.8, 0.3, 0.1), 1.5, rough), M_GENTLE, 1.5))
    sc.sphere((1.7, 0.81, 0.2), 0.8, b(sc.lambertian((0.3, 0.5, 0.8)), M_WAVES, -1.0))


def sky(rtmi, maps=True):
    """a map on each of the five shapes, under the seven materials that take one: the lambertian panel (rectangle), metal and
    dielectric spheres, a rough-metal cylinder, a smooth plastic mesh ball (triangles with vt), a rough-glass quad standing
    behind them and a turned pbr box (quads), under the sky gradient"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    b = _Map(sc, maps)
    _floor(sc, b)
    sc.sphere((-2.9, 0.71, 0.3), 0.7, b(sc.metal((0.9, 0.9, 0.85), 0.1), M_WAVES, 1.0))
    sc.sphere((-1.4, 0.71, 0.6), 0.7, b(sc.dielectric(1.5), M_DIMPLES, 0.8))
    sc.cylinder(0.45, -0.6, 0.6, b(sc.rough_metal((0.9, 0.7, 0.4), 0.3), M_RIPPLE, 1.0), rotate=((1, 0.2, 0), 80.0), translate=(0.1, 0.65, 0.2))
    _mesh(sc, (1.5, 0.66, 0.5), 0.65, 6, 8, [b(sc.plastic((0.2, 0.6, 0.3), 1.5, 0.3), M_GENTLE, 1.5)])
    sc.quad((-1.6, 0.02, -1.6), (3.2, 0.0, 0.4), (0.0, 1.9, -0.3), b(sc.rough_glass(1.5, 0.2), M_RIPPLE, 1.0))
    sc.box((-0.5, 0.0, -0.5), (0.5, 1.0, 0.5), b(sc.pbr((0.8, 0.5, 0.3), 0.5, 0.4), M_DIMPLES, 1.0), rotate=((0, 1, 0), 30.0), translate=(2.9, 0.02, 0.2))
    return sc


def prims(rtmi, maps=True, w=NS.REF_W, h=NS.REF_H):
    """smooth and flat triangles with vt (two mesh balls), a turned mapped box, a mapped cylinder, and a strongly rippled
    dielectric sheet (scale 2) over them that the camera sees from above and the light coming back from the floor meets from
    below: back-face vertices through glass, and grazing ones where a guard keeps n"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0), w=w, h=h)
    b = _Map(sc, maps)
    _floor(sc, b)
    sc.cylinder(0.4, -0.5, 0.5, b(sc.metal((0.8, 0.8, 0.9), 0.1), M_WAVES, 1.0), rotate=((1, 0, 0), 90.0), translate=(1.7, 0.52, 0.0))
    _mesh(sc, (-1.5, 1.07, 0.1), 1.05, 4, 6, [b(sc.plastic((0.2, 0.6, 0.3), 1.5, 0.3), M_DIMPLES, 2.0), b(sc.lambertian((0.8, 0.4, 0.3)), M_DIMPLES, 2.0)], every=6)
    _mesh(sc, (0.0, 0.47, 1.3), 0.45, 5, 7, [b(sc.lambertian((0.4, 0.4, 0.8)), M_WAVES, 1.0)], smooth=False)
    sc.box((-0.4, 0.0, -0.4), (0.4, 0.8, 0.4), b(sc.rough_metal((0.9, 0.8, 0.6), 0.35), M_RIPPLE, 1.0), rotate=((0.1, 1, 0), 35.0), translate=(0.5, 0.02, -0.7))
    sc.xz_rect(-2.6, 2.6, -1.2, 2.2, 1.5, b(sc.dielectric(1.33), M_RIPPLE, 2.0))
    return sc


def lights(rtmi, maps=True, w=NS.REF_W, h=NS.REF_H, spp=1):
    """the stage under a rectangle emitter and a point light; roulette 0.9 (light sampling is switched on by the caller)"""
    sc = _frame(rtmi, w=w, h=h, spp=spp)
    b = _Map(sc, maps)
    _stage(sc, b, rough=0.5)
    sc.xz_rect(-1.4, 1.4, -0.8, 1.6, 3.2, sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.point_light((2.8, 2.3, 1.0), (4.0, 5.0, 6.0))
    sc.set_russian_roulette(0.9)
    return sc


def env(rtmi, maps=True):
    """the stage under scenes/env_sun.json's map (the caller switches light sampling on)"""
    sc = _frame(rtmi, background=(0.1, 0.2, 0.3))
    b = _Map(sc, maps)
    _stage(sc, b, rough=0.5)
    e, scale, rotate = NS._sun_map()
    sc.set_environment(e, scale, rotate)
    return sc


def fog(rtmi, maps=True):
    """the stage under an emitter, the camera inside thin fog"""
    sc = rtmi.Scene.new(MS.REF_W, MS.REF_H, 1, 6)
    sc.set_background((0.05, 0.06, 0.08), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.6, 0.0), (0, 1, 0), 45.0)
    b = _Map(sc, maps)
    _stage(sc, b)
    sc.xz_rect(-1.0, 1.0, -1.0, 1.0, 3.5, sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9))
    return sc


def motion(rtmi, maps=True):
    """the mapped static stage with an unmapped moving sphere in front"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    b = _Map(sc, maps)
    _stage(sc, b)
    sc.add_moving_sphere((-1.6, 0.55, 2.2), (1.4, 0.55, 1.6), 0.55, sc.lambertian((0.9, 0.9, 0.2)))
    return sc


def nested(rtmi, maps=True, w=NS.REF_W, h=NS.REF_H):
    """bump_scenes.nested's clump with maps: a 288-triangle smooth sphere of radius 0.15 with vt among 100 small spheres, the
    nested grid on; wedges of 24 triangles in mapped plastic, lambertian and glass"""
    sc = rtmi.Scene.new(w, h, 1, 5)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((-1.0, 0.7, 1.9), (-1.0, 0.5, 1.0), (0, 1, 0), 26.0)
    b = _Map(sc, maps)
    rng = np.random.default_rng(3)
    small = [sc.lambertian((0.7, 0.3, 0.3)), sc.metal((0.8, 0.8, 0.8), 0.15)]
    for k in range(100):
        c = rng.uniform(-4, 4, 3)
        sc.sphere((float(c[0]), float(c[1]), float(c[2])), 0.02, small[k % 2])
    m = [b(sc.plastic((0.9, 0.88, 0.8), 1.5, 0.3), M_DIMPLES, 1.0), b(sc.lambertian((1.0, 0.6, 0.2)), M_WAVES, 1.0), b(sc.dielectric(1.5), M_RIPPLE, 1.0)]
    _mesh(sc, (-1.0, 0.5, 1.0), 0.15, 10, 16, m, every=24)
    sc.set_nested_grid(True)
    return sc


# name -> (family bits the kernel must report, builder, light sampling on, the nm_* keys of ref64.tally() it is there for)
CASES = {
    "nm_sky": (0, sky, False, ("nm_lambertian", "nm_metal", "nm_dielectric", "nm_rough_metal", "nm_plastic", "nm_rough_glass", "nm_pbr",
                               "nm_on_sphere", "nm_on_rect", "nm_on_cylinder", "nm_on_triangle", "nm_on_quad")),
    "nm_prims": (0, prims, False, ("nm_on_triangle", "nm_on_quad", "nm_on_cylinder", "nm_dielectric", "nm_back", "nm_kept")),
    "nm_lights": (NEE, lights, True, ("nm_lambertian", "nm_rough_metal", "nm_plastic", "nm_light_samples")),
    "nm_env": (ENV | NEE, env, True, ("nm_lambertian", "nm_rough_metal", "nm_plastic", "nm_light_samples")),
    "nm_fog": (MEDIA, fog, False, ("nm_lambertian", "nm_rough_metal", "nm_plastic")),
    "nm_motion": (MOTION, motion, False, ("nm_lambertian", "nm_rough_metal", "nm_plastic")),
}
# the deliberate mistakes of the normal map (ref64_normal_map.PERTURBATIONS), each on the case that exercises it
MISTAKES = (("nm_sky", "nm_off"), ("nm_sky", "nm_swap_tb"), ("nm_prims", "nm_back_unsigned"), ("nm_prims", "nm_not_about_n"),
            ("nm_sky", "nm_2c_minus_1"))


family, seed_of, inputs = FS.bindings(CASES.__getitem__)


def scene(rtmi, name, maps=True):
    sc = CASES[name][1](rtmi, maps)
    sc.set_light_sampling(CASES[name][2])
    return sc


def plain_twin(rtmi, name):
    """the twin without maps, made plain (feature_scenes.cleared): what the plain
    kernel renders"""
    return FS.cleared(CASES[name][1](rtmi, False))


def check_contents(name, tally):
    """the case met the vertices it is there for, each at least once per hundred samples (nee_scenes.REQUIRED_EVENTS), and at
    least 15 % of its samples touch a mapped vertex"""
    for what in CASES[name][3]:
        assert tally[what] >= NS.REQUIRED_EVENTS, (name, what, tally[what])
    assert tally["nm_share"] >= MIN_MAP_SHARE, (name, tally["nm_share"])


# ------------------------------------------------------------------------------------ the frame against the parametrisation
SHAPES = ("sphere", "rect", "cylinder", "triangle", "quad")


def shape_scene(rtmi, shape, seed=11, count=40):
    """a scene of `count` seeded primitives of one shape (rectangles of all three kinds, rotated cylinders, rotated quads and
    -- every fourth of them -- a rotated box, whose six faces the host builds; triangles with random vt, every fifth with
    det = 0), for test_normal_map's frame check"""
    rng = np.random.default_rng(seed)
    sc = rtmi.Scene.new(16, 9, 1, 2)
    m = sc.lambertian((0.5, 0.5, 0.5))
    f = lambda a: tuple(float(x) for x in a)
    for k in range(count):
        c = rng.uniform(-2, 2, 3)
        if shape == "sphere":
            sc.sphere(f(c), float(rng.uniform(0.3, 1.5)), m)
        elif shape == "rect":
            a0, b0 = rng.uniform(-2, 0, 2)
            a1, b1 = rng.uniform(0.5, 2, 2)
            (sc.xy_rect, sc.xz_rect, sc.yz_rect)[k % 3](float(a0), float(a1), float(b0), float(b1), float(c[2]), m)
        elif shape == "cylinder":
            sc.cylinder(float(rng.uniform(0.2, 1.0)), float(rng.uniform(-1, 0)), float(rng.uniform(0.2, 1.5)), m,
                        rotate=(f(rng.normal(size=3)), float(rng.uniform(-180, 180))), translate=f(c))
        elif shape == "triangle":
            v = c + rng.uniform(-1, 1, (3, 3))
            uv = rng.uniform(-1, 2, (3, 2))
            if k % 5 == 4:
                uv[2] = uv[0] + 0.5 * (uv[1] - uv[0])  # collinear vt: det = 0 (exactly, below: made of halves)
                uv = np.round(uv * 4) / 4
                uv[2] = uv[0] + 0.5 * (uv[1] - uv[0])
            sc.triangle(f(v[0]), f(v[1]), f(v[2]), m, f(uv[0]), f(uv[1]), f(uv[2]))
        elif k % 4 == 3:
            lo = rng.uniform(-1, 0, 3)
            sc.box(f(lo), f(lo + rng.uniform(0.3, 1.5, 3)), m, rotate=(f(rng.normal(size=3)), float(rng.uniform(-180, 180))), translate=f(c))
        else:
            sc.quad(f(c), f(rng.uniform(-1, 1, 3)), f(rng.uniform(-1, 1, 3)), m, rotate=(f(rng.normal(size=3)), float(rng.uniform(-180, 180))),
                    translate=f(rng.uniform(-1, 1, 3)))
    return sc


# ------------------------------------------------------------------------------------ records of the fp32-against-fp64 check
RECORD_WORDS, OUTPUT_WORDS = 20, 4


@functools.lru_cache(maxsize=None)
def records(shape, n=20000, seed=5):
    """[n][20] uint32 (tests/normal_map_host_driver.cpp): the raw frame T.xyz, B.xyz as the shape gives it at a seeded point (a
    sphere's at a random outward normal, a rectangle's signed axes, a cylinder's under a random rotation, a triangle's from random
    corners and vt -- every tenth with det = 0 --, a quad's two random edges), the texel word r8 | g8 << 8 | b8 << 16 (random
    bytes; every sixteenth (128, 128, b), every sixteenth with b8 <= 128), s uniform in [-2, 2], the geometric unit normal g
    (unit(T x B) or its opposite: both sides equally often, `front` says which), the shading normal n up to 30 degrees off g,
    a direction d with d . n < 0 and d . g < 0 (length in [0.5, 2]), front"""
    rng = np.random.default_rng(seed + 100 * SHAPES.index(shape))
    out = np.zeros((n, RECORD_WORDS), np.uint32)
    f32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    unit = lambda a: a / np.sqrt((a * a).sum(axis=1))[:, None]
    if shape == "sphere":
        o = unit(rng.normal(size=(n, 3)))
        Tr = np.stack([o[:, 2], np.zeros(n), -o[:, 0]], axis=1)
        Br = np.cross(o, Tr)
    elif shape == "rect":
        kind = rng.integers(0, 3, n)
        aa, ba = np.array([0, 0, 1])[kind], np.array([1, 2, 2])[kind]
        Tr, Br = np.zeros((n, 3)), np.zeros((n, 3))
        Tr[np.arange(n), aa] = rng.choice([-1.0, 1.0], n)
        Br[np.arange(n), ba] = rng.choice([-1.0, 1.0], n)
    elif shape == "cylinder":
        q = unit(rng.normal(size=(n, 4)))  # a random rotation from a unit quaternion
        w, x, y, z = q.T
        Rm = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                       np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                       np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)
        ph, rad = rng.uniform(0, 2 * np.pi, n), rng.uniform(0.2, 1.5, n)
        Tr = np.einsum("nij,nj->ni", Rm, np.stack([-rad * np.sin(ph), rad * np.cos(ph), np.zeros(n)], axis=1))
        Br = Rm[:, :, 2] * rng.choice([-1.0, 1.0], n)[:, None]
    elif shape == "triangle":
        e1, e2 = rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3))
        du1, du2, dv1, dv2 = rng.uniform(-1, 1, (4, n))
        flat = np.arange(n) % 10 == 9
        du2, dv2 = np.where(flat, 0.5 * du1, du2), np.where(flat, 0.5 * dv1, dv2)
        du1, du2, dv1, dv2 = (a.astype(np.float32).astype(np.float64) for a in (du1, du2, dv1, dv2))
        with np.errstate(all="ignore"):
            det = du1 * dv2 - du2 * dv1
            det = np.where(flat, 0.0, det)
            Tr = (dv2[:, None] * e1 - dv1[:, None] * e2) / det[:, None]
            Br = (du1[:, None] * e2 - du2[:, None] * e1) / det[:, None]
        g_src = np.cross(e1, e2)
    else:
        Tr, Br = rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3))
    with np.errstate(all="ignore"):
        Tr, Br = Tr.astype(np.float32), Br.astype(np.float32)
        g = unit(g_src if shape == "triangle" else np.cross(Tr.astype(np.float64), Br.astype(np.float64)))
    front = rng.integers(0, 2, n).astype(bool)
    g = np.where(front[:, None], g, -g)
    # the shading normal: g turned by up to 30 degrees about a random axis in the plane
    axis = unit(np.cross(g, rng.normal(size=(n, 3))))
    ang = rng.uniform(0, np.pi / 6, n) * rng.integers(0, 2, n)  # (half of them: n is g)
    nrm = g * np.cos(ang)[:, None] + np.cross(axis, g) * np.sin(ang)[:, None]
    d = unit(rng.normal(size=(n, 3)))
    d = np.where(((d * g).sum(axis=1) > 0)[:, None], -d, d)
    d = np.where(((d * nrm).sum(axis=1) > 0)[:, None], -g, d) * rng.uniform(0.5, 2.0, n)[:, None]
    rgb = rng.integers(0, 256, (n, 3))
    k = np.arange(n) % 16
    rgb[k == 3, 0:2] = 128
    rgb[k == 7, 2] = rng.integers(0, 129, (k == 7).sum())
    rgb[k > 7, 2] = rng.integers(160, 256, (k > 7).sum())  # (half of them: the steep-but-plausible texels of real maps)
    out[:, 0:3], out[:, 3:6] = f32(Tr), f32(Br)
    out[:, 6] = (rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16)).astype(np.uint32)
    out[:, 7] = f32(rng.uniform(-2.0, 2.0, n))
    out[:, 8:11], out[:, 11:14], out[:, 14:17] = f32(g), f32(nrm), f32(d)
    out[:, 17] = front.astype(np.uint32)
    out.setflags(write=False)
    return out


def statement(rec, T, perturb=()):
    """(n' [n][3], replaced [n]) of every record from ref64_normal_map at dtype T, as float64"""
    Tr, Br = rec[:, 0:3].view(np.float32).astype(T), rec[:, 3:6].view(np.float32).astype(T)
    w = rec[:, 6].astype(np.int64)
    rgb = np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], axis=1)
    s = rec[:, 7].view(np.float32)
    g, nrm, d = (rec[:, a:a + 3].view(np.float32).astype(T) for a in (8, 11, 14))
    front = rec[:, 17] != 0
    xyz, active = NM.decode(rgb, T, perturb)
    nb, ok = NM.normal(nrm, g, d, front, s, Tr, Br, xyz, active, T, perturb)
    return nb.astype(np.float64), ok


def share(got, ref):
    """the share of records with every component within 1e-4 (the project's per-sample tolerance; |n'| = 1)"""
    return float((np.abs(got - ref).max(axis=1) <= 1e-4).mean())
