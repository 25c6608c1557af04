"""Scenes of the glossy materials shared by test_glossy.py (CPU) and test_gpu_glossy.py, with their lambertian
twins, and the seeded records of the fp32-against-fp64 check of csrc/rt_glossy.h.

Every case uses the frame, sample count, seed and draw budget of nee_scenes.REF_* (48 x 27 pixels x 13 one-sample frames =
16 848 samples; the media and motion cases use their families' seed through ext_scenes.seed_of's rule).  Roughnesses are
{0.15, 0.4, 0.8} and one material at 0.02, below the light-sample threshold.  A builder called with glossy=False builds the
case's TWIN: every rough_metal replaced by lambertian(F0) and every plastic by lambertian of its texture -- the geometry the
plain kernel is pinned on, the baseline of criterion (b).  The reference of a case or of its twin is ref64.reference /
ref64.trace on its RefScene, called plainly: glossy_mesh's shading normals come with ref64's hit record.

What was adjusted, and why (the fp64 and fp32 references were run on the CPU on every case before it was fixed; a case stays
only if the fp32 reference alone meets criterion (a) with at most 1 % of the samples flipping a branch):
  * no checker lies on y = 0 (the floor is lifted by nee_scenes.LIFT), as in every other module: the parity flips there with
    the last bit of the hit point;
  * glossy_mesh's spheres are 6 x 8 UV-sphere meshes (80 triangles each) with exact radial vertex normals, so that the shading
    normal leaves the face normal by up to ~20 degrees and grazing camera rays meet faces from below their shading normal
    (the absorbed-by-wo vertices the case is there for); its image textures are small and random, with distinct corner (u, v);
  * glossy_lights keeps its r = 0.02 material on a sphere that sees both emitters, so that near-mirror rays end on them at full
    weight, and sets the roulette to 0.9.
"""
import functools

import numpy as np

import ext_scenes as X
import feature_scenes as FS
import media_scenes as MS
import nee_scenes as NS
import ref64 as R
import ref64_glossy as G
import smooth_scenes as SM

NEE, ENV, MEDIA, MOTION, FAMILIES = FS.NEE, FS.ENV, FS.MEDIA, FS.MOTION, FS.FAMILIES
ROUGHNESSES = (0.15, 0.4, 0.8)
SMOOTH_R = 0.02
LIFT = NS.LIFT


class _Mats:
    """the glossy constructors, or their lambertian stand-ins in a twin"""

    def __init__(self, sc, glossy):
        self.sc, self.glossy = sc, glossy

    def rough(self, f0, r):
        return self.sc.rough_metal(f0, r) if self.glossy else self.sc.lambertian(f0)

    def plastic(self, colour_or_texture, ior, r):
        return self.sc.plastic(colour_or_texture, ior, r) if self.glossy else self.sc.lambertian(colour_or_texture)


def _frame(rtmi, depth=6, sky=False, background=(0.02, 0.02, 0.03), w=NS.REF_W, h=NS.REF_H, spp=1):
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background(background, sky_gradient=sky, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    return sc


def sky(rtmi, glossy=True):
    """rough-metal spheres of three roughnesses and a solid-plastic sphere on a checker-plastic floor, under the sky gradient"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    m = _Mats(sc, glossy)
    sc.xz_rect(-20, 20, -20, 20, LIFT, m.plastic(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.4, 0.2)), 1.5, 0.4))
    for x, r, f0 in ((-2.4, 0.15, (0.95, 0.64, 0.54)), (-0.8, 0.4, (0.91, 0.92, 0.92)), (0.8, 0.8, (1.0, 0.78, 0.34))):
        sc.sphere((x, 0.65 + LIFT, 0.3), 0.6, m.rough(f0, r))
    sc.sphere((2.4, 0.65 + LIFT, 0.3), 0.6, m.plastic((0.7, 0.15, 0.1), 1.5, 0.15))
    sc.sphere((0.0, 0.4 + LIFT, 1.9), 0.35, m.plastic((0.1, 0.3, 0.7), 1.8, 0.8))
    return sc


def _textured_sphere_mesh(sc, centre, radius, mat, rings=6, segs=8, smooth=True):
    """smooth_scenes.uv_sphere with corner (u, v) of each triangle taken from its corners' positions (distinct, asymmetric)"""
    v, n = SM.uv_sphere(centre, radius, rings, segs)
    c = np.asarray(centre, np.float64)
    for k in range(len(v)):
        uv = [((0.37 * (p[0] - c[0]) + 0.11 * (p[2] - c[2])) / radius * 0.5 + 0.5, (0.41 * (p[1] - c[1]) - 0.07 * (p[0] - c[0])) / radius * 0.5 + 0.5)
              for p in v[k].astype(np.float64)]
        sc.triangle(v[k][0], v[k][1], v[k][2], mat, uv[0], uv[1], uv[2], normals=n[k] if smooth else None)


def mesh(rtmi, glossy=True):
    """image-textured plastic and a rough metal on smooth-shaded sphere meshes, an image-textured plastic floor quad pair"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    m = _Mats(sc, glossy)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.55, 0.55, 0.5)))
    _textured_sphere_mesh(sc, (-1.3, 0.95, 0.2), 0.9, m.plastic(sc.image_texture(X.image(5, 7, 51)), 1.5, 0.4))
    _textured_sphere_mesh(sc, (1.3, 0.95, 0.2), 0.9, m.rough((0.9, 0.8, 0.6), 0.15))
    a, b, c, d = (-1.5, 0.04, 1.3), (1.5, 0.04, 1.3), (1.5, 0.04, 3.2), (-1.5, 0.04, 3.2)
    tex = m.plastic(sc.image_texture(X.image(4, 6, 52)), 1.33, 0.8)
    up = np.array([(0.1, 0.99, 0.05), (-0.08, 0.99, 0.06), (0.05, 0.99, -0.1), (-0.06, 0.99, -0.04)])
    up /= np.sqrt((up * up).sum(axis=1))[:, None]
    uv = X.QUAD_UV
    sc.triangle(a, c, b, tex, uv[0], uv[2], uv[1], normals=(up[0], up[2], up[1]))
    sc.triangle(a, d, c, tex, uv[0], uv[3], uv[2], normals=(up[0], up[3], up[2]))
    return sc


def lights(rtmi, glossy=True, w=NS.REF_W, h=NS.REF_H, spp=1):
    """a rectangle and a sphere emitter over glossy spheres of every roughness, a checker-plastic floor and an r = 0.02 sphere;
    roulette 0.9 (light sampling is switched on by the caller)"""
    sc = _frame(rtmi, w=w, h=h, spp=spp)
    m = _Mats(sc, glossy)
    sc.xz_rect(-20, 20, -20, 20, LIFT, m.plastic(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.4, 0.2)), 1.5, 0.4))
    sc.sphere((-2.0, 0.65 + LIFT, 0.4), 0.6, m.rough((0.95, 0.64, 0.54), 0.15))
    sc.sphere((0.0, 0.95 + LIFT, 0.0), 0.9, m.rough((0.9, 0.9, 0.9), SMOOTH_R))
    sc.sphere((1.6, 0.65 + LIFT, 0.6), 0.6, m.plastic((0.7, 0.15, 0.1), 1.5, 0.15))
    sc.sphere((3.0, 0.65 + LIFT, 0.0), 0.6, m.rough((0.91, 0.92, 0.92), 0.8))
    sc.sphere((-0.7, 0.35 + LIFT, 1.9), 0.3, m.plastic((0.2, 0.5, 0.3), 1.5, SMOOTH_R))
    sc.xz_rect(-1.6, 1.6, -1.0, 2.2, 2.6, sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.sphere((2.6, 2.1, 1.2), 0.35, sc.diffuse_light((5.0, 6.0, 7.0)))
    sc.set_russian_roulette(0.9)
    return sc


def env(rtmi, glossy=True):
    """glossy spheres and a plastic floor under scenes/env_sun.json's map (the caller switches light sampling on)"""
    sc = _frame(rtmi, background=(0.1, 0.2, 0.3))
    m = _Mats(sc, glossy)
    sc.xz_rect(-20, 20, -20, 20, LIFT, m.plastic(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.4, 0.2)), 1.5, 0.4))
    sc.sphere((-1.5, 0.65 + LIFT, 0.4), 0.6, m.rough((0.95, 0.64, 0.54), 0.15))
    sc.sphere((0.0, 0.65 + LIFT, 0.0), 0.6, m.rough((0.91, 0.92, 0.92), 0.4))
    sc.sphere((1.5, 0.65 + LIFT, 0.5), 0.6, m.plastic((0.7, 0.15, 0.1), 1.5, 0.8))
    e, scale, rotate = NS._sun_map()
    sc.set_environment(e, scale, rotate)
    return sc


def fog(rtmi, glossy=True):
    """glossy spheres and a plastic floor under an emitter, the camera inside thin fog"""
    sc = rtmi.Scene.new(MS.REF_W, MS.REF_H, 1, 6)
    sc.set_background((0.05, 0.06, 0.08), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.6, 0.0), (0, 1, 0), 45.0)
    m = _Mats(sc, glossy)
    sc.xz_rect(-20, 20, -20, 20, LIFT, m.plastic(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.4, 0.2)), 1.5, 0.4))
    sc.sphere((-1.6, 0.65 + LIFT, 0.4), 0.6, m.rough((0.95, 0.64, 0.54), 0.15))
    sc.sphere((0.0, 0.65 + LIFT, -0.6), 0.6, m.rough((0.91, 0.92, 0.92), 0.8))
    sc.sphere((1.6, 0.65 + LIFT, 0.6), 0.6, m.plastic((0.7, 0.15, 0.1), 1.5, 0.15))
    sc.xz_rect(-1.0, 1.0, -1.0, 1.0, 3.5, sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9))
    return sc


def motion(rtmi, glossy=True):
    """a moving plastic sphere in front of a static rough-metal one, on a lambertian floor under the sky gradient"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    m = _Mats(sc, glossy)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.55, 0.55, 0.5)))
    sc.sphere((0.6, 0.8, -0.4), 0.8, m.rough((0.95, 0.64, 0.54), 0.4))
    sc.sphere((-1.8, 0.5, 0.2), 0.5, m.rough((0.91, 0.92, 0.92), 0.15))
    sc.add_moving_sphere((-2.2, 0.55, 2.2), (1.8, 0.55, 1.4), 0.55, m.plastic((0.2, 0.5, 0.8), 1.5, 0.4))
    return sc


# name -> (family bits the kernel must report, builder, light sampling on, the glossy keys of ref64.tally() it is there for)
CASES = {
    "glossy_sky": (0, sky, False, ("rough_vertices", "coat_vertices", "body_vertices")),
    "glossy_mesh": (0, mesh, False, ("coat_vertices", "body_vertices", "rough_vertices")),
    "glossy_lights": (NEE, lights, True, ("glossy_light_samples", "smooth_glossy_vertices", "smooth_glossy_full_weight_hits",
                                            "absorbed_wi_light_samples", "roulette_losses")),
    "glossy_env": (ENV | NEE, env, True, ("glossy_env_picks", "glossy_escapes_after_light_sample")),
    "glossy_fog": (MEDIA, fog, False, ("medium_then_glossy", "glossy_then_medium")),
    "glossy_motion": (MOTION, motion, False, ("glossy_mover_vertices", "glossy_static_vertices")),
}


family, seed_of, inputs = FS.bindings(CASES.__getitem__)


def scene(rtmi, name, glossy=True):
    sc = CASES[name][1](rtmi, glossy)
    sc.set_light_sampling(CASES[name][2])
    return sc


def plain_twin(rtmi, name):
    """the lambertian twin made plain (feature_scenes.cleared): what the plain kernel renders"""
    return FS.cleared(CASES[name][1](rtmi, False))


def check_contents(name, tally):
    """the case met the vertices it is there for, each at least once per hundred samples (nee_scenes.REQUIRED_EVENTS) -- but the
    absorbed-by-wo vertices of glossy_mesh, which only a grazing ray on a smooth-shaded face makes: at least one, as the case's
    definition asks -- and every roughness it names"""
    for what in CASES[name][3]:
        assert tally[what] >= NS.REQUIRED_EVENTS, (name, what, tally[what])
    if name == "glossy_mesh":
        assert tally["below_vertices"] >= 1 and tally["below_light_samples"] == 0, tally
        assert tally["image_vertices"] >= NS.REQUIRED_EVENTS, tally
    if name == "glossy_sky":
        assert [round(r, 2) for r in tally["roughnesses"]] == [0.15, 0.4, 0.8], tally["roughnesses"]
    if name == "glossy_lights":
        assert tally["smooth_glossy_light_samples"] == 0 and tally["below_light_samples"] == 0, tally
        assert SMOOTH_R in [round(r, 2) for r in tally["roughnesses"]], tally["roughnesses"]


# ------------------------------------------------------------------------------------ records of the fp32-against-fp64 check
RECORD_WORDS, OUTPUT_WORDS = 20, 26


@functools.lru_cache(maxsize=None)
def records(n=20000, seed=5):
    """[n][20] fp32: n.xyz d.xyz alpha F0.rgb r0 rho.rgb ul u1 u2 wl.xyz -- unit normals uniform on the sphere, wo uniform by
    cos(theta) in [0.02, 1] about them (d = -wo scaled to a length in [0.5, 3]), r uniform in [0.05, 1], F0 and rho uniform in
    [0, 1]^3, the coat's index uniform in [1.05, 2.5], the uniforms multiples of 2^-24, wl uniform on the upper hemisphere"""
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.sqrt((nrm * nrm).sum(axis=1))[:, None]).astype(np.float32)
    n64 = nrm.astype(np.float64)
    t1, t2 = G.frame(n64, np.float64)

    def hemisphere(z_min):
        z, ph = rng.uniform(z_min, 1, n), rng.uniform(0, 2 * np.pi, n)
        s = np.sqrt(1 - z * z)
        return (s * np.cos(ph))[:, None] * t1 + (s * np.sin(ph))[:, None] * t2 + z[:, None] * n64
    d = (-hemisphere(0.02) * rng.uniform(0.5, 3, n)[:, None]).astype(np.float32)
    wl = hemisphere(0.0).astype(np.float32)
    alpha = G.alpha_of(rng.uniform(0.05, 1, n).astype(np.float32))
    f0 = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    r0 = G.r0_of(rng.uniform(1.05, 2.5, n).astype(np.float32))
    rho = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    u = rng.integers(0, 2 ** 24, (n, 3)).astype(np.float32) * np.float32(2.0 ** -24)
    out = np.concatenate([nrm, d, alpha[:, None], f0, r0[:, None], rho, u, wl], axis=1).astype(np.float32)
    out.setflags(write=False)
    return out


def statement(rec, T):
    """what tests/glossy_host_driver.cpp writes for the records, from ref64_glossy at dtype T: [n][26] float64"""
    r = rec.astype(T)
    n, d, alpha, f0, r0, rho, ul, u1, u2, wl = (r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7:10], r[:, 10], r[:, 11:14], r[:, 14], r[:, 15],
                                                r[:, 16], r[:, 17:20])
    ud = R._unit(d)
    out = np.zeros((len(r), OUTPUT_WORDS), np.float64)
    for k, (plastic, f) in enumerate(((False, f0), (True, np.repeat(r0[:, None], 3, axis=1)))):
        P = np.full(len(r), plastic)
        wi, at, pdf, below, absorbed, lobe = G.glossy_sample(n, ud, alpha, P, f, rho, ul, u1, u2, T)
        fc, pw = G.glossy_eval(n, ud, alpha, P, f, rho, wl, T)
        o = out[:, 12 * k:]
        o[:, 0] = np.where(below, 1, np.where(absorbed, 2, 0))
        o[:, 1:4], o[:, 4:7], o[:, 7], o[:, 8:11], o[:, 11] = wi, at, pdf, fc, pw
        if plastic:
            o[:, 12] = lobe
    return out


def share(got, ref):
    """ref64.judge's measure on whole records: within 1e-4 max(1, |ref|) in every component"""
    return float((np.abs(got - ref) <= 1e-4 * np.maximum(1.0, np.abs(ref))).all(axis=1).mean())
