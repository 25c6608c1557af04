"""Scenes of rough glass shared by test_glass.py (CPU) and test_gpu_glass.py, with their dielectric twins, and the
seeded records of the fp32-against-fp64 check of csrc/rt_glass.h.

Every case uses the frame, sample count, seed and draw budget of nee_scenes.REF_* (48 x 27 pixels x 13 one-sample frames =
16 848 samples; the media and motion cases use their families' seed, as glossy_scenes does).  A builder called with glass=False
builds the case's TWIN: every rough_glass replaced by dielectric of the same ir -- the precision baseline for refractive paths,
criterion (b).  The reference of a case and of a twin is ref64.reference on its RefScene.

No checker lies on y = 0 (nee_scenes.LIFT).  glass_mesh's torus is a small one made here (12 x 8 quads of two triangles, exact
vertex normals), so that the list-scanning reference stays quick and grazing rays meet faces from below their shading normal.
"""
import functools

import numpy as np

import feature_scenes as FS
import media_scenes as MS
import nee_scenes as NS
import ref64 as R
import ref64_glass as GL
import ref64_glossy as G

NEE, ENV, MEDIA, MOTION, FAMILIES = FS.NEE, FS.ENV, FS.MEDIA, FS.MOTION, FS.FAMILIES
LIFT = NS.LIFT
SMOOTH_R = 0.02
TINT = (0.9, 0.35, 0.15)  # an absorption coefficient per unit length


class _Mats:
    """rough_glass, or dielectric of the same index in a twin"""

    def __init__(self, sc, glass):
        self.sc, self.glass = sc, glass

    def rough_glass(self, ir, r, sigma=None):
        return self.sc.rough_glass(ir, r, sigma) if self.glass else self.sc.dielectric(ir)


def _frame(rtmi, depth=8, sky=False, background=(0.02, 0.02, 0.03), w=NS.REF_W, h=NS.REF_H, spp=1):
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background(background, sky_gradient=sky, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    return sc


def sky(rtmi, glass=True):
    """balls at r = 0.02, 0.1, 0.3 and 0.6, a tinted ball and a tinted box of quads on a checker floor under the sky gradient"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    m = _Mats(sc, glass)
    sc.xz_rect(-20, 20, -20, 20, LIFT, sc.lambertian(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.4, 0.2))))
    for x, r in ((-2.7, SMOOTH_R), (-1.35, 0.1), (0.0, 0.3), (1.35, 0.6)):
        sc.sphere((x, 0.65 + LIFT, 0.0), 0.6, m.rough_glass(1.5, r))
    sc.sphere((2.7, 0.65 + LIFT, 0.0), 0.6, m.rough_glass(1.33, 0.15, TINT))
    sc.box((-0.9, LIFT + 0.01, 1.4), (0.7, 0.8, 2.3), m.rough_glass(1.6, 0.2, (0.2, 0.6, 1.1)), rotate=((0, 1, 0), 25.0))
    return sc


def torus(R0=1.0, r0=0.42, segs=12, sides=8, centre=(0.0, 0.75, 0.2), tilt=35.0):
    """(triangles [n][3][3], vertex normals [n][3][3]) of a torus about the y axis, tilted about x by `tilt` degrees"""
    a = np.radians(tilt)
    rot = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])

    def at(i, j):
        u, v = 2 * np.pi * i / segs, 2 * np.pi * j / sides
        nrm = np.array([np.cos(u) * np.cos(v), np.sin(v), np.sin(u) * np.cos(v)])
        p = np.array([R0 * np.cos(u), 0.0, R0 * np.sin(u)]) + r0 * nrm
        return rot @ p + np.asarray(centre), rot @ nrm
    tris, nrms = [], []
    for i in range(segs):
        for j in range(sides):
            (p00, n00), (p10, n10), (p11, n11), (p01, n01) = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            tris += [(p00, p11, p10), (p00, p01, p11)]
            nrms += [(n00, n11, n10), (n00, n01, n11)]
    return np.array(tris, np.float32), np.array(nrms, np.float32)


def mesh(rtmi, glass=True):
    """a smooth-shaded, bumped, tinted torus over a lambertian floor, under the sky gradient"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    m = _Mats(sc, glass)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.55, 0.55, 0.5)))
    mat = m.rough_glass(1.5, 0.25, (0.5, 0.2, 0.8))
    sc.set_bump(mat, sc.noise_texture((0, 0, 0), (1, 1, 1), "fbm", scale=6.0, octaves=2, seed=11), 0.08)
    v, n = torus()
    for k in range(len(v)):
        sc.triangle(v[k][0], v[k][1], v[k][2], mat, normals=n[k])
    return sc


def lights(rtmi, glass=True, w=NS.REF_W, h=NS.REF_H, spp=1):
    """rough glass at r = 0.02 and 0.3 (one tinted) over a lambertian floor under one small quad light; roulette 0.9 (light
    sampling is switched on by the caller)"""
    sc = _frame(rtmi, w=w, h=h, spp=spp)
    m = _Mats(sc, glass)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.6, 0.55)))
    sc.sphere((-0.9, 1.5, 2.0), 0.9, m.rough_glass(1.5, 0.15, (0.3, 0.1, 0.6)))
    sc.sphere((1.5, 0.9, 0.0), 0.9, m.rough_glass(1.5, SMOOTH_R))
    sc.sphere((-1.9, 0.4, 1.6), 0.4, m.rough_glass(1.7, 0.3))
    # (the light stands behind the tinted ball as the camera sees it: rays refracted out of the ball's far side end on it, the
    #  emitter hits that count at full weight; grazing reflections off the small ball in front of it end on it weighted)
    sc.quad((-2.0, 0.5, 0.45), (1.4, 0.0, 0.0), (0.0, 1.2, 0.0), sc.diffuse_light((14.0, 12.0, 10.0)))
    sc.set_russian_roulette(0.9)
    return sc


def env(rtmi, glass=True):
    """rough glass spheres on a lambertian floor under scenes/env_sun.json's map (the caller switches light sampling on)"""
    sc = _frame(rtmi, background=(0.1, 0.2, 0.3))
    m = _Mats(sc, glass)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.6, 0.55)))
    sc.sphere((-1.4, 0.75, 0.2), 0.75, m.rough_glass(1.5, 0.15))
    sc.sphere((0.3, 0.75, -0.2), 0.75, m.rough_glass(1.5, 0.5, TINT))
    sc.sphere((1.8, 0.5, 0.9), 0.5, m.rough_glass(1.33, SMOOTH_R))
    e, scale, rotate = NS._sun_map()
    sc.set_environment(e, scale, rotate)
    return sc


def fog(rtmi, glass=True):
    """a medium inside a rough glass shell (a sphere and a box of quads), an emitter overhead"""
    sc = rtmi.Scene.new(MS.REF_W, MS.REF_H, 1, 8)
    sc.set_background((0.25, 0.3, 0.4), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.6, 0.0), (0, 1, 0), 45.0)
    m = _Mats(sc, glass)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.6, 0.55)))
    sc.sphere((-1.2, 1.0, 0.0), 1.0, m.rough_glass(1.5, 0.2, (0.15, 0.3, 0.05)))
    sc.add_medium_sphere((-1.2, 1.0, 0.0), 0.9, 1.2, (0.9, 0.9, 0.9))
    sc.box((0.6, 0.02, -0.6), (2.2, 1.4, 0.8), m.rough_glass(1.5, 0.4))
    sc.add_medium_box((0.7, 0.1, -0.5), (2.1, 1.3, 0.7), 0.8, (0.8, 0.85, 0.9))
    sc.xz_rect(-1.0, 1.0, -1.0, 1.0, 3.5, sc.diffuse_light((6.0, 5.0, 4.0)))
    return sc


def motion(rtmi, glass=True):
    """a moving rough-glass sphere in front of a static one, on a lambertian floor under the sky gradient"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    m = _Mats(sc, glass)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.55, 0.55, 0.5)))
    sc.sphere((0.8, 0.8, -0.6), 0.8, m.rough_glass(1.5, 0.4))
    sc.add_moving_sphere((-2.0, 0.6, 1.8), (1.2, 0.6, 1.2), 0.6, m.rough_glass(1.5, 0.2, TINT))
    return sc


# name -> (family bits the kernel must report, builder, light sampling on, the keys of the tally that must be nonzero)
_CORE = ("glass_reflections", "glass_refractions", "glass_tir", "glass_absorbed_reflections")
_COMMON = _CORE + ("glass_absorbed_refractions",)  # (rare: a refracted direction above the surface; glass_lights met none)
CASES = {
    "glass_sky": (0, sky, False, _COMMON + ("glass_tinted_back_hits",)),
    "glass_mesh": (0, mesh, False, _COMMON + ("glass_below_events", "glass_tinted_back_hits")),
    "glass_lights": (NEE, lights, True, _CORE + ("glass_light_samples", "glass_light_evaluations", "glass_tinted_back_hits",
                                                     "glass_full_weight_hits_behind_refraction", "glass_mis_hits_behind_reflection")),
    "glass_env": (ENV | NEE, env, True, _COMMON + ("glass_light_samples", "glass_tinted_back_hits")),
    "glass_fog": (MEDIA, fog, False, _COMMON + ("medium_events", "glass_then_medium", "glass_tinted_back_hits")),
    "glass_motion": (MOTION, motion, False, _COMMON + ("glass_mover_vertices", "glass_tinted_back_hits")),
}
# the case each deliberate mistake is shown on (one that contains the vertices it touches)
MISTAKES = (("glass_sky", "fresnel_draw_last"), ("glass_sky", "g1_for_g2"), ("glass_sky", "eta_from_wrong_side"),
            ("glass_sky", "no_absorption"), ("glass_lights", "refraction_mis_weighted"))


family, seed_of, inputs = FS.bindings(CASES.__getitem__)


def scene(rtmi, name, glass=True):
    sc = CASES[name][1](rtmi, glass)
    sc.set_light_sampling(CASES[name][2])
    return sc


def plain_twin(rtmi, name):
    """the dielectric twin made plain (feature_scenes.cleared): what the plain kernel renders"""
    return FS.cleared(CASES[name][1](rtmi, False))


def check_contents(name, tally):
    """the case holds what it is there for: every count nonzero; no light sample at a vertex below its surface or at r = 0.02"""
    for what in CASES[name][3]:
        assert tally[what] > 0, (name, what, tally[what])
    assert tally["glass_below_light_samples"] == 0, tally
    if name == "glass_sky":
        assert [round(r, 2) for r in tally["glass_roughnesses"]] == [0.02, 0.1, 0.15, 0.2, 0.3, 0.6], tally["glass_roughnesses"]


# ------------------------------------------------------------------------------------ records of the fp32-against-fp64 check
RECORD_WORDS, OUTPUT_WORDS = 20, 16
RECORD_SEED = 5


@functools.lru_cache(maxsize=None)
def records(n=20000, seed=RECORD_SEED):
    """[n][20] fp32: n.xyz d.xyz alpha ir front sigma.rgb dist uf u1 u2 wl.xyz _ -- unit normals uniform on the sphere, wo uniform
    by cos(theta) in [0.02, 1] about them (d = -wo scaled to a length in [0.5, 3]), r uniform in [0, 1], ir in [1.1, 2.4], both
    sides, sigma x dist in [0, 5] per channel, the uniforms multiples of 2^-24, wl uniform on the whole sphere"""
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.sqrt((nrm * nrm).sum(axis=1))[:, None]).astype(np.float32)
    n64 = nrm.astype(np.float64)
    t1, t2 = G.frame(n64, np.float64)

    def about(z):
        ph = rng.uniform(0, 2 * np.pi, n)
        s = np.sqrt(1 - z * z)
        return (s * np.cos(ph))[:, None] * t1 + (s * np.sin(ph))[:, None] * t2 + z[:, None] * n64
    d = (-about(rng.uniform(0.02, 1, n)) * rng.uniform(0.5, 3, n)[:, None]).astype(np.float32)
    wl = about(rng.uniform(-1, 1, n)).astype(np.float32)
    alpha = G.alpha_of(rng.uniform(0, 1, n).astype(np.float32))
    ir = rng.uniform(1.1, 2.4, n).astype(np.float32)
    front = (rng.uniform(0, 1, n) < 0.5).astype(np.float32)
    dist = rng.uniform(0.1, 4, n)
    sigma = rng.uniform(0, 5, (n, 3)) / dist[:, None]
    u = rng.integers(0, 2 ** 24, (n, 3)).astype(np.float32) * np.float32(2.0 ** -24)
    out = np.concatenate([nrm, d, alpha[:, None], ir[:, None], front[:, None], sigma, dist[:, None], u, wl, np.zeros((n, 1))],
                         axis=1).astype(np.float32)
    out.setflags(write=False)
    return out


def statement(rec, T, perturb=()):
    """what tests/glass_host_driver.cpp writes for the records, from ref64_glass at dtype T: [n][16] float64 --
    branch (0 reflected, 1 refracted, 2 absorbed by wo, 3 absorbed by wi), wi.xyz, attenuation.rgb, pdf_b, f cos.rgb, pdf_b(wl),
    Tr.rgb, F at normal incidence"""
    r = rec.astype(T)
    n, d, alpha, ir, front, sigma, dist, uf, u1, u2, wl = (r[:, 0:3], r[:, 3:6], r[:, 6], rec[:, 7], rec[:, 8] != 0, r[:, 9:12], r[:, 12],
                                                           r[:, 13], r[:, 14], r[:, 15], r[:, 16:19])
    ud = R._unit(d)
    eta = GL.eta_of(ir, front, T, perturb)
    tr = np.where(front[:, None], T(1), GL.tint(sigma, dist, T))
    wi, at, pdf, below, absorbed, refl = GL.glass_sample(n, ud, alpha, eta, tr, uf, u1, u2, T, perturb)
    fc, pw = GL.glass_eval(n, ud, alpha, eta, tr, wl, T)
    out = np.zeros((len(r), OUTPUT_WORDS), np.float64)
    out[:, 0] = np.where(below, 2, np.where(absorbed, 3, np.where(refl, 0, 1)))
    out[:, 1:4], out[:, 4:7], out[:, 7], out[:, 8:11], out[:, 11], out[:, 12:15] = wi, at, pdf, fc, pw, tr
    out[:, 15] = GL.fresnel(eta, np.ones(len(r), T))[0]
    return out


def share(got, ref):
    """(share of the records with the same branch that lie within 1e-4 max(1, |ref|) in every component, share whose branch differs)"""
    same = got[:, 0] == ref[:, 0]
    within = (np.abs(got - ref) <= 1e-4 * np.maximum(1.0, np.abs(ref))).all(axis=1)
    return float(within[same].mean()), float(1 - same.mean())
