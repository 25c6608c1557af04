"""Scenes of bump mapping shared by test_bump.py (CPU) and test_gpu_bump.py, with their unbumped twins, the seeded
records of the fp32-against-fp64 check of csrc/rt_noise.h's gradient and bump rule, and the scenes whose packed tables must not
change with the feature.

Every case uses the frame, sample count, seed and draw budget of nee_scenes.REF_* (48 x 27 pixels x 13 one-sample frames =
16 848 samples; the media and motion cases use their families' seed, as glossy_scenes.py and noise_scenes.py do).  A builder
called with bump=False builds the case's TWIN: the same primitives and materials, in the same order, with no bump and without
the height textures -- the baseline of criterion (b), and the scene whose feature buffers and query records a bump must leave
alone.  The reference of a case and of its twin is ref64.reference.

Where fp32 can hold the per-sample tolerance (measured on the CPU with fp32 numpy against fp64): bumped
surfaces lie within 4 units of the origin, every height texture has a scale <= 3 that is no power of two (with one, q = f p is
exact and the error hides) and at most 5 octaves, and |k| <= 0.5.

What was adjusted, and why (the fp64 and fp32 references were run on the CPU on every case before it was fixed; a case stays
only if the fp32 reference alone meets criteria (a) and (b)):
  * the heights are gentle: scale 1.1 to 1.7 and one or two octaves.  The first draft had scale 2.3 to 2.9 and two or three
    octaves, and the fp32 reference alone missed (b) on four cases (bump_sky: 99.25 % of the stable samples against the twin's
    99.98 %; bump_env 97.99 %).  The error is the hit point's: fp32 and fp64 find p about 1e-6 apart, and n' moves by k x the
    Hessian of s x that, where the Hessian grows with scale^2 x 2^octaves (about 440 in the draft, 50 now).  With these heights
    the fp32 reference has 99.75 % (bump_env) to 99.99 % (bump_fog) of the stable samples;
  * turbulence and marble -- whose gradient flips sign with an octave near n_o = 0 -- are used with one octave, on one object
    each; test_bump.py prints the float32 statement's share next to the code's for every style;
  * the bumped floor is a bounded panel, lifted 0.01 over a flat far floor, so that no bumped point lies beyond 4 units.
"""
import functools
import os

import numpy as np

import feature_scenes as FS
import media_scenes as MS
import nee_scenes as NS
import ref64_bump as B
import ref64_noise as N
import smooth_pack_cases as PC
import smooth_scenes as SM

NEE, ENV, MEDIA, MOTION, FAMILIES = FS.NEE, FS.ENV, FS.MEDIA, FS.MOTION, FS.FAMILIES
MIN_BUMP_SHARE = 0.15  # of a case's samples touch a bumped vertex: a mistake can then pull the agreement below 97 %

H_FBM = dict(style="fbm", scale=1.3, octaves=2, seed=31)
H_PEEL = dict(style="fbm", scale=1.7, octaves=1, seed=8)
H_TURB = dict(style="turbulence", scale=1.1, octaves=1, seed=7)
H_MARBLE = dict(style="marble", scale=1.2, octaves=1, seed=3, axis="y", distortion=1.0)
H_RIPPLE = dict(style="fbm", scale=1.4, octaves=2, seed=19)


class _Bump:
    """puts a bump on a material, or -- in a twin -- does nothing; a height texture is made once per parameter set"""

    def __init__(self, sc, on):
        self.sc, self.on, self.made = sc, on, {}

    def __call__(self, material, height, k):
        if self.on:
            key = tuple(sorted(height.items()))
            if key not in self.made:
                self.made[key] = self.sc.noise_texture((0, 0, 0), (1, 1, 1), **height)
            self.sc.set_bump(material, self.made[key], k)
        return material


def _frame(rtmi, depth=6, sky=False, background=(0.02, 0.02, 0.03), w=NS.REF_W, h=NS.REF_H, spp=1):
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background(background, sky_gradient=sky, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    return sc


def _floor(sc, b):
    """the far floor (flat) and the bumped floor panel, lifted 0.01 over it"""
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.5, 0.5, 0.45)))
    sc.xz_rect(-3.4, 3.4, -2.4, 2.4, 0.01, b(sc.lambertian((0.7, 0.65, 0.5)), H_FBM, 0.3))


def _stage(sc, b, rough=0.3):
    """the floor and three bumped balls: hammered rough metal, orange-peel plastic, lambertian"""
    _floor(sc, b)
    sc.sphere((-1.7, 0.81, 0.2), 0.8, b(sc.rough_metal((0.9, 0.7, 0.4), rough), H_TURB, 0.25))
    sc.sphere((0.0, 0.81, 0.2), 0.8, b(sc.plastic((0.8, 0.3, 0.1), 1.5, rough), H_PEEL, 0.1))
    sc.sphere((1.7, 0.81, 0.2), 0.8, b(sc.lambertian((0.3, 0.5, 0.8)), H_FBM, -0.4))


def sky(rtmi, bump=True):
    """bumped lambertian, metal, dielectric, rough-metal and plastic spheres over the bumped panel, under the sky gradient"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    b = _Bump(sc, bump)
    _floor(sc, b)
    x = (-3.0, -1.5, 0.0, 1.5, 3.0)
    sc.sphere((x[0], 0.71, 0.0), 0.7, b(sc.lambertian((0.3, 0.5, 0.8)), H_FBM, 0.4))
    sc.sphere((x[1], 0.71, 0.0), 0.7, b(sc.metal((0.9, 0.9, 0.85), 0.1), H_FBM, -0.2))
    sc.sphere((x[2], 0.71, 0.0), 0.7, b(sc.dielectric(1.5), H_MARBLE, 0.15))
    sc.sphere((x[3], 0.71, 0.0), 0.7, b(sc.rough_metal((0.9, 0.7, 0.4), 0.3), H_TURB, 0.25))
    sc.sphere((x[4], 0.71, 0.0), 0.7, b(sc.plastic((0.8, 0.3, 0.1), 1.5, 0.3), H_PEEL, 0.1))
    return sc


def prims(rtmi, bump=True, w=NS.REF_W, h=NS.REF_H):
    """every primitive type: the bumped rect panel, a bumped metal cylinder, a smooth-shaded mesh ball in bumped plastic and
    lambertian, and a strongly rippled dielectric sheet (k = 0.5) over them that the camera sees from above and the light
    coming back from the floor meets from below: back-face vertices, and grazing ones where a guard keeps n"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0), w=w, h=h)
    b = _Bump(sc, bump)
    _floor(sc, b)
    sc.cylinder(0.4, -0.5, 0.5, b(sc.metal((0.8, 0.8, 0.9), 0.1), H_FBM, 0.3), rotate=((1, 0, 0), 90.0), translate=(1.6, 0.52, 0.0))
    m = [b(sc.plastic((0.2, 0.6, 0.3), 1.5, 0.3), H_PEEL, 0.2), b(sc.lambertian((0.8, 0.4, 0.3)), H_FBM, 0.3)]
    v, n = SM.uv_sphere((-1.2, 0.62, 0.3), 0.6, 6, 8)
    for k in range(len(v)):
        sc.triangle(v[k][0], v[k][1], v[k][2], m[(k // 8) % 2], normals=n[k])
    sc.xz_rect(-2.6, 2.6, -1.2, 2.2, 1.5, b(sc.dielectric(1.33), H_RIPPLE, 0.5))
    return sc


def lights(rtmi, bump=True, w=NS.REF_W, h=NS.REF_H, spp=1):
    """the stage under a rectangle emitter and a sphere emitter; roulette 0.9 (light sampling is switched on by the caller)"""
    sc = _frame(rtmi, w=w, h=h, spp=spp)
    b = _Bump(sc, bump)
    _stage(sc, b, rough=0.5)
    sc.xz_rect(-1.4, 1.4, -0.8, 1.6, 3.2, sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.sphere((2.8, 2.3, 1.0), 0.3, sc.diffuse_light((5.0, 6.0, 7.0)))
    sc.set_russian_roulette(0.9)
    return sc


def env(rtmi, bump=True):
    """the stage under scenes/env_sun.json's map (the caller switches light sampling on)"""
    sc = _frame(rtmi, background=(0.1, 0.2, 0.3))
    b = _Bump(sc, bump)
    _stage(sc, b, rough=0.5)
    e, scale, rotate = NS._sun_map()
    sc.set_environment(e, scale, rotate)
    return sc


def fog(rtmi, bump=True):
    """the stage under an emitter, the camera inside thin fog"""
    sc = rtmi.Scene.new(MS.REF_W, MS.REF_H, 1, 6)
    sc.set_background((0.05, 0.06, 0.08), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.6, 0.0), (0, 1, 0), 45.0)
    b = _Bump(sc, bump)
    _stage(sc, b)
    sc.xz_rect(-1.0, 1.0, -1.0, 1.0, 3.5, sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9))
    return sc


def motion(rtmi, bump=True):
    """the bumped static stage with an unbumped moving sphere in front"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    b = _Bump(sc, bump)
    _stage(sc, b)
    sc.add_moving_sphere((-1.6, 0.55, 2.2), (1.4, 0.55, 1.6), 0.55, sc.lambertian((0.9, 0.9, 0.2)))
    return sc


def nested(rtmi, bump=True, w=NS.REF_W, h=NS.REF_H):
    """noise_scenes.nested's clump with bumps: a 288-triangle smooth sphere of radius 0.15 among 100 small spheres, the nested
    grid on; wedges of 24 triangles in bumped plastic, bumped lambertian and bumped glass (bump_prims itself has no cell that
    nests)"""
    sc = rtmi.Scene.new(w, h, 1, 5)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((-1.0, 0.7, 1.9), (-1.0, 0.5, 1.0), (0, 1, 0), 26.0)
    b = _Bump(sc, bump)
    rng = np.random.default_rng(3)
    small = [sc.lambertian((0.7, 0.3, 0.3)), sc.metal((0.8, 0.8, 0.8), 0.15)]
    for k in range(100):
        c = rng.uniform(-4, 4, 3)
        sc.sphere((float(c[0]), float(c[1]), float(c[2])), 0.02, small[k % 2])
    m = [b(sc.plastic((0.9, 0.88, 0.8), 1.5, 0.3), H_PEEL, 0.2), b(sc.lambertian((1.0, 0.6, 0.2)), H_FBM, 0.3), b(sc.dielectric(1.5), H_RIPPLE, 0.3)]
    v, n = SM.uv_sphere((-1.0, 0.5, 1.0), 0.15, 10, 16)
    for k in range(len(v)):
        sc.triangle(v[k][0], v[k][1], v[k][2], m[(k // 24) % 3], normals=n[k])
    sc.set_nested_grid(True)
    return sc


# name -> (family bits the kernel must report, builder, light sampling on, the bump_* keys of ref64.tally() it is there for)
CASES = {
    "bump_sky": (0, sky, False, ("bump_lambertian", "bump_metal", "bump_dielectric", "bump_rough_metal", "bump_plastic")),
    "bump_prims": (0, prims, False, ("bump_lambertian", "bump_metal", "bump_plastic", "bump_dielectric", "bump_back", "bump_kept")),
    "bump_lights": (NEE, lights, True, ("bump_lambertian", "bump_rough_metal", "bump_plastic", "bump_light_samples")),
    "bump_env": (ENV | NEE, env, True, ("bump_lambertian", "bump_rough_metal", "bump_plastic", "bump_light_samples")),
    "bump_fog": (MEDIA, fog, False, ("bump_lambertian", "bump_rough_metal", "bump_plastic")),
    "bump_motion": (MOTION, motion, False, ("bump_lambertian", "bump_rough_metal", "bump_plastic")),
}
# the deliberate mistakes of the bump (ref64_bump.PERTURBATIONS), each on the case that exercises it
MISTAKES = (("bump_sky", "bump_off"), ("bump_sky", "bump_full_gradient"), ("bump_prims", "bump_back_unsigned"),
            ("bump_sky", "bump_cubic_fade_derivative"))


family, seed_of, inputs = FS.bindings(CASES.__getitem__)


def scene(rtmi, name, bump=True):
    sc = CASES[name][1](rtmi, bump)
    sc.set_light_sampling(CASES[name][2])
    return sc


def plain_twin(rtmi, name):
    """the unbumped twin made plain (feature_scenes.cleared): what the plain kernel renders"""
    return FS.cleared(CASES[name][1](rtmi, False))


def check_contents(name, tally):
    """the case met the vertices it is there for, each at least once per hundred samples (nee_scenes.REQUIRED_EVENTS), and at
    least 15 % of its samples touch a bumped vertex"""
    for what in CASES[name][3]:
        assert tally[what] >= NS.REQUIRED_EVENTS, (name, what, tally[what])
    assert tally["bump_share"] >= MIN_BUMP_SHARE, (name, tally["bump_share"])


# ------------------------------------------------------------------------------------ the packed tables a bump must not move
SHIPPED_BEFORE = ("env_sun", "fog_room", "glossy_balls", "marble_hall", "mesh_light", "mixed_emissive", "motion_balls", "smooth_mesh",
                  "three_sphere")


def digest_cases(rtmi, scenes_dir, tmp):
    """name -> builder: every scene shipped before the feature and every case of smooth_pack_cases.py
    (tests/golden/bump_off_pack_digests.json was written from these by the commit before the feature)"""
    out = {"shipped " + n: (lambda n=n: rtmi.Scene.load(os.path.join(scenes_dir, n + ".json"))) for n in SHIPPED_BEFORE}
    for name, build in PC.cases(rtmi, scenes_dir, tmp).items():
        out["pack " + name] = build
    return out


digest = PC.digest

# ------------------------------------------------------------------------------------ records of the fp32-against-fp64 check
RECORD_WORDS, OUTPUT_WORDS = 16, 8


@functools.lru_cache(maxsize=None)
def records(style, n=20000, seed=5):
    """[n][16] uint32 (tests/bump_host_driver.cpp): p.xyz uniform within 4 units of the origin ([-2.3, 2.3]^3), scale uniform in
    [0.6, 3] (a power of two has measure zero), distortion in [0, 3], a random seed, style | axis << 2 | octaves << 4 with 1 to
    5 octaves (turbulence and marble: 1 or 2) and a random axis, k uniform in [-0.5, 0.5], a unit normal uniform on the sphere, a
    direction d with d . n < 0 (uniform in that hemisphere, length in [0.5, 2]), front (both sides equally often), and a zero"""
    rng = np.random.default_rng(seed + 100 * style)
    out = np.zeros((n, RECORD_WORDS), np.uint32)
    f32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    out[:, 0:3] = f32(rng.uniform(-2.3, 2.3, (n, 3)))
    out[:, 3] = f32(rng.uniform(0.6, 3.0, n))
    out[:, 4] = f32(rng.uniform(0.0, 3.0, n))
    out[:, 5] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    octaves = rng.integers(1, 6 if style == N.FBM else 3, n).astype(np.uint32)
    out[:, 6] = np.uint32(style) | (rng.integers(0, 3, n).astype(np.uint32) << np.uint32(2)) | (octaves << np.uint32(4))
    out[:, 7] = f32(rng.uniform(-0.5, 0.5, n))
    nrm = rng.normal(size=(n, 3))
    nrm /= np.sqrt((nrm * nrm).sum(axis=1))[:, None]
    nrm = nrm.astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    d = np.where(((d * nrm).sum(axis=1) > 0)[:, None], -d, d) * rng.uniform(0.5, 2.0, n)[:, None]
    out[:, 8:11], out[:, 11:14] = f32(nrm), f32(d)
    out[:, 14] = rng.integers(0, 2, n).astype(np.uint32)
    out.setflags(write=False)
    return out


def statement(rec, T, perturb=()):
    """(grad s [n][3], n' [n][3], accepted [n]) of every record from ref64_bump at dtype T, as float64"""
    p = rec[:, 0:3].view(np.float32)
    scale, dist, k = rec[:, 3].view(np.float32), rec[:, 4].view(np.float32), rec[:, 7].view(np.float32)
    nrm, d = rec[:, 8:11].view(np.float32).astype(T), rec[:, 11:14].view(np.float32).astype(T)
    front = rec[:, 14] != 0
    G = np.zeros((len(rec), 3), T)
    for w in np.unique(rec[:, 6]):  # (style, axis and octaves are one each per call; scale, seed and distortion one per point)
        m = rec[:, 6] == w
        G[m] = B.value_gradient(p[m], int(w) & 3, scale[m], (int(w) >> 4) & 15, rec[m, 5], (int(w) >> 2) & 3, dist[m], T, perturb)
    nb, ok = B.bump(nrm, nrm, d, front, k, G, T, perturb)
    return G.astype(np.float64), nb.astype(np.float64), ok


def share(got, ref):
    """the share of records with every component within 1e-4 (the project's per-sample tolerance; |n'| = 1)"""
    return float((np.abs(got - ref).max(axis=1) <= 1e-4).mean())
