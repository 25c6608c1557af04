"""Scenes of the noise textures shared by test_noise.py (CPU) and test_gpu_noise.py, with their solid-colour twins,
and the seeded records of the fp32-against-fp64 check of csrc/rt_noise.h.

Every case uses the frame, sample count, seed and draw budget of nee_scenes.REF_* (48 x 27 pixels x 13 one-sample frames =
16 848 samples; the media and motion cases use their families' seed, as glossy_scenes.py does).  A builder called with
noise=False builds the case's TWIN: every noise texture replaced by the solid colour (c0 + c1) / 2 under the same material --
the geometry the plain kernel is pinned on, the baseline of criterion (b).  The reference of a case and of its twin is ref64.reference.

Together the cases carry fbm, turbulence and marble on lambertian, plastic (r = 0.3 and 0.5: both take light samples; one at
r = 0.02, which takes none) and diffuse_light, one case per render family and one in a nested cell.

What was adjusted, and why (the fp64 and fp32 references were run on the CPU on every case before it was fixed; a case stays
only if the fp32 reference alone meets criterion (a) with at most 1 % of the samples flipping a branch):
  * noise lies on objects within 2.5 units of the origin and on a bounded floor PANEL (|x|, |z| <= 2.4, lifted 0.01 over the
    floor), with scale <= 4 and octaves <= 4: the fp32 statement follows fp64 within 1e-4 there, while at |p| = 20
    a fifth of marble's values would not.  The far floor is solid;
  * no checker anywhere: the cases are about a texture that is continuous in the hit point;
  * noise_nested looks at its clump through 26 degrees where smooth_scenes.nested_scene has 35: at 35 only 10.5 % of the samples
    touched a noise texture, below the 15 % every case must have;
  * noise_env's textures are gentle (two octaves, half the scale, distortion 2, no colour channel below 0.4): a sample that
    picks the sun carries its radiance, far above 1, where the tolerance is RELATIVE (1e-4 |ref|), and a colour of 0.1 with an
    fp32 error of 3e-5 is off by 3e-4 of itself.  With the stage's own textures the fp32 reference alone stood at 99.44 % and the
    kernel at 99.29 %, below the twin's 100 % less the half point of criterion (b); with these the fp32 reference has 99.91 %;
  * the emitter panel's two colours differ by a third, so that its hits vary by more than the tolerance across the panel.
"""
import functools

import numpy as np

import feature_scenes as FS
import media_scenes as MS
import nee_scenes as NS
import ref64_noise as N
import smooth_scenes as SM

NEE, ENV, MEDIA, MOTION, FAMILIES = FS.NEE, FS.ENV, FS.MEDIA, FS.MOTION, FS.FAMILIES
MIN_NOISE_SHARE = 0.15  # of a case's samples touch a noise texture: a mistake can then pull the agreement below 97 %


class _Tex:
    """the noise constructor, or its solid stand-in in a twin"""

    def __init__(self, sc, noise):
        self.sc, self.noise = sc, noise

    def __call__(self, c0, c1, **kw):
        if self.noise:
            return self.sc.noise_texture(c0, c1, **kw)
        return self.sc.solid_color(tuple(0.5 * (a + b) for a, b in zip(c0, c1)))


MARBLE = dict(style="marble", scale=3.0, octaves=4, seed=11, axis="y", distortion=5.0)
TURB = dict(style="turbulence", scale=4.0, octaves=3, seed=5)
FBM = dict(style="fbm", scale=2.0, octaves=4, seed=2023)


def _frame(rtmi, depth=6, sky=False, background=(0.02, 0.02, 0.03), w=NS.REF_W, h=NS.REF_H, spp=1):
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background(background, sky_gradient=sky, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    return sc


def _stage(sc, t, plastic_r=0.3, gentle=False):
    """the far floor (solid), the fbm floor panel, a marble plastic ball and a turbulence lambertian ball.  gentle: two octaves,
    half the scale and distortion, and no colour below 0.4 -- for the case whose samples carry a sun's radiance"""
    k = (lambda d: dict(d, octaves=2, scale=0.5 * d["scale"], **({"distortion": 2.0} if "distortion" in d else {}))) if gentle else (lambda d: d)
    dark = (lambda c: tuple(0.4 + 0.6 * x for x in c)) if gentle else (lambda c: c)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.5, 0.5, 0.45)))
    sc.xz_rect(-2.4, 2.4, -2.4, 2.4, 0.01, sc.lambertian(t(dark((0.15, 0.2, 0.5)), (0.95, 0.9, 0.8), **k(FBM))))
    sc.sphere((-1.1, 0.91, 0.2), 0.9, sc.plastic(t((0.9, 0.88, 0.8), dark((0.15, 0.2, 0.3)), **k(MARBLE)), 1.5, plastic_r))
    sc.sphere((1.1, 0.91, 0.2), 0.9, sc.lambertian(t(dark((0.1, 0.1, 0.1)), (1.0, 0.6, 0.2), **k(TURB))))


def sky(rtmi, noise=True):
    """the stage under the sky gradient, and a small near-mirror (r = 0.02) turbulence plastic ball in front"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    t = _Tex(sc, noise)
    _stage(sc, t)
    sc.sphere((0.0, 0.36, 1.9), 0.35, sc.plastic(t((0.8, 0.2, 0.1), (0.1, 0.3, 0.8), **dict(TURB, seed=6)), 1.5, 0.02))
    return sc


EMITTER_COLOURS = ((1.5, 1.4, 1.2), (2.25, 2.1, 1.8))  # the panel's two colours (the brightest emission of the case is 7.0)


def lights(rtmi, noise=True, w=NS.REF_W, h=NS.REF_H, spp=1):
    """the stage under a rectangle emitter and a sphere emitter, with a marble-mottled emitter panel behind it (an unlisted
    light: a BSDF ray that reaches it keeps full weight); roulette 0.9 (light sampling is switched on by the caller)"""
    sc = _frame(rtmi, w=w, h=h, spp=spp)
    t = _Tex(sc, noise)
    _stage(sc, t, plastic_r=0.5)
    sc.xz_rect(-1.4, 1.4, -0.8, 1.6, 3.2, sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.sphere((2.4, 2.3, 1.0), 0.3, sc.diffuse_light((5.0, 6.0, 7.0)))
    sc.xy_rect(-2.0, 2.0, 0.3, 2.3, -1.6, sc.diffuse_light(t(EMITTER_COLOURS[0], EMITTER_COLOURS[1], style="marble", scale=2.0, octaves=2,
                                                               seed=9, axis="x", distortion=3.0)))
    sc.set_russian_roulette(0.9)
    return sc


def env(rtmi, noise=True):
    """the stage under scenes/env_sun.json's map (the caller switches light sampling on)"""
    sc = _frame(rtmi, background=(0.1, 0.2, 0.3))
    t = _Tex(sc, noise)
    _stage(sc, t, gentle=True)
    e, scale, rotate = NS._sun_map()
    sc.set_environment(e, scale, rotate)
    return sc


def fog(rtmi, noise=True):
    """the stage under an emitter, the camera inside thin fog"""
    sc = rtmi.Scene.new(MS.REF_W, MS.REF_H, 1, 6)
    sc.set_background((0.05, 0.06, 0.08), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.6, 0.0), (0, 1, 0), 45.0)
    t = _Tex(sc, noise)
    _stage(sc, t)
    sc.xz_rect(-1.0, 1.0, -1.0, 1.0, 3.5, sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9))
    return sc


def motion(rtmi, noise=True):
    """a moving sphere carrying an fbm lambertian (the texture swims in world space, as the checker does) in front of the stage"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    t = _Tex(sc, noise)
    _stage(sc, t)
    sc.add_moving_sphere((-1.6, 0.55, 2.2), (1.4, 0.55, 1.6), 0.55, sc.lambertian(t((0.9, 0.9, 0.2), (0.1, 0.5, 0.2), **dict(FBM, scale=4.0, seed=77))))
    return sc


def nested(rtmi, noise=True, w=NS.REF_W, h=NS.REF_H):
    """smooth_scenes.nested_scene with the clump in noise: a 288-triangle smooth sphere of radius 0.15 among 100 small spheres,
    the nested grid on (the reference scans every primitive: 288 keep it to seconds); wedges of 24 triangles in marble plastic, turbulence lambertian and glass"""
    sc = rtmi.Scene.new(w, h, 1, 5)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((-1.0, 0.7, 1.9), (-1.0, 0.5, 1.0), (0, 1, 0), 26.0)
    t = _Tex(sc, noise)
    rng = np.random.default_rng(3)
    small = [sc.lambertian((0.7, 0.3, 0.3)), sc.metal((0.8, 0.8, 0.8), 0.15)]
    for k in range(100):
        c = rng.uniform(-4, 4, 3)
        sc.sphere((float(c[0]), float(c[1]), float(c[2])), 0.02, small[k % 2])
    m = [sc.plastic(t((0.9, 0.88, 0.8), (0.15, 0.2, 0.3), **dict(MARBLE, scale=4.0)), 1.5, 0.3),
         sc.lambertian(t((0.1, 0.1, 0.1), (1.0, 0.6, 0.2), **TURB)), sc.dielectric(1.5)]
    v, n = SM.uv_sphere((-1.0, 0.5, 1.0), 0.15, 10, 16)
    for k in range(len(v)):
        sc.triangle(v[k][0], v[k][1], v[k][2], m[(k // 24) % 3], normals=n[k])
    sc.set_nested_grid(True)
    return sc


# name -> (family bits the kernel must report, builder, light sampling on, the noise_* keys of ref64.tally() it is there for)
CASES = {
    "noise_sky": (0, sky, False, ("noise_lambertian", "noise_plastic")),
    "noise_lights": (NEE, lights, True, ("noise_lambertian", "noise_plastic", "noise_emitter", "noise_plastic_light_samples")),
    "noise_env": (ENV | NEE, env, True, ("noise_lambertian", "noise_plastic", "noise_plastic_light_samples")),
    "noise_fog": (MEDIA, fog, False, ("noise_lambertian", "noise_plastic")),
    "noise_motion": (MOTION, motion, False, ("noise_lambertian", "noise_mover")),
    "noise_nested": (0, nested, False, ("noise_lambertian", "noise_plastic")),
}
NESTED_LAYOUT = 52


family, seed_of, inputs = FS.bindings(CASES.__getitem__)


def scene(rtmi, name, noise=True):
    sc = CASES[name][1](rtmi, noise)
    sc.set_light_sampling(CASES[name][2])
    return sc


def plain_twin(rtmi, name):
    """the solid-colour twin made plain (feature_scenes.cleared): what the plain kernel renders"""
    return FS.cleared(CASES[name][1](rtmi, False))


def check_contents(name, tally):
    """the case met the vertices it is there for, each at least once per hundred samples (nee_scenes.REQUIRED_EVENTS), and at
    least 15 % of its samples touch a noise texture"""
    for what in CASES[name][3]:
        assert tally[what] >= NS.REQUIRED_EVENTS, (name, what, tally[what])
    assert tally["noise_share"] >= MIN_NOISE_SHARE, (name, tally["noise_share"])


# ------------------------------------------------------------------------------------ records of the fp32-against-fp64 check
RECORD_WORDS, OUTPUT_WORDS = 8, 4


@functools.lru_cache(maxsize=None)
def records(style, n=20000, seed=5):
    """[n][8] uint32 (tests/noise_host_driver.cpp): p.xyz uniform in [-2.5, 2.5]^3, scale uniform in [0.5, 4], distortion in
    [0, 6], a random seed, style | axis << 2 | octaves << 4 with 1 to 4 octaves and a random axis, and a zero"""
    rng = np.random.default_rng(seed + 100 * style)
    out = np.zeros((n, RECORD_WORDS), np.uint32)
    out[:, 0:3] = rng.uniform(-2.5, 2.5, (n, 3)).astype(np.float32).view(np.uint32)
    out[:, 3] = rng.uniform(0.5, 4.0, n).astype(np.float32).view(np.uint32)
    out[:, 4] = rng.uniform(0.0, 6.0, n).astype(np.float32).view(np.uint32)
    out[:, 5] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    out[:, 6] = np.uint32(style) | (rng.integers(0, 3, n).astype(np.uint32) << np.uint32(2)) | (rng.integers(1, 5, n).astype(np.uint32) << np.uint32(4))
    out.setflags(write=False)
    return out


def statement(rec, T, perturb=()):
    """the texture's scalar s of every record from ref64_noise at dtype T: [n] float64"""
    p = rec[:, 0:3].view(np.float32)
    scale, dist = rec[:, 3].view(np.float32), rec[:, 4].view(np.float32)
    out = np.zeros(len(rec), np.float64)
    for w in np.unique(rec[:, 6]):  # (style, axis and octaves are one each per call; scale, seed and distortion one per point)
        m = rec[:, 6] == w
        out[m] = N.value(p[m], int(w) & 3, scale[m], (int(w) >> 4) & 15, rec[m, 5], (int(w) >> 2) & 3, dist[m], T, perturb)
    return out


def share(got, ref):
    """ref64.judge's measure: within 1e-4 max(1, |ref|) (s lies in [0, 1]: within 1e-4)"""
    return float((np.abs(got - ref) <= 1e-4 * np.maximum(1.0, np.abs(ref))).mean())
