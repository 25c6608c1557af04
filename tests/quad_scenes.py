"""Scenes of the quads (parallelograms, boxes, rigid transforms) shared by test_quads.py (CPU) and test_gpu_quads.py,
with their triangle twins.

Every per-sample case uses the frame, sample count, seeds and draw budget of nee_scenes.REF_* (48 x 27 pixels x 13 one-sample
frames = 16 848 samples).  A builder called with tri=True builds the case's TWIN: every quad as the two triangles
(Q, Q + u, Q + u + v) and (Q, Q + u + v, Q + v) of the quad the scene stores (a box: of its six stored quads, read back from a
scratch scene, so the twin needs no transform code of its own).  plain_twin() is that twin with light sampling off and its
environment, media and movers cleared: what the plain kernel renders, the baseline of criterion (b).

What was fixed, and why (the fp64 and the fp32 reference were run on the CPU on every case; a case stays only if the fp32
reference alone meets criterion (a) with at most 1 % of the samples flipping a branch -- test_quads.py asserts it):
  * no checker lies on a quad's own plane: checker floors are lifted by nee_scenes.LIFT and the checker box is turned about y by
    an angle that puts none of its faces on a plane of parity;
  * every box stands a little above the floor it is over (BOX_GAP), so that no two surfaces share a plane and no face ends in
    the floor's plane: a tie between a box's bottom and the floor would hang on the last bit of t;
  * the sky case's ground sphere has radius 100, not the series' 1000 (GROUND_R says why);
  * the boxes are turned by angles whose sines and cosines are no short binary fractions, so that camera rays do not run along
    a face; the glass cube is large enough for a few hundred samples to pass through it.
"""
import numpy as np

import ext_scenes as X
import feature_scenes as FS
import media_scenes as MS
import nee_scenes as NS
import ref64 as R

NEE, ENV, MEDIA, MOTION, FAMILIES = FS.NEE, FS.ENV, FS.MEDIA, FS.MOTION, FS.FAMILIES
LIFT = NS.LIFT
BOX_GAP = 0.013
# The ground sphere of the sky case.  The fp32 sphere test's error grows with |o - c|^2: under the series' radius of 1000 a
# scattered ray re-meets the ground it leaves in 0.36 % of the samples at fp32 -- always towards darker, so the fp32 NumPy
# reference itself is biased against fp64 (z = -7.4) and criterion (c) cannot be asked of any fp32 code.  At 100 the error is a
# hundredth of that; the ground falls 0.03 under the boxes furthest out, which stand on BOX_GAP anyway.
GROUND_R = 100.0
QUAD = R.QUAD


class Geo:
    """quad() and box() of a scene, or (tri=True) the same surfaces as triangle pairs"""

    def __init__(self, rtmi, sc, tri):
        self.rtmi, self.sc, self.tri = rtmi, sc, tri

    def _pairs(self, recs, material):
        for p in recs:
            m = p["m"].astype(np.float64)
            Q, u, v = m[0:3], m[3:6], m[6:9]
            a, b, c, d = Q, Q + u, Q + u + v, Q + v
            self.sc.triangle(a, b, c, material, (0, 0), (1, 0), (1, 1))
            self.sc.triangle(a, c, d, material, (0, 0), (1, 1), (0, 1))

    def _scratch(self):
        tmp = self.rtmi.Scene.new(8, 8, 1, 1)
        return tmp, tmp.lambertian((0.5, 0.5, 0.5))

    def quad(self, q, u, v, material, rotate=None, translate=None):
        if not self.tri:
            return self.sc.quad(q, u, v, material, rotate, translate)
        tmp, m = self._scratch()
        tmp.quad(q, u, v, m, rotate, translate)
        self._pairs(tmp.prims(), material)

    def box(self, lo, hi, material, rotate=None, translate=None):
        if not self.tri:
            return self.sc.box(lo, hi, material, rotate, translate)
        tmp, m = self._scratch()
        tmp.box(lo, hi, m, rotate, translate)
        self._pairs(tmp.prims(), material)


def _frame(rtmi, depth=6, sky=False, background=(0.02, 0.02, 0.03), w=NS.REF_W, h=NS.REF_H, spp=1):
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background(background, sky_gradient=sky, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    return sc


def _boxes(sc, g, y=0.0, glass=True):
    """four turned boxes on the level y: lambertian, fuzz-0.3 metal, checker lambertian, and a glass cube"""
    y += BOX_GAP
    g.box((-0.5, 0.0, -0.5), (0.5, 1.6, 0.5), sc.lambertian((0.7, 0.3, 0.2)), rotate=((0, 1, 0), 17.0), translate=(-1.9, y, -0.6))
    g.box((-0.45, 0.0, -0.45), (0.45, 0.9, 0.45), sc.metal((0.8, 0.7, 0.6), 0.3), rotate=((0, 1, 0), -23.0), translate=(1.8, y, -0.3))
    g.box((-0.4, 0.0, -0.4), (0.4, 0.7, 0.4), sc.lambertian(sc.checker_texture((0.8, 0.8, 0.8), (0.1, 0.3, 0.1))),
          rotate=((0, 1, 0), 31.0), translate=(-0.6, y, 1.3))
    if glass:
        g.box((-0.55, 0.0, -0.55), (0.55, 1.1, 0.55), sc.dielectric(1.5), rotate=((0.1, 1, 0.05), 41.0), translate=(0.55, y + 0.05, 0.9))


def sky(rtmi, tri=False):
    """turned boxes of lambertian, metal, checker and a glass cube over a ground sphere, under the sky gradient"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    sc.sphere((0.0, -GROUND_R, 0.0), GROUND_R, sc.lambertian((0.5, 0.5, 0.45)))
    _boxes(sc, Geo(rtmi, sc, tri))
    return sc


def boxes_on_a_floor(rtmi, tri=False):
    """the sky case with a floor quad in place of the ground sphere: every primitive a quad (the ray queries' scene -- a ray that
    grazes a sphere of radius 100 carries an fp32 error in t of its own, which is the sphere test's and not this feature's)"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    g = Geo(rtmi, sc, tri)
    g.quad((-20, 0.0, -20), (0, 0, 40), (40, 0, 0), sc.lambertian((0.5, 0.5, 0.45)))
    _boxes(sc, g)
    return sc


ROOM = (-3.0, 3.0, 0.0, 4.5, -3.0)  # x0, x1, y0, y1, z of the back wall (the room is open towards the camera)


def cornell(rtmi, tri=False, w=NS.REF_W, h=NS.REF_H, spp=1):
    """five walls, a quad light and a rect light under the ceiling, a tall and a short turned box; roulette 0.85"""
    sc = _frame(rtmi, w=w, h=h, spp=spp)
    g = Geo(rtmi, sc, tri)
    x0, x1, y0, y1, z0 = ROOM
    white, red, green = sc.lambertian((0.73, 0.73, 0.73)), sc.lambertian((0.65, 0.05, 0.05)), sc.lambertian((0.12, 0.45, 0.15))
    g.quad((x0, y0, z0), (0, 0, 10), (x1 - x0, 0, 0), white)              # floor, normal +y
    g.quad((x0, y1, z0), (x1 - x0, 0, 0), (0, 0, 10), white)              # ceiling, normal -y
    g.quad((x0, y0, z0), (x1 - x0, 0, 0), (0, y1 - y0, 0), white)         # back, normal +z
    g.quad((x0, y0, z0), (0, y1 - y0, 0), (0, 0, 10), red)                # left, normal +x
    g.quad((x1, y0, z0), (0, 0, 10), (0, y1 - y0, 0), green)              # right, normal -x
    g.quad((-0.8, y1 - 0.02, -0.2), (1.3, 0, 0.3), (-0.2, 0, 1.2), sc.diffuse_light((9.0, 7.5, 6.0)))  # the quad light, skewed
    sc.xz_rect(1.2, 2.0, -1.8, -1.0, y1 - 0.03, sc.diffuse_light((4.0, 5.0, 7.0)))
    g.box((-0.6, 0.0, -0.6), (0.6, 2.4, 0.6), white, rotate=((0, 1, 0), 19.0), translate=(-1.1, BOX_GAP, -1.2))
    g.box((-0.6, 0.0, -0.6), (0.6, 1.2, 0.6), sc.metal((0.8, 0.8, 0.85), 0.3), rotate=((0, 1, 0), -22.0), translate=(1.0, BOX_GAP, 0.6))
    sc.set_russian_roulette(0.85)
    return sc


def textured(rtmi, tri=False):
    """an image-textured leaning quad, a marble-textured box and a bumped floor quad, under the sky gradient"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    g = Geo(rtmi, sc, tri)
    floor = sc.lambertian((0.6, 0.55, 0.5))
    sc.set_bump(floor, sc.noise_texture((0, 0, 0), (1, 1, 1), style="fbm", scale=1.3, octaves=2, seed=31), 0.25)
    g.quad((-20, 0.0, -20), (0, 0, 40), (40, 0, 0), floor)
    # a picture leaning against nothing: turned about x by -25 degrees and about y through its own skew
    g.quad((-1.6, 0.0, -1.0), (2.6, 0.0, 0.5), (0.1, 2.2, -0.9), sc.lambertian(sc.image_texture(X.image(6, 9, 61))),
           rotate=((0, 1, 0), 9.0), translate=(-0.6, BOX_GAP, -0.4))
    marble = sc.lambertian(sc.noise_texture((0.9, 0.88, 0.8), (0.15, 0.2, 0.3), style="marble", scale=3.0, octaves=3, seed=11, axis="y",
                                            distortion=4.0))
    g.box((-0.5, 0.0, -0.5), (0.5, 1.0, 0.5), marble, rotate=((0, 1, 0), 33.0), translate=(1.5, BOX_GAP, 0.9))
    return sc


def env(rtmi, tri=False):
    """the boxes on a checker floor quad under scenes/env_sun.json's map (light sampling on: the caller's)"""
    sc = _frame(rtmi, background=(0.1, 0.2, 0.3))
    g = Geo(rtmi, sc, tri)
    g.quad((-20, LIFT, -20), (0, 0, 40), (40, 0, 0), sc.lambertian(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.4, 0.2))))
    _boxes(sc, g, y=LIFT)
    e, scale, rotate = NS._sun_map()
    sc.set_environment(e, scale, rotate)
    return sc


def fog(rtmi, tri=False):
    """the boxes under a quad emitter, the camera inside thin fog"""
    sc = rtmi.Scene.new(MS.REF_W, MS.REF_H, 1, 6)
    sc.set_background((0.05, 0.06, 0.08), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.6, 0.0), (0, 1, 0), 45.0)
    g = Geo(rtmi, sc, tri)
    g.quad((-20, 0.0, -20), (0, 0, 40), (40, 0, 0), sc.lambertian((0.6, 0.5, 0.4)))
    _boxes(sc, g)
    g.quad((-1.0, 3.5, -1.0), (2.0, 0, 0), (0, 0, 2.0), sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9))
    return sc


def motion(rtmi, tri=False):
    """a mover passing in front of a box and behind the glass cube, under the sky gradient"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0))
    g = Geo(rtmi, sc, tri)
    g.quad((-20, 0.0, -20), (0, 0, 40), (40, 0, 0), sc.lambertian((0.5, 0.5, 0.45)))
    _boxes(sc, g)
    sc.add_moving_sphere((-2.4, 0.56, 0.6), (1.6, 0.56, 0.2), 0.55, sc.lambertian((0.2, 0.4, 0.8)))
    return sc


NESTED_LAYOUT = 52


def nested(rtmi, w=NS.REF_W, h=NS.REF_H):
    """noise_scenes.nested with the clump made of boxes: 48 small turned boxes (288 quads; lambertian, metal and glass) within 0.15
    of a point among 100 small spheres, the nested grid on"""
    sc = rtmi.Scene.new(w, h, 1, 5)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((-1.0, 0.7, 1.9), (-1.0, 0.5, 1.0), (0, 1, 0), 26.0)
    rng = np.random.default_rng(3)
    small = [sc.lambertian((0.7, 0.3, 0.3)), sc.metal((0.8, 0.8, 0.8), 0.15)]
    for k in range(100):
        c = rng.uniform(-4, 4, 3)
        sc.sphere((float(c[0]), float(c[1]), float(c[2])), 0.02, small[k % 2])
    m = [sc.lambertian((0.2, 0.5, 0.8)), sc.metal((0.8, 0.7, 0.6), 0.3), sc.dielectric(1.5)]
    for k in range(48):
        c = np.array((-1.0, 0.5, 1.0)) + rng.uniform(-0.13, 0.13, 3)
        e = rng.uniform(0.012, 0.03, 3)
        sc.box(tuple(-e), tuple(e), m[k % 3], rotate=(tuple(rng.normal(size=3)), float(rng.uniform(0, 90))), translate=tuple(c))
    sc.set_nested_grid(True)
    return sc


# name -> (family bits the kernel must report, builder, light sampling, the tally keys the case is there for)
CASES = {
    "quad_sky": (0, sky, False, ("quad_vertices", "quad_refractions", "quad_back_hits")),
    "quad_cornell": (NEE, cornell, True, ("quad_picks", "other_picks", "quad_shadow_stops", "quad_mis_hits")),
    "quad_textured": (0, textured, False, ("quad_vertices", "image_vertices")),
    "quad_env": (ENV | NEE, env, True, ("quad_vertices", "quad_shadow_stops", "quad_refractions")),
    "quad_fog": (MEDIA, fog, False, ("quad_vertices", "quad_emitter_hits", "medium_events")),
    "quad_motion": (MOTION, motion, False, ("quad_vertices", "mover_then_static", "static_then_mover")),
}
CORNELL = "quad_cornell"
MISTAKES = (("quad_textured", "quad_uv_swapped"), (CORNELL, "quad_light_half_area"), ("quad_sky", "quad_front_flipped"))


family, seed_of, inputs = FS.bindings(CASES.__getitem__)


def scene(rtmi, name, tri=False):
    sc = CASES[name][1](rtmi, tri)
    sc.set_light_sampling(CASES[name][2])
    return sc


def plain_twin(rtmi, name):
    """the two-triangle twin, made plain (feature_scenes.cleared): what the plain kernel renders"""
    return FS.cleared(CASES[name][1](rtmi, True))


def check_contents(name, tally_):
    """the case holds what it is there for, each at least nee_scenes.REQUIRED_EVENTS times (1 % of the samples)"""
    for what in CASES[name][3]:
        assert tally_[what] >= NS.REQUIRED_EVENTS, (name, what, tally_[what])
