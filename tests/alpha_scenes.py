"""Scenes of alpha cutouts shared by test_alpha.py (CPU) and test_gpu_alpha.py, with their twins.

Every case uses the frame, sample count, seed and draw budget of nee_scenes.REF_* (48 x 27 pixels x 13 one-sample frames =
16 848 samples; the motion case uses its family's seed, as normal_map_scenes.py does).  A builder takes `masks`:
    True       the case: every mask set
    False      the TWIN: the same primitives, materials and image textures (alpha planes included), no mask set
    "opaque"   every mask's plane all 255: no hit is a hole, the frame is the twin's
    "clear"    every mask's plane all 0: every masked hit is a hole
    "deleted"  the primitives whose material would carry a mask are left out (what "clear" must look like)
Primitives that carry a mask go in through _Mask.add, which is what "deleted" leaves out.

All images are made in memory and tiny, 2 x 2 to 8 x 8 texels plus one 1 x 1: nearest-texel lookup makes a sample flip where
the fp32 and the fp64 (u, v) fall on different texels, and a coarse mask has few edges to straddle.  The masks cover about half
of their surface.  Each case's conditions (check_contents) are asserted from the reference's tally alone.
"""
import numpy as np

import feature_scenes as FS
import nee_scenes as NS
import ref64 as R

NEE, ENV, MEDIA, MOTION, FAMILIES = FS.NEE, FS.ENV, FS.MEDIA, FS.MOTION, FS.FAMILIES
MIN_MASKED_SHARE = 0.15   # of a case's samples meet a masked hit
MIN_VERDICT_SHARE = 0.05  # of the masked hits are passes, and as many are opaque
MIN_SHADOW_THROUGH = 500  # shadow queries through a hole, in the cases with light sampling


def checker(rows, cols, block=1, lo=0, hi=255, phase=0):
    """[rows][cols] uint8 alpha: blocks of block x block texels, lo and hi alternating"""
    r, c = np.meshgrid(np.arange(rows) // block, np.arange(cols) // block, indexing="ij")
    return np.where((r + c + phase) % 2 == 0, lo, hi).astype(np.uint8)


def bars(rows, cols, along_rows=True, lo=0, hi=255):
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return np.where((r if along_rows else c) % 2 == 0, lo, hi).astype(np.uint8)


# name -> alpha plane.  "edge": bytes on both sides of the default cutoff byte 128 (127 is a hole, 128 is not)
PLANES = {
    "checker4": checker(4, 4),
    "blocks8": checker(8, 8, block=2),
    "two": checker(2, 2),
    "bars": bars(4, 8, along_rows=False),
    "rows": bars(6, 3, along_rows=True),
    "edge": np.where(checker(4, 4) == 0, 127, 128).astype(np.uint8),
    "lattice": checker(8, 8, phase=1),
    "one": np.array([[100]], np.uint8),
}


def colours(plane, a=(60, 140, 50), b=(200, 180, 90)):
    """[rows][cols][3] uint8: a two-colour image of the plane's size (the base colour an RGBA leaf would carry)"""
    rows, cols = plane.shape
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return np.where(((r + 2 * c) % 3 == 0)[..., None], np.array(a, np.uint8), np.array(b, np.uint8)).astype(np.uint8)


class _Mask:
    """makes the RGBA image textures and puts masks on materials (see the module's text for `masks`)"""

    def __init__(self, sc, masks):
        self.sc, self.masks, self.made, self.masked = sc, masks, {}, set()

    def texture(self, plane):
        """the image texture of a plane, made once in the order of first use, in every mode"""
        if plane not in self.made:
            a = PLANES[plane]
            if self.masks == "opaque":
                a = np.full_like(a, 255)
            elif self.masks == "clear":
                a = np.zeros_like(a)
            self.made[plane] = self.sc.image_texture(colours(PLANES[plane]), alpha=a)
        return self.made[plane]

    def __call__(self, material, plane, cutoff=0.5):
        t = self.texture(plane)
        self.masked.add(material)
        if self.masks and self.masks != "deleted":
            self.sc.set_alpha(material, t, cutoff)
        return material

    def add(self, place, material):
        """place(material) adds a primitive; "deleted" leaves out those whose material carries a mask"""
        if not (self.masks == "deleted" and material in self.masked):
            place(material)


def _frame(rtmi, depth=6, sky=False, background=(0.02, 0.02, 0.03), w=NS.REF_W, h=NS.REF_H, spp=1):
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background(background, sky_gradient=sky, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.8, 0.0), (0, 1, 0), 45.0)
    return sc


def sky(rtmi, masks=True, w=NS.REF_W, h=NS.REF_H):
    """masked lambertian (its own RGBA image as base colour), metal, dielectric and plastic spheres, a standing rectangle, a
    cylinder and a quad under the sky gradient; the big lambertian sphere is seen into through its holes (back-face hits)"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0), w=w, h=h)
    b = _Mask(sc, masks)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.5, 0.5, 0.45)))
    leaf = b(sc.lambertian(b.texture("blocks8")), "blocks8")
    b.add(lambda m: sc.sphere((0.0, 1.0, 0.0), 1.0, m), leaf)
    b.add(lambda m: sc.sphere((-2.4, 0.7, 0.8), 0.7, m), b(sc.metal((0.9, 0.9, 0.85), 0.1), "checker4"))
    b.add(lambda m: sc.sphere((2.4, 0.7, 0.8), 0.7, m), b(sc.dielectric(1.5), "two"))
    b.add(lambda m: sc.sphere((-1.1, 0.45, 2.2), 0.45, m), b(sc.plastic((0.8, 0.3, 0.1), 1.5, 0.3), "edge"))
    b.add(lambda m: sc.xy_rect(-3.6, -1.2, 0.0, 2.4, -1.6, m), b(sc.lambertian((0.8, 0.4, 0.3)), "bars"))
    b.add(lambda m: sc.cylinder(0.4, -0.7, 0.7, m, rotate=((1, 0, 0), 90.0), translate=(1.2, 0.72, 2.0)),
          b(sc.rough_metal((0.9, 0.7, 0.4), 0.3), "rows"))
    b.add(lambda m: sc.quad((1.2, 0.02, -1.8), (2.6, 0.0, 0.5), (0.0, 2.2, -0.2), m), b(sc.pbr((0.3, 0.5, 0.8), 0.2, 0.5), "lattice"))
    b.add(lambda m: sc.sphere((0.9, 0.25, 3.0), 0.25, m), b(sc.lambertian((0.9, 0.1, 0.1)), "one"))  # (a8 = 100 < 128: never seen)
    return sc


def layers(rtmi, masks=True, w=NS.REF_W, h=NS.REF_H):
    """three parallel masked quads and a masked triangle pair with vt in front of a wall: several passes in one query"""
    sc = _frame(rtmi, sky=True, background=(0.0, 0.0, 0.0), w=w, h=h)
    b = _Mask(sc, masks)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.5, 0.5, 0.45)))
    sc.xy_rect(-6, 6, 0.0, 5.0, -2.5, sc.lambertian((0.7, 0.6, 0.4)))
    mats = [b(sc.lambertian((0.2, 0.6, 0.3)), "checker4"), b(sc.plastic((0.7, 0.2, 0.2), 1.5, 0.4), "blocks8"),
            b(sc.lambertian((0.3, 0.3, 0.8)), "lattice")]
    for k, m in enumerate(mats):
        z = 1.6 - 1.1 * k
        b.add(lambda mm, z=z: sc.quad((-2.6, 0.05, z), (5.2, 0.0, 0.0), (0.0, 2.6, 0.0), mm), m)
    tm = b(sc.metal((0.85, 0.85, 0.9), 0.15), "bars")
    v = [(-2.0, 0.1, 2.6), (2.0, 0.1, 2.6), (2.0, 1.7, 2.6), (-2.0, 1.7, 2.6)]
    b.add(lambda mm: sc.triangle(v[0], v[1], v[2], mm, (0.0, 0.0), (1.0, 0.0), (1.0, 1.0)), tm)
    b.add(lambda mm: sc.triangle(v[0], v[2], v[3], mm, (0.0, 0.0), (1.0, 1.0), (0.0, 1.0)), tm)
    return sc


def _fence_stage(sc, b):
    """receivers -- a floor, a lambertian and a plastic ball -- behind a masked fence quad and under a masked canopy"""
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.6, 0.55)))
    sc.sphere((-1.0, 0.6, -0.4), 0.6, sc.lambertian((0.3, 0.5, 0.8)))
    sc.sphere((1.1, 0.5, 0.2), 0.5, sc.plastic((0.8, 0.3, 0.1), 1.5, 0.4))
    b.add(lambda m: sc.quad((-2.8, 0.0, 1.2), (5.6, 0.0, 0.0), (0.0, 2.0, 0.0), m), b(sc.lambertian((0.5, 0.5, 0.5)), "lattice"))
    b.add(lambda m: sc.quad((-2.6, 1.9, -1.8), (5.2, 0.0, 0.0), (0.0, 0.0, 3.4), m), b(sc.rough_metal((0.8, 0.8, 0.8), 0.5), "blocks8"))


def lights(rtmi, masks=True, w=NS.REF_W, h=NS.REF_H, spp=1):
    """the fence stage between a small quad light above the canopy, a point light in front of the fence, and the receivers;
    roulette 0.9 (light sampling is switched on by the caller)"""
    sc = _frame(rtmi, w=w, h=h, spp=spp)
    b = _Mask(sc, masks)
    _fence_stage(sc, b)
    sc.quad((-0.6, 3.4, -0.6), (1.2, 0.0, 0.0), (0.0, 0.0, 1.2), sc.diffuse_light((14.0, 12.0, 10.0)))
    sc.point_light((0.5, 1.2, 3.4), (5.0, 6.0, 7.0))
    sc.set_russian_roulette(0.9)
    return sc


def env(rtmi, masks=True):
    """the fence stage under scenes/env_sun.json's map (the caller switches light sampling on)"""
    sc = _frame(rtmi, background=(0.1, 0.2, 0.3))
    b = _Mask(sc, masks)
    _fence_stage(sc, b)
    e, scale, rotate = NS._sun_map()
    sc.set_environment(e, scale, rotate)
    return sc


def motion(rtmi, masks=True):
    """masked static primitives (sky's) beside two unmasked moving spheres"""
    sc = sky(rtmi, masks)
    sc.add_moving_sphere((-1.6, 0.55, 3.2), (1.4, 0.55, 2.8), 0.4, sc.lambertian((0.9, 0.9, 0.2)))
    sc.add_moving_sphere((2.0, 2.2, 0.0), (2.3, 1.8, 0.4), 0.35, sc.metal((0.8, 0.8, 0.8), 0.2))
    return sc


def nested(rtmi, masks=True, w=NS.REF_W, h=NS.REF_H):
    """a masked clump in a room: a 288-triangle sphere of radius 0.15 with vt among 100 small spheres, the nested grid on;
    wedges of 24 triangles in masked plastic, lambertian and metal"""
    import normal_map_scenes as NMS
    sc = rtmi.Scene.new(w, h, 1, 5)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((-1.0, 0.7, 1.9), (-1.0, 0.5, 1.0), (0, 1, 0), 26.0)
    b = _Mask(sc, masks)
    rng = np.random.default_rng(3)
    small = [sc.lambertian((0.7, 0.3, 0.3)), sc.metal((0.8, 0.8, 0.8), 0.15)]
    for k in range(100):
        c = rng.uniform(-4, 4, 3)
        sc.sphere((float(c[0]), float(c[1]), float(c[2])), 0.02, small[k % 2])
    m = [b(sc.plastic((0.9, 0.88, 0.8), 1.5, 0.3), "blocks8"), b(sc.lambertian((1.0, 0.6, 0.2)), "checker4"), b(sc.metal((0.8, 0.8, 0.9), 0.1), "lattice")]
    if masks != "deleted":
        NMS._mesh(sc, (-1.0, 0.5, 1.0), 0.15, 10, 16, m, smooth=False, every=24)
    sc.set_nested_grid(True)
    return sc


def stack(rtmi, n=70, masks=True):
    """n stacked all-transparent masked quads, each of its own colour, in front of a white wall, seen head-on: the query of the
    centre pixel passes through 64 of them and the 65th is opaque (the cap)"""
    sc = rtmi.Scene.new(9, 9, 1, 2)
    sc.set_background((1.0, 1.0, 1.0), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 0.0, 10.0), (0.0, 0.0, 0.0), (0, 1, 0), 20.0)
    clear = sc.image_texture(np.zeros((2, 2, 3), np.uint8), alpha=np.zeros((2, 2), np.uint8))
    sc.xy_rect(-5, 5, -5, 5, -8.0, sc.lambertian(STACK_WALL))
    for k in range(n):
        m = sc.lambertian(stack_colour(k))
        if masks:
            sc.set_alpha(m, clear, 0.5)
        sc.quad((-4.0, -4.0, 4.0 - 0.1 * k), (8.0, 0.0, 0.0), (0.0, 8.0, 0.0), m)
    return sc


STACK_WALL = (0.3, 0.3, 0.3)


def stack_colour(k):
    return (0.1 + 0.01 * k, 0.9 - 0.01 * k, 0.5)


# name -> (family bits the kernel must report, builder, light sampling on)
CASES = {
    "al_sky": (0, sky, False),
    "al_layers": (0, layers, False),
    "al_lights": (NEE, lights, True),
    "al_env": (ENV | NEE, env, True),
    "al_motion": (MOTION, motion, False),
}
# the deliberate mistakes (ref64.trace's al_* names), each on the case that exercises it
MISTAKES = (("al_sky", "al_off"), ("al_sky", "al_inverted"), ("al_sky", "al_uv_swapped"), ("al_lights", "al_shadow_opaque"),
            ("al_layers", "al_counts_bounce"))


family, seed_of, inputs = FS.bindings(CASES.__getitem__)


def scene(rtmi, name, masks=True):
    sc = CASES[name][1](rtmi, masks)
    sc.set_light_sampling(CASES[name][2])
    return sc


def plain_twin(rtmi, name):
    """the twin without masks, made plain (feature_scenes.cleared): what the plain
    kernel renders"""
    return FS.cleared(CASES[name][1](rtmi, False))


def nested_tally(rtmi):
    """the reference's alpha tally of the nested clump (the reference scans the lists: the grid, nested or flat, is the
    kernels' business), on the case's 48 x 27 x 13 samples"""
    words = R.uniforms(rtmi, NS.REF_SEED, NS.REF_W, NS.REF_H, 0, NS.REF_K, NS.REF_DRAWS)
    return R.reference(R.RefScene(nested(rtmi)), words)[3]


def check_contents(name, tally):
    """the case's conditions, from the reference's tally (ref64.tally's alpha_* keys) alone"""
    assert tally["alpha_masked_share"] >= MIN_MASKED_SHARE, (name, tally["alpha_masked_share"])
    assert tally["alpha_pass_share"] >= MIN_VERDICT_SHARE, (name, tally["alpha_pass_share"])
    assert tally["alpha_opaque_share"] >= MIN_VERDICT_SHARE, (name, tally["alpha_opaque_share"])
    if name == "al_layers":
        assert tally["alpha_max_passes"] >= 2, (name, tally["alpha_max_passes"])
    if name in ("al_lights", "al_env"):
        assert tally["alpha_shadow_through"] >= MIN_SHADOW_THROUGH, (name, tally["alpha_shadow_through"])
