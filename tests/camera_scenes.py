"""Scenes of the camera projections shared by test_camera.py (CPU) and test_gpu_camera.py, with their twins.

Every case uses the frame, sample count, seed and draw budget of nee_scenes.REF_* (48 x 27 pixels x 13 one-sample frames =
16 848 samples; the media and motion cases use their families' seed).  27 rows are no multiple of the 8 x 8 tile, and at
a = 16 / 9 most of a fisheye frame's columns lie outside the image circle.  One modest room -- a floor, a back wall, side
walls, a ceiling light, balls of four materials around the camera -- seen through each projection; a builder takes
`projection`: True the case's own, False the TWIN, the same scene with the perspective projection.

A projection is no part of ref64.RefScene: the reference of a case is ref64_camera's (reference(rtmi, name) below).  Each
case's conditions (check_contents) are asserted from that reference's tally["camera"] alone.
"""
import numpy as np

import feature_scenes as FS
import nee_scenes as NS
import ref64 as R
import ref64_camera as RC

NEE, ENV, MEDIA, MOTION, FAMILIES = FS.NEE, FS.ENV, FS.MEDIA, FS.MOTION, FS.FAMILIES
MIN_SIDE = 200     # fisheye: samples on either side of r = 1
MIN_CENTRE = 10    # fisheye: samples with r < 0.05
MIN_POLE = 20      # panorama: samples within 2 degrees of either pole
MIN_SEAM = 20      # panorama: samples within 2 degrees of the seam, on either side


def _room(rtmi, lookfrom=(0.0, 1.2, 0.5), lookat=(0.0, 1.1, -2.0), depth=6, blur=False, aperture=0.0, focus=0.0, light=True,
          background=(0.03, 0.03, 0.04), sky=False):
    """the room: 8 x 4 x 8 around the origin, the camera inside it; objects on every side, so that a panorama sees some"""
    sc = rtmi.Scene.new(NS.REF_W, NS.REF_H, 1, depth)
    sc.set_background(background, sky_gradient=sky, defocus_blur=blur)
    sc.camera(lookfrom, lookat, (0, 1, 0), 60.0, 0.0, aperture, focus)
    grey, red, green = sc.lambertian((0.6, 0.6, 0.55)), sc.lambertian((0.7, 0.25, 0.2)), sc.lambertian((0.25, 0.6, 0.3))
    sc.xz_rect(-4, 4, -4, 4, 0.0, grey)
    sc.xy_rect(-4, 4, 0, 4, -4.0, sc.lambertian(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.3, 0.6))))
    sc.yz_rect(0, 4, -4, 4, -4.0, red)
    sc.yz_rect(0, 4, -4, 4, 4.0, green)
    sc.sphere((-1.4, 0.6, -2.2), 0.6, sc.lambertian((0.3, 0.5, 0.8)))
    sc.sphere((1.3, 0.5, -1.6), 0.5, sc.metal((0.85, 0.85, 0.8), 0.1))
    sc.sphere((0.2, 0.4, -2.9), 0.4, sc.dielectric(1.5))
    sc.sphere((2.2, 0.7, 1.4), 0.7, sc.plastic((0.8, 0.3, 0.1), 1.5, 0.3))
    sc.sphere((-2.0, 0.5, 2.0), 0.5, sc.lambertian((0.8, 0.7, 0.2)))
    sc.quad((-0.8, 0.0, 2.8), (1.6, 0.0, 0.0), (0.0, 1.5, 0.3), sc.lambertian((0.5, 0.3, 0.6)))
    if light:
        sc.xz_rect(-1.0, 1.0, -2.0, 0.0, 3.9, sc.diffuse_light((9.0, 8.5, 8.0)))
    return sc


def _project(sc, projection, kind, *params):
    if projection:
        sc.set_projection(kind, *params)
    return sc


def ortho_plain(rtmi, projection=True):
    """an elevation of the room's far half from outside the light's reach: parallel rays, 5.4 world units high"""
    return _project(_room(rtmi, (0.4, 1.5, 3.0), (0.2, 1.3, -2.0), sky=True, background=(0.0, 0.0, 0.0)), projection, "orthographic", 5.4)


def ortho_blur(rtmi, projection=True):
    """the same elevation through a wide lens focused on the balls' depth: the far wall is out of focus"""
    return _project(_room(rtmi, (0.4, 1.5, 3.0), (0.2, 1.3, -2.0), blur=True, aperture=0.5, focus=5.0, sky=True, background=(0.0, 0.0, 0.0)),
                    projection, "orthographic", 5.4)


def pano_nee(rtmi, projection=True):
    """the whole room from its middle, lit by the ceiling light (light sampling on, roulette 0.9)"""
    sc = _room(rtmi)
    sc.set_russian_roulette(0.9)
    return _project(sc, projection, "panoramic")


def pano_fog(rtmi, projection=True):
    """the room under the sky gradient with a ball of fog in front of the camera and a thin haze box (media)"""
    sc = _room(rtmi, light=False, sky=True, background=(0.0, 0.0, 0.0))
    sc.add_medium_sphere((0.0, 1.0, -1.6), 0.9, 0.8, (0.9, 0.9, 0.95))
    sc.add_medium_box((-3.9, 0.05, 0.8), (3.9, 2.5, 3.9), 0.15, (0.8, 0.85, 0.9))
    return _project(sc, projection, "panoramic")


def fisheye_env(rtmi, projection=True):
    """a 180 degree dome shot: the room without its light, open to scenes/env_sun.json's map"""
    sc = _room(rtmi, (0.0, 0.4, 1.0), (0.0, 2.0, -0.5), light=False, background=(0.1, 0.2, 0.3))
    e, scale, rotate = NS._sun_map()
    sc.set_environment(e, scale, rotate)
    return _project(sc, projection, "fisheye", 180.0)


def fisheye_blur_nee(rtmi, projection=True):
    """220 degrees -- the rim looks backwards -- through a lens, light sampling on"""
    sc = _room(rtmi, blur=True, aperture=0.3, focus=2.5)
    sc.set_russian_roulette(0.9)
    return _project(sc, projection, "fisheye", 220.0)


def pano_motion(rtmi, projection=True):
    """the panorama with two balls on the move, one of them across the seam behind the camera"""
    sc = _room(rtmi, sky=True, background=(0.0, 0.0, 0.0), light=False)
    sc.add_moving_sphere((-0.9, 0.9, -1.4), (0.7, 1.1, -1.2), 0.35, sc.lambertian((0.9, 0.9, 0.2)))
    sc.add_moving_sphere((-0.5, 1.3, 2.4), (0.6, 1.2, 2.2), 0.4, sc.metal((0.8, 0.8, 0.8), 0.2))
    return _project(sc, projection, "panoramic")


def ortho_nested(rtmi, projection=True):
    """a plan view of a clump of 300 small balls on the floor, the nested grid on (layout 52)"""
    sc = rtmi.Scene.new(NS.REF_W, NS.REF_H, 1, 3)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((0.3, 6.0, 0.2), (0.3, 0.0, 0.1), (0, 0, -1), 30.0)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.5, 0.5, 0.45)))
    rng = np.random.default_rng(5)
    mats = [sc.lambertian((0.7, 0.3, 0.3)), sc.metal((0.8, 0.8, 0.8), 0.15), sc.lambertian((0.2, 0.4, 0.8))]
    for k in range(60):
        c = rng.uniform(-8, 8, 2)
        sc.sphere((float(c[0]), 0.2, float(c[1])), 0.2, mats[k % 3])
    for k in range(300):
        c = rng.normal(0.0, 0.12, 3)
        sc.sphere((0.3 + float(c[0]), 0.3 + abs(float(c[1])), 0.1 + float(c[2])), 0.02, mats[2 * (k % 2)])  # (diffuse: a clump of mirrors
        # amplifies a rounding difference at every bounce, and the samples' fp32 and fp64 branches part)
    sc.set_nested_grid(True)
    return _project(sc, projection, "orthographic", 3.2)  # (the twin's scale: its 30 degrees span 3.2 at the floor)


# name -> (family bits the kernel must report, builder, light sampling on)
CASES = {
    "cam_ortho": (0, ortho_plain, False),
    "cam_ortho_blur": (0, ortho_blur, False),
    "cam_pano_nee": (NEE, pano_nee, True),
    "cam_pano_fog": (MEDIA, pano_fog, False),
    "cam_fisheye_env": (ENV, fisheye_env, False),
    "cam_fisheye_blur_nee": (NEE, fisheye_blur_nee, True),
    "cam_pano_motion": (MOTION, pano_motion, False),
    "cam_ortho_nested": (0, ortho_nested, False),
}
NESTED = ("cam_ortho_nested",)
# the deliberate mistakes (ref64_camera.PERTURBATIONS), each on a case that exercises it
MISTAKES = (("cam_pano_nee", "pano_mirrored"), ("cam_pano_nee", "pano_t_from_top"), ("cam_fisheye_env", "fisheye_equisolid"),
            ("cam_fisheye_env", "fisheye_circle_on_width"), ("cam_ortho_blur", "lens_keeps_direction"), ("cam_ortho", "ortho_fixed_origin"))


family, seed_of, inputs = FS.bindings(CASES.__getitem__)


def scene(rtmi, name, projection=True):
    sc = CASES[name][1](rtmi, projection)
    sc.set_light_sampling(CASES[name][2])
    return sc


def plain_twin(rtmi, name):
    """the twin with the perspective projection, made plain (feature_scenes.cleared): what the plain kernel renders"""
    return FS.cleared(CASES[name][1](rtmi, False))


def twin(rtmi, name):
    """the same scene, family and all, through the perspective camera"""
    return scene(rtmi, name, False)


def reference(rtmi, name, words, shutter=None, sc=None):
    """(RefScene, Frame, ref64_camera.reference(...)) of the case on the samples `words`"""
    sc = scene(rtmi, name) if sc is None else sc
    S, F = R.RefScene(sc), RC.Frame(sc)
    return S, F, RC.reference(S, F, words, shutter)


def check_contents(name, tally):
    """the case's conditions, from the reference's tally["camera"] (ref64_camera.film_tally) alone"""
    c = tally["camera"]
    assert c["samples"] >= 16000, (name, c)
    if "fisheye" in name:
        assert c["inside"] >= MIN_SIDE and c["outside"] >= MIN_SIDE and c["centre"] >= MIN_CENTRE, (name, c)
    if "pano" in name:
        assert min(c["north"], c["south"]) >= MIN_POLE and min(c["seam_left"], c["seam_right"]) >= MIN_SEAM, (name, c)
