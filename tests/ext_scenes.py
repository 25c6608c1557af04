"""Scenes with triangles and image textures for the four render families that exist only in the build that carries them
(light sampling, environment, media, motion), shared by test_ext_reference.py (CPU) and test_gpu_ext_reference.py.

Every case uses the frame, sample count, seed and draw budget of its family's own module (nee_scenes.REF_*, media_scenes.REF_SEED
with motion_scenes.shutter_times).  Images are small, non-square and asymmetric with random texels that include 0 and 255;
triangle corners carry distinct, asymmetric (u1, u2, u3), so that a transposed lookup or the natural pairing of the area
weights changes what is read.  No checker lies on y = 0 and no textured surface is coplanar with another."""
import numpy as np

import media_scenes as MS
import motion_scenes as MO
import nee_scenes as NS
import ref64 as R
from feature_scenes import NEE, ENV, MEDIA, MOTION  # (the family bits of rt_stats.kernel_variant)

MIN_IMAGE_SHARE = 0.20  # of a case's samples read an image texel at some vertex


def image(rows, cols, seed):
    px = np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    px[0, cols - 1], px[rows - 1, 0] = (0, 255, 37), (255, 0, 201)
    return px


def quad(sc, a, b, c, d, mat, uv):
    """two triangles (a, b, c) and (a, c, d) with the corner coordinates uv = (ua, ub, uc, ud)"""
    sc.triangle(a, b, c, mat, uv[0], uv[1], uv[2])
    sc.triangle(a, c, d, mat, uv[0], uv[2], uv[3])


QUAD_UV = ((0.08, 0.21), (0.93, 0.12), (0.71, 0.96), (0.04, 0.78))


def pyramid(sc, apex, half, drop, mat):
    """four side triangles under an apex, the base left open"""
    x, y, z = apex
    base = [(x - half, y - drop, z - half), (x + half, y - drop, z - half), (x + half, y - drop, z + half), (x - half, y - drop, z + half)]
    for k in range(4):
        sc.triangle(apex, base[k], base[(k + 1) % 4], mat, (0.5, 0.9), (0.1, 0.15), (0.85, 0.3))


def mesh(sc, y=1.35, textured=True):
    """a lambertian, a metal(0.3) and a glass pyramid side by side: 12 triangles"""
    lam = sc.lambertian(sc.image_texture(image(3, 5, 21))) if textured else sc.lambertian((0.7, 0.4, 0.3))
    pyramid(sc, (-0.9, y, 0.3), 0.45, 0.6, lam)
    pyramid(sc, (0.0, y + 0.1, -0.2), 0.45, 0.6, sc.metal((0.8, 0.7, 0.6), 0.3))
    pyramid(sc, (0.9, y, 0.4), 0.45, 0.6, sc.dielectric(1.5))


def textured_objects(sc, floor=True, y=0.0):
    """an image-textured floor rectangle, sphere, cylinder, yz_rect and triangle pair, each with an image of its own"""
    if floor:
        sc.xz_rect(-7, 7, -7, 7, y, sc.lambertian(sc.image_texture(image(5, 7, 11))))
    sc.sphere((-1.2, 0.62 + y, 0.5), 0.6, sc.lambertian(sc.image_texture(image(3, 4, 12))))
    sc.cylinder(0.3, -0.7, 0.7, sc.lambertian(sc.image_texture(image(8, 2, 13))), rotate=((1.0, 0.2, 0.0), 80.0), translate=(1.4, 0.75 + y, 0.9))
    sc.yz_rect(0.02 + y, 2.2 + y, -2.0, 1.5, -2.6, sc.lambertian(sc.image_texture(image(4, 3, 14))))
    quad(sc, (0.2, 0.03 + y, -2.0), (3.2, 0.03 + y, -1.5), (3.1, 2.5 + y, -1.1), (0.3, 2.3 + y, -1.5),
         sc.lambertian(sc.image_texture(image(7, 5, 15))), QUAD_UV)


def _frame(rtmi, depth=6, background=(0.02, 0.02, 0.03)):
    sc = rtmi.Scene.new(NS.REF_W, NS.REF_H, 1, depth)
    sc.set_background(background, sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    return sc


def _receivers(rtmi, depth=6, rr=0.0):
    sc = _frame(rtmi, depth)
    textured_objects(sc)
    sc.xz_rect(-0.7, 0.7, -0.7, 0.7, 2.6, sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.sphere((2.1, 2.0, 1.2), 0.3, sc.diffuse_light((5.0, 6.0, 7.0)))
    if rr > 0:
        sc.set_russian_roulette(rr)
    sc.set_light_sampling(True)
    return sc


def _mesh_under_the_light(rtmi):
    sc = _frame(rtmi)
    sc.xz_rect(-7, 7, -7, 7, 0.0, sc.lambertian(sc.image_texture(image(5, 7, 11))))
    mesh(sc)
    sc.xz_rect(-1.2, 1.2, -1.0, 1.0, 2.8, sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.set_light_sampling(True)
    return sc


def _unlisted(rtmi):
    """one listed rectangle light beside a triangle emitter and an image-textured rectangle emitter, neither of them a light"""
    sc = _frame(rtmi)
    sc.xz_rect(-7, 7, -7, 7, 0.0, sc.lambertian(sc.image_texture(image(5, 7, 11))))
    sc.sphere((-1.2, 0.62, 0.5), 0.6, sc.lambertian(sc.image_texture(image(3, 4, 12))))
    sc.xz_rect(-0.5, 0.5, -0.5, 0.5, 2.6, sc.diffuse_light((6.0, 5.0, 4.0)))
    quad(sc, (0.8, 0.4, -2.0), (3.0, 0.4, -1.4), (3.0, 2.4, -1.4), (0.8, 2.4, -2.0), sc.diffuse_light((2.0, 1.5, 1.0)), QUAD_UV)
    sc.yz_rect(0.3, 2.3, -1.5, 1.5, -2.8, sc.diffuse_light(sc.image_texture(image(4, 3, 16))))
    sc.set_light_sampling(True)
    return sc


def _env(nee):
    def build(rtmi):
        sc = NS.env_geometry(rtmi)
        textured_objects(sc, floor=False, y=NS.LIFT)
        sc.xy_rect(-6, 6, NS.LIFT + 0.01, 5.0, -3.2, sc.lambertian(sc.image_texture(image(5, 8, 17))))
        mesh(sc, y=2.2)
        env, scale, rotate = NS._sun_map()
        sc.set_environment(env, scale, rotate)
        sc.set_light_sampling(nee)
        return sc
    return build


def _fog(rtmi):
    """media_scenes.room with an image-textured floor and lambertian sphere and a triangle pair, the camera inside thin fog"""
    sc = rtmi.Scene.new(MS.REF_W, MS.REF_H, 1, 6)
    sc.set_background((0.05, 0.06, 0.08), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.6, 0.0), (0, 1, 0), 45.0)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian(sc.image_texture(image(5, 7, 31))))
    sc.sphere((-1.6, 0.6, 0.4), 0.6, sc.lambertian(sc.image_texture(image(3, 4, 32))))
    sc.sphere((0.0, 0.6, -0.6), 0.6, sc.metal((0.8, 0.7, 0.6), 0.3))
    sc.sphere((1.6, 0.6, 0.6), 0.6, sc.dielectric(1.5))
    sc.xz_rect(-1.0, 1.0, -1.0, 1.0, 3.5, sc.diffuse_light((6.0, 5.0, 4.0)))
    quad(sc, (-2.8, 0.05, -2.2), (-0.4, 0.05, -2.6), (-0.5, 1.9, -2.3), (-2.7, 1.7, -2.0), sc.lambertian(sc.image_texture(image(7, 5, 33))), QUAD_UV)
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9))
    return sc


def _movers(rtmi):
    """an image-textured lambertian mover and an image-textured emissive mover in front of static triangles and an image wall"""
    sc = MO.room(rtmi, spp=1, light=False)
    quad(sc, (0.4, 0.05, -2.0), (2.8, 0.05, -1.7), (2.7, 1.9, -1.4), (0.5, 1.7, -1.6), sc.lambertian(sc.image_texture(image(7, 5, 41))), QUAD_UV)
    pyramid(sc, (-0.6, 1.9, -1.6), 0.5, 0.7, sc.lambertian((0.7, 0.6, 0.3)))
    sc.yz_rect(0.02, 2.4, -2.0, 2.0, -3.0, sc.lambertian(sc.image_texture(image(4, 3, 42))))
    sc.add_moving_sphere((-2.2, 0.55, 2.2), (1.8, 0.55, 1.4), 0.55, sc.lambertian(sc.image_texture(image(3, 4, 43))))
    sc.add_moving_sphere((1.6, 2.0, 0.6), (-1.4, 2.3, 0.0), 0.45, sc.diffuse_light(sc.image_texture(image(2, 5, 44))))
    return sc


RECEIVERS = "textured receivers"
# name -> (family mask the kernel must report, builder, the tally keys the case is there for)
CASES = {
    RECEIVERS: (NEE, _receivers, ("image_vertices_with_light_sample", "triangle_vertices_with_light_sample", "shadow_stopped_by_image_prim")),
    "mesh under the light": (NEE, _mesh_under_the_light, ("shadow_stopped_by_triangle", "triangle_vertices")),
    "unlisted emitters": (NEE, _unlisted, ("unlisted_emitter_hits_after_light_sample",)),
    "textured, roulette 0.85, max_depth 3": (NEE, lambda rtmi: _receivers(rtmi, depth=3, rr=0.85),
                                             ("image_vertices_with_light_sample", "triangle_vertices_with_light_sample")),
    "env + textures + mesh, plain": (ENV, _env(False), ("image_vertices", "triangle_vertices")),
    "env + textures + mesh, light sampling": (ENV | NEE, _env(True), ("image_vertices", "triangle_vertices", "texel_picks")),
    "fog over textures": (MEDIA, _fog, ("medium_then_image_surface", "medium_events")),
    "textured movers": (MOTION, _movers, ("image_mover_vertices", "mover_then_static", "static_then_mover")),
}
LIGHT_SAMPLING_CASES = [n for n, c in CASES.items() if c[0] == NEE]
# the cases whose plain twins differ (the two environment cases share theirs)
DISTINCT_TWINS = [n for n, c in CASES.items() if c[0] != ENV | NEE]


def family(name):
    return CASES[name][0]


def seed_of(name):
    return NS.REF_SEED if family(name) & (NEE | ENV) else MS.REF_SEED


def scene(rtmi, name):
    sc = CASES[name][1](rtmi)
    if name == "unlisted emitters":
        assert len(sc.lights()) == 1, sc.lights()  # the premise: the triangle and the image-textured emitters are no lights
    return sc


def plain_twin(rtmi, name):
    """the case with light sampling off and its environment, media and movers cleared: what the plain kernel and the checker render"""
    sc = CASES[name][1](rtmi)
    sc.set_light_sampling(False)
    sc.set_environment(None)
    sc.clear_media()
    sc.clear_moving_spheres()
    return sc


def inputs(rtmi, name):
    """(uniforms, shutter times or None) of the case's 48 x 27 x 13 samples"""
    words = R.uniforms(rtmi, seed_of(name), NS.REF_W, NS.REF_H, 0, NS.REF_K, NS.REF_DRAWS)
    shutter = MO.shutter_times(rtmi, seed_of(name), NS.REF_W, NS.REF_H, 0, NS.REF_K) if family(name) == MOTION else None
    return words, shutter


def check_contents(name, tally, samples):
    """the case met what it is there for: each named vertex at least nee_scenes.REQUIRED_EVENTS times (1 % of the samples), and an
    image texel read by at least a fifth of the samples"""
    # (the environment is that case's only light: every light pick is a texel pick)
    counts = dict(tally, texel_picks=tally["bucket_picks"] + tally["alias_picks"])
    for what in CASES[name][2]:
        assert counts[what] >= NS.REQUIRED_EVENTS, (name, what, counts[what])
    assert tally["image_samples"] >= MIN_IMAGE_SHARE * samples, (name, tally["image_samples"], samples)
