"""Scenes shared by the tests of light sampling in participating media, CPU and GPU: media_scenes' rooms with light
sampling and the switch, the thin-fog room with an asymmetry and under point / spot lights, the closed emitter of
test_gpu_media.py's test 3, the white furnace, and the showcase's lamp.  scene() / seed_of() / family() / FAMILIES make the
module one per_sample.check_same_bytes can drive."""
import os

import numpy as np

import media_scenes as MS
from nee_scenes import REF_DRAWS, REF_H, REF_K, REF_W  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes")
NEE, MEDIA = 256, MS.MEDIA
FAMILIES = NEE | MEDIA
REF_SEED = 97

FURNACE_SIDE, FURNACE_SIGMA, FURNACE_DEPTH = 4.0, 0.5, 64
FURNACE_G = (0.0, 0.7, -0.5)


def switch_on(sc):
    sc.set_light_sampling(True)
    sc.set_media_light_sampling(True)
    return sc


def thin_fog(rtmi, g=0.0):
    sc = MS.room(rtmi)
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9), g=g)
    return sc


def thin_fog_analytic(rtmi):
    """the thin-fog room lit by one point and one spot light instead of the rectangle (every other primitive as it is)"""
    sc = rtmi.Scene.new(REF_W, REF_H, 16, 6)
    sc.set_background((0.05, 0.06, 0.08), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.6, 0.0), (0, 1, 0), 45.0)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.5, 0.4)))
    sc.sphere((-1.6, 0.6, 0.4), 0.6, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((0.0, 0.6, -0.6), 0.6, sc.metal((0.8, 0.7, 0.6), 0.3))
    sc.sphere((1.6, 0.6, 0.6), 0.6, sc.dielectric(1.5))
    sc.point_light((0.5, 3.2, 0.5), (9.0, 8.0, 7.0))
    sc.spot_light((-2.5, 3.5, 2.0), (1.6, -3.0, -1.4), (40.0, 20.0, 10.0), 14.0, 24.0)
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9))
    return sc


def closed_emitter(rtmi, g=0.0):
    """test_gpu_media.py's scene 3: the camera and a medium of albedo 1/2 inside a closed sphere emitter of radiance 1"""
    depth = 8
    sc = rtmi.Scene.new(64, 36, 1, depth)
    sc.set_background((0, 0, 0), sky_gradient=False, defocus_blur=False)
    sc.camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0)
    sc.sphere((0, 0, 0), 50.0, sc.diffuse_light((1, 1, 1)))
    sc.add_medium_sphere((0, 0, 0), 4.0, 0.5, (0.5, 0.5, 0.5), g=g)
    return sc


def furnace(rtmi, g=0.0, w=64, h=36, spp=64):
    """a closed box of six emissive quads of radiance 1 about the origin, filled by a medium of albedo 1; the camera inside"""
    a = FURNACE_SIDE / 2
    sc = rtmi.Scene.new(w, h, spp, FURNACE_DEPTH)
    sc.set_background((0, 0, 0), sky_gradient=False, defocus_blur=False)
    sc.camera((0.3, -0.2, 0.5), (0.0, 0.1, -2.0), (0, 1, 0), 70.0)
    light = sc.diffuse_light((1, 1, 1))
    s = FURNACE_SIDE
    for q, u, v in (((-a, -a, -a), (s, 0, 0), (0, s, 0)), ((-a, -a, a), (s, 0, 0), (0, s, 0)),
                    ((-a, -a, -a), (0, s, 0), (0, 0, s)), ((a, -a, -a), (0, s, 0), (0, 0, s)),
                    ((-a, -a, -a), (0, 0, s), (s, 0, 0)), ((-a, a, -a), (0, 0, s), (s, 0, 0))):
        sc.quad(q, u, v, light)
    sc.add_medium_box((-a - 0.5,) * 3, (a + 0.5,) * 3, FURNACE_SIGMA, (1, 1, 1), g=g)
    return sc


def check_furnace_closed(sc):
    """the premise of the white furnace, on the scene as it is: six quads, each one whole face of the cube [-a, a]^3, every face
    taken once; every material an emitter of radiance (1, 1, 1); the camera strictly inside; the medium covers the cube"""
    a = FURNACE_SIDE / 2
    prims, mats, texs, (med,) = sc.prims(), sc.materials(), sc.textures(), sc.media()
    assert len(prims) == 6 and (prims["type"] == 6).all()  # quads
    faces = set()
    for p in prims:
        m = p["m"].astype(np.float64)
        q, u, v = m[0:3], m[3:6], m[6:9]
        corners = np.stack([q, q + u, q + v, q + u + v])
        assert np.isin(np.abs(corners), (a,)).all(), corners  # every corner is a corner of the cube
        fixed = [k for k in range(3) if (corners[:, k] == corners[0, k]).all()]
        assert len(fixed) == 1 and abs(u @ v) == 0 and np.linalg.norm(np.cross(u, v)) == FURNACE_SIDE ** 2
        faces.add((fixed[0], float(corners[0, fixed[0]])))
        mt = mats[p["material"]]
        assert mt["type"] == 3 and texs[mt["texture"]]["type"] == 0 and (texs[mt["texture"]]["c0"][:3] == 1).all()
    assert faces == {(k, sgn * a) for k in range(3) for sgn in (-1.0, 1.0)}
    org = np.array(sc.get_camera().origin[:])
    assert (np.abs(org) < a).all()
    assert med["shape"] == 1 and (med["f"][:3] < -a).all() and (med["f"][3:] > a).all() and (med["albedo"] == 1).all()


def beams(rtmi, lamp_only=False, w=64, h=36, spp=64):
    """scenes/fog_beams.json at a test's size, with light sampling and the switch; lamp_only: without its two spotlights"""
    sc = rtmi.Scene.load(os.path.join(SCENES, "fog_beams.json"))
    sc.override(width=w, height=h, spp=spp)
    if lamp_only:
        sc.clear_analytic_lights()
    return switch_on(sc)


def ref_cases():
    """the per-sample cases: media_scenes.ref_cases()' five, the thin-fog room with g = 0.7 and g = -0.5 and under a point and a
    spot light -- and the white furnace at g = 0.7, where nearly every path ends on an emitter behind a medium vertex"""
    cases = dict(MS.ref_cases())
    cases["thin fog, g = 0.7"] = lambda rtmi: thin_fog(rtmi, 0.7)
    cases["thin fog, g = -0.5"] = lambda rtmi: thin_fog(rtmi, -0.5)
    cases["thin fog, point and spot light"] = thin_fog_analytic
    cases["white furnace, g = 0.7"] = lambda rtmi: furnace(rtmi, 0.7, REF_W, REF_H, 16)
    return cases


# which case shows which of the four deliberate mistakes of DESIGN 7z that ref64.trace()'s `perturb` knows (the others may too)
MISTAKES = {"no_transmittance": "camera inside thin fog", "isotropic_pdf": "thin fog, g = 0.7",
            "shadow_flight_draw": "camera inside thin fog", "medium_full_weight": "white furnace, g = 0.7"}


# ---- what per_sample.check_same_bytes asks of a scenes module
def scene(rtmi, name):
    return switch_on(ref_cases()[name](rtmi))


def seed_of(name):
    return REF_SEED


def family(name):
    return FAMILIES
