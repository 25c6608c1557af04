"""Scenes shared by the anisotropic-media tests, CPU and GPU: spheres with solid lambertian and diffuse_light
materials, a constant or sky-gradient background, a pinhole camera, media with an asymmetry g."""
from nee_scenes import REF_DRAWS, REF_H, REF_K, REF_W  # noqa: F401 (the per-sample comparison's frame, as media_scenes takes it)

MEDIA = 2048  # rt_stats.kernel_variant: a media kernel
REF_SEED = 113  # the per-sample comparison's seed, of its own
# what the comparison's premises read of ref64.tally()
TALLY_KEYS = ("anisotropic_events", "isotropic_events", "surface_after_anisotropic", "both_on_one_path", "media_with_events")


def room(rtmi, w=REF_W, h=REF_H, spp=16, depth=6, rr=0.0, sky=False):
    """a ground sphere with three lambertian spheres under a sphere emitter, dim background, no lens blur"""
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.05, 0.06, 0.08), sky_gradient=sky, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.9, 0.0), (0, 1, 0), 45.0)
    sc.sphere((0.0, -100.0, 0.0), 100.0, sc.lambertian((0.6, 0.5, 0.4)))  # (the ground, at three_sphere.json's radius: fp32 roots stay sharp)
    sc.sphere((-1.7, 0.6, 0.4), 0.6, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((0.0, 0.6, -0.8), 0.6, sc.lambertian((0.7, 0.7, 0.7)))
    sc.sphere((1.7, 0.6, 0.6), 0.6, sc.lambertian((0.7, 0.3, 0.3)))
    sc.sphere((0.0, 3.6, 0.0), 0.8, sc.diffuse_light((6.0, 5.0, 4.0)))
    if rr > 0:
        sc.set_russian_roulette(rr)
    return sc


def _thin_fog(rtmi):
    sc = room(rtmi)
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9), g=0.8)  # (the camera stands inside)
    return sc


def _dense_ball(rtmi):
    sc = room(rtmi)
    sc.add_medium_sphere((-0.2, 1.7, 2.6), 1.0, 6.0, (0.8, 0.6, 0.4), g=-0.5)
    return sc


def _overlap(rtmi):
    """a forward-scattering box and an isotropic ball inside each other: a vertex of the first takes two draws, one of the second
    the rejection loop's 3 per attempt"""
    sc = room(rtmi, sky=True)
    sc.add_medium_box((-2.5, 0.2, -1.0), (1.5, 2.6, 3.5), 0.8, (0.9, 0.5, 0.5), g=0.9)
    sc.add_medium_sphere((0.0, 1.5, 2.0), 1.2, 1.5, (0.4, 0.6, 0.9))
    return sc


def _roulette(rtmi):
    sc = room(rtmi, rr=0.8)
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9), g=0.8)
    sc.add_medium_sphere((-0.2, 1.7, 2.6), 1.0, 3.0, (0.8, 0.6, 0.4), g=-0.5)
    return sc


OVERLAP = "two overlapping media, g 0.9 and 0"


def ref_cases():
    return {"camera inside thin forward fog": _thin_fog, "dense back-scattering ball": _dense_ball, OVERLAP: _overlap,
            "russian roulette": _roulette}


# what per_sample.check_same_bytes asks of a scenes module
FAMILIES = MEDIA


def scene(rtmi, name):
    return ref_cases()[name](rtmi)


def seed_of(name):
    return REF_SEED


def family(name):
    return MEDIA


def isotropic_twin(sc):
    """the scene with every asymmetry set to 0 (a clone: the scene stays as it is)"""
    twin = sc.clone()
    for i in range(len(twin.media())):
        twin.set_medium_phase(i, 0.0)
    return twin


def plain_twin(sc):
    twin = sc.clone()
    twin.clear_media()
    return twin
