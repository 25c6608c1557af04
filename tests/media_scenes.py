"""Scenes shared by the participating-media tests, CPU and GPU."""
import os

import numpy as np

from nee_scenes import REF_DRAWS, REF_H, REF_K, REF_W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEDIA = 2048  # rt_stats.kernel_variant / rt_table_info.kernel_variant: a media kernel

# the per-sample comparison: nee_scenes' frame, one-sample frames and uniforms requested per sample, under a seed of its own
REF_SEED = 91


def room(rtmi, w=REF_W, h=REF_H, spp=16, depth=6, rr=0.0):
    """a floor with a lambertian, a fuzzy-metal and a glass sphere under a rectangular emitter, dim background, no lens blur"""
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.05, 0.06, 0.08), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.6, 0.0), (0, 1, 0), 45.0)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.5, 0.4)))
    sc.sphere((-1.6, 0.6, 0.4), 0.6, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((0.0, 0.6, -0.6), 0.6, sc.metal((0.8, 0.7, 0.6), 0.3))
    sc.sphere((1.6, 0.6, 0.6), 0.6, sc.dielectric(1.5))
    sc.xz_rect(-1.0, 1.0, -1.0, 1.0, 3.5, sc.diffuse_light((6.0, 5.0, 4.0)))
    if rr > 0:
        sc.set_russian_roulette(rr)
    return sc


def _thin_fog(rtmi):
    sc = room(rtmi)
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9))  # (the camera stands inside)
    return sc


def _dense_sphere(rtmi):
    sc = room(rtmi)
    sc.add_medium_sphere((-0.2, 1.6, 1.5), 0.7, 6.0, (0.8, 0.6, 0.4))
    return sc


def _overlap(rtmi):
    sc = room(rtmi)
    sc.add_medium_box((-2.5, 0.2, -1.0), (0.5, 2.2, 2.5), 0.6, (0.9, 0.5, 0.5))
    sc.add_medium_sphere((0.3, 1.4, 1.2), 1.0, 1.5, (0.4, 0.6, 0.9))
    return sc


def _glass_shell(rtmi):
    sc = room(rtmi)
    sc.sphere((0.2, 1.9, 2.0), 0.7, sc.dielectric(1.5))
    sc.add_medium_sphere((0.2, 1.9, 2.0), 0.65, 4.0, (0.9, 0.3, 0.2))
    return sc


def _roulette(rtmi):
    sc = room(rtmi, rr=0.8)
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9))
    sc.add_medium_sphere((-0.2, 1.6, 1.5), 0.7, 3.0, (0.8, 0.6, 0.4))
    return sc


def ref_cases():
    return {"camera inside thin fog": _thin_fog, "dense sphere": _dense_sphere, "two overlapping media": _overlap,
            "medium inside a glass shell": _glass_shell, "russian roulette": _roulette}


def mixed_scene(rtmi, w=96, h=54, spp=4, depth=8):
    """rectangles, a cylinder, spheres (enough of them for a grid), a checker and an image texture: wide tables without media"""
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.6, 0.7, 0.9), sky_gradient=True, defocus_blur=True)
    sc.camera((0.0, 2.0, 7.0), (0.0, 0.8, 0.0), (0, 1, 0), 40.0, aperture=0.05)
    sc.xz_rect(-15, 15, -15, 15, 0.0, sc.lambertian(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.3, 0.2))))
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)
    sc.sphere((0.0, 1.0, 0.0), 1.0, sc.lambertian(sc.image_texture(img)))
    sc.cylinder(0.4, -0.8, 0.8, sc.metal((0.7, 0.7, 0.8), 0.1), rotate=((1, 0, 0), 90.0), translate=(2.2, 0.8, 0.5))
    sc.xy_rect(-3, 3, 0, 3, -3.0, sc.metal((0.9, 0.9, 0.9), 0.0))
    glass, red = sc.dielectric(1.5), sc.lambertian((0.7, 0.2, 0.2))
    for i in range(40):
        x, z = rng.uniform(-5, 5), rng.uniform(-2.5, 4)
        sc.sphere((x, 0.2, z), 0.2, glass if i % 3 == 0 else red)
    sc.sphere((-2.0, 2.5, 1.0), 0.4, sc.diffuse_light((5, 5, 4)))
    return sc


def bury_medium_mixed(sc):
    """A dense medium no ray of mixed_scene can reach: a box under the middle of the opaque floor (y = 0, |x|, |z| <= 15).  Every
    ray origin -- the camera, a surface vertex -- lies on or above the floor inside its outline; the segment from such a point
    to a point of the box crosses y = 0 at a convex combination of the two, inside the outline: the floor is hit first, and the
    ray's stay in the box, clipped to the surface hit, is empty.  So the media kernel takes no draw and must give the plain
    kernel's bytes."""
    return sc.add_medium_box((-2, -9, -2), (2, -3, 2), 5.0, (0.9, 0.9, 0.9))


def bury_medium_three_spheres(sc):
    """... and of the three-sphere scene: a ball deep inside the opaque ground sphere (centre (0, -100.5, -1), radius 100)"""
    return sc.add_medium_sphere((0, -100.5, -1), 80.0, 5.0, (0.9, 0.9, 0.9))


def check_buried_mixed(rtmi, sc):
    """the premise of bury_medium_mixed, asserted on the scene as it is: the floor is the opaque rectangle y = 0 over the outline,
    the camera and every other primitive lie above it inside the outline, the box lies below it inside the outline -- and, as
    a spot check through the host evaluation of the device's interval, rays from the scene's bounding box towards the box have
    an empty stay in it once clipped to the floor"""
    prims, mats, (med,) = sc.prims(), sc.materials(), sc.media()
    floor = prims[0]
    assert floor["type"] == 2 and floor["f"][4] == 0.0 and mats[floor["material"]]["type"] == 0  # xz_rect, y = 0, lambertian
    x0, x1, z0, z1 = (float(v) for v in floor["f"][:4])
    lo, hi = np.array([x0, 0.0, z0]), np.array([x1, np.inf, z1])
    for p in prims[1:]:
        f = p["f"]
        if p["type"] == 0:
            bmin, bmax = f[:3] - abs(f[3]), f[:3] + abs(f[3])
        elif p["type"] == 1:  # xy_rect
            bmin, bmax = np.array([f[0], f[2], f[4]]), np.array([f[1], f[3], f[4]])
        elif p["type"] == 4:  # cylinder: its axis ends, grown by the rim's reach
            m = p["m"].reshape(3, 4)
            ends = np.stack([m[:, :3] @ np.array([0, 0, z]) + m[:, 3] for z in (f[1], f[2])])
            axis = m[:, :3] @ np.array([0.0, 0.0, 1.0])  # (a rigid transform: unit length); the rim reaches r sqrt(1 - axis_k^2) along world axis k
            reach = f[0] * np.sqrt(np.maximum(0.0, 1.0 - axis * axis))
            bmin, bmax = ends.min(axis=0) - reach, ends.max(axis=0) + reach
        else:
            raise AssertionError(f"primitive type {p['type']}: extend this check before adding it to mixed_scene")
        assert (bmin >= lo - 1e-6).all() and (bmax <= hi).all(), (p["type"], bmin, bmax)
    org = np.array(sc.get_camera().origin[:])
    assert (org > lo).all() and (org < hi).all()
    assert med["shape"] == 1 and med["f"][4] < 0 and x0 < med["f"][0] and med["f"][3] < x1 and z0 < med["f"][2] and med["f"][5] < z1
    rng = np.random.default_rng(1)
    top = max(float(org[1]), 4.0)
    for _ in range(500):
        o = rng.uniform([x0, 0.0, z0], [x1, top, z1])
        d = rng.uniform(med["f"][:3], med["f"][3:]) - o
        t_floor = -o[1] / d[1]  # where the ray meets y = 0: inside the outline, so the floor is the surface hit (or something nearer)
        q = o + t_floor * d
        assert x0 <= q[0] <= x1 and z0 <= q[2] <= z1
        assert not rtmi.medium_interval(med, o, d, t_floor)[0]


def check_buried_three_spheres(rtmi, sc):
    """... and of bury_medium_three_spheres: the medium ball lies strictly inside the opaque ground sphere, everything else outside it"""
    prims, mats, (med,) = sc.prims(), sc.materials(), sc.media()
    ground = prims[np.argmax(np.abs(prims["f"][:, 3]))]
    c, r = ground["f"][:3].astype(np.float64), float(ground["f"][3])
    assert ground["type"] == 0 and mats[ground["material"]]["type"] == 0  # a lambertian sphere
    assert med["shape"] == 0 and np.linalg.norm(med["f"][:3] - c) + med["f"][3] < r - 1.0
    for p in prims:
        if p.tobytes() != ground.tobytes():
            assert p["type"] == 0 and np.linalg.norm(p["f"][:3] - c) + abs(p["f"][3]) >= r - 1e-3 and np.linalg.norm(p["f"][:3] - c) > r
    org = np.array(sc.get_camera().origin[:], np.float64)
    assert np.linalg.norm(org - c) > r
    rng = np.random.default_rng(2)
    for _ in range(500):
        o = c + (r + rng.uniform(0, 5)) * (lambda v: v / np.linalg.norm(v))(rng.normal(size=3))
        d = (c + rng.uniform(-40, 40, 3)) - o
        oc = o - c
        A, hb, cc = d @ d, oc @ d, oc @ oc - r * r
        t_ground = (-hb - np.sqrt(hb * hb - A * cc)) / A  # the ray enters the ground sphere here
        assert not rtmi.medium_interval(med, o, d, max(t_ground, 0.0011))[0]


def three_spheres(rtmi, w=96, h=54, spp=4):
    sc = rtmi.Scene.load(os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "three_sphere.json"))
    sc.override(width=w, height=h, spp=spp)
    return sc
