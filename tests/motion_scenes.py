"""Scenes shared by the motion-blur tests, CPU and GPU."""
import numpy as np

import media_scenes as MS

MOTION = 4096  # rt_stats.kernel_variant / rt_table_info.kernel_variant: a motion kernel


def shutter_times(rtmi, seed, width, height, first, count):
    """[count * height * width] shutter times, samples ordered (sample, y, x) as ref64.uniforms orders its words"""
    return np.array([rtmi.shutter_time(seed, pix, first + k) for k in range(count) for pix in range(height * width)], np.float64)


# ---- the movers no ray can reach (test 1) -------------------------------------------------------------------------------------
def bury_mover_three_spheres(sc):
    """A mover that stays deep inside the opaque ground sphere of the three-sphere scene (centre (0, -100.5, -1), radius 100) for
    its whole travel: every ray that could reach it meets the ground first, and a mover's root only counts up to that hit."""
    return sc.add_moving_sphere((-30, -100.5, -1), (30, -100.5, -1), 20.0, 0)


def bury_mover_mixed(sc, n=1):
    """... and n movers under the middle of mixed_scene's opaque floor (y = 0, |x|, |z| <= 15), by bury_medium_mixed's argument"""
    return [sc.add_moving_sphere((-4 + 0.1 * i, -5, -1), (4, -5 - 0.05 * i, 1), 2.0, 0) for i in range(n)]


def _camera_rays(sc):
    """the camera ray through every pixel corner-to-corner position u = x / (W - 1), v = y / (H - 1), from the lens centre"""
    cam, info = sc.get_camera(), sc.info
    org, ll, hor, ver = (np.array(getattr(cam, k)[:], np.float64) for k in ("origin", "lower_left", "horizontal", "vertical"))
    u, v = np.meshgrid(np.arange(info.width) / (info.width - 1), np.arange(info.height) / (info.height - 1))
    d = ll + u.reshape(-1, 1) * hor + v.reshape(-1, 1) * ver - org
    return np.broadcast_to(org, d.shape), d


def _no_hit_before(rtmi, movers, o, d, t_cover):
    """the host evaluation of the device's test: no mover is hit before t_cover (the opaque cover's ray parameter; inf: the ray
    misses the cover), at the ends and in the middle of the shutter interval"""
    for mv in movers:
        for s in (0.0, 0.5, 1.0 - 2.0 ** -24):
            for oo, dd, tc in zip(o, d, t_cover):
                assert not rtmi.moving_sphere_hit(mv, s, oo, dd, tc)[0], (s, oo, dd, tc)


def check_buried_three_spheres(rtmi, sc):
    """the premise of bury_mover_three_spheres, asserted on the scene as it is: the mover's sweep lies strictly inside the opaque
    ground sphere, everything else outside it -- and, through the host evaluation, no camera ray and no ray from outside the
    ground towards the mover's track meets the mover before the ground"""
    prims, mats, movers = sc.prims(), sc.materials(), sc.moving_spheres()
    ground = prims[np.argmax(np.abs(prims["f"][:, 3]))]
    c, r = ground["f"][:3].astype(np.float64), float(ground["f"][3])
    assert ground["type"] == 0 and mats[ground["material"]]["type"] == 0  # a lambertian sphere
    for mv in movers:  # (the distance to c is convex along the track: its ends bound it)
        assert max(np.linalg.norm(mv["center0"] - c), np.linalg.norm(mv["center1"] - c)) + mv["radius"] < r - 1.0
    for p in prims:
        if p.tobytes() != ground.tobytes():
            assert p["type"] == 0 and np.linalg.norm(p["f"][:3] - c) - abs(p["f"][3]) >= r - 1e-3
    org = np.array(sc.get_camera().origin[:], np.float64)
    assert np.linalg.norm(org - c) > r

    def t_ground(o, d):
        oc = o - c
        A, hb, cc = (d * d).sum(1), (oc * d).sum(1), (oc * oc).sum(1) - r * r
        disc = hb * hb - A * cc
        with np.errstate(invalid="ignore"):
            t = (-hb - np.sqrt(disc)) / A
        return np.where((disc > 0) & (t > 0), np.maximum(t, 0.0011), np.inf)
    o, d = _camera_rays(sc)
    _no_hit_before(rtmi, movers, o, d, t_ground(o, d))
    rng = np.random.default_rng(2)
    u = rng.normal(size=(300, 3))
    o = c + (r + rng.uniform(0, 5, (300, 1))) * u / np.linalg.norm(u, axis=1, keepdims=True)
    d = (c + rng.uniform(-40, 40, (300, 3))) - o
    _no_hit_before(rtmi, movers, o, d, t_ground(o, d))


def check_buried_mixed(rtmi, sc):
    """... and of bury_mover_mixed: the floor is the opaque rectangle y = 0 over its outline, the camera and every primitive lie
    above it inside the outline (media_scenes.check_buried_mixed's assertions, which need a medium: restated for the parts
    that matter here), the movers' sweeps lie below it inside the outline; camera rays and rays from above the floor towards
    the movers meet the floor first"""
    prims, mats, movers = sc.prims(), sc.materials(), sc.moving_spheres()
    floor = prims[0]
    assert floor["type"] == 2 and floor["f"][4] == 0.0 and mats[floor["material"]]["type"] == 0  # xz_rect, y = 0, lambertian
    x0, x1, z0, z1 = (float(v) for v in floor["f"][:4])
    for p in prims[1:]:
        if p["type"] == 0:
            assert p["f"][1] - abs(p["f"][3]) >= -1e-6 and x0 < p["f"][0] < x1 and z0 < p["f"][2] < z1
    org = np.array(sc.get_camera().origin[:], np.float64)
    assert org[1] > 0 and x0 < org[0] < x1 and z0 < org[2] < z1
    for mv in movers:
        for cen in (mv["center0"], mv["center1"]):
            assert cen[1] + mv["radius"] < -0.5 and x0 < cen[0] - mv["radius"] and cen[0] + mv["radius"] < x1
            assert z0 < cen[2] - mv["radius"] and cen[2] + mv["radius"] < z1

    def t_floor(o, d):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -o[:, 1] / d[:, 1]
        q = o + np.nan_to_num(t)[:, None] * d
        on = (d[:, 1] < 0) & (q[:, 0] >= x0) & (q[:, 0] <= x1) & (q[:, 2] >= z0) & (q[:, 2] <= z1)
        return np.where(on, t, np.inf)
    o, d = _camera_rays(sc)
    _no_hit_before(rtmi, movers[:2], o, d, t_floor(o, d))
    rng = np.random.default_rng(1)
    o = rng.uniform([x0, 0.0, z0], [x1, max(float(org[1]), 4.0), z1], (300, 3))
    d = rng.uniform([-6, -7, -3], [6, -3, 3], (300, 3)) - o
    tf = t_floor(o, d)
    assert np.isfinite(tf).all()
    _no_hit_before(rtmi, movers[:2], o, d, tf)


# ---- the composition scene (test 2) and the comparison cases (test 4) ----------------------------------------------------------
def room(rtmi, w=MS.REF_W, h=MS.REF_H, spp=16, depth=6, blur=False, light=True):
    """media_scenes.room -- a floor with a lambertian, a fuzzy-metal and a glass sphere under a rectangular emitter -- with
    the lens blur as a choice"""
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.05, 0.06, 0.08) if light else (0.02, 0.02, 0.03), sky_gradient=False, defocus_blur=blur)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.6, 0.0), (0, 1, 0), 45.0, aperture=0.08 if blur else 0.0)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.5, 0.4)))
    sc.sphere((-1.6, 0.6, 0.4), 0.6, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((0.0, 0.6, -0.6), 0.6, sc.metal((0.8, 0.7, 0.6), 0.3))
    sc.sphere((1.6, 0.6, 0.6), 0.6, sc.dielectric(1.5))
    if light:
        sc.xz_rect(-1.0, 1.0, -1.0, 1.0, 3.5, sc.diffuse_light((6.0, 5.0, 4.0)))
    return sc


def two_movers(rtmi, spp=48):
    sc = room(rtmi, w=64, h=36, spp=spp)
    sc.add_moving_sphere((-2.4, 0.5, 2.0), (2.4, 0.5, 1.2), 0.45, sc.lambertian((0.8, 0.3, 0.2)))
    sc.add_moving_sphere((1.0, 1.6, -1.5), (-1.0, 1.9, 1.5), 0.35, sc.metal((0.9, 0.9, 0.9), 0.0))
    return sc


def _three_materials(rtmi):
    """a mover of each material on tracks that pass in front of one static sphere and behind another, lens blur on"""
    sc = room(rtmi, blur=True)
    sc.add_moving_sphere((-2.6, 0.5, 1.9), (2.4, 0.5, -1.3), 0.45, sc.lambertian((0.8, 0.3, 0.2)))
    sc.add_moving_sphere((2.6, 0.45, 2.0), (-2.2, 0.45, -1.6), 0.4, sc.metal((0.9, 0.8, 0.7), 0.1))
    sc.add_moving_sphere((-1.2, 1.5, 1.8), (1.4, 1.2, -1.6), 0.4, sc.dielectric(1.5))
    return sc


def _glass_mover(rtmi):
    """a glass mover sweeping between the camera and the static balls: they are seen through it"""
    sc = room(rtmi)
    sc.add_moving_sphere((-1.2, 1.1, 2.6), (1.2, 1.3, 2.6), 0.7, sc.dielectric(1.5))
    return sc


def _emissive_mover(rtmi):
    """an emissive mover over the floor, the room's own emitter removed, light sampling off"""
    sc = room(rtmi, light=False)
    sc.add_moving_sphere((-2.0, 1.8, 0.5), (2.0, 2.2, 0.0), 0.4, sc.diffuse_light((8.0, 7.0, 5.0)))
    return sc


ZERO_V = ((-0.3, 0.5, 2.0), 0.5)  # where the zero-velocity mover stands, and its twin's static sphere


def _zero_velocity(rtmi):
    sc = room(rtmi)
    sc.add_moving_sphere(ZERO_V[0], ZERO_V[0], ZERO_V[1], sc.lambertian((0.7, 0.7, 0.2)))
    return sc


def static_twin(rtmi):
    """the zero-velocity case with a static sphere (last in the list, as a mover counts) in the mover's place"""
    sc = room(rtmi)
    sc.sphere(ZERO_V[0], ZERO_V[1], sc.lambertian((0.7, 0.7, 0.2)))
    return sc


IN_FRONT = "a mover of each material passing in front of and behind static spheres"


def ref_cases():
    return {IN_FRONT: _three_materials, "a glass mover with the balls seen through it": _glass_mover,
            "an emissive mover over the floor": _emissive_mover, "a zero-velocity mover": _zero_velocity}


# ---- the known answer: coverage (test 3) ---------------------------------------------------------------------------------------
COV_W, COV_H, COV_SPP, COV_SEED = 64, 36, 24, 77
COV_CAP = 1e-5  # |disc| / half_b^2 below which fp32 and fp64 may disagree on a sample


def coverage_scene(rtmi):
    """white background, no gradient, no blur, depth 2; a black lambertian mover crosses the frame: every sample is 0 or 1"""
    sc = rtmi.Scene.new(COV_W, COV_H, COV_SPP, 2)
    sc.set_background((1, 1, 1), sky_gradient=False, defocus_blur=False)
    sc.camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0)
    sc.sphere((0, 0, 60), 1.0, sc.lambertian((0.5, 0.5, 0.5)))  # (behind the camera: no ray meets it)
    sc.add_moving_sphere((-4.5, -0.4, -5.0), (4.5, 0.6, -5.0), 1.0, sc.lambertian((0, 0, 0)))
    return sc


def coverage_reference(rtmi, sc):
    """per sample (sample, y, x), in fp64 from the sample's own jitter and shutter time: does the camera ray meet the mover,
    the discriminant relative to half_b^2, and the shutter time"""
    W, H, n = COV_W, COV_H, COV_SPP
    cam = sc.get_camera()
    org, ll, hor, ver = (np.array(getattr(cam, k)[:], np.float64) for k in ("origin", "lower_left", "horizontal", "vertical"))
    (mv,) = sc.moving_spheres()
    c0, r = mv["center0"].astype(np.float64), float(mv["radius"])
    vel = (mv["center1"] - mv["center0"]).astype(np.float64)  # (fp32 subtraction: the model's v)
    pix = np.arange(H * W)
    hit, rel, time = (np.empty((n, H * W)) for _ in range(3))
    for k in range(n):
        w = np.stack([rtmi.sample_stream(COV_SEED, p, k, 2) for p in pix])
        xi = (w >> 8).astype(np.float64) * 2.0 ** -24
        s = np.array([rtmi.shutter_time(COV_SEED, p, k) for p in pix], np.float64)
        u, v = ((pix % W) + xi[:, 0]) / (W - 1), ((pix // W) + xi[:, 1]) / (H - 1)
        d = ll + u[:, None] * hor + v[:, None] * ver - org
        oc = org - (c0 + s[:, None] * vel)
        A, hb, cc = (d * d).sum(1), (oc * d).sum(1), (oc * oc).sum(1) - r * r
        disc = hb * hb - A * cc
        hit[k], rel[k], time[k] = (disc >= 0) & (hb < 0), disc / (hb * hb), s  # (the camera is outside: a real root in front)
    return hit.astype(bool), rel, time


def assert_motion_is_seen(hit, s):
    """hit, s: [spp][pixels].  Some pixels are covered only early in the shutter interval, some only late, some partly"""
    count = hit.sum(axis=0)
    covered = count > 0
    early = covered & np.where(hit, s < 0.25, True).all(axis=0)
    late = covered & np.where(hit, s > 0.75, True).all(axis=0)
    partly = (count > 0) & (count < len(hit))
    assert early.sum() > 10 and late.sum() > 10 and partly.sum() > 100, (int(early.sum()), int(late.sum()), int(partly.sum()))
