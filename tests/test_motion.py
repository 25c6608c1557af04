"""Motion blur without a GPU: the scene interface of the moving spheres and its errors, the JSON round trip and the
clone, the tables of a scene without movers, the shutter time against the Philox block it is defined by, and the host evaluation
of the device's intersection (rt_moving_sphere_hit) against an fp64 derivation on random rays and times, in the style -- and
with the margin and the tolerance -- of test_primitives_fuzz.py."""
import ctypes
import os

import numpy as np
import pytest

import media_scenes as MS
import motion_scenes as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(rtmi):
    sc = rtmi.Scene.new(32, 18, 2, 5)
    sc.camera((0, 1, 6), (0, 0.5, 0), (0, 1, 0), 40.0)
    sc.sphere((0, -100, 0), 100.0, sc.lambertian((0.5, 0.5, 0.5)))
    return sc


def _status(rtmi, call):
    with pytest.raises(rtmi.RtmiError) as e:
        call()
    return e.value.status


def test_add_get_clear_and_errors(rtmi):
    sc = _scene(rtmi)
    m = sc.metal((0.8, 0.8, 0.8), 0.1)
    assert len(sc.moving_spheres()) == 0 and rtmi._lib.rt_scene_moving_sphere_count(sc._h) == 0
    assert sc.add_moving_sphere((0, 1, 0), (1, 1.5, 0), 0.5, m) == 0
    assert sc.add_moving_sphere((2, 1, 0), (2, 1, 0), 0.25, 0) == 1
    got = sc.moving_spheres()
    assert got.dtype == rtmi.MOVING_SPHERE_DTYPE and rtmi.MOVING_SPHERE_DTYPE.itemsize == rtmi.struct_size(18)
    assert got["center0"].tolist() == [[0, 1, 0], [2, 1, 0]] and got["center1"].tolist() == [[1, 1.5, 0], [2, 1, 0]]
    assert got["radius"].tolist() == [0.5, 0.25] and got["material"].tolist() == [m, 0]
    assert rtmi._lib.rt_scene_moving_sphere_count(sc._h) == 2
    assert len(sc.prims()) == 1  # (movers are not primitives)
    # RT_ERR_SCENE (4): radius, centres, material
    for bad in (lambda: sc.add_moving_sphere((0, 0, 0), (1, 0, 0), 0.0, 0), lambda: sc.add_moving_sphere((0, 0, 0), (1, 0, 0), -1.0, 0),
                lambda: sc.add_moving_sphere((0, 0, 0), (1, 0, 0), float("nan"), 0),
                lambda: sc.add_moving_sphere((0, float("inf"), 0), (1, 0, 0), 1.0, 0),
                lambda: sc.add_moving_sphere((0, 0, 0), (1, float("nan"), 0), 1.0, 0),
                lambda: sc.add_moving_sphere((0, 0, 0), (1, 0, 0), 1.0, 99), lambda: sc.add_moving_sphere((0, 0, 0), (1, 0, 0), 1.0, -1)):
        assert _status(rtmi, bad) == 4
    assert len(sc.moving_spheres()) == 2
    # RT_ERR_ARG (1): null pointers
    f3 = (ctypes.c_float * 3)(0, 0, 0)
    assert rtmi._lib.rt_scene_add_moving_sphere(None, f3, f3, 1.0, 0) == -1
    assert rtmi._lib.rt_scene_add_moving_sphere(sc._h, None, f3, 1.0, 0) == -1
    assert rtmi._lib.rt_scene_add_moving_sphere(sc._h, f3, None, 1.0, 0) == -1
    assert rtmi._lib.rt_scene_get_moving_spheres(None, None, 0) == -1 and rtmi._lib.rt_scene_moving_sphere_count(None) == -1
    assert rtmi._lib.rt_scene_clear_moving_spheres(None) == 1
    assert rtmi._lib.rt_moving_sphere_hit(None, 0.0, f3, f3, 1.0, None) == -1
    # RT_ERR_LIMIT (6): the 65th
    for i in range(2, rtmi.MAX_MOVING_SPHERES):
        assert sc.add_moving_sphere((i, 0, 0), (i, 1, 0), 0.1, 0) == i
    assert _status(rtmi, lambda: sc.add_moving_sphere((0, 0, 0), (1, 0, 0), 0.1, 0)) == 6
    assert len(sc.moving_spheres()) == 64
    sc.clear_moving_spheres()
    assert len(sc.moving_spheres()) == 0


def test_json_round_trip_and_clone(rtmi):
    sc = _scene(rtmi)
    sc.add_moving_sphere((0.1, 1, 0), (1, 1.5, -0.3), 0.5, sc.dielectric(1.5))
    sc.add_moving_sphere((2, 1, 0), (2.5, 1, 0.25), 0.25, 0)
    text = sc.to_json()
    assert text.count('"moving_sphere"') == 2 and '"center0"' in text and '"center1"' in text
    back = rtmi.Scene.parse(text)
    assert back.moving_spheres().tobytes() == sc.moving_spheres().tobytes()
    assert back.prims().tobytes() == sc.prims().tobytes()
    assert back.to_json() == text
    assert sc.clone().moving_spheres().tobytes() == sc.moving_spheres().tobytes()
    # a mover's own error comes with its place in the file; a mover between primitives keeps both lists in order
    assert _status(rtmi, lambda: rtmi.Scene.parse(text.replace('"radius": 0.25', '"radius": -0.25'))) == 4
    shipped = rtmi.Scene.load(os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "motion_balls.json"))
    assert len(shipped.moving_spheres()) >= 4 and shipped.table_info().kernel_variant & MO.MOTION
    kinds = {int(shipped.materials()[m]["type"]) for m in shipped.moving_spheres()["material"]}
    assert kinds == {0, 1, 2, 3}  # a ball of each material


def test_a_scene_without_movers_keeps_its_tables(rtmi):
    for build in (MS.three_spheres, MS.mixed_scene):
        plain, sc = build(rtmi), build(rtmi)
        info = plain.table_info()
        image = plain.table_image()
        assert info.kernel_variant & MO.MOTION == 0
        v0 = sc.to_json()
        sc.clear_moving_spheres()  # (clearing an empty list changes nothing)
        assert sc.table_image().tobytes() == image.tobytes()
        sc.add_moving_sphere((0, 5, 0), (1, 5, 0), 0.5, 0)
        with_mover = sc.table_info()
        assert with_mover.kernel_variant & MO.MOTION and with_mover.grid_wide == 1
        assert with_mover.kernel_variant & 255 in (16, 36, 44)
        sc.clear_moving_spheres()
        again = sc.table_info()
        assert sc.table_image().tobytes() == image.tobytes() and sc.to_json() == v0
        assert bytes(again) == bytes(info)  # (every offset and count of the packed tables: RenderParams as exported)


def test_mover_records_lie_behind_the_primitive_tables(rtmi):
    plain, sc = MS.mixed_scene(rtmi), MS.mixed_scene(rtmi)
    MS.bury_medium_mixed(plain), MS.bury_medium_mixed(sc)  # (wide tables on both sides without a mover)
    plain.clear_media(), sc.clear_media()
    sc.add_moving_sphere((0, 5, 0), (1, 5.5, 0.25), 0.5, 1)
    a, b = plain.table_image().ravel().view(np.uint32), sc.table_image().ravel().view(np.uint32)
    assert len(b) == len(a) + 12
    diff = np.flatnonzero(a != b[:len(a)])
    assert len(diff) == 2, diff  # the count and the offset in the camera block; everything else is the image it was
    tail = b[len(a):].view(np.float32)
    assert tail[:8].tolist() == [0, 5, 0, 0.5, 1, 0.5, 0.25, 2.0]
    assert b[len(a) + 8] == 1 and b[diff[0]] == 1 and b[diff[1]] * 4 == len(a)


def test_shutter_time_is_the_philox_word(rtmi):
    for seed, pixel, sample in ((1, 0, 0), (91, 1295, 12), (2 ** 40 + 17, 2 ** 20 + 3, 4000), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 23)):
        w = rtmi.philox4x32_10((pixel, sample, 1, 0), (seed & 0xFFFFFFFF, seed >> 32))
        s = rtmi.shutter_time(seed, pixel, sample)
        assert s == float(int(w[0]) >> 8) * 2.0 ** -24 and 0.0 <= s < 1.0
        # not the block that seeds the stream, whose counter word 2 is 0
        assert int(w[0]) != int(rtmi.philox4x32_10((pixel, sample, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))[0])
    s = np.array([rtmi.shutter_time(5, p, k) for p in range(200) for k in range(20)])
    assert abs(s.mean() - 0.5) < 0.02 and s.min() < 0.01 and s.max() > 0.99


T_MIN = 1e-3


def test_moving_sphere_hit_against_fp64(rtmi):
    rng = np.random.default_rng(3)
    n = 4000
    mv = np.zeros(1, rtmi.MOVING_SPHERE_DTYPE)[0]
    mv["center0"], mv["center1"], mv["radius"] = (-0.7, -0.2, 0.1), (0.9, 0.4, -0.3), 0.9
    s = (rng.integers(0, 2 ** 24, n) * 2.0 ** -24)
    c0 = mv["center0"].astype(np.float64)
    vel = (mv["center1"] - mv["center0"]).astype(np.float64)
    c = c0 + s[:, None] * vel
    o = rng.uniform(-4, 4, (n, 3))
    inside = rng.uniform(size=n) < 0.15  # (origins inside the sphere: the far root)
    o[inside] = c[inside] + rng.uniform(-0.45, 0.45, (int(inside.sum()), 3))
    o = o.astype(np.float32).astype(np.float64)
    d = ((c + rng.normal(0.0, 0.7, (n, 3)) - o) * rng.uniform(0.2, 3.0, (n, 1))).astype(np.float32).astype(np.float64)
    t_max = np.where(rng.uniform(size=n) < 0.5, np.inf, rng.uniform(0.2, 3.0, n)).astype(np.float32).astype(np.float64)
    got = [rtmi.moving_sphere_hit(mv, s[i], o[i], d[i], t_max[i]) for i in range(n)]
    hit32, t32 = np.array([g[0] for g in got]), np.array([g[1] for g in got], np.float64)
    r = float(mv["radius"])
    oc = o - c
    a, hb, cc = (d * d).sum(1), (oc * d).sum(1), (oc * oc).sum(1) - r * r
    disc = hb * hb - a * cc
    sq = np.sqrt(np.maximum(disc, 0.0))
    t0, t1 = (-hb - sq) / a, (-hb + sq) / a
    first = (t0 >= T_MIN) & (t0 <= t_max)
    t64 = np.where(first, t0, t1)
    hit64 = (disc >= 0) & (t64 >= T_MIN) & (t64 <= t_max)
    # how far the fp64 geometry is from flipping its verdict: the discriminant, and each root against each end of the range
    scale = np.maximum(hb * hb, 1e-30)
    ends = np.minimum.reduce([np.abs(t0 - T_MIN), np.abs(t1 - T_MIN), np.abs(t0 - t_max), np.abs(t1 - t_max)]) / np.maximum(1.0, np.abs(t1)) * 10
    margin = np.where(disc < 0, np.abs(disc) / scale, np.minimum(np.abs(disc) / scale, np.nan_to_num(ends, posinf=1.0)))
    decided = margin > 2e-3  # (test_primitives_fuzz.py's margin)
    assert decided.mean() > 0.8, decided.mean()
    bad = decided & (hit32 != hit64)
    assert not bad.any(), (int(bad.sum()), int(np.flatnonzero(bad)[0]))
    both = decided & hit64
    assert both.sum() > 500 and (both & ~first).sum() > 50 and (decided & ~hit64 & (disc >= 0)).sum() > 50
    rel = np.abs(t32[both] - t64[both]) / np.maximum(1.0, np.abs(t64[both]))
    assert rel.max() < 2e-5, rel.max()  # (test_primitives_fuzz.py's tolerance)
    # a root equal to t_max is a hit (the later entry wins a tie), one ulp beyond it is not
    i = int(np.flatnonzero(both)[0])
    t = np.float32(t32[i])
    assert rtmi.moving_sphere_hit(mv, s[i], o[i], d[i], float(t)) == (True, float(t))
    below = rtmi.moving_sphere_hit(mv, s[i], o[i], d[i], float(np.nextafter(t, np.float32(0))))
    assert (not below[0]) or below[1] > t


def test_the_coverage_cap_is_rare(rtmi):
    """the premise of the GPU coverage test, from the reference alone: samples whose fp64 discriminant is within 1e-5 half_b^2 of
    zero -- the only ones on which kernel and fp64 may disagree -- are under 0.5 % of the samples, and the motion is there"""
    sc = MO.coverage_scene(rtmi)
    hit, rel, s = MO.coverage_reference(rtmi, sc)
    assert (np.abs(rel) < MO.COV_CAP).mean() < 0.005
    MO.assert_motion_is_seen(hit, s)


def test_buried_movers_are_unreachable(rtmi):
    sc = MS.three_spheres(rtmi)
    MO.bury_mover_three_spheres(sc)
    MO.check_buried_three_spheres(rtmi, sc)
    sc = MS.mixed_scene(rtmi)
    MO.bury_mover_mixed(sc)
    MO.check_buried_mixed(rtmi, sc)
