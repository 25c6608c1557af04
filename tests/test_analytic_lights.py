"""Analytic lights (point, spot and distant lights among the sampled emitters) without a GPU:
  1. the interface -- C, C++, Python, JSON, every argument rule and its status code, "target" against "direction", an unknown
     key, the round trip to the same packed image, rt_struct_size and the ABI version;
  2. rt_scene_get_lights -- the order (area emitters, analytic lights, environment), the probabilities against the fp64
     weights, and ref64.RefScene finding the alias table of such a scene unedited;
  3. the packed record's words for each type against fp64;
  4. with light sampling off and after clear_analytic_lights the packed image is that of the scene without the lights, and
     every scene recorded in tests/golden/bump_off_pack_digests.json keeps its digest (read here, not rewritten);
  5. a scene whose only light is a point light reports the light-sampling family;
  6. csrc/rt_lights.h compiled by the host compiler against the fp64 statement of ref64_analytic_lights.py (7r's rule: the C++
     code's share within tolerance is at least the fp32 numpy statement's minus 0.5 points);
  7. closed forms in fp64: alpha = 0 returns t bit for bit, the falloff at its edges, and the fold by quadrature over the cone.
The refusals with movers, media and the nested grid happen at render time, behind the device: test_gpu_analytic_lights.py
asserts them, and holds the kernels to the reference."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import analytic_light_scenes as AL
import bump_scenes as BS
import ref64 as R
import ref64_analytic_lights as RA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_ARG, RT_ERR_SCENE = 1, 4
NEE = 256
NAN, INF = float("nan"), float("inf")


def _base(rtmi):
    sc = rtmi.Scene.new(32, 18, 1, 4)
    sc.set_background((0, 0, 0), sky_gradient=False, defocus_blur=False)
    sc.camera((0, 1, 5), (0, 0.5, 0), (0, 1, 0), 40.0)
    sc.xz_rect(-4, 4, -4, 4, 0.0, sc.lambertian((0.5, 0.5, 0.5)))
    sc.sphere((0.0, 0.5, 0.0), 0.5, sc.lambertian((0.3, 0.5, 0.7)))
    return sc


def _three(rtmi):
    sc = _base(rtmi)
    ids = [sc.point_light((0.5, 2.0, 1.0), (3.0, 2.0, 1.0)), sc.spot_light((1.0, 3.0, 0.0), (0.0, -2.0, 0.5), (9.0, 8.0, 7.0), 10.0, 25.0),
           sc.distant_light((0.0, -3.0, -4.0), (2.0, 2.0, 1.5), 2.5)]
    return sc, ids


# ------------------------------------------------------------------------------------------------------------ 1. interface
def test_constructors_and_the_list(rtmi):
    assert rtmi.abi_version() == 3 and rtmi.struct_size(25) == rtmi.ANALYTIC_LIGHT_DTYPE.itemsize == 48
    assert (rtmi.LIGHT_POINT, rtmi.LIGHT_SPOT, rtmi.LIGHT_DISTANT) == (101, 102, 103)
    sc, ids = _three(rtmi)
    assert ids == [0, 1, 2]
    a = sc.analytic_lights()
    assert list(a["type"]) == [101, 102, 103]
    assert list(a[0]["position"]) == [0.5, 2.0, 1.0] and list(a[0]["color"]) == [3.0, 2.0, 1.0] and list(a[0]["angle"]) == [0, 0]
    assert list(a[1]["direction"]) == [0.0, -2.0, 0.5] and list(a[1]["angle"]) == [10.0, 25.0]          # (as given, not normalised)
    assert list(a[2]["direction"]) == [0.0, -3.0, -4.0] and list(a[2]["angle"]) == [2.5, 0.0] and list(a[2]["color"]) == [2.0, 2.0, 1.5]
    assert not sc.light_sampling  # (the constructors do not switch it on: only a JSON "lights" without a "light_sampling" key)
    v = sc.info
    sc.clear_analytic_lights()
    assert len(sc.analytic_lights()) == 0 and len(sc.lights()) == 0
    assert v.width == 32


def _c_lib(rtmi):
    lib = ctypes.CDLL(rtmi.LIB_PATH)
    lib.rt_scene_new.restype = ctypes.c_void_p
    lib.rt_scene_new.argtypes = [ctypes.c_int] * 4
    lib.rt_scene_free.argtypes, lib.rt_scene_free.restype = [ctypes.c_void_p], None
    lib.rt_last_error.restype = ctypes.c_char_p
    fp = ctypes.POINTER(ctypes.c_float)
    lib.rt_scene_add_point_light.argtypes, lib.rt_scene_add_point_light.restype = [ctypes.c_void_p, fp, fp], ctypes.c_int
    lib.rt_scene_add_spot_light.argtypes = [ctypes.c_void_p, fp, fp, fp, ctypes.c_float, ctypes.c_float]
    lib.rt_scene_add_distant_light.argtypes = [ctypes.c_void_p, fp, fp, ctypes.c_float]
    lib.rt_scene_get_analytic_lights.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.rt_scene_clear_analytic_lights.argtypes = [ctypes.c_void_p]
    lib.rt_struct_size.restype, lib.rt_struct_size.argtypes = ctypes.c_size_t, [ctypes.c_int]
    return lib


def test_the_c_entry_points_and_their_argument_rules(rtmi):
    lib = _c_lib(rtmi)
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    assert lib.rt_struct_size(25) == 48 and lib.rt_abi_version() == 3
    s = lib.rt_scene_new(8, 8, 1, 2)
    point, spot, distant = lib.rt_scene_add_point_light, lib.rt_scene_add_spot_light, lib.rt_scene_add_distant_light
    x, d, c = f3(0, 1, 0), f3(0, -1, 0), f3(1, 1, 1)
    try:
        assert point(s, x, c) == 0 and spot(s, x, d, c, 10.0, 20.0) == 1 and distant(s, d, c, 0.0) == 2
        assert spot(s, x, d, c, 0.0, 179.0) == 3 and spot(s, x, d, c, 30.0, 30.0) == 4 and distant(s, d, c, 45.0) == 5
        assert point(s, x, f3(0, 0, 1e-30)) == 6  # (a colour with one tiny positive channel is a colour)
        bad = [lambda: point(s, x, f3(0, 0, 0)), lambda: point(s, x, f3(-1, 1, 1)), lambda: point(s, x, f3(NAN, 1, 1)), lambda: point(s, x, f3(1, INF, 1)),
               lambda: point(s, f3(NAN, 0, 0), c), lambda: point(s, f3(0, INF, 0), c), lambda: point(s, None, c), lambda: point(s, x, None),
               lambda: point(None, x, c),
               lambda: spot(s, x, f3(0, 0, 0), c, 10.0, 20.0), lambda: spot(s, x, f3(0, NAN, 0), c, 10.0, 20.0), lambda: spot(s, x, f3(INF, 0, 0), c, 10.0, 20.0),
               lambda: spot(s, x, d, c, 20.0, 10.0), lambda: spot(s, x, d, c, -1.0, 10.0), lambda: spot(s, x, d, c, 0.0, 0.0),
               lambda: spot(s, x, d, c, 10.0, 179.5), lambda: spot(s, x, d, c, NAN, 20.0), lambda: spot(s, x, d, c, 10.0, NAN),
               lambda: spot(s, x, d, f3(0, 0, 0), 10.0, 20.0), lambda: spot(s, x, None, c, 10.0, 20.0), lambda: spot(s, f3(0, NAN, 0), d, c, 10.0, 20.0),
               lambda: distant(s, f3(0, 0, 0), c, 1.0), lambda: distant(s, f3(NAN, 0, 0), c, 1.0), lambda: distant(s, d, c, -0.1),
               lambda: distant(s, d, c, 45.5), lambda: distant(s, d, c, NAN), lambda: distant(s, d, f3(0, -1, 0), 1.0), lambda: distant(s, d, f3(0, 0, 0), 1.0),
               lambda: distant(s, None, c, 1.0), lambda: distant(None, d, c, 1.0)]
        for k, call in enumerate(bad):
            assert call() == -RT_ERR_ARG, k
            assert lib.rt_last_error(), k
        assert lib.rt_scene_get_analytic_lights(s, None, 0) == 7  # (a refused light is not added)
        out = np.zeros(7, rtmi.ANALYTIC_LIGHT_DTYPE)
        assert lib.rt_scene_get_analytic_lights(s, out.ctypes.data_as(ctypes.c_void_p), 7) == 7
        assert list(out["type"]) == [101, 102, 103, 102, 102, 103, 101] and list(out[4]["angle"]) == [30.0, 30.0]
        assert lib.rt_scene_clear_analytic_lights(s) == 0 and lib.rt_scene_get_analytic_lights(s, None, 0) == 0
        assert lib.rt_scene_clear_analytic_lights(None) == RT_ERR_ARG and lib.rt_scene_get_analytic_lights(None, None, 0) == -RT_ERR_ARG
    finally:
        lib.rt_scene_free(s)
    sc = rtmi.Scene.new(8, 8, 1, 2)
    for call in (lambda: sc.point_light((0, 0, 0), (0, 0, 0)), lambda: sc.spot_light((0, 0, 0), (0, 0, 0), (1, 1, 1), 1, 2),
                 lambda: sc.spot_light((0, 0, 0), (0, 1, 0), (1, 1, 1), 3, 2), lambda: sc.distant_light((0, -1, 0), (1, 1, 1), 46)):
        with pytest.raises(rtmi.RtmiError) as e:
            call()
        assert e.value.status == RT_ERR_ARG


def test_json_reads_writes_and_refuses(rtmi):
    sc, _ = _three(rtmi)
    sc.set_light_sampling(True)
    text = sc.to_json()
    d = json.loads(text)
    assert d["light_sampling"] is True
    assert d["lights"] == [{"type": "point", "position": [0.5, 2, 1], "intensity": [3, 2, 1]},
                           {"type": "spot", "position": [1, 3, 0], "direction": [0, -2, 0.5], "inner_angle": 10, "outer_angle": 25, "intensity": [9, 8, 7]},
                           {"type": "distant", "direction": [0, -3, -4], "irradiance": [2, 2, 1.5], "angular_radius": 2.5}]
    back = rtmi.Scene.parse(text)
    assert back.analytic_lights().tobytes() == sc.analytic_lights().tobytes() and back.lights().tobytes() == sc.lights().tobytes()
    assert back.light_sampling and back.table_image().tobytes() == sc.table_image().tobytes()

    def with_lights(lights, **top):
        e = json.loads(text)
        e["lights"] = lights
        e.pop("light_sampling")
        e.update(top)
        return json.dumps(e)
    # "lights" without a "light_sampling" key switches light sampling on; an explicit false is respected, and written back
    assert rtmi.Scene.parse(with_lights(d["lights"])).light_sampling
    off = rtmi.Scene.parse(with_lights(d["lights"], light_sampling=False))
    assert not off.light_sampling and len(off.analytic_lights()) == 3 and json.loads(off.to_json())["light_sampling"] is False
    assert not rtmi.Scene.parse(off.to_json()).light_sampling
    e = json.loads(text)
    e.pop("light_sampling"), e.pop("lights")
    assert not rtmi.Scene.parse(json.dumps(e)).light_sampling
    # "target" against "direction": the direction is target - position; the angular radius defaults to 0
    spot = dict(d["lights"][1])
    aim = {k: v for k, v in spot.items() if k != "direction"}
    aim["target"] = [1, 1, 0.5]
    got = rtmi.Scene.parse(with_lights([aim])).analytic_lights()[0]
    assert list(got["direction"]) == [0.0, -2.0, 0.5] and "target" not in rtmi.Scene.parse(with_lights([aim])).to_json()
    sun = {k: v for k, v in d["lights"][2].items() if k != "angular_radius"}
    assert list(rtmi.Scene.parse(with_lights([sun])).analytic_lights()[0]["angle"]) == [0, 0]
    point = d["lights"][0]
    bad = [dict(point, radius=1), dict(point, direction=[0, 1, 0]), dict(point, color=[1, 1, 1]), {k: v for k, v in point.items() if k != "intensity"},
           {k: v for k, v in point.items() if k != "position"}, dict(point, intensity=[0, 0, 0]), dict(point, intensity=[1, -1, 1]),
           dict(point, intensity=[1, 1]), dict(point, type="area"), {k: v for k, v in point.items() if k != "type"}, "point",
           dict(spot, target=[0, 0, 0]), aim | {"falloff": 2}, {k: v for k, v in aim.items() if k != "target"}, dict(aim, target=spot["position"]),
           dict(spot, inner_angle=30), dict(spot, outer_angle=180), dict(spot, inner_angle=-1), {k: v for k, v in spot.items() if k != "outer_angle"},
           dict(spot, irradiance=[1, 1, 1]), dict(sun, position=[0, 0, 0]), dict(sun, intensity=[1, 1, 1]), dict(sun, angular_radius=50),
           dict(sun, angular_radius=-1), dict(sun, direction=[0, 0, 0]), dict(sun, irradiance=[0, 0, 0]), dict(sun, target=[0, 0, 0])]
    for k, light in enumerate(bad):
        with pytest.raises(rtmi.RtmiError) as err:
            rtmi.Scene.parse(with_lights([light]))
        assert err.value.status == RT_ERR_SCENE, (k, str(err.value))
    with pytest.raises(rtmi.RtmiError) as err:
        rtmi.Scene.parse(with_lights({"data": []}))
    assert err.value.status == RT_ERR_SCENE


def test_the_shipped_scene_and_the_cpp_wrapper(rtmi, scenes_dir, tmp_path):
    sc = rtmi.Scene.load(os.path.join(scenes_dir, "spot_stage.json"))
    a = sc.analytic_lights()
    assert sorted(a["type"]) == [101, 102, 102, 103]
    assert not sc.light_sampling  # (an explicit false: left to --nee, as in every shipped scene)
    sc.set_light_sampling(True)
    sun = a[a["type"] == 103][0]
    assert 0 < sun["angle"][0] <= 2 and len(sc.lights()) == 4 and sc.table_info().kernel_variant & NEE
    assert len(np.unique(sc.materials()["type"])) >= 4
    src = tmp_path / "w.cpp"
    src.write_text('#include "rtmi.hpp"\n#include <cstdio>\nint main() {\n'
                   "  rtmi::scene s(16, 9, 1, 3);\n"
                   "  if (s.point_light(rtmi::point3(0, 2, 0), rtmi::color(1, 2, 3)) != 0) return 2;\n"
                   "  if (s.spot_light(rtmi::point3(1, 2, 0), rtmi::vec3(0, -1, 0), rtmi::color(4, 4, 4), 10.0f, 20.0f) != 1) return 3;\n"
                   "  if (s.distant_light(rtmi::vec3(0, -1, 1), rtmi::color(2, 2, 2)) != 2) return 4;\n"
                   "  if (s.analytic_lights().size() != 3 || s.analytic_lights()[2].angle[0] != 0.0f) return 5;\n"
                   "  try { s.distant_light(rtmi::vec3(0, 0, 0), rtmi::color(2, 2, 2), 1.0f); return 6; } catch (const std::exception &) {}\n"
                   '  std::vector<char> b(1 << 16);\n  size_t n = rt_scene_to_json(s.handle(), b.data(), b.size());\n'
                   '  if (n == 0 || n > b.size()) return 1;\n  fputs(b.data(), stdout);\n'
                   "  s.clear_analytic_lights();\n  return s.analytic_lights().empty() ? 0 : 7;\n}\n")
    exe = str(tmp_path / "w")
    pkg = os.path.dirname(rtmi.LIB_PATH)
    build = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src), "-L", pkg, "-lrtmi", "-Wl,-rpath," + pkg],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    lights = json.loads(out.stdout)["lights"]
    assert [l["type"] for l in lights] == ["point", "spot", "distant"] and lights[1]["outer_angle"] == 20 and lights[2]["angular_radius"] == 0


# ------------------------------------------------------------------------------------------------------------ 2. the list
def _mixed(rtmi):
    """a quad light, a sphere light, one light of each new type and an environment"""
    sc = _base(rtmi)
    sc.quad((-0.5, 2.8, -1.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.sphere((2.3, 1.9, -1.0), 0.25, sc.diffuse_light((5.0, 6.0, 7.0)))
    sc.point_light((0.5, 2.0, 1.0), (3.0, 2.0, 1.0))
    sc.spot_light((1.0, 3.0, 0.0), (0.0, -2.0, 0.5), (9.0, 8.0, 7.0), 10.0, 25.0)
    sc.distant_light((0.0, -3.0, -4.0), (0.2, 0.2, 0.15), 2.5)
    env = np.full((4, 8, 3), 0.05, np.float32)
    env[1, 2] = (3.0, 2.5, 2.0)
    sc.set_environment(env, 1.0, 0.0)
    return sc


def test_the_list_of_lights_its_order_and_probabilities(rtmi):
    sc = _mixed(rtmi)
    L = sc.lights()
    assert list(L["shape"]) == [6, 0, 101, 102, 103, 100] and list(L["prim"][2:]) == [-1, -1, -1, -1] and (L["prim"][:2] >= 0).all()
    r = RA.bound_radius(sc.prims())
    recs = [RA.record(al, r) for al in sc.analytic_lights()]
    ci, co = np.cos(np.radians(10.0)), np.cos(np.radians(25.0))
    assert np.allclose([x["measure"] for x in recs], [4 * np.pi, 2 * np.pi * (1 - (ci + co) / 2), np.pi * r * r], rtol=1e-14)
    assert np.allclose(L["area"][2:5], [x["measure"] for x in recs], rtol=1e-6)
    lum = RA.luminance
    want = [4 * lum((3, 2, 1)), 2 * (1 - (ci + co) / 2) * lum((9, 8, 7)), r * r * lum(np.array((0.2, 0.2, 0.15), np.float32))]
    assert np.allclose([x["weight"] for x in recs], want, rtol=1e-12)
    # the area emitters' weights are area x mean luminance; the environment's is what is left: every ratio holds
    area = [L["area"][0].astype(np.float64) * lum(L["emission"][0]), L["area"][1].astype(np.float64) * lum(L["emission"][1])]
    p = L["probability"].astype(np.float64)
    assert abs(p.sum() - 1) < 1e-6
    w = np.array(area + want)
    assert np.allclose(p[:5] / p[0], w / w[0], rtol=2e-6)
    # the colour words: as given for point and spot, a distant light's with the fold 2 / (1 + cos alpha), in fp64 rounded once
    assert list(L["emission"][2]) == [3, 2, 1] and list(L["emission"][3]) == [9, 8, 7] and np.array_equal(L["emission"], L["emission_odd"])
    fold = 2 / (1 + np.cos(np.radians(2.5)))
    assert np.array_equal(L["emission"][4], (np.array((0.2, 0.2, 0.15), np.float32).astype(np.float64) * fold).astype(np.float32))
    # with exactly these words ref64 finds the light records and the alias table in the packed image, once
    sc.set_light_sampling(True)
    S = R.RefScene(sc)
    assert len(S.thr) == 6 and sorted(S.analytic) == [2, 3, 4]
    assert np.allclose(R.implied_alias_probability(S.thr, S.alias), p, atol=1e-6)
    # a light whose weight is not positive and finite is left out: a distant light in a scene without primitives
    empty = rtmi.Scene.new(8, 8, 1, 2)
    empty.distant_light((0, -1, 0), (1, 1, 1), 1.0)
    empty.point_light((0, 1, 0), (1, 1, 1))
    assert list(empty.lights()["shape"]) == [101] and len(empty.analytic_lights()) == 2


# ------------------------------------------------------------------------------------------------------------ 3. the record
def _records_at(sc):
    """the 28 words of every light record of the packed image, found by {shape, -1 or id, probability} of the first light"""
    L = sc.lights()
    w = np.ascontiguousarray(sc.table_image(), np.float32).reshape(-1)
    thr, _ = R.find_alias_table(w, L)
    bits = w.view(np.int32)
    at = [k for k in np.flatnonzero(w[2::4] == L["probability"][0]) * 4
          if k + 28 * len(L) <= len(w) and np.array_equal(w[k + 2:k + 28 * len(L):28], L["probability"])
          and (L["shape"][0] == 100 or np.array_equal(w[k + 4:k + 7], L["emission"][0])) and 0 <= bits[k] <= 8
          and np.isclose(w[k + 3], 1 / np.float64(L["area"][0]), rtol=1e-6)]
    assert len(at) == 1, at
    return w[at[0]:at[0] + 28 * len(L)].reshape(len(L), 28), bits[at[0]:at[0] + 28 * len(L)].reshape(len(L), 28)


def test_the_packed_records(rtmi):
    sc = _mixed(rtmi)
    sc.spot_light((0.0, 2.0, 0.0), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 30.0, 30.0)   # inner == outer: inv = FLT_MAX
    sc.distant_light((0.0, 5.0, 0.0), (0.3, 0.2, 0.1), 0.0)                           # straight up, alpha = 0
    sc.set_light_sampling(True)
    L = sc.lights()
    assert list(L["shape"]) == [6, 0, 101, 102, 103, 102, 103, 100]
    f, b = _records_at(sc)
    assert list(b[:, 0]) == [5, 0, 6, 7, 8, 7, 8, 3] and list(b[2:, 1]) == [-1] * 6
    assert np.allclose(f[:, 3], 1 / L["area"].astype(np.float64), rtol=1e-6)
    for i in range(2, 7):
        assert np.array_equal(f[i, 4:7], L["emission"][i]) and np.array_equal(f[i, 8:11], L["emission"][i]) and b[i, 7] == 0 and b[i, 11] == 0
    r = RA.bound_radius(sc.prims())
    recs = [RA.record(al, r) for al in sc.analytic_lights()]
    zeros = lambda x: not np.any(x)
    # point: {x, 0} and nothing else
    assert list(f[2, 12:15]) == [0.5, 2.0, 1.0] and zeros(f[2, 15:])
    # spot: {x, 0} {a, 0} {cos_o, inv, 0, 0}; the axis normalised in fp64
    for i, rec, axis in ((3, recs[1], (0.0, -2.0, 0.5)), (5, recs[3], (1.0, 1.0, 1.0))):
        a = np.array(axis, np.float64)
        assert np.array_equal(f[i, 12:15], rec["x"]) and f[i, 15] == 0
        assert np.array_equal(f[i, 16:19], (a / np.sqrt((a * a).sum())).astype(np.float32)) and f[i, 19] == 0
        assert f[i, 20] == rec["cos_o"] and f[i, 21] == rec["inv"] and zeros(f[i, 22:])
    ci, co = np.cos(np.radians(10.0)), np.cos(np.radians(25.0))
    assert f[3, 20] == np.float32(co) and f[3, 21] == np.float32(1 / (ci - co))
    assert f[5, 20] == np.float32(np.cos(np.radians(30.0))) and f[5, 21] == np.finfo(np.float32).max
    # distant: {t towards the light, 1 - cos alpha} {D = 4 r, 0, 0, 0}
    assert np.array_equal(f[4, 12:15], np.array([0.0, 0.6, 0.8], np.float32)) and f[4, 15] == np.float32(1 - np.cos(np.radians(2.5)))
    assert f[4, 16] == np.float32(4 * r) and zeros(f[4, 17:])
    assert list(f[6, 12:16]) == [0.0, -1.0, 0.0, 0.0] and not np.signbit(f[6, 12:15:2]).any() and f[6, 16] == np.float32(4 * r)
    assert np.array_equal(f[6, 4:7], np.array((0.3, 0.2, 0.1), np.float32))  # (alpha = 0: the fold is 1)
    # the environment's selection probability is still the last light's (the kernels read it from the parameters)
    assert sc.table_info().kernel_variant & NEE


# ------------------------------------------------------------------------------------------------------------ 4. switched off
def test_off_and_cleared_pack_the_scene_without_the_lights(rtmi):
    for build in (_base, lambda m: AL.spots(m), lambda m: AL.sun_env(m)):
        sc = build(rtmi)
        had = len(sc.analytic_lights())
        for ls in (False, True):
            sc.set_light_sampling(ls)
            bare = rtmi.Scene.parse(sc.to_json())
            bare.clear_analytic_lights()
            assert bare.light_sampling == ls
            want = bare.table_image().tobytes()
            if build is _base:
                sc.point_light((0, 2, 0), (1, 1, 1)), sc.spot_light((0, 2, 0), (0, -1, 0), (1, 1, 1), 5, 9), sc.distant_light((0, -1, 0), (1, 1, 1), 1)
            lit = sc.table_image().tobytes()
            assert (lit == want) == (not ls), (ls, had)     # off: the bytes of the scene without them; on: other tables
            if build is _base:
                sc.clear_analytic_lights()
                assert sc.table_image().tobytes() == want
    # clearing a scene that has none leaves its version alone (the device copy stays valid)
    sc = _base(rtmi)
    before = sc.table_image().tobytes()
    sc.clear_analytic_lights()
    assert sc.table_image().tobytes() == before


def test_scenes_without_the_lights_pack_as_before(rtmi, scenes_dir, golden_dir, tmp_path):
    """every scene and pack case recorded before the feature: the digests tests/golden/bump_off_pack_digests.json holds"""
    with open(os.path.join(golden_dir, "bump_off_pack_digests.json")) as f:
        want = json.load(f)
    cases = BS.digest_cases(rtmi, scenes_dir, str(tmp_path))
    assert set(cases) == set(want) and len(want) >= 20
    for name, build in cases.items():
        sc = build()
        assert len(sc.analytic_lights()) == 0 and BS.digest(sc) == want[name], name


# ------------------------------------------------------------------------------------------------------------ 5. the family
def test_a_point_light_alone_makes_a_light_sampling_scene(rtmi):
    sc = rtmi.Scene.new(32, 18, 1, 4)
    sc.sphere((0, 0, 0), 1.0, sc.lambertian((0.5, 0.5, 0.5)))
    plain = sc.table_info().kernel_variant
    assert not plain & NEE
    sc.point_light((0, 3, 0), (5, 5, 5))
    assert sc.table_info().kernel_variant == plain     # light sampling is off
    sc.set_light_sampling(True)
    v = sc.table_info().kernel_variant
    assert v & NEE and v & 255 in (16, 36, 44), v      # (sphere-only as it is: the wide tables and the general kernels)
    sc.clear_analytic_lights()
    assert sc.table_info().kernel_variant == plain


# --------------------------------------------------------------------------------------------- 6. fp32 code, fp64 statement
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("analytic_lights")
    exe, fin, fout = (str(d / n) for n in ("analytic_light_host_driver", "in.bin", "out.bin"))
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "analytic_light_host_driver.cpp"), "-lm"], check=True)
    rec = AL.records()
    rec.tofile(fin)
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    return rec, np.fromfile(fout, np.float32).reshape(-1, AL.OUTPUT_WORDS)


def test_the_fp32_code_against_the_fp64_statement(driver):
    """Measured here: per type, the C++ code's and the float32 numpy statement's share of the same-branch records
    within 1e-4 max(1, |ref|), and the share on another branch (a spot sample made by one and not by the other: the vertex
    sits on the outer edge)."""
    rec, got = driver
    assert rec.shape == (60000, AL.RECORD_WORDS)
    got = got.astype(np.float64)
    ref, ref32 = AL.statement(rec, np.float64), AL.statement(rec, np.float32)
    for t, name in ((RA.POINT, "point"), (RA.SPOT, "spot"), (RA.DISTANT, "distant")):
        k = rec[:, 0] == t
        assert k.sum() == 20000
        (code, code_flips), (numpy32, numpy_flips) = AL.share(got[k], ref[k]), AL.share(ref32[k], ref[k])
        print(f"\nrt_lights.h on the host, {name}: within tolerance {100 * code:.3f} % of the same-branch records, branch differs on "
              f"{100 * code_flips:.3f} %; the numpy statement at float32 {100 * numpy32:.3f} %, {100 * numpy_flips:.3f} %")
        assert numpy_flips <= 0.005 and code_flips <= 0.005, (name, numpy_flips, code_flips)
        assert code >= numpy32 - 0.005, (name, code, numpy32)
    # the records hold what they are there for: spot vertices near both edges on both sides, inner == outer, alpha = 0 and beyond
    s = rec[:, 0] == RA.SPOT
    fall = ref[s, 4]
    assert (fall == 0).mean() > 0.2 and (fall == 1).mean() > 0.1 and ((fall > 0) & (fall < 0.05)).sum() > 100 and ((fall > 0.95) & (fall < 1)).sum() > 100
    assert (rec[s, 13] == np.finfo(np.float32).max).sum() > 1000
    d = rec[:, 0] == RA.DISTANT
    assert (rec[d, 14] == 0).sum() > 3000 and (rec[d, 14] > 0.29).sum() > 10 and rec[d, 14].max() <= np.float32(1 - np.cos(np.pi / 4))


# ------------------------------------------------------------------------------------------------------- 7. closed forms
def test_alpha_zero_returns_the_direction_bit_for_bit(driver):
    rec, got = driver
    k = (rec[:, 0] == RA.DISTANT) & (rec[:, 14] == 0)
    assert k.sum() > 3000
    # the driver's ld is D w in one fp32 product: w = t exactly iff ld = D t
    assert np.array_equal(got[k, 0:3], rec[k, 15][:, None] * rec[k, 6:9])
    # and the fp64 statement, with zeros of either sign among the components and the pole of the frame
    rng = np.random.default_rng(1)
    t = rng.normal(size=(500, 3))
    t /= np.sqrt((t * t).sum(axis=1))[:, None]
    t = np.concatenate([t, np.eye(3), -np.eye(3)])
    w = RA.cone_direction(t, 0.0, rng.uniform(0, 1, len(t)), rng.uniform(0, 1, len(t)), np.float64)
    assert np.array_equal(w, t)


def test_the_falloff_at_its_edges(rtmi):
    T = np.float64
    for inner, outer in ((10.0, 25.0), (0.0, 40.0), (60.0, 179.0)):
        sc = _base(rtmi)
        sc.spot_light((0, 2, 0), (0, -3, 0), (1, 1, 1), inner, outer)
        sc.set_light_sampling(True)
        f, _ = _records_at(sc)
        rec = dict(axis=f[0, 16:19], cos_o=f[0, 20], inv=f[0, 21])   # the product's record
        mine = RA.record(sc.analytic_lights()[0], 1.0)
        assert np.array_equal(rec["axis"], mine["axis"]) and rec["cos_o"] == mine["cos_o"] and rec["inv"] == mine["inv"]
        exact = dict(axis=np.array([0.0, -1.0, 0.0]), cos_o=np.cos(np.radians(outer)), inv=1 / (np.cos(np.radians(inner)) - np.cos(np.radians(outer))))
        at = lambda deg: -np.array([[np.sin(np.radians(deg)), -np.cos(np.radians(deg)), 0.0]]) * 2.5   # ld of a vertex at deg from the axis
        assert abs(RA.falloff_of(exact, at(outer), T)[0]) < 1e-12 and abs(RA.falloff_of(exact, at(inner), T)[0] - 1) < 1e-12
        assert RA.falloff_of(exact, at(outer + 0.5), T)[0] == 0 and RA.falloff_of(exact, at(max(inner - 0.5, 0)), T)[0] == 1
        mid = RA.falloff_of(exact, at(np.degrees(np.arccos((np.cos(np.radians(inner)) + np.cos(np.radians(outer))) / 2))), T)[0]
        assert abs(mid - 0.5) < 1e-12
        # the record's fp32 words give the same to fp32 precision
        assert abs(RA.falloff_of(rec, at((inner + outer) / 2), T)[0] - RA.falloff_of(exact, at((inner + outer) / 2), T)[0]) < 1e-5
        f = RA.falloff_of(exact, np.concatenate([at(x) for x in np.linspace(inner, outer, 50)]), T)
        assert (np.diff(f) <= 0).all()


def test_the_fold_by_quadrature_over_the_cone(rtmi):
    """the lambertian irradiance under a distant light of radiance E / (pi sin^2 alpha) over its cone is E cos(theta0) while the
    whole cone is above the horizon; the estimator's mean, fcos x (E fold) with fcos = cos / pi x pi (irradiance), is the same"""
    E = 2.0
    n = 800
    u1, u2 = np.meshgrid((np.arange(n) + 0.5) / n, (np.arange(n) + 0.5) / n, indexing="ij")
    u1, u2 = u1.ravel(), u2.ravel()
    for alpha in (1.0, 10.0, 30.0):
        a = np.radians(alpha)
        for theta0 in (0.0, 25.0, 89.5 - alpha):
            t0 = np.radians(theta0)
            t = np.array([np.sin(t0), np.cos(t0), 0.0])
            w = RA.cone_direction(t, 1 - np.cos(a), u1, u2, np.float64)
            assert np.allclose((w * w).sum(axis=1), 1, atol=1e-12) and (w @ t >= np.cos(a) - 1e-12).all()
            cos = w[:, 1]
            assert (cos > 0).all()
            # the integral of L cos over the cone, by the uniform samples: L Omega mean(cos)
            omega = 2 * np.pi * (1 - np.cos(a))
            irradiance = E / (np.pi * np.sin(a) ** 2) * omega * cos.mean()
            assert abs(irradiance - E * np.cos(t0)) < 1e-6 * E, (alpha, theta0, irradiance)
            # and the estimator with the fold: mean(cos) x E x 2 / (1 + cos alpha)
            sc = _base(rtmi)
            sc.distant_light(tuple(-t), (E, E, E), alpha)
            rec = RA.record(sc.analytic_lights()[0], 3.0)
            assert abs(rec["fold"] - omega / (np.pi * np.sin(a) ** 2)) < 1e-12
            colour = sc.lights()[0]["emission"]      # the product's folded colour
            assert np.array_equal(colour, rec["colour"])
            assert abs(cos.mean() * float(colour[0]) - E * np.cos(t0)) < 2e-6 * E
