"""Tangent-space normal maps (an image texture's texel, read in the surface's tangent frame, replaces the shading
normal) without a GPU:
  1. the interface -- C, Python, C++, JSON, every argument rule, the bump / map exclusion, the round trip, the unchanged ABI --
     and the packed records; every scene of the recorded digests packs to the bytes it packed to;
  2. the frame against the parametrisation, independently: for each of the five shapes the unit T and B of the numpy statement
     (ref64_normal_map.raw_tangents) against central differences of ref64.hit_uv in the plane of the surface;
  3. csrc/rt_tangent.h compiled by the host compiler against the fp64 statement on 20 000 seeded records per shape (the code's
     share within tolerance is at least the fp32 numpy statement's minus 0.5 points; guards and keep-n cases on every record);
  4. the model: n' is unit, n' . n > 0, s -> -s mirrors the tangential part, both sides see one relief, the texels that leave n;
  5. ref64_normal_map.trace: ref64.trace's results exactly on a case without maps; a case holds its vertices and the deliberate
     mistakes change it.
test_gpu_normal_map.py holds the kernels to that reference."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bump_scenes as BS
import nee_scenes as NS
import normal_map_scenes as NMS
import ref64 as R
import ref64_normal_map as NM
import smooth_pack_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
RT_ERR_ARG, RT_ERR_SCENE = 1, 4
T = np.float64


# ------------------------------------------------------------------------------------------------------------ 1. interface
def _seven(rtmi):
    """a sphere of every material that takes a map and an emitter, two map images, a noise and a solid texture"""
    sc = rtmi.Scene.new(32, 18, 1, 4)
    sc.camera((0, 1, 6), (0, 0.5, 0), (0, 1, 0), 40.0)
    img = [sc.image_texture(NMS.relief(**NMS.M_WAVES)), sc.image_texture(NMS.relief(rows=8, cols=12, **NMS.M_DIMPLES))]
    solid = sc.solid_color((0.5, 0.5, 0.5))
    noise = sc.noise_texture((0, 0, 0), (1, 1, 1), style="fbm", scale=1.5, octaves=3, seed=7)
    ids = [sc.lambertian(solid), sc.metal((0.8, 0.8, 0.8), 0.1), sc.dielectric(1.5), sc.rough_metal((0.9, 0.7, 0.4), 0.3), sc.plastic(solid, 1.5, 0.3),
           sc.rough_glass(1.5, 0.2), sc.pbr(solid, 0.5, 0.4), sc.diffuse_light((4.0, 4.0, 4.0))]
    for k, m in enumerate(ids):
        sc.sphere((k - 3.5, 0.5, 0.0), 0.4, m)
    return sc, img, solid, noise, ids


def test_python_sets_gets_removes_and_refuses(rtmi):
    sc, img, solid, noise, ids = _seven(rtmi)
    assert rtmi.MATERIAL_DTYPE.itemsize == 28 == rtmi.struct_size(3) and rtmi.abi_version() == 3
    before = sc.materials().tobytes()
    assert all(sc.normal_map(m) is None for m in ids)
    for k, m in enumerate(ids[:7]):
        sc.set_normal_map(m, img[k % 2], 0.25 * (k + 1) * (-1) ** k)
        assert sc.normal_map(m) == (img[k % 2], float(np.float32(0.25 * (k + 1) * (-1) ** k)))
    sc.set_normal_map(ids[0], img[0])
    assert sc.normal_map(ids[0]) == (img[0], 1.0)  # (the default scale)
    assert sc.materials().tobytes() == before  # (a side table: the material records do not change)
    assert sc.clone().normal_map(ids[3]) == sc.normal_map(ids[3])
    nan, inf = float("nan"), float("inf")
    light = ids[7]
    for call in (lambda: sc.set_normal_map(99, img[0], 0.5), lambda: sc.set_normal_map(-1, img[0], 0.5), lambda: sc.set_normal_map(light, img[0], 0.5),
                 lambda: sc.set_normal_map(light, -1, 0.0), lambda: sc.set_normal_map(ids[0], solid, 0.5), lambda: sc.set_normal_map(ids[0], noise, 0.5),
                 lambda: sc.set_normal_map(ids[0], 99, 0.5), lambda: sc.set_normal_map(ids[0], -2, 0.5), lambda: sc.set_normal_map(ids[0], img[0], nan),
                 lambda: sc.set_normal_map(ids[0], img[0], inf), lambda: sc.set_normal_map(ids[0], img[0], -inf), lambda: sc.set_normal_map(ids[0], -1, nan),
                 lambda: sc.normal_map(99), lambda: sc.normal_map(-1),
                 lambda: sc.set_bump(ids[1], noise, 0.2)):  # (a material carries a bump or a map, not both)
        with pytest.raises(rtmi.RtmiError) as e:
            call()
        assert e.value.status == RT_ERR_ARG, str(e.value)
    assert sc.normal_map(ids[0]) == (img[0], 1.0) and sc.bump(ids[1]) is None  # (a refused call changes nothing)
    sc.set_normal_map(ids[0], -1, 0.7)
    sc.set_normal_map(ids[1], img[1], 0.0)
    assert sc.normal_map(ids[0]) is None and sc.normal_map(ids[1]) is None and sc.normal_map(ids[2]) is not None
    # the exclusion the other way round, and removal of either frees the material for the other
    sc.set_bump(ids[0], noise, 0.2)
    with pytest.raises(rtmi.RtmiError) as e:
        sc.set_normal_map(ids[0], img[0], 1.0)
    assert e.value.status == RT_ERR_ARG and sc.normal_map(ids[0]) is None and sc.bump(ids[0]) is not None
    sc.set_normal_map(ids[0], -1, 0.0)  # (removing what is not there: allowed beside a bump)
    sc.set_bump(ids[2], -1, 0.0)        # (and the other way round)
    assert sc.normal_map(ids[2]) is not None
    sc.set_bump(ids[0], -1, 0.0)
    sc.set_normal_map(ids[0], img[0], 1.0)
    for name in ("rt_scene_set_normal_map", "rt_scene_get_normal_map"):
        assert name in rtmi.C_SYMBOLS


def test_the_c_entry_points(rtmi):
    lib = ctypes.CDLL(rtmi.LIB_PATH)
    sc, img, solid, noise, ids = _seven(rtmi)
    lib.rt_scene_set_normal_map.argtypes, lib.rt_scene_set_normal_map.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float], ctypes.c_int
    lib.rt_scene_get_normal_map.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)]
    lib.rt_scene_get_normal_map.restype = ctypes.c_int
    lib.rt_scene_set_bump.argtypes, lib.rt_scene_set_bump.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float], ctypes.c_int
    lib.rt_last_error.restype = ctypes.c_char_p
    s = sc._h
    t, k = ctypes.c_int(5), ctypes.c_float(5)
    assert lib.rt_scene_get_normal_map(s, ids[2], ctypes.byref(t), ctypes.byref(k)) == 0 and (t.value, k.value) == (-1, 0.0)
    assert lib.rt_scene_set_normal_map(s, ids[2], img[0], 0.25) == 0
    assert lib.rt_scene_get_normal_map(s, ids[2], ctypes.byref(t), ctypes.byref(k)) == 0 and (t.value, k.value) == (img[0], 0.25)
    assert lib.rt_scene_get_normal_map(s, ids[2], None, None) == 0 and lib.rt_scene_get_normal_map(s, ids[2], ctypes.byref(t), None) == 0
    for call in (lambda: lib.rt_scene_set_normal_map(None, ids[2], img[0], 0.25), lambda: lib.rt_scene_set_normal_map(s, len(ids), img[0], 0.25),
                 lambda: lib.rt_scene_set_normal_map(s, ids[7], img[0], 0.25), lambda: lib.rt_scene_set_normal_map(s, ids[1], solid, 0.25),
                 lambda: lib.rt_scene_set_normal_map(s, ids[1], noise, 0.25), lambda: lib.rt_scene_set_normal_map(s, ids[1], img[0], float("nan")),
                 lambda: lib.rt_scene_set_bump(s, ids[2], noise, 0.25),
                 lambda: lib.rt_scene_get_normal_map(None, 0, None, None), lambda: lib.rt_scene_get_normal_map(s, len(ids), ctypes.byref(t), ctypes.byref(k))):
        assert call() == RT_ERR_ARG and lib.rt_last_error()
    assert lib.rt_scene_set_normal_map(s, ids[2], -1, 0.0) == 0 and sc.normal_map(ids[2]) is None
    assert lib.rt_scene_set_bump(s, ids[2], noise, 0.25) == 0 and lib.rt_scene_set_normal_map(s, ids[2], img[0], 1.0) == RT_ERR_ARG


def test_json_reads_writes_and_refuses(rtmi):
    sc, img, solid, noise, ids = _seven(rtmi)
    for k, m in enumerate(ids[:7]):
        sc.set_normal_map(m, img[k % 2], 0.125 * (k + 1))
    text = sc.to_json()
    mats = json.loads(text)["material"]["data"]
    assert [m.get("normal_map") for m in mats] == [{"texture": img[k % 2], "scale": 0.125 * (k + 1)} for k in range(7)] + [None]
    back = rtmi.Scene.parse(text)
    assert [back.normal_map(m) for m in ids] == [sc.normal_map(m) for m in ids]
    assert back.table_image().tobytes() == sc.table_image().tobytes()
    assert back.to_json() == text

    def with_material(i, x):
        d = json.loads(text)
        d["material"]["data"][i] = x
        return json.dumps(d)
    for i in range(7):
        rtmi.Scene.parse(with_material(i, mats[i]))
    nm = {"texture": img[0], "scale": 0.5}
    bad = [(7, dict(mats[7], normal_map=nm))]  # a diffuse_light
    for i in range(7):
        bad += [(i, dict(mats[i], normal_map=dict(nm, strength=1))), (i, dict(mats[i], normal_map={"scale": 0.5})),
                (i, dict(mats[i], normal_map=dict(nm, texture=solid))), (i, dict(mats[i], normal_map=dict(nm, texture=noise))),
                (i, dict(mats[i], normal_map=dict(nm, texture=99))), (i, dict(mats[i], normal_map=dict(nm, texture=1.5))),
                (i, dict(mats[i], normal_map=dict(nm, scale="x"))), (i, dict(mats[i], normal_map=[img[0], 0.5])), (i, dict(mats[i], normal_map=3)),
                (i, dict(mats[i], bump={"texture": noise, "strength": 0.2}))]  # (a bump beside the map)
    for k, (i, x) in enumerate(bad):
        with pytest.raises(rtmi.RtmiError) as e:
            rtmi.Scene.parse(with_material(i, x))
        assert e.value.status == RT_ERR_SCENE, (k, str(e.value))
        assert "material %d" % i in str(e.value), str(e.value)
    # the scale defaults to 1; scale 0 in a file: no map
    assert rtmi.Scene.parse(with_material(0, dict(mats[0], normal_map={"texture": img[1]}))).normal_map(0) == (img[1], 1.0)
    assert rtmi.Scene.parse(with_material(0, dict(mats[0], normal_map={"texture": img[0], "scale": 0}))).normal_map(0) is None


def test_the_cpp_wrapper(rtmi, tmp_path):
    """include/rtmi.hpp: normal_mapped() carries the map through the scene's build"""
    src = tmp_path / "w.cpp"
    src.write_text('#include "rtmi.hpp"\n#include <cstdio>\nint main() {\n'
                   "  rtmi::scene s(16, 9, 1, 3);\n"
                   "  std::vector<unsigned char> px(4 * 4 * 3, 128);\n"
                   "  for (int k = 0; k < 16; ++k) px[3 * k] = (unsigned char)(120 + k), px[3 * k + 2] = 250;\n"
                   "  auto map = rtmi::image_texture(4, 4, px);\n"
                   "  auto glass = rtmi::dielectric(1.5f);\n"
                   "  s.add(rtmi::sphere(rtmi::point3(0, 0, 0), 1.0f, rtmi::normal_mapped(glass, map, 0.25f)));\n"
                   "  s.add(rtmi::sphere(rtmi::point3(2, 0, 0), 1.0f, glass));\n"
                   "  s.add(rtmi::sphere(rtmi::point3(4, 0, 0), 1.0f, rtmi::normal_mapped(rtmi::metal(rtmi::color(0.5f, 0.5f, 0.5f), 0.0f), map)));\n"
                   "  int bad = 0;\n"
                   "  try { s.add(rtmi::sphere(rtmi::point3(6, 0, 0), 1.0f, rtmi::normal_mapped(rtmi::diffuse_light(rtmi::color(1, 1, 1)), map, 1.0f))); }\n"
                   "  catch (const rtmi::error &) { bad = 1; }\n"
                   "  if (!bad) return 2;\n"
                   '  std::vector<char> b(1 << 16);\n  size_t n = rt_scene_to_json(s.handle(), b.data(), b.size());\n'
                   '  if (n == 0 || n > b.size()) return 1;\n  fputs(b.data(), stdout);\n  return 0;\n}\n')
    exe = str(tmp_path / "w")
    pkg = os.path.dirname(rtmi.LIB_PATH)
    build = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src), "-L", pkg, "-lrtmi", "-Wl,-rpath," + pkg],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    doc = json.loads(out.stdout)
    assert doc["material"]["data"][:3] == [{"type": "dielectric", "index_of_refraction": 1.5, "normal_map": {"texture": 0, "scale": 0.25}},
                                          {"type": "dielectric", "index_of_refraction": 1.5},
                                          {"type": "metal", "albedo": [0.5, 0.5, 0.5], "fuzz": 0, "normal_map": {"texture": 0, "scale": 1}}]


def test_the_packed_records(rtmi):
    """a mapped material's word 11 (c1.w) holds MINUS the offset of its record {word offset of the map's texels (bits), rows
    (bits), cols (bits), scale}; the records lie in material order behind the bump records; every other word of the image is
    the unmapped scene's"""
    sc, img, solid, noise, ids = _seven(rtmi)
    sc.set_bump(ids[3], noise, 0.2)  # (one bump beside them: its record comes first, its word stays positive)
    flat = sc.table_image().reshape(-1).copy()
    scale = {ids[4]: 0.5, ids[0]: -1.25, ids[2]: 2.0}
    tex = {ids[4]: img[0], ids[0]: img[1], ids[2]: img[1]}
    for m in scale:
        sc.set_normal_map(m, tex[m], scale[m])
    w = sc.table_image().reshape(-1)
    bits, fbits = w.view(np.int32), flat.view(np.int32)
    # (three records more; the pbr material's side record, which lies behind them, moves by three: its offset is word 1 of its row)
    assert w.size == flat.size + 3 * 4 and sc.table_info().image_floats == w.size
    # the material table: found by the rough metal's kind word and F0 (the one bumped material: its word 11 is positive)
    at = [k for k in range(0, flat.size - 12, 4) if list(flat[k + 4:k + 7]) == [np.float32(0.9), np.float32(0.7), np.float32(0.4)] and fbits[k + 11] > 0]
    assert len(at) == 1, at
    rec = lambda i: at[0] + 12 * (i - ids[3])
    first = int(fbits[rec(ids[3]) + 11]) + 1  # (behind the bump record)
    shape = {img[0]: (16, 16), img[1]: (8, 12)}
    texels = {}
    for m in ids:
        r = rec(m)
        if m in scale:
            o = -int(bits[r + 11])
            assert o == first + sorted(scale).index(m), (m, o)
            assert (int(bits[4 * o + 1]), int(bits[4 * o + 2])) == shape[tex[m]] and w[4 * o + 3] == np.float32(scale[m]), m
            texels.setdefault(tex[m], set()).add(int(bits[4 * o]))
            word = int(bits[4 * o])
            px = sc.get_image(tex[m]).reshape(-1, 3).astype(np.int64)
            assert np.array_equal(bits[word:word + len(px)], px[:, 0] | (px[:, 1] << 8) | (px[:, 2] << 16)), m
        else:
            assert bits[r + 11] == fbits[r + 11] and (bits[r + 11] > 0) == (m == ids[3]), m
    assert all(len(v) == 1 for v in texels.values()) and len(texels) == 2
    # every other word: the records behind the new ones sit three records later; the one word that names such a record moved with it
    new_at = 4 * first
    moved = np.concatenate([w[:new_at], w[new_at + 12:]]).view(np.int32)
    differs = np.flatnonzero(moved != fbits)
    allowed = {rec(m) + 11 for m in scale} | {rec(ids[6]) + 1}
    assert set(differs.tolist()) <= allowed, sorted(set(differs.tolist()) - allowed)
    assert int(bits[rec(ids[6]) + 1]) == int(fbits[rec(ids[6]) + 1]) + 3
    # removing them gives the unmapped bytes back
    for m in scale:
        sc.set_normal_map(m, -1, 0.0)
    assert sc.table_image().tobytes() == flat.tobytes()
    # a scene with a map takes the general kernels over the wide tables
    a = rtmi.Scene.new(32, 18, 1, 4)
    a.sphere((0, 0, 0), 1.0, a.metal((0.5, 0.5, 0.5), 0.0))
    assert a.table_info().kernel_variant in (2, 6) and a.table_info().grid_wide == 0
    a.set_normal_map(0, a.image_texture(NMS.flat_map()), 1.0)
    assert a.table_info().kernel_variant in (16, 36, 44) and a.table_info().grid_wide == 1


def test_scenes_without_a_map_pack_as_before(rtmi, scenes_dir, golden_dir, tmp_path):
    """the recorded digests, read and not rewritten: every scene of bump_off_pack_digests.json and smooth_pack_digests.json"""
    with open(os.path.join(golden_dir, "bump_off_pack_digests.json")) as f:
        want = json.load(f)
    cases = BS.digest_cases(rtmi, scenes_dir, str(tmp_path))
    assert set(cases) == set(want) and len(want) >= 20
    for name, build in cases.items():
        assert BS.digest(build()) == want[name], name
    with open(os.path.join(golden_dir, "smooth_pack_digests.json")) as f:
        want = json.load(f)
    cases = PC.cases(rtmi, scenes_dir, str(tmp_path))
    assert sorted(cases) == sorted(want)
    for name, build in cases.items():
        assert PC.digest(build()) == want[name], name


# ------------------------------------------------------------------------------------- 2. the frame against the parametrisation
def _surface_points(S, rng, n):
    """(prim index [n], surface point [n][3]) of n seeded points on the primitives of S, kept off the (u, v) discontinuities (a
    sphere's seam and poles, a cylinder's seam: none lies within 1e-3 of one, so no point is left out) and inside a triangle"""
    idx = rng.integers(0, len(S.prims), n)
    p = np.zeros((n, 3))
    for i in np.unique(idx):
        m = idx == i
        k = int(m.sum())
        pr = S.prims[i]
        ty, f = int(pr["type"]), pr["f"].astype(T)
        if ty == R.SPHERE:
            ph, th = rng.uniform(-np.pi + 1e-3, np.pi - 1e-3, k), rng.uniform(0.02, np.pi - 0.02, k)
            o = np.stack([np.sin(th) * np.cos(ph), -np.cos(th), -np.sin(th) * np.sin(ph)], axis=1)
            p[m] = f[:3] + f[3] * o
        elif ty in (R.XY_RECT, R.XZ_RECT, R.YZ_RECT):
            na, aa, ba = R._rect_axes(ty)
            p[m, aa], p[m, ba], p[m, na] = rng.uniform(f[0], f[1], k), rng.uniform(f[2], f[3], k), f[4]
        elif ty == R.CYLINDER:
            M, tr = R._affine(pr["m_inv"], T)
            ph = rng.uniform(-np.pi + 1e-3, np.pi - 1e-3, k)
            op = np.stack([f[0] * np.cos(ph), f[0] * np.sin(ph), rng.uniform(f[1], f[2], k)], axis=1)
            p[m] = (op - tr) @ np.linalg.inv(M).T
        elif ty == R.TRIANGLE:
            w = rng.dirichlet((1, 1, 1), k) * 0.94 + 0.02
            v = pr["m"].astype(T)[:9].reshape(3, 3)
            p[m] = w @ v
        else:
            q, u, v, _, _, _ = R.quad_record(pr, T)
            p[m] = q + rng.uniform(0.01, 0.99, (k, 1)) * u + rng.uniform(0.01, 0.99, (k, 1)) * v
    return idx, p


@pytest.mark.parametrize("shape", NMS.SHAPES)
def test_the_frame_against_central_differences_of_the_parametrisation(rtmi, shape):
    """20 000 seeded surface points per shape, both sides, h = 1e-6 in fp64: in the plane of the surface the gradients of u and
    v come from central differences of ref64.hit_uv along two orthonormal axes; dp/du is the in-plane direction along which v
    stands still and u grows, dp/dv alike.  Their unit vectors against the unit T and B of the statement: 1e-6 per component.
    Triangles with det = 0 must report a frame that is not finite (keep n) and are left out of the comparison, as the issue says;
    no point lies within h of a discontinuity of (u, v), so none is left out for that"""
    sc = NMS.shape_scene(rtmi, shape)
    S = R.RefScene(sc)
    rng = np.random.default_rng(23 + NMS.SHAPES.index(shape))
    n = 20000
    idx, p = _surface_points(S, rng, n)
    _, g, _ = R.hit_record(S, p - 1.0, np.ones_like(p), np.ones(n), idx, T, ("flat_normals", "nm_off"))  # (any ray: the geometric normal's line)
    g = np.where((rng.integers(0, 2, n) != 0)[:, None], g, -g)
    a1 = R._unit(np.cross(g, rng.normal(size=(n, 3))))
    a2 = np.cross(g, a1)
    d = R._unit(-g + 0.3 * a1 * rng.uniform(-1, 1, (n, 1)) + 0.3 * a2 * rng.uniform(-1, 1, (n, 1)))  # from the side g faces

    def uv(q):
        return R.hit_uv(S, q - d, d, np.ones(n), idx, T)
    h = 1e-6
    gu, gv = np.zeros((n, 3)), np.zeros((n, 3))
    for a in (a1, a2):
        (u1, v1), (u0, v0) = uv(p + h * a), uv(p - h * a)
        gu += ((u1 - u0) / (2 * h))[:, None] * a
        gv += ((v1 - v0) / (2 * h))[:, None] * a
    Tr, Br = np.zeros((n, 3)), np.zeros((n, 3))
    for i in np.unique(idx):
        m = idx == i
        Tr[m], Br[m] = NM.raw_tangents(S.prims[i], p[m], T)
    usable = np.isfinite(Tr).all(axis=1) & np.isfinite(Br).all(axis=1)
    flat = ~usable
    if shape == "triangle":
        # det = 0 exactly on every fifth triangle, and nowhere else; there both gradients are parallel (or zero)
        dets = np.array([(lambda c: (c[2] - c[0]) * (c[5] - c[1]) - (c[4] - c[0]) * (c[3] - c[1]))(pr["m_inv"].astype(T)) for pr in S.prims])
        assert np.array_equal(flat, dets[idx] == 0) and 0.1 < flat.mean() < 0.3
        assert np.abs(np.cross(gu[flat], gv[flat])).max() < 1e-6
    else:
        assert not flat.any()
    k = usable
    # the plane's normal from the gradients' side: T_fd is perpendicular to grad v, B_fd to grad u, both in the plane
    gg = g[k]
    T_fd = R._unit(np.cross(gg, gv[k]))
    T_fd *= np.sign(R._dot(T_fd, gu[k]))[:, None]
    B_fd = R._unit(np.cross(gg, gu[k]))
    B_fd *= np.sign(R._dot(B_fd, gv[k]))[:, None]
    eT, eB = np.abs(R._unit(Tr[k]) - T_fd).max(), np.abs(R._unit(Br[k]) - B_fd).max()
    print(f"\n{shape}: {k.sum()} points, max |unit T - central difference| {eT:.2e}, |unit B - ...| {eB:.2e}; kept n on {flat.sum()}")
    assert (~k).sum() == flat.sum() and (shape == "triangle" or k.all())
    assert eT <= 1e-6 and eB <= 1e-6, (eT, eB)
    # dp/du and dp/dv as derivatives, where the statement gives them at full length (triangle, quad): du(T) = 1, du(B) = 0, ...
    # (relative to the factors' lengths: a nearly singular vt makes a long T)
    if shape in ("triangle", "quad"):
        ln = lambda a: np.sqrt(R._dot(a, a))
        for grad, tan, want in ((gu, Tr, 1), (gv, Br, 1), (gu, Br, 0), (gv, Tr, 0)):
            assert (np.abs(R._dot(grad[k], tan[k]) - want) / np.maximum(1, ln(grad[k]) * ln(tan[k]))).max() < 1e-6


def test_a_cylinders_linear_part_is_a_rotation(rtmi):
    """csrc/rt_tangent.h takes the inverse of a cylinder's linear part as its transpose (and keeps cross products): scene.cpp
    builds it from an axis and an angle alone.  Asserted on the seeded cylinders' records, to fp32 rounding"""
    S = R.RefScene(NMS.shape_scene(rtmi, "cylinder"))
    for pr in S.prims:
        M, _ = R._affine(pr["m_inv"], T)
        assert np.abs(M @ M.T - np.eye(3)).max() < 5e-7 and abs(np.linalg.det(M) - 1) < 5e-7


# --------------------------------------------------------------------------------------------- 3. the device text on the host
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/normal_map_host_driver.cpp built with the host compiler; run(records [n][20] uint32) -> (n' [n][3], replaced [n])"""
    d = tmp_path_factory.mktemp("normal_map_driver")
    exe = str(d / "normal_map_host_driver")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "normal_map_host_driver.cpp"), "-lm"], check=True)

    def run(rec):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(rec, np.uint32).tofile(fin)
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
        out = np.fromfile(fout, np.uint32).reshape(-1, NMS.OUTPUT_WORDS)
        return out[:, 0:3].view(np.float32).astype(np.float64), out[:, 3] != 0

    def frames(rec):
        """records [n][20] uint32 of the driver's `frames` mode -> (T [n][3], B [n][3]) as rt_tangent.h's functions give them"""
        fin, fout = str(d / "fin.bin"), str(d / "fout.bin")
        np.ascontiguousarray(rec, np.uint32).tofile(fin)
        p = subprocess.run([exe, "frames", fin, fout], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
        out = np.fromfile(fout, np.float32).reshape(-1, 8).astype(np.float64)
        return out[:, 0:3], out[:, 3:6]
    run.frames = frames
    return run


@pytest.mark.parametrize("shape", NMS.SHAPES)
def test_the_raw_tangents_on_the_host(rtmi, driver, shape):
    """tangent_sphere / _rect / _cylinder / _triangle / _quad of csrc/rt_tangent.h under the host compiler, fed what the kernel
    hands them (the outward normal, the record's extents, the third row of a cylinder's matrix, a triangle's corners and vt in
    the kernel's pairing, a quad's normal and dual vectors), on 20 000 seeded surface points of shape_scene's primitives, against
    ref64_normal_map.raw_tangents in fp64: the unit T and B within 1e-4 per component on the share the numpy statement at float32
    reaches, minus 0.5 points; a det = 0 triangle not finite in both.  Half of the rectangles and cylinders have their extents
    REVERSED here (x1 < x0, zmax < zmin: records no scene file of the tests holds), so that the sign branches run: the frame
    must turn with them."""
    S = R.RefScene(NMS.shape_scene(rtmi, shape))
    rng = np.random.default_rng(71 + NMS.SHAPES.index(shape))
    n = 20000
    idx, p = _surface_points(S, rng, n)
    prims = S.prims.copy()
    flipped = np.zeros(len(prims), bool)
    for i, pr in enumerate(prims):
        ty = int(pr["type"])
        if i % 2 == 0 and ty in (R.XY_RECT, R.XZ_RECT, R.YZ_RECT):
            which = i // 2 % 3  # u alone, v alone, both
            if which != 1:
                prims["f"][i][[0, 1]] = prims["f"][i][[1, 0]]
            if which != 0:
                prims["f"][i][[2, 3]] = prims["f"][i][[3, 2]]
            flipped[i] = True
        if i % 2 == 0 and ty == R.CYLINDER:
            prims["f"][i][[1, 2]] = prims["f"][i][[2, 1]]
            flipped[i] = True
    rec = np.zeros((n, 20), np.float32)
    code = np.zeros(n, np.uint32)
    T64, B64, T32, B32 = (np.zeros((n, 3)) for _ in range(4))
    for i in np.unique(idx):
        m = idx == i
        pr = prims[i]
        T64[m], B64[m] = NM.raw_tangents(pr, p[m], T)
        T32[m], B32[m] = NM.raw_tangents(pr, p[m].astype(np.float32), np.float32)
        ty, f = int(pr["type"]), pr["f"].astype(T)
        if ty == R.SPHERE:
            code[m], rec[m, 1:4] = 0, (p[m] - f[:3]) / f[3]
        elif ty in (R.XY_RECT, R.XZ_RECT, R.YZ_RECT):
            code[m] = 1
            rec[m, 1] = np.array([{R.XY_RECT: 0, R.XZ_RECT: 1, R.YZ_RECT: 2}[ty]], np.uint32).view(np.float32)[0]
            rec[m, 2:6] = f[:4]
        elif ty == R.CYLINDER:
            M, tr = R._affine(pr["m_inv"], T)
            op = p[m] @ M.T + tr
            o_obj = np.stack([op[:, 0], op[:, 1], np.zeros(len(op))], axis=1) / f[0]
            code[m], rec[m, 1:4], rec[m, 4:7], rec[m, 7], rec[m, 8] = 2, M[2], o_obj @ M, f[1], f[2]
        elif ty == R.TRIANGLE:
            code[m], rec[m, 1:10], rec[m, 10:16] = 3, pr["m"][:9], pr["m_inv"][:6]
        else:
            _, _, _, qn, A, B = R.quad_record(pr, T)
            code[m], rec[m, 1:4], rec[m, 4:7], rec[m, 7:10] = 4, qn, A, B
    words = rec.view(np.uint32).copy()
    words[:, 0] = code
    Tc, Bc = driver.frames(words)
    if shape in ("rect", "cylinder"):
        assert 0.2 < flipped[idx].mean() < 0.8
        # the frame turns with the extents: against the records as the scene holds them, the flipped axes are reversed
        for i in np.unique(idx[flipped[idx]])[:6]:
            m = idx == i
            T0, B0 = NM.raw_tangents(S.prims[i], p[m], T)
            assert (R._dot(T0, T64[m]) < 0).all() or (R._dot(B0, B64[m]) < 0).all()
    finite = np.isfinite(T64).all(axis=1) & np.isfinite(B64).all(axis=1)
    assert np.array_equal(finite, np.isfinite(Tc).all(axis=1) & np.isfinite(Bc).all(axis=1))
    assert finite.all() or shape == "triangle"
    k = finite
    unit = lambda a: a / np.sqrt((a * a).sum(axis=1))[:, None]
    with np.errstate(all="ignore"):
        err = np.maximum(np.abs(unit(Tc[k]) - unit(T64[k])).max(axis=1), np.abs(unit(Bc[k]) - unit(B64[k])).max(axis=1))
        e32 = np.maximum(np.abs(unit(T32[k].astype(T)) - unit(T64[k])).max(axis=1), np.abs(unit(B32[k].astype(T)) - unit(B64[k])).max(axis=1))
    share, numpy32 = float((err <= 1e-4).mean()), float((e32 <= 1e-4).mean())
    print(f"\nraw tangents on the host, {shape}: unit T, B within 1e-4 on {100 * share:.3f} % of {k.sum()} points (median {np.median(err):.1e}); "
          f"numpy at float32 {100 * numpy32:.3f} %; not finite {(~k).sum()}")
    assert numpy32 >= 0.97 and share >= numpy32 - 0.005, (share, numpy32)


@pytest.mark.parametrize("shape", NMS.SHAPES)
def test_the_fp32_code_against_the_fp64_statement(driver, shape):
    """Measured here, share of the 20 000 records with every component of n' within 1e-4: C++ and numpy float32
    100.000 % on sphere, rect, cylinder and quad, 99.985 % both on triangles (a frame from a nearly singular vt, |det| ~ 1e-6)."""
    rec = NMS.records(shape)
    assert rec.shape == (20000, NMS.RECORD_WORDS)
    nb, ok = driver(rec)
    n64, ok64 = NMS.statement(rec, np.float64)
    n32, _ = NMS.statement(rec, np.float32)
    code, numpy32 = NMS.share(nb, n64), NMS.share(n32, n64)
    print(f"\nrt_tangent.h on the host, {shape}: n' within 1e-4 on {100 * code:.3f} % of {len(rec)} records, max {np.abs(nb - n64).max():.2e}; "
          f"the numpy statement at float32 {100 * numpy32:.3f} %, max {np.abs(n32 - n64).max():.2e}; replaced {100 * ok64.mean():.1f} %")
    assert numpy32 >= 0.97, numpy32
    assert code >= numpy32 - 0.005, (code, numpy32)
    # the two guards and the keep-n cases agree on every record
    assert np.array_equal(ok, ok64)
    assert np.array_equal(nb[~ok64], rec[~ok64, 11:14].view(np.float32).astype(np.float64))  # (n bit for bit where it stays)
    # the records cover both sides, both signs of s, smooth and flat normals, texels that leave n, and both outcomes of the guards
    s = rec[:, 7].view(np.float32)
    w = rec[:, 6].astype(np.int64)
    still = ((w & 255) == 128) & (((w >> 8) & 255) == 128)
    assert 0.4 < (rec[:, 17] != 0).mean() < 0.6 and s.min() < -1.9 and s.max() > 1.9
    assert still.sum() >= 1000 and (((w >> 16) & 255) <= 128).sum() >= 1000 and not ok64[still].any() and not ok64[((w >> 16) & 255) <= 128].any()
    tilting = ~still & (((w >> 16) & 255) > 128)
    assert 0.03 < (~ok64[tilting]).mean() < 0.6
    off = 1 - (rec[:, 8:11].view(np.float32).astype(T) * rec[:, 11:14].view(np.float32).astype(T)).sum(axis=1)
    assert 0.3 < (off > 1e-3).mean() < 0.7 and off.max() <= 1 - np.cos(np.pi / 6) + 1e-6
    moved = np.abs(n64 - rec[:, 11:14].view(np.float32)).max(axis=1)
    assert np.median(moved[ok64]) > 0.05
    # and a deliberate mistake of the statement is seen by the same measure
    for mistake in ("nm_swap_tb", "nm_back_unsigned", "nm_not_about_n", "nm_2c_minus_1"):
        assert NMS.share(NMS.statement(rec[:2000], np.float64, (mistake,))[0], n64[:2000]) < 0.9, mistake


# --------------------------------------------------------------------------------------------------------------- 4. the model
def test_sanity_of_the_model():
    rng = np.random.default_rng(11)
    n_pts = 5000
    unit = lambda a: a / np.sqrt((a * a).sum(axis=1))[:, None]
    g = unit(rng.normal(size=(n_pts, 3)))
    Tr = np.cross(g, rng.normal(size=(n_pts, 3))) * rng.uniform(0.2, 3, (n_pts, 1))
    Br = (np.cross(g, Tr) + 0.3 * Tr) * rng.uniform(0.2, 3, (n_pts, 1))  # (skewed, of any length)
    axis = unit(np.cross(g, rng.normal(size=(n_pts, 3))))
    ang = rng.uniform(0, np.pi / 6, n_pts)
    n = g * np.cos(ang)[:, None] + np.cross(axis, g) * np.sin(ang)[:, None]
    d = rng.normal(size=(n_pts, 3))
    d = np.where(((d * g).sum(axis=1) > 0)[:, None], -d, d)
    rgb = np.stack([rng.integers(60, 196, n_pts), rng.integers(60, 196, n_pts), rng.integers(180, 256, n_pts)], axis=1)
    xyz, active = NM.decode(rgb, T)
    assert active.all() and np.abs(xyz[:, :2]).max() <= 68 / 127
    assert NM.decode(np.array([[128, 128, 255], [255, 0, 129]]), T)[0].tolist() == [[0.0, 0.0, 1.0], [1.0, -1.0, 1 / 127]]  # (byte 128: 0; 255: 1; 0: -1)
    front = rng.integers(0, 2, n_pts) != 0
    s = rng.uniform(-2, 2, n_pts).astype(np.float32)
    nb, ok = NM.normal(n, g, d, front, s, Tr, Br, xyz, active, T)
    assert np.abs(np.sqrt((nb * nb).sum(axis=1)) - 1).max() < 1e-12           # unit
    assert ((nb * n).sum(axis=1) > 0).all()                                      # z > 0: never below the surface it started from
    assert ((nb * d).sum(axis=1) < 0)[ok].all() and ((nb * g).sum(axis=1) > 0)[ok].all() and 0.3 < ok.mean() < 1.0  # the guards; some kept n
    assert np.array_equal(nb[~ok], n[~ok])
    # the frame is orthonormal about n, T' on T's side, B' on B's
    Tp, Bp, usable = NM.frame(n, front, Tr, Br, T)
    assert usable.all()
    for a, b, want in ((Tp, Tp, 1), (Bp, Bp, 1), (Tp, Bp, 0), (Tp, n, 0), (Bp, n, 0)):
        assert np.abs((a * b).sum(axis=1) - want).max() < 1e-12
    assert ((Tp * Tr).sum(axis=1) > 0).all() and ((Bp * Br).sum(axis=1) > 0).all()
    # s -> -s mirrors the tangential part
    wide = -n  # (a direction along -n, and g = n: the guards accept every tilt)
    up, oku = NM.normal(n, n, wide, front, s, Tr, Br, xyz, active, T)
    down, okd = NM.normal(n, n, wide, front, -s, Tr, Br, xyz, active, T)
    assert oku.all() and okd.all()
    tang = lambda a: a - (a * n).sum(axis=1)[:, None] * n
    assert np.abs(tang(up) + tang(down)).max() < 1e-12 and np.abs((up * n).sum(axis=1) - (down * n).sum(axis=1)).max() < 1e-12
    # both sides of a point see one relief: the outward normal tilts the same way
    f, _ = NM.normal(n, n, wide, np.ones(n_pts, bool), s, Tr, Br, xyz, active, T)
    bk, _ = NM.normal(-n, -n, -wide, np.zeros(n_pts, bool), s, Tr, Br, xyz, active, T)
    assert np.abs(f + bk).max() < 1e-12
    # a (128, 128, b) texel and a z <= 0 texel leave n bit for bit, whatever the frame
    for still in ([128, 128, 255], [128, 128, 140], [128, 128, 3], [200, 90, 128], [200, 90, 0], [10, 250, 127]):
        xyz0, act0 = NM.decode(np.tile(still, (n_pts, 1)), T)
        same, ok0 = NM.normal(n, g, d, front, s, Tr, Br, xyz0, act0, T)
        assert not act0.any() and not ok0.any() and same.tobytes() == n.tobytes(), still
    # a frame that cannot be built keeps n: T along n (a sphere's pole), a NaN frame (a triangle's det = 0)
    ez = np.tile([0.0, 0.0, 1.0], (4, 1))  # (an axis: T - (T.n) n is exactly zero)
    kept, okk = NM.normal(ez, ez, -ez, front[:4], 1.0, 2 * ez, Br[:4], xyz[:4], active[:4], T)
    assert np.array_equal(kept, ez) and not okk.any()
    kept, okk = NM.normal(n[:4], g[:4], d[:4], front[:4], 1.0, np.full((4, 3), np.nan), np.full((4, 3), np.nan), xyz[:4], active[:4], T)
    assert np.array_equal(kept, n[:4]) and not okk.any()
    # B parallel to T: B' = cross(sigma n, T'), still a frame
    ex = np.tile([1.0, 0.0, 0.0], (4, 1))  # (axes again: what is left of B is exactly zero)
    for side in (np.ones(4, bool), np.zeros(4, bool)):
        Tp2, Bp2, us2 = NM.frame(ez, side, 2 * ex, 3 * ex, T)
        assert us2.all() and np.array_equal(Tp2, ex) and np.array_equal(Bp2, np.cross(np.where(side[:, None], ez, -ez), ex))


# ------------------------------------------------------------------------------------------------------ 5. the cases on the CPU
def test_a_case_holds_its_vertices_and_the_mistakes_change_it(rtmi):
    """nm_prims at fp64 on the CPU (the other cases: test_gpu_normal_map.py): the vertices it is there for, the twin's first
    hits, a constant (128, 128, 255) map IS the twin, and every deliberate mistake moves a clear share of the samples"""
    name = "nm_prims"
    words, shutter = NMS.inputs(rtmi, name)
    words = words[:4 * NS.REF_W * NS.REF_H]
    sc = NMS.scene(rtmi, name)
    S = R.RefScene(sc)
    log = R.new_log()
    rgb, sig, draws = R.trace(S, words, log=log)
    tally = R.tally(sig, S, log)
    assert tally["nm_share"] >= NMS.MIN_MAP_SHARE and min(tally[k] for k in NMS.CASES[name][3]) >= 50, tally
    assert log["nm_mapped"] >= tally["nm_vertices"]
    twin = NMS.scene(rtmi, name, maps=False)
    rgb_t, sig_t, _ = R.trace(R.RefScene(twin), words)
    assert np.array_equal(sig[:, R.SAMPLE_COLUMNS + R.C_PRIM], sig_t[:, R.SAMPLE_COLUMNS + R.C_PRIM])  # (the geometry is the twin's)
    far = lambda a, b: (np.abs(a - b).max(axis=1) > 1e-4 * np.maximum(1, np.abs(b).max(axis=1))).mean()
    assert far(rgb_t, rgb) > 0.15
    off, _, _ = R.trace(S, words, perturb=("nm_off",))
    assert np.array_equal(off, rgb_t)  # (nm_off IS the twin)
    still = NMS.scene(rtmi, name, maps="flat")
    assert np.array_equal(R.trace(R.RefScene(still), words)[0], rgb_t)  # (and so is a map of texels that leave n)
    for mistake in NM.PERTURBATIONS:
        wrong, _, _ = R.trace(S, words, perturb=(mistake,))
        moved = far(wrong, rgb)
        print(f"{name}, {mistake}: {100 * moved:.1f} % of the samples move")
        assert moved > 0.05, (mistake, moved)


def test_removal_is_allowed_beside_the_other_in_both_spellings(rtmi):
    """`texture = -1` and `scale = 0` (`strength = 0`) both remove, and removing is always allowed: a valid image with scale 0
    on a bumped material is a removal of nothing, not the exclusion's RT_ERR_ARG -- as set_bump with strength 0 on a mapped one"""
    sc, img, _, noise, ids = _seven(rtmi)
    sc.set_bump(ids[0], noise, 0.2)
    sc.set_normal_map(ids[0], img[0], 0.0)
    sc.set_normal_map(ids[0], -1, 1.0)
    assert sc.bump(ids[0]) is not None and sc.normal_map(ids[0]) is None
    sc.set_normal_map(ids[1], img[1], 0.5)
    sc.set_bump(ids[1], noise, 0.0)
    sc.set_bump(ids[1], -1, 0.3)
    assert sc.normal_map(ids[1]) == (img[1], 0.5) and sc.bump(ids[1]) is None


def test_the_tool_writes_the_shipped_scene(scenes_dir):
    """tools/make_normal_maps.py reproduces scenes/normal_map_wall.json byte for byte, and the file stays small"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_normal_maps
    finally:
        sys.path.pop(0)
    with open(os.path.join(scenes_dir, "normal_map_wall.json")) as f:
        text = f.read()
    assert make_normal_maps.scene_text() == text
    assert len(text) < 64 * 1024
