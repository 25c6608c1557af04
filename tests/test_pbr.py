"""The metallic-roughness material without a GPU:
  1. the interface -- C, C++, Python, JSON, the argument rules and their status codes, the round trip to the same packed image,
     the packed records' words, the map set and removed; scenes without the material pack to the digests recorded before
     (tests/golden/bump_off_pack_digests.json, smooth_pack_digests.json, mesh_lights_off_digests.json: read here);
  2. csrc/rt_pbr.h compiled by the host compiler against the fp64 statement of ref64_pbr.py: the integers and the choice exactly,
     ul' and alpha by 7r's rule; the closed forms;
  3. scenes without the material trace as pinned (the pinned fixture); every GPU case
     holds the vertices it is about and is reachable (the fp32 statement against the fp64 one: share >= 0.98, flips <= 0.5 %);
     each deliberate mistake changes the reference.
test_gpu_pbr.py holds the kernels to that reference."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import bump_scenes as BS
import mesh_light_scenes as ML
import nee_scenes as NS
import pbr_scenes as PS
import ref64 as R
import ref64_pbr as RP
import smooth_pack_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_ARG, RT_ERR_SCENE = 1, 4
MK_PBR = 18


# ------------------------------------------------------------------------------------------------------------ 1. interface
def _scene(rtmi):
    sc = rtmi.Scene.new(32, 18, 1, 4)
    sc.camera((0, 1, 5), (0, 0.5, 0), (0, 1, 0), 40.0)
    ck = sc.checker_texture((0.2, 0.3, 0.4), (0.9, 0.8, 0.7))
    nz = sc.noise_texture((0.0, 0.1, 0.2), (1, 1, 1), style="turbulence", scale=2.0, octaves=2, seed=3)
    im = sc.image_texture(PS.images()[1])
    ids = [sc.pbr((0.5, 0.25, 0.75), 0.3, 0.4), sc.pbr(ck, 1.0, 0.9, 1.33, metallic_roughness=nz), sc.pbr(nz, 0.25, 0.125, 2.0, metallic_roughness=im),
           sc.pbr((0.1, 0.2, 0.3))]
    for k, m in enumerate(ids):
        sc.sphere((k - 1.5, 0.5, 0.0), 0.4, m)
    return sc, ids, (ck, nz, im)


def test_constructors_and_the_material_table(rtmi):
    sc, ids, (ck, nz, im) = _scene(rtmi)
    m = sc.materials()
    assert rtmi.MATERIAL_DTYPE.itemsize == 28 == rtmi.struct_size(3) and rtmi.abi_version() == 3
    a, b, c, d = (m[i] for i in ids)
    assert a["type"] == 7 and list(a["albedo"]) == [np.float32(0.3), 0, 0] and a["fuzz"] == np.float32(0.4) and a["ir"] == np.float32(1.5)
    assert b["type"] == 7 and b["texture"] == ck and list(b["albedo"]) == [1, 0, 0] and b["fuzz"] == np.float32(0.9) and b["ir"] == np.float32(1.33)
    assert d["albedo"][0] == 0 and d["fuzz"] == np.float32(0.5) and d["ir"] == np.float32(1.5)  # (the defaults)
    assert [sc.pbr_map(i) for i in ids] == [None, nz, im, None]
    assert sc.table_info().kernel_variant in (16, 36, 44)  # the general kernels over the wide tables, spheres only as it is
    # a bump is accepted, on the C side and in JSON
    sc.set_bump(ids[0], nz, 0.1)
    assert sc.bump(ids[0]) == (nz, pytest.approx(0.1))
    back = rtmi.Scene.parse(sc.to_json())
    assert back.bump(ids[0]) == sc.bump(ids[0]) and [back.pbr_map(i) for i in ids] == [None, nz, im, None]
    assert back.table_image().tobytes() == sc.table_image().tobytes()
    sc.add_moving_sphere((0, 2, 0), (1, 2, 0), 0.3, ids[1])  # a moving sphere may carry it
    assert len(sc.moving_spheres()) == 1


def test_the_map_is_set_replaced_and_removed(rtmi):
    sc, ids, (ck, nz, im) = _scene(rtmi)
    plain = sc.table_image().tobytes()
    sc.set_pbr_map(ids[0], ck)
    assert sc.pbr_map(ids[0]) == ck and sc.table_image().tobytes() != plain
    sc.set_pbr_map(ids[0], im)
    assert sc.pbr_map(ids[0]) == im
    sc.set_pbr_map(ids[0], -1)
    assert sc.pbr_map(ids[0]) is None and sc.table_image().tobytes() == plain
    sc.set_pbr_map(ids[0], -1)  # (removing what is not there is no error)
    lam = sc.lambertian((0.5, 0.5, 0.5))
    plain = sc.table_image().tobytes()
    for call in (lambda: sc.set_pbr_map(lam, ck), lambda: sc.set_pbr_map(99, ck), lambda: sc.set_pbr_map(-1, ck), lambda: sc.set_pbr_map(ids[0], 99),
                 lambda: sc.set_pbr_map(ids[0], -2), lambda: sc.pbr_map(lam), lambda: sc.pbr_map(99)):
        with pytest.raises(rtmi.RtmiError) as e:
            call()
        assert e.value.status == RT_ERR_ARG
    assert sc.table_image().tobytes() == plain


def test_the_c_entry_points_and_their_argument_rules(rtmi):
    lib = ctypes.CDLL(rtmi.LIB_PATH)
    lib.rt_scene_new.restype = ctypes.c_void_p
    lib.rt_scene_new.argtypes = [ctypes.c_int] * 4
    f3 = ctypes.c_float * 3
    add, setm, getm, solid = lib.rt_scene_add_pbr, lib.rt_scene_set_pbr_map, lib.rt_scene_get_pbr_map, lib.rt_scene_add_solid_color
    add.argtypes, add.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float], ctypes.c_int
    setm.argtypes, setm.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int], ctypes.c_int
    getm.argtypes, getm.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)], ctypes.c_int
    solid.argtypes, solid.restype = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)], ctypes.c_int
    lib.rt_scene_add_lambertian.argtypes, lib.rt_scene_add_lambertian.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int
    lib.rt_scene_free.argtypes, lib.rt_scene_free.restype = [ctypes.c_void_p], None
    lib.rt_last_error.restype = ctypes.c_char_p
    s = lib.rt_scene_new(8, 8, 1, 2)
    try:
        t0, t1 = solid(s, f3(0.5, 0.5, 0.5)), solid(s, f3(1.0, 0.5, 0.25))
        assert (t0, t1) == (0, 1)
        assert add(s, t0, 0.0, 0.0, 1.5) == 0 and add(s, t0, 1.0, 1.0, 2.4) == 1
        lam = lib.rt_scene_add_lambertian(s, t0)
        got = ctypes.c_int(7)
        assert getm(s, 0, ctypes.byref(got)) == 0 and got.value == -1
        assert setm(s, 0, t1) == 0 and getm(s, 0, ctypes.byref(got)) == 0 and got.value == t1 and getm(s, 0, None) == 0
        assert setm(s, 0, -1) == 0 and getm(s, 0, ctypes.byref(got)) == 0 and got.value == -1
        nan, inf = float("nan"), float("inf")
        bad = [lambda: add(s, -1, 0.5, 0.5, 1.5), lambda: add(s, 2, 0.5, 0.5, 1.5), lambda: add(s, t0, -0.01, 0.5, 1.5), lambda: add(s, t0, 1.01, 0.5, 1.5),
               lambda: add(s, t0, nan, 0.5, 1.5), lambda: add(s, t0, inf, 0.5, 1.5), lambda: add(s, t0, 0.5, -0.01, 1.5), lambda: add(s, t0, 0.5, 1.01, 1.5),
               lambda: add(s, t0, 0.5, nan, 1.5), lambda: add(s, t0, 0.5, 0.5, 1.0), lambda: add(s, t0, 0.5, 0.5, 0.9), lambda: add(s, t0, 0.5, 0.5, nan),
               lambda: add(s, t0, 0.5, 0.5, inf), lambda: add(None, t0, 0.5, 0.5, 1.5)]
        for k, call in enumerate(bad):
            assert call() == -RT_ERR_ARG, k
            assert lib.rt_last_error(), k
        bad = [lambda: setm(s, lam, t1), lambda: setm(s, 3, t1), lambda: setm(s, -1, t1), lambda: setm(s, 0, 2), lambda: setm(s, 0, -2), lambda: setm(None, 0, t1),
               lambda: getm(s, lam, ctypes.byref(got)), lambda: getm(s, 3, ctypes.byref(got)), lambda: getm(None, 0, ctypes.byref(got))]
        for k, call in enumerate(bad):
            assert call() == RT_ERR_ARG, k
            assert lib.rt_last_error(), k
    finally:
        lib.rt_scene_free(s)
    sc = rtmi.Scene.new(8, 8, 1, 2)
    for call in (lambda: sc.pbr((1, 1, 1), 1.5), lambda: sc.pbr((1, 1, 1), 0.5, 2.0), lambda: sc.pbr((1, 1, 1), 0.5, 0.5, 1.0), lambda: sc.pbr(5),
                 lambda: sc.pbr((1, 1, 1), metallic_roughness=9)):
        with pytest.raises(rtmi.RtmiError) as e:
            call()
        assert e.value.status == RT_ERR_ARG


def test_json_reads_writes_and_refuses(rtmi):
    sc, ids, (ck, nz, im) = _scene(rtmi)
    text = sc.to_json()
    mats = json.loads(text)["material"]["data"]
    assert mats[ids[0]] == {"type": "pbr", "texture": sc.materials()[ids[0]]["texture"], "metallic": 0.3, "roughness": 0.4, "ior": 1.5}
    assert mats[ids[1]] == {"type": "pbr", "texture": ck, "metallic": 1, "roughness": 0.9, "ior": 1.33, "metallic_roughness": nz}
    back = rtmi.Scene.parse(text)
    assert back.materials().tobytes() == sc.materials().tobytes() and back.prims().tobytes() == sc.prims().tobytes()
    assert back.table_image().tobytes() == sc.table_image().tobytes()

    def with_material(m):
        d = json.loads(text)
        d["material"]["data"][ids[0]] = m
        return json.dumps(d)
    good = {"type": "pbr", "texture": ck, "metallic": 0.5, "roughness": 0.25}
    got = rtmi.Scene.parse(with_material(good))
    assert got.materials()[ids[0]]["ir"] == np.float32(1.5) and got.pbr_map(ids[0]) is None  # (the default index, no map)
    assert rtmi.Scene.parse(with_material(dict(good, metallic_roughness=im, ior=1.7))).pbr_map(ids[0]) == im
    assert rtmi.Scene.parse(with_material(dict(good, metallic_roughness=-1))).pbr_map(ids[0]) is None
    bad = [dict(good, metallic=1.5), dict(good, metallic=-0.1), dict(good, metallic="x"), dict(good, roughness=1.5), dict(good, roughness=-0.1),
           dict(good, ior=1.0), dict(good, ior=0.5), dict(good, texture=99), dict(good, texture=-1), dict(good, metallic_roughness=99),
           dict(good, metallic_roughness=-2), {k: v for k, v in good.items() if k != "metallic"}, {k: v for k, v in good.items() if k != "roughness"},
           {k: v for k, v in good.items() if k != "texture"}, dict(good, albedo=[0, 0, 0]), dict(good, fuzz=0.1), dict(good, ir=1.5), dict(good, metalic=0.5),
           {"type": "plastic", "texture": ck, "ior": 1.5, "roughness": 0.3, "metallic_roughness": im}]
    for k, m in enumerate(bad):
        with pytest.raises(rtmi.RtmiError) as e:
            rtmi.Scene.parse(with_material(m))
        assert e.value.status == RT_ERR_SCENE, (k, str(e.value))


def test_the_shipped_scene_and_the_cpp_wrapper(rtmi, tmp_path):
    sc = rtmi.Scene.load(os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "pbr_wear.json"))
    m, t = sc.materials(), sc.textures()
    pbr = np.flatnonzero(m["type"] == 7)
    assert len(pbr) == 11 and not (t["type"] == R.IMAGE).any()  # (noise and checker maps only: no image file)
    assert sorted(set(float(x) for x in m["albedo"][pbr][1:10, 0])) == [0.0, 0.5, 1.0]
    maps = {int(i): sc.pbr_map(int(i)) for i in pbr}
    assert t["type"][maps[0]] == R.CHECKER and t["type"][maps[10]] == 3 and sum(v is not None for v in maps.values()) == 2
    assert not sc.light_sampling  # (left to --nee, as in every shipped scene)
    sc.set_light_sampling(True)
    assert len(sc.lights()) == 1 and sc.table_info().kernel_variant & 255 in (16, 36, 44)
    assert rtmi.Scene.parse(sc.to_json()).table_image().tobytes() == sc.table_image().tobytes()
    src = tmp_path / "w.cpp"
    src.write_text('#include "rtmi.hpp"\n#include <cstdio>\nint main() {\n'
                   "  rtmi::scene s(16, 9, 1, 3);\n"
                   "  auto orm = rtmi::checker_texture(rtmi::color(1, 0.25f, 0), rtmi::color(1, 1, 1));\n"
                   "  auto a = rtmi::pbr(rtmi::color(0.5f, 0.25f, 1.0f), 0.75f, 0.25f, 1.4f, orm);\n"
                   "  s.add(rtmi::sphere(rtmi::point3(0, 0, 0), 1.0f, a));\n"
                   "  auto b = s.pbr(rtmi::solid_color(rtmi::color(1, 1, 1)));\n"
                   "  s.add(rtmi::sphere(rtmi::point3(2, 0, 0), 1.0f, b));\n"
                   "  if (s.pbr_map(b) != -1) return 6;\n"
                   "  s.set_pbr_map(b, orm);\n  const int with = s.pbr_map(b);\n  if (with != s.pbr_map(a) || with < 0) return 7;\n"
                   "  s.set_pbr_map(b, nullptr);\n  if (s.pbr_map(b) != -1) return 8;\n"
                   "  try { s.add(rtmi::sphere(rtmi::point3(4, 0, 0), 1.0f, rtmi::pbr(rtmi::color(1, 1, 1), 2.0f))); return 9; } catch (const std::exception &) {}\n"
                   '  std::vector<char> b2(1 << 16);\n  size_t n = rt_scene_to_json(s.handle(), b2.data(), b2.size());\n'
                   '  if (n == 0 || n > b2.size()) return 1;\n  fputs(b2.data(), stdout);\n  return 0;\n}\n')
    exe = str(tmp_path / "w")
    pkg = os.path.dirname(rtmi.LIB_PATH)
    build = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src), "-L", pkg, "-lrtmi", "-Wl,-rpath," + pkg],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    mats = json.loads(out.stdout)["material"]["data"]
    assert {k: v for k, v in mats[0].items() if k not in ("texture", "metallic_roughness")} == {"type": "pbr", "metallic": 0.75, "roughness": 0.25, "ior": 1.4}
    assert "metallic_roughness" in mats[0] and mats[1] == {"type": "pbr", "texture": mats[1]["texture"], "metallic": 0, "roughness": 0.5, "ior": 1.5}


def test_the_packed_records(rtmi):
    """{kind 18, side record, r0, base type | map type << 4}{base c0}{base c1, bump} and the side record {mf, rf, 0, 0}{map c0}{map c1}:
    found in the packed image by the kind, every word against fp64"""
    sc, ids, (ck, nz, im) = _scene(rtmi)
    w = sc.table_image().reshape(-1)
    bits = w.view(np.int32)
    m, t = sc.materials(), sc.textures()
    r0 = lambda ior: np.float32(((np.float64(np.float32(ior)) - 1) / (np.float64(np.float32(ior)) + 1)) ** 2)
    at = [k for k in np.flatnonzero(bits[::4] == MK_PBR) * 4 if k + 48 <= len(w) and all(bits[k + 12 * j] == MK_PBR for j in range(4))
          and abs(w[k + 2] - r0(1.5)) < 1e-8 and abs(w[k + 14] - r0(1.33)) < 1e-8]
    assert len(at) == 1, at
    want_types = [0 | 0 << 4, 1 | 3 << 4, 3 | 2 << 4, 0 | 0 << 4]
    sides = []
    for j, i in enumerate(ids):
        q = w[at[0] + 12 * j:at[0] + 12 * j + 12]
        qb = q.view(np.int32)
        assert abs(np.float64(q[2]) - np.float64(r0(m[i]["ir"]))) <= 1e-7 * r0(m[i]["ir"]) and qb[3] == want_types[j], (j, q)
        side = qb[1] * 4
        sides.append(int(qb[1]))
        s = w[side:side + 12]
        assert s[0] == m[i]["albedo"][0] and s[1] == m[i]["fuzz"] and s[2] == 0 and s[3] == 0
        base = t[m[i]["texture"]]
        if base["type"] in (R.SOLID, R.CHECKER, 3):
            assert list(q[4:7]) == list(base["c0"]) and (base["type"] == R.SOLID or list(q[8:11]) == list(base["c1"]))
        mp = sc.pbr_map(i)
        if mp is None:
            assert list(s[4:7]) == [1, 1, 1] and not s[7:12].any()  # (no map: solid white)
        elif t[mp]["type"] == 3:
            assert list(s[4:7]) == list(t[mp]["c0"]) and list(s[8:11]) == list(t[mp]["c1"]) and s.view(np.int32)[7] > 0
        else:  # the image: {first texel word, rows, cols}; its texels are the bytes given
            word, rows, cols = (int(x) for x in s.view(np.int32)[4:7])
            img = PS.images()[1]
            assert (rows, cols) == img.shape[:2]
            texels = w.view(np.uint32)[word:word + rows * cols]
            assert np.array_equal(texels, img[..., 0].ravel().astype(np.uint32) | img[..., 1].ravel().astype(np.uint32) << 8 | img[..., 2].ravel().astype(np.uint32) << 16)
    assert sides == list(range(sides[0], sides[0] + 12, 3))  # three rows each, in material order
    assert bits[at[0] + 7] == 0 and bits[at[0] + 12 * 2 + 7] > 0   # (c0.w: a noise base's record, else nothing)
    assert (bits[3::4] == MK_PBR).sum() >= 4  # the spheres' cold records carry the kind too
    sc.set_bump(ids[1], nz, 0.2)
    w2 = sc.table_image().reshape(-1).view(np.int32)
    assert w2[at[0] + 12 + 11] > 0 and w2[at[0] + 11] == 0


def test_scenes_without_the_material_pack_as_before(rtmi, scenes_dir, golden_dir, tmp_path):
    """every scene and pack case recorded before earlier features: the digests the three golden files hold"""
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
    with open(os.path.join(golden_dir, "mesh_lights_off_digests.json")) as f:
        want = json.load(f)
    cases = ML.digest_cases(rtmi, scenes_dir)
    assert sorted(cases) == sorted(want)
    for name, make in cases.items():
        assert ML.digest(make()) == want[name], name


# --------------------------------------------------------------------------------------------- 2. fp32 code, fp64 statement
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("pbr")
    exe = str(d / "pbr_host_driver")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "pbr_host_driver.cpp"), "-lm"], check=True)

    def run(rec):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(rec, np.float32).tofile(fin)
        subprocess.run([exe, fin, fout], check=True, timeout=120)
        return np.fromfile(fout, np.float32).reshape(-1, PS.OUTPUT_WORDS)
    return run


def test_the_fp32_code_against_the_fp64_statement(driver):
    """Measured here: of the 20 000 records of seed 5, 0.070 % are excluded; the integers and the choice of the others
    are the fp64 statement's; ul' and alpha within tolerance on 100.000 % (C++) and 100.000 % (numpy float32)."""
    rec = PS.records()
    assert rec.shape == (20000, PS.RECORD_WORDS)
    got = driver(rec).astype(np.float64)
    ref, ref32 = PS.statement(rec, np.float64), PS.statement(rec, np.float32)
    out = PS.excluded(rec)
    print(f"\nexcluded (a byte within 1e-4 of a tie, or ul within 1e-6 of m): {100 * out.mean():.3f} % of {len(rec)} records")
    assert out.mean() <= 0.002, out.mean()
    keep = ~out
    assert np.array_equal(got[keep, 0:6], ref[keep, 0:6])  # c8, r8, m8 and the choice: exactly
    within = lambda a: float((np.abs(a[keep, 6:8] - ref[keep, 6:8]) <= 1e-4 * np.maximum(1.0, np.abs(ref[keep, 6:8]))).all(axis=1).mean())
    code, numpy32 = within(got), within(ref32)
    print(f"rt_pbr.h on the host: ul' and alpha within tolerance on {100 * code:.3f} %; the numpy statement at float32 {100 * numpy32:.3f} %")
    assert numpy32 >= 0.97 and code >= numpy32 - 0.005, (code, numpy32)
    # the records cover both choices, both ends of the factors, and alpha's floor
    assert 0.2 < ref[:, 5].mean() < 0.8 and (ref[:, 4] == 0).sum() > 500 and (ref[:, 4] == 255).sum() > 20 and (ref[:, 7] == float(np.float32(1e-3))).sum() > 100


def test_closed_forms(driver):
    rng = np.random.default_rng(8)
    n = 4096
    ul = np.concatenate([rng.uniform(0, 1, n - 2), [0.0, np.nextafter(np.float32(1), np.float32(0))]]).astype(np.float32)
    rec = np.zeros((n, PS.RECORD_WORDS), np.float32)
    rec[:, 0:3], rec[:, 3], rec[:, 5], rec[:, 7] = rng.uniform(0, 1, (n, 3)), 1.0, rng.uniform(0, 1, n), ul
    # m8 = 0 (mf = 0, and B = 0 under mf = 1): never metal, ul' == ul bit for bit
    for mf, B in ((0.0, 1.0), (1.0, 0.0)):
        rec[:, 4], rec[:, 6] = B, mf
        got = driver(rec)
        assert (got[:, 4] == 0).all() and (got[:, 5] == 0).all() and np.array_equal(got[:, 6].view(np.uint32), ul.view(np.uint32))
    # m8 = 255: always metal
    rec[:, 4], rec[:, 6] = 1.0, 1.0
    got = driver(rec)
    assert (got[:, 4] == 255).all() and (got[:, 5] == 1).all()
    # a factor of 1 with a map byte k gives x8 == k, for all 256 k, in every byte
    k = np.arange(256)
    rec = np.zeros((256, PS.RECORD_WORDS), np.float32)
    texel = (k.astype(np.float32) / np.float32(255))  # (what image_texel hands on)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5], rec[:, 6], rec[:, 7] = texel, texel[::-1], texel, texel, texel[::-1], 1.0, 1.0, 0.5
    got = driver(rec)
    assert np.array_equal(got[:, 0], k) and np.array_equal(got[:, 1], k[::-1]) and np.array_equal(got[:, 2], k)
    assert np.array_equal(got[:, 3], k) and np.array_equal(got[:, 4], k[::-1])
    # the fp64 statement's own: the expectation of the choice is m, ul' is uniform on [0, 1) over the plastic vertices
    u = (np.arange(100000) + 0.5) / 100000
    metal, ulp = RP.choose(np.full(len(u), 77.0), u, np.float64)
    assert abs(metal.mean() - 77 / 255) < 1e-5 and abs(ulp[~metal].mean() - 0.5) < 1e-5 and ulp[~metal].min() >= 0 and ulp[~metal].max() < 1
    assert float(RP.alpha_of(np.array([0.0, 0.02, 0.5]), np.float64)[1]) == float(np.float32(1e-3))


# -------------------------------------------------------------------------------------------------- 3. the fp64 path tracer
@pytest.mark.parametrize("name", ["light sampling", "environment", "medium"])
def test_installed_leaves_the_pinned_cases_alone(rtmi, golden_dir, name):
    """test_glossy.py's three pinned cases with pbr among ref64.trace's own vertices: the draws and the signature are exact, the
    radiance within 1e-9.  (Named for the wrapper the material once was installed by; test_glass.py's test of this name shows
    that no extension's model is reached on these cases.)"""
    from test_glossy import _existing_cases
    pin = np.load(os.path.join(golden_dir, "ref64_trace_pin.npz"))
    sc, seed = _existing_cases(rtmi)[name]
    words = R.uniforms(rtmi, seed, NS.REF_W, NS.REF_H, 0, 1, NS.REF_DRAWS)
    S = R.RefScene(sc)
    assert not S.pbr_maps and not S.analytic and not S.noise
    for tag, dtype in (("64", np.float64), ("32", np.float32)):
        rgb, sig, draws = R.trace(S, words, dtype=dtype)
        assert np.array_equal(draws, pin[f"{name}/draws{tag}"]), (name, tag)
        assert hashlib.sha256(np.ascontiguousarray(sig).tobytes()).hexdigest() == str(pin[f"{name}/sig{tag}"]), (name, tag)
        assert np.allclose(rgb, pin[f"{name}/rgb{tag}"], rtol=1e-9, atol=1e-12), (name, tag)


@pytest.fixture(scope="module")
def references(rtmi):
    made, words = {}, PS.inputs(rtmi, "room")[0]

    def of(name):
        if name not in made:
            sc = PS.scene(rtmi, name)
            S = R.RefScene(sc)
            made[name] = (sc, S, words, R.reference(S, words))
        return made[name]
    return of


@pytest.mark.parametrize("name", list(PS.CASES) + list(PS.EXTRA))
def test_the_cases_hold_their_vertices_and_are_reachable(rtmi, references, name):
    """every GPU case: the reference stays within its draws, its tally shows the vertices the case is about, and the fp32
    statement meets share >= 0.98 and flips <= 0.5 % against the fp64 one -- the per-sample thresholds (0.97, 1 %) are then
    reachable by a correct kernel"""
    sc, S, words, (ref, stable, draws, tally) = references(name)
    assert len(words) >= 16000 and draws.max() <= NS.REF_DRAWS
    PS.check_contents(name, tally)
    rgb32, _, _ = R.trace(S, words, dtype=np.float32)
    j = R.judge(rgb32, ref, stable)
    print("\n" + R.row(name + " (fp32 reference)", j))
    print("    " + ", ".join(f"{k[4:]} {v}" for k, v in tally.items() if k.startswith("pbr_") and v))
    assert j["flips"] <= 0.005 and j["share"] >= 0.98, j
    twin, m = PS.plain_twin(rtmi, name), sc.materials()
    g = m["type"] == RP.PBR
    assert g.any() and not (twin.materials()["type"] == RP.PBR).any() and twin.prims().tobytes() == sc.prims().tobytes()
    assert (twin.materials()["type"][g] == R.LAMBERTIAN).all() and (twin.materials()["texture"][g] == m["texture"][g]).all()
    assert not twin.light_sampling and sc.table_info().kernel_variant & PS.FAMILIES == PS.family(name)


@pytest.mark.parametrize("name,mistake", PS.MISTAKES)
def test_the_perturbations_change_the_reference(references, name, mistake):
    sc, S, words, (ref, stable, _, _) = references(name)
    wrong, _, _ = R.trace(S, words, perturb=(mistake,))
    j = R.judge(wrong, ref, stable)
    print(f"\n{name}, {mistake}: the perturbed reference agrees with the reference on {100 * j['share']:.1f} % of the samples")
    assert j["share"] < 0.97, j


def test_a_map_across_the_threshold_is_traced_per_hit(rtmi):
    """The material the wrappers once refused -- a checker map whose G = 0.02 / 0.6 carries r8 = 5 / 153 across the light-sample
    threshold of r8 = 13 -- on the case built around it: the decision is each hit's, so this ONE pbr material shows vertices
    without a light sample (its smooth tiles) and vertices with one (its rough tiles), and no other glossy material is there"""
    name = "a map across the threshold"
    sc = PS.scene(rtmi, name)
    S = R.RefScene(sc)
    assert (S.mats["type"] == RP.PBR).sum() == 1 and not np.isin(S.mats["type"], (R.ROUGH_METAL, R.PLASTIC, R.ROUGH_GLASS)).any()
    words = PS.inputs(rtmi, "room")[0][:NS.REF_W * NS.REF_H * 3]
    log = R.new_log()
    rgb, sig, draws = R.trace(S, words, log=log)
    tally = R.tally(sig, S, log)
    print("\n    " + ", ".join(f"{k[4:]} {v}" for k, v in tally.items() if k.startswith("pbr_") and v))
    assert np.isfinite(rgb).all() and draws.max() <= NS.REF_DRAWS
    assert tally["pbr_smooth_vertices"] >= 100 and tally["glossy_light_samples"] >= 100 and tally["pbr_lit"] >= 50, tally
    # (every glossy vertex is this material's: those that drew and took no light sample are the smooth ones, roulette losses aside)
    assert tally["glossy_light_samples"] == tally["pbr_light_evaluations"] and tally["pbr_checker_map_hits"] == tally["pbr_vertices"]
    assert tally["pbr_vertices"] - tally["pbr_below"] > tally["pbr_smooth_vertices"] > 0


def test_m0_is_the_plastic_of_ref64(rtmi):
    """with m = 0, no map, colour and roughness on the 8-bit grid: ref64_pbr gives unmodified ref64's radiance on the plastic
    twin, sample by sample (the draws and the model coincide; a rough_metal twin takes two draws where pbr takes three, so m = 1
    is a statistical statement: test_gpu_pbr.py)"""
    words = PS.inputs(rtmi, "room")[0][:NS.REF_W * NS.REF_H * 3]
    sc, tw = PS.grid_scene(rtmi, "pbr0"), PS.grid_scene(rtmi, "plastic")
    a, _, da = R.trace(R.RefScene(sc), words)
    b, _, db = R.trace(R.RefScene(tw), words)
    assert np.array_equal(da, db) and np.allclose(a, b, rtol=1e-12, atol=1e-15), float(np.abs(a - b).max())
