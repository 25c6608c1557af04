"""The glossy materials (GGX rough metal, coated plastic) without a GPU:
  1. the interface -- C, Python, JSON, the argument rules, the material tables, the packed records;
  2. csrc/rt_glossy.h compiled by the host compiler against the fp64 statement of ref64_glossy.py (criterion (b)'s form: the
     C++ code's share within tolerance is at least the fp32 numpy statement's minus 0.5 points);
  3. the estimator against itself in fp64: pdf_b integrates to 1 with the absorbed share, the mean attenuation is the integral
     of f cos, reciprocity, and a white rough metal reflects no more than it receives;
  4. ref64.trace, which holds the glossy vertices, still returns on scenes without glossy materials what it returned before
     they joined it (a pinned fixture), never evaluates the glossy model there, and its glossy perturbations change what
     they name.
test_gpu_glossy.py holds the kernels to that reference."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import glossy_scenes as GS
import media_scenes as MS
import nee_scenes as NS
import ref64 as R
import ref64_glossy as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_ARG, RT_ERR_SCENE = 1, 4
MK_ROUGH_METAL, MK_PLASTIC_SOLID, MK_PLASTIC_CHECKER, MK_PLASTIC_IMAGE = 9, 10, 11, 12


# ------------------------------------------------------------------------------------------------------------ 1. interface
def _three(rtmi):
    """one material of every packed kind, on a sphere each"""
    sc = rtmi.Scene.new(32, 18, 1, 4)
    sc.camera((0, 1, 5), (0, 0.5, 0), (0, 1, 0), 40.0)
    ids = [sc.rough_metal((0.9, 0.8, 0.7), 0.3),
           sc.plastic((0.2, 0.3, 0.4), roughness=0.02),
           sc.plastic(sc.checker_texture((0.8, 0.8, 0.8), (0.1, 0.3, 0.1)), 1.33, 0.4),
           sc.plastic(sc.image_texture(np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)), 2.0, 1.0)]
    for k, m in enumerate(ids):
        sc.sphere((k - 1.5, 0.5, 0.0), 0.4, m)
    return sc, ids


def test_constructors_and_the_material_table(rtmi):
    sc, ids = _three(rtmi)
    m = sc.materials()
    assert rtmi.MATERIAL_DTYPE.itemsize == 28 == rtmi.struct_size(3) and rtmi.abi_version() == 3

    class Mirror(ctypes.Structure):  # rt_material, field by field
        _fields_ = [("type", ctypes.c_int32), ("texture", ctypes.c_int32), ("albedo", ctypes.c_float * 3), ("fuzz", ctypes.c_float),
                    ("ir", ctypes.c_float)]
    assert ctypes.sizeof(Mirror) == 28
    rough, solid, checker, image = (m[i] for i in ids)
    assert rough["type"] == 4 and rough["texture"] == -1 and list(rough["albedo"]) == [np.float32(0.9), np.float32(0.8), np.float32(0.7)]
    assert rough["fuzz"] == np.float32(0.3)
    assert solid["type"] == 5 and solid["fuzz"] == np.float32(0.02) and solid["ir"] == np.float32(1.5)  # (ior's default)
    assert checker["type"] == 5 and checker["ir"] == np.float32(1.33) and image["fuzz"] == 1.0 and image["ir"] == 2.0
    tex = sc.textures()
    assert [int(tex[int(x["texture"])]["type"]) for x in (solid, checker, image)] == [R.SOLID, R.CHECKER, R.IMAGE]
    # such a scene runs the general kernels over the wide tables, spheres only as it is
    assert sc.table_info().kernel_variant in (16, 36, 44)


def test_the_c_entry_points_and_their_argument_rules(rtmi):
    lib = ctypes.CDLL(rtmi.LIB_PATH)
    lib.rt_scene_new.restype = ctypes.c_void_p
    lib.rt_scene_new.argtypes = [ctypes.c_int] * 4
    f3 = ctypes.c_float * 3
    for fn, args in ((lib.rt_scene_add_rough_metal, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_float]),
                     (lib.rt_scene_add_plastic, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float]),
                     (lib.rt_scene_add_solid_color, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]), (lib.rt_scene_free, [ctypes.c_void_p])):
        fn.argtypes, fn.restype = args, ctypes.c_int
    lib.rt_scene_free.restype = None
    lib.rt_last_error.restype = ctypes.c_char_p
    s = lib.rt_scene_new(8, 8, 1, 2)
    try:
        t = lib.rt_scene_add_solid_color(s, f3(0.5, 0.5, 0.5))
        assert t == 0
        assert lib.rt_scene_add_rough_metal(s, f3(1.0, 0.0, 0.5), 0.0) == 0
        assert lib.rt_scene_add_plastic(s, t, 1.5, 1.0) == 1
        nan, inf = float("nan"), float("inf")
        bad = [lambda: lib.rt_scene_add_rough_metal(s, f3(1.0, 0.0, 0.5), -0.01), lambda: lib.rt_scene_add_rough_metal(s, f3(1.0, 0.0, 0.5), 1.01),
               lambda: lib.rt_scene_add_rough_metal(s, f3(1.0, 0.0, 0.5), nan), lambda: lib.rt_scene_add_rough_metal(s, f3(1.1, 0.0, 0.5), 0.5),
               lambda: lib.rt_scene_add_rough_metal(s, f3(0.5, -0.1, 0.5), 0.5), lambda: lib.rt_scene_add_rough_metal(s, f3(0.5, 0.5, nan), 0.5),
               lambda: lib.rt_scene_add_rough_metal(s, f3(0.5, inf, 0.5), 0.5), lambda: lib.rt_scene_add_rough_metal(s, None, 0.5),
               lambda: lib.rt_scene_add_rough_metal(None, f3(0.5, 0.5, 0.5), 0.5),
               lambda: lib.rt_scene_add_plastic(s, t, 1.0, 0.5), lambda: lib.rt_scene_add_plastic(s, t, 0.9, 0.5),
               lambda: lib.rt_scene_add_plastic(s, t, nan, 0.5), lambda: lib.rt_scene_add_plastic(s, t, inf, 0.5),
               lambda: lib.rt_scene_add_plastic(s, t, 1.5, 1.5), lambda: lib.rt_scene_add_plastic(s, t, 1.5, nan),
               lambda: lib.rt_scene_add_plastic(s, t + 1, 1.5, 0.5), lambda: lib.rt_scene_add_plastic(s, -1, 1.5, 0.5),
               lambda: lib.rt_scene_add_plastic(None, t, 1.5, 0.5)]
        for k, call in enumerate(bad):
            assert call() == -RT_ERR_ARG, k
            assert lib.rt_last_error(), k
    finally:
        lib.rt_scene_free(s)
    # the same rules through Python
    sc = rtmi.Scene.new(8, 8, 1, 2)
    for call in (lambda: sc.rough_metal((0.5, 0.5, 0.5), 2.0), lambda: sc.plastic((0.5, 0.5, 0.5), 1.0, 0.3), lambda: sc.plastic(7, 1.5, 0.3)):
        with pytest.raises(rtmi.RtmiError) as e:
            call()
        assert e.value.status == RT_ERR_ARG


def test_json_reads_writes_and_refuses(rtmi):
    sc, ids = _three(rtmi)
    text = sc.to_json()
    doc = json.loads(text)
    mats = doc["material"]["data"]
    assert mats[ids[0]] == {"type": "rough_metal", "albedo": [0.9, 0.8, 0.7], "roughness": 0.3}
    assert mats[ids[2]]["type"] == "plastic" and set(mats[ids[2]]) == {"type", "texture", "ior", "roughness"}
    back = rtmi.Scene.parse(text)
    assert back.materials().tobytes() == sc.materials().tobytes() and back.textures().tobytes() == sc.textures().tobytes()
    assert back.prims().tobytes() == sc.prims().tobytes()
    assert back.table_image().tobytes() == sc.table_image().tobytes()

    def with_material(m):
        d = json.loads(text)
        d["material"]["data"][ids[0]] = m
        return json.dumps(d)
    good = {"type": "plastic", "texture": 0, "ior": 1.5, "roughness": 0.3}
    rtmi.Scene.parse(with_material(good))
    bad = [dict(good, roughness=1.5), dict(good, roughness=-0.1), dict(good, ior=1.0), dict(good, texture=99), dict(good, texture=-1),
           dict(good, fuzz=0.1), {k: v for k, v in good.items() if k != "ior"}, dict(good, roughness="x"),
           {"type": "rough_metal", "albedo": [0.5, 0.5, 1.5], "roughness": 0.3}, {"type": "rough_metal", "albedo": [0.5, 0.5, 0.5], "roughness": 2},
           {"type": "rough_metal", "albedo": [0.5, 0.5, 0.5]}, {"type": "rough_metal", "albedo": [0.5, 0.5, 0.5], "roughness": 0.3, "fuzz": 0.1},
           {"type": "rough_metal", "albedo": [0.5, 0.5], "roughness": 0.3}, {"type": "rough_plastic", "roughness": 0.3}]
    for k, m in enumerate(bad):
        with pytest.raises(rtmi.RtmiError) as e:
            rtmi.Scene.parse(with_material(m))
        assert e.value.status == RT_ERR_SCENE, (k, str(e.value))


def test_the_shipped_scene_and_the_cpp_wrappers(rtmi, tmp_path):
    sc = rtmi.Scene.load(os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "glossy_balls.json"))
    m = sc.materials()
    rough = m[m["type"] == 4]["fuzz"]
    assert len(rough) >= 4 and (np.diff(rough) > 0).all()            # a row of rising roughness
    sc.set_light_sampling(True)  # (the file leaves it to --nee: test_light_sampling.py loads every shipped scene with it off)
    assert (m["type"] == 5).sum() == 2 and len(sc.lights()) == 1
    p = sc.prims()
    tri = p[p["type"] == R.TRIANGLE]
    assert len(tri) > 100 and int(m[tri["material"][0]]["type"]) == 5 and np.any(tri["f"][:, :6] != 0)  # the smooth plastic torus
    floor = m[p[0]["material"]]
    assert floor["type"] == 5 and sc.textures()[floor["texture"]]["type"] == R.CHECKER
    # include/rtmi.hpp: the two wrappers register their materials through the C entry points
    src = tmp_path / "w.cpp"
    src.write_text('#include "rtmi.hpp"\n#include <cstdio>\nint main() {\n'
                   "  rtmi::scene s(16, 9, 1, 3);\n"
                   "  s.add(rtmi::sphere(rtmi::point3(0, 0, 0), 1.0f, rtmi::rough_metal(rtmi::color(0.9f, 0.8f, 0.7f), 0.25f)));\n"
                   "  s.add(rtmi::sphere(rtmi::point3(2, 0, 0), 1.0f, rtmi::plastic(rtmi::color(0.1f, 0.2f, 0.3f), 1.4f, 0.5f)));\n"
                   '  std::vector<char> b(1 << 16);\n  size_t n = rt_scene_to_json(s.handle(), b.data(), b.size());\n'
                   '  if (n == 0 || n > b.size()) return 1;\n  fputs(b.data(), stdout);\n  return 0;\n}\n')
    exe = str(tmp_path / "w")
    pkg = os.path.dirname(rtmi.LIB_PATH)
    build = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src), "-L", pkg, "-lrtmi", "-Wl,-rpath," + pkg],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    mats = json.loads(out.stdout)["material"]["data"]
    assert mats[0] == {"type": "rough_metal", "albedo": [0.9, 0.8, 0.7], "roughness": 0.25}
    assert mats[1]["type"] == "plastic" and mats[1]["ior"] == 1.4 and mats[1]["roughness"] == 0.5


def test_the_packed_records(rtmi):
    """kind, alpha = max(r^2, 1e-3), r0 = ((ior - 1) / (ior + 1))^2, r and the texture words, found in the packed image by
    the rough metal's record (kind 9, alpha, 0, r, F0)"""
    sc, ids = _three(rtmi)
    w = sc.table_image().reshape(-1)
    bits = w.view(np.int32)
    alpha = lambda r: max(np.float32(r) * np.float32(r), np.float32(1e-3))
    r0 = lambda ior: ((np.float32(ior) - np.float32(1)) / (np.float32(ior) + np.float32(1))) ** 2
    at = [k for k in np.flatnonzero(bits[::4] == MK_ROUGH_METAL) * 4
          if w[k + 1] == alpha(0.3) and w[k + 3] == np.float32(0.3) and list(w[k + 4:k + 7]) == [np.float32(0.9), np.float32(0.8), np.float32(0.7)]]
    assert len(at) == 1, at
    rec = lambda i: (w[at[0] + 12 * (i - ids[0]):][:12], bits[at[0] + 12 * (i - ids[0]):][:12])
    f, b = rec(ids[0])
    assert f[2] == 0
    f, b = rec(ids[1])
    assert b[0] == MK_PLASTIC_SOLID and f[1] == np.float32(1e-3) and f[2] == r0(1.5) and f[3] == np.float32(0.02)
    assert list(f[4:7]) == [np.float32(0.2), np.float32(0.3), np.float32(0.4)]
    f, b = rec(ids[2])
    assert b[0] == MK_PLASTIC_CHECKER and f[1] == alpha(0.4) and f[2] == r0(1.33) and f[3] == np.float32(0.4)
    assert list(f[4:7]) == [np.float32(0.8)] * 3 and list(f[8:11]) == [np.float32(0.1), np.float32(0.3), np.float32(0.1)]
    f, b = rec(ids[3])
    assert b[0] == MK_PLASTIC_IMAGE and f[1] == 1.0 and f[2] == r0(2.0) and f[3] == 1.0 and (b[5], b[6]) == (2, 3)
    texels = bits[b[4]:b[4] + 6]
    assert list(texels & 255) == [0, 3, 6, 9, 12, 15]
    # the spheres' cold records carry the kinds too
    kinds = sorted(int(k) for k in bits[3::4][np.isin(bits[3::4], (9, 10, 11, 12))])
    assert kinds[:4] == [9, 10, 11, 12]


# --------------------------------------------------------------------------------------------- 2. fp32 code, fp64 statement
def test_the_fp32_code_against_the_fp64_statement(tmp_path):
    """Measured here: C++ 100.000 %, numpy float32 99.995 % of the 20 000 records."""
    exe, fin, fout = (str(tmp_path / n) for n in ("glossy_host_driver", "in.bin", "out.bin"))
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "glossy_host_driver.cpp"), "-lm"], check=True)
    rec = GS.records()
    assert rec.shape == (20000, GS.RECORD_WORDS)
    rec.tofile(fin)
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    got = np.fromfile(fout, np.float32).reshape(-1, GS.OUTPUT_WORDS).astype(np.float64)
    ref, ref32 = GS.statement(rec, np.float64), GS.statement(rec, np.float32)
    code, numpy32 = GS.share(got, ref), GS.share(ref32, ref)
    print(f"\nrt_glossy.h on the host: within tolerance {100 * code:.3f} % of {len(rec)} records; the numpy statement at float32 {100 * numpy32:.3f} %")
    assert numpy32 >= 0.97, numpy32          # (below: an ill-conditioned expression in the specification's order of evaluation)
    assert code >= numpy32 - 0.005, (code, numpy32)
    # the records cover both lobes and both ends of the ranges
    assert 0.2 < ref[:, 24].mean() < 0.8 and (ref[:, 0] == 0).mean() > 0.8 and (ref[:, 11] > 0).mean() > 0.95


# ------------------------------------------------------------------------------------------- 3. the estimator against itself
GRID = [(z, r) for z in (0.1, 0.5, 0.95) for r in (0.1, 0.4, 0.9)]
T = np.float64


def _vertex(woz, n):
    wo = np.array([np.sqrt(1 - woz * woz), 0.0, woz])
    return wo, np.tile([0.0, 0.0, 1.0], (n, 1)), np.tile(-wo, (n, 1))


def _integrals(woz, r, plastic, f0, rho, ns, nphi):
    """(integral of pdf_b, integral of f cos per channel) over the sphere of directions by the midpoint rule in (theta, phi) about
    the mirror direction, theta = pi s^3 with s uniform (the lobe sits at that pole) and phi over half the circle, twice (the
    integrand is symmetric about the plane of incidence); f cos and pdf_b are zero below the surface"""
    alpha = float(G.alpha_of(r))
    wo = np.array([np.sqrt(1 - woz * woz), 0.0, woz])
    m = np.array([[-wo[0], 0.0, wo[2]]])
    a, b = G.frame(m, T)
    s = (np.arange(ns) + 0.5) / ns
    th = np.pi * s ** 3
    w_th = np.sin(th) * 3 * np.pi * s * s / ns
    ph = (np.arange(nphi) + 0.5) / nphi * np.pi
    total = np.zeros(4)
    for i in range(0, ns, 64):
        t = th[i:i + 64][:, None]
        w = (w_th[i:i + 64][:, None] * (2 * np.pi / nphi) * np.ones(nphi)[None, :]).ravel()
        wi = ((np.sin(t) * np.cos(ph))[..., None] * a + (np.sin(t) * np.sin(ph))[..., None] * b + np.cos(t)[..., None] * m).reshape(-1, 3)
        k = len(wi)
        _, n, ud = _vertex(woz, k)
        fc, pdf = G.glossy_eval(n, ud, np.full(k, alpha), np.full(k, plastic), np.tile(f0, (k, 1)), np.tile(rho, (k, 1)), wi, T)
        total[0] += (pdf * w).sum()
        total[1:] += (fc * w[:, None]).sum(axis=0)
    return total


def _converged(woz, r, plastic, f0, rho):
    """doubled until the four integrals move by less than 1e-4 (asserted)"""
    ns = 64
    prev = _integrals(woz, r, plastic, f0, rho, ns, ns)
    while ns < 4096:
        ns *= 2
        cur = _integrals(woz, r, plastic, f0, rho, ns, ns)
        if np.abs(cur - prev).max() < 1e-4:
            return cur
        prev = cur
    raise AssertionError(f"the quadrature did not settle: {woz}, {r}, {plastic}")


def _stratified(seed, n=256):
    """n^2 = 2^16 draws: (u1, u2) jittered on an n x n grid, ul jittered on n^2 strata in a random order"""
    rng = np.random.default_rng(seed)
    i, j = np.divmod(np.arange(n * n), n)
    return (rng.permutation(n * n) + rng.random(n * n)) / (n * n), (i + rng.random(n * n)) / n, (j + rng.random(n * n)) / n


@pytest.mark.parametrize("plastic", [False, True], ids=["rough_metal", "plastic"])
def test_the_estimator_is_consistent_with_itself(plastic):
    f0 = np.array([0.04] * 3 if plastic else [1.0, 0.8, 0.5])
    rho = np.array([0.8, 0.5, 0.2])
    worst = 0.0
    for woz, r in GRID:
        quad = _converged(woz, r, plastic, f0, rho)
        ul, u1, u2 = _stratified(int(1000 * woz + 10 * r))
        k = len(ul)
        _, n, ud = _vertex(woz, k)
        wi, att, pdf, below, absorbed, lobe = G.glossy_sample(n, ud, np.full(k, float(G.alpha_of(r))), np.full(k, plastic), np.tile(f0, (k, 1)),
                                                            np.tile(rho, (k, 1)), ul, u1, u2, T)
        assert not below.any()
        # pdf_b integrates to one, with the share of the draws that came out below the surface
        p = absorbed.mean()
        assert abs(quad[0] + p - 1) < 1e-4 + 5 * np.sqrt(p * (1 - p) / k) + 1e-3 * p, (woz, r, quad[0], p)
        # the mean attenuation (an absorbed draw: zero) is the integral of f cos
        mean, se = att.mean(axis=0), att.std(axis=0) / np.sqrt(k)
        assert (np.abs(mean - quad[1:]) < 5 * se + 1e-4).all(), (woz, r, mean, quad[1:], se)
        # the drawn direction's pdf_b and attenuation are what the evaluation gives for it
        ok = ~absorbed
        fc, pw = G.glossy_eval(n[ok], ud[ok], np.full(ok.sum(), float(G.alpha_of(r))), np.full(ok.sum(), plastic), np.tile(f0, (ok.sum(), 1)),
                               np.tile(rho, (ok.sum(), 1)), wi[ok], T)
        assert np.allclose(pw, pdf[ok], rtol=1e-7) and np.allclose(fc / pw[:, None], att[ok], rtol=1e-7, atol=1e-12)
        worst = max(worst, float(quad[1:].max()))
        if not plastic:  # a white metal reflects no more than it receives
            white = _converged(woz, r, False, np.ones(3), rho)
            assert white[1] <= 1 + 1e-4, (woz, r, white[1])
    print(f"\nlargest directional albedo over the grid ({'plastic, rho <= 0.8' if plastic else 'rough metal, F0 <= 1.0'}): {worst:.4f}")


def test_reciprocity():
    """f cos(wo, wi) / wi.z = f cos(wi, wo) / wo.z for both materials"""
    rng = np.random.default_rng(11)
    k = 4000

    def hemi():
        z, ph = rng.uniform(0.02, 1, k), rng.uniform(0, 2 * np.pi, k)
        return np.stack([np.sqrt(1 - z * z) * np.cos(ph), np.sqrt(1 - z * z) * np.sin(ph), z], axis=1)
    a, b = hemi(), hemi()
    n = np.tile([0.0, 0.0, 1.0], (k, 1))
    alpha = G.alpha_of(rng.uniform(0.05, 1, k)).astype(T)
    f0, rho = rng.uniform(0, 1, (k, 3)), rng.uniform(0, 1, (k, 3))
    for plastic in (False, True):
        f = np.repeat(f0[:, :1], 3, axis=1) if plastic else f0
        P = np.full(k, plastic)
        fab, _ = G.glossy_eval(n, -a, alpha, P, f, rho, b, T)
        fba, _ = G.glossy_eval(n, -b, alpha, P, f, rho, a, T)
        assert np.allclose(fab / b[:, 2:3], fba / a[:, 2:3], rtol=1e-9, atol=1e-300)


# -------------------------------------------------------------------------------------------------- 4. the fp64 path tracer
def _existing_cases(rtmi):
    import ext_scenes as XS
    nee = NS.nee_cases()["metal1.0 x xz"](rtmi)
    nee.set_light_sampling(True)
    env = XS.scene(rtmi, "env + textures + mesh, light sampling")
    fog = XS.scene(rtmi, "fog over textures")
    return {"light sampling": (nee, NS.REF_SEED), "environment": (env, NS.REF_SEED), "medium": (fog, MS.REF_SEED)}


@pytest.mark.parametrize("name", ["light sampling", "environment", "medium"])
def test_the_tracer_is_pinned_on_scenes_without_glossy_materials(rtmi, golden_dir, name):
    """golden/ref64_trace_pin.npz holds what ref64.trace returned on these cases before the glossy materials joined its loop
    (golden/make_ref64_trace_pin.py; the first sample of each pixel).  The draws and the signature are exact: a branch or an
    order of draws that changed shows there.  rgb to rtol 1e-9: a libm whose log / sin / arccos differ in the last bit moves
    a path of a few hundred fp64 operations by far less, and the kernels are held to 1e-4."""
    pin = np.load(os.path.join(golden_dir, "ref64_trace_pin.npz"))
    sc, seed = _existing_cases(rtmi)[name]
    words = R.uniforms(rtmi, seed, NS.REF_W, NS.REF_H, 0, 1, NS.REF_DRAWS)
    S = R.RefScene(sc)
    for tag, dtype in (("64", np.float64), ("32", np.float32)):
        rgb, sig, draws = R.trace(S, words, dtype=dtype)
        assert np.array_equal(draws, pin[f"{name}/draws{tag}"]), (name, tag)
        assert hashlib.sha256(np.ascontiguousarray(sig).tobytes()).hexdigest() == str(pin[f"{name}/sig{tag}"]), (name, tag)
        assert rgb.dtype == dtype and np.allclose(rgb, pin[f"{name}/rgb{tag}"], rtol=1e-9, atol=1e-12), (name, tag)
        assert rgb.any()


def test_the_glossy_block_is_inert_without_glossy_materials(rtmi, monkeypatch):
    """on the pinned cases neither the glossy sample nor the glossy evaluation is ever called"""
    def never(*a, **k):
        raise AssertionError("the glossy model was evaluated on a scene without glossy materials")
    for module in (R, G):
        monkeypatch.setattr(module, "glossy_sample", never)
        monkeypatch.setattr(module, "glossy_eval", never)
    for name, (sc, seed) in _existing_cases(rtmi).items():
        words = R.uniforms(rtmi, seed, NS.REF_W, NS.REF_H, 0, 1, NS.REF_DRAWS)
        rgb, _, _ = R.trace(R.RefScene(sc), words)
        assert rgb.any(), name
    with pytest.raises(AssertionError, match="glossy model"):  # ... and the swap does reach the tracer
        R.trace(R.RefScene(GS.scene(rtmi, "glossy_sky")), words[:64])


@pytest.fixture(scope="module")
def references(rtmi):
    made = {}

    def of(name):
        if name not in made:
            sc = GS.scene(rtmi, name)
            words, shutter = GS.inputs(rtmi, name)
            S = R.RefScene(sc)
            made[name] = (S, words, shutter, R.reference(S, words, shutter))
        return made[name]
    return of


@pytest.mark.parametrize("name", list(GS.CASES))
def test_the_cases_hold_what_they_are_there_for(rtmi, references, name):
    """every case: the reference stays within its draws, contains its vertices, and the fp32 reference alone meets criterion
    (a) with at most 1 % of the samples flipping a branch (the condition under which a scene was kept)"""
    S, words, shutter, (ref, stable, draws, tally) = references(name)
    assert len(words) >= 16000 and draws.max() <= NS.REF_DRAWS
    GS.check_contents(name, tally)
    rgb32, _, _ = R.trace(S, words, shutter=shutter, dtype=np.float32)
    j = R.judge(rgb32, ref, stable)
    print("\n" + R.row(name + " (fp32 reference)", j))
    assert j["flips"] <= 0.01 and j["share"] >= 0.97, j
    # the twin has the same geometry and no glossy material
    twin = GS.plain_twin(rtmi, name)
    assert not np.isin(twin.materials()["type"], (G.ROUGH_METAL, G.PLASTIC)).any()
    assert twin.prims().tobytes() == GS.scene(rtmi, name).prims().tobytes()


@pytest.mark.parametrize("name,mistake", [("glossy_sky", "g1_for_g2"), ("glossy_sky", "lobe_draw_last"), ("glossy_lights", "nee_albedo_pdf")])
def test_the_perturbations_change_the_reference(references, name, mistake):
    S, words, shutter, (ref, stable, _, _) = references(name)
    wrong, _, _ = R.trace(S, words[:4000], shutter=shutter, perturb=(mistake,))
    j = R.judge(wrong, ref[:4000], stable[:4000])
    print(f"\n{name}, {mistake}: the perturbed reference agrees with the reference on {100 * j['share']:.1f} % of the samples")
    assert j["share"] < 0.9, j["share"]
