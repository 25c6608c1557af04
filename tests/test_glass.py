"""Rough glass (GGX transmission with a Beer-Lambert tint) without a GPU:
  1. the interface -- C, C++, Python, JSON, the argument rules and their status codes, tint / tint_distance against absorption,
     the round trip to the same packed image, the packed record's words, the bump; scenes without the material pack to the
     digests recorded before (tests/golden/bump_off_pack_digests.json, read here);
  2. csrc/rt_glass.h compiled by the host compiler against the fp64 statement of ref64_glass.py (7m's rule: the C++ code's share
     within tolerance is at least the fp32 numpy statement's minus 0.5 points; branch flips counted apart, at most 0.5 %);
  3. closed forms of the model in fp64;
  4. the estimator against a quadrature of itself in fp64;
  5. no extension's model is reached on scenes without it, which trace as pinned (the pinned fixture), the cases hold
     what they are there for, and each deliberate mistake changes the reference.
test_gpu_glass.py holds the kernels to that reference."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import bump_scenes as BS
import glass_scenes as GS
import nee_scenes as NS
import ref64 as R
import ref64_glass as GL
import ref64_glossy as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_ARG, RT_ERR_SCENE = 1, 4
MK_ROUGH_GLASS = 16
T = np.float64


# ------------------------------------------------------------------------------------------------------------ 1. interface
def _two(rtmi):
    sc = rtmi.Scene.new(32, 18, 1, 4)
    sc.camera((0, 1, 5), (0, 0.5, 0), (0, 1, 0), 40.0)
    ids = [sc.rough_glass(1.5, 0.3), sc.rough_glass(1.33, 0.02, (0.25, 0.5, 2.0)), sc.rough_glass()]
    for k, m in enumerate(ids):
        sc.sphere((k - 1.0, 0.5, 0.0), 0.4, m)
    return sc, ids


def test_constructors_and_the_material_table(rtmi):
    sc, ids = _two(rtmi)
    m = sc.materials()
    assert rtmi.MATERIAL_DTYPE.itemsize == 28 == rtmi.struct_size(3) and rtmi.abi_version() == 3
    clear, tinted, default = (m[i] for i in ids)
    assert clear["type"] == 6 and clear["texture"] == -1 and clear["ir"] == np.float32(1.5) and clear["fuzz"] == np.float32(0.3)
    assert list(clear["albedo"]) == [0, 0, 0]
    assert tinted["type"] == 6 and list(tinted["albedo"]) == [np.float32(0.25), np.float32(0.5), np.float32(2.0)] and tinted["fuzz"] == np.float32(0.02)
    assert default["ir"] == np.float32(1.5) and default["fuzz"] == np.float32(0.3)
    # such a scene runs the general kernels over the wide tables, spheres only as it is
    assert sc.table_info().kernel_variant in (16, 36, 44)
    # a bump is accepted, on the C side and in JSON
    t = sc.noise_texture((0, 0, 0), (1, 1, 1))
    sc.set_bump(ids[0], t, 0.1)
    assert sc.bump(ids[0]) == (t, pytest.approx(0.1))
    back = rtmi.Scene.parse(sc.to_json())
    assert back.bump(ids[0]) == sc.bump(ids[0]) and back.table_image().tobytes() == sc.table_image().tobytes()
    # a moving sphere may carry it
    sc.add_moving_sphere((0, 2, 0), (1, 2, 0), 0.3, ids[1])
    assert len(sc.moving_spheres()) == 1


def test_the_c_entry_point_and_its_argument_rules(rtmi):
    lib = ctypes.CDLL(rtmi.LIB_PATH)
    lib.rt_scene_new.restype = ctypes.c_void_p
    lib.rt_scene_new.argtypes = [ctypes.c_int] * 4
    f3 = ctypes.c_float * 3
    add = lib.rt_scene_add_rough_glass
    add.argtypes, add.restype = [ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_float)], ctypes.c_int
    lib.rt_scene_free.argtypes, lib.rt_scene_free.restype = [ctypes.c_void_p], None
    lib.rt_last_error.restype = ctypes.c_char_p
    s = lib.rt_scene_new(8, 8, 1, 2)
    try:
        assert add(s, 1.5, 0.0, None) == 0
        assert add(s, 2.4, 1.0, f3(0.0, 3.0, 0.5)) == 1
        nan, inf = float("nan"), float("inf")
        bad = [lambda: add(s, 1.0, 0.5, None), lambda: add(s, 0.9, 0.5, None), lambda: add(s, nan, 0.5, None), lambda: add(s, inf, 0.5, None),
               lambda: add(s, 1.5, -0.01, None), lambda: add(s, 1.5, 1.01, None), lambda: add(s, 1.5, nan, None),
               lambda: add(s, 1.5, 0.5, f3(-0.1, 0, 0)), lambda: add(s, 1.5, 0.5, f3(0, nan, 0)), lambda: add(s, 1.5, 0.5, f3(0, 0, inf)),
               lambda: add(None, 1.5, 0.5, None)]
        for k, call in enumerate(bad):
            assert call() == -RT_ERR_ARG, k
            assert lib.rt_last_error(), k
    finally:
        lib.rt_scene_free(s)
    sc = rtmi.Scene.new(8, 8, 1, 2)
    for call in (lambda: sc.rough_glass(1.0, 0.3), lambda: sc.rough_glass(1.5, 2.0), lambda: sc.rough_glass(1.5, 0.3, (0, -1, 0))):
        with pytest.raises(rtmi.RtmiError) as e:
            call()
        assert e.value.status == RT_ERR_ARG


def test_json_reads_writes_and_refuses(rtmi):
    sc, ids = _two(rtmi)
    text = sc.to_json()
    mats = json.loads(text)["material"]["data"]
    assert mats[ids[0]] == {"type": "rough_glass", "ir": 1.5, "roughness": 0.3, "absorption": [0, 0, 0]}
    assert mats[ids[1]] == {"type": "rough_glass", "ir": 1.33, "roughness": 0.02, "absorption": [0.25, 0.5, 2]}
    back = rtmi.Scene.parse(text)
    assert back.materials().tobytes() == sc.materials().tobytes() and back.prims().tobytes() == sc.prims().tobytes()
    assert back.table_image().tobytes() == sc.table_image().tobytes()

    def with_material(m):
        d = json.loads(text)
        d["material"]["data"][ids[0]] = m
        return json.dumps(d)
    good = {"type": "rough_glass", "ir": 1.5, "roughness": 0.3}
    assert list(rtmi.Scene.parse(with_material(good)).materials()[ids[0]]["albedo"]) == [0, 0, 0]
    # a tint is converted in fp64, sigma = -ln(tint) / tint_distance, rounded once, and written back as absorption
    tint, d = [0.9, 0.5, 1.0], 0.7
    got = rtmi.Scene.parse(with_material(dict(good, tint=tint, tint_distance=d)))
    want = [np.float32(-np.log(c) / d) for c in tint]
    assert list(got.materials()[ids[0]]["albedo"]) == want and want[2] == 0 and not np.signbit(got.materials()[ids[0]]["albedo"][2])
    written = json.loads(got.to_json())["material"]["data"][ids[0]]
    assert set(written) == {"type", "ir", "roughness", "absorption"} and [np.float32(x) for x in written["absorption"]] == want
    assert rtmi.Scene.parse(got.to_json()).table_image().tobytes() == got.table_image().tobytes()
    bad = [dict(good, ir=1.0), dict(good, ir="x"), dict(good, roughness=1.5), dict(good, roughness=-0.1), {k: v for k, v in good.items() if k != "ir"},
           {k: v for k, v in good.items() if k != "roughness"}, dict(good, absorption=[0, -1, 0]), dict(good, absorption=[0, 1]),
           dict(good, absorption=[0, 0, 0], tint=tint, tint_distance=d), dict(good, absorption=[0, 0, 0], tint_distance=d),
           dict(good, tint=tint), dict(good, tint_distance=d), dict(good, tint=tint, tint_distance=0), dict(good, tint=tint, tint_distance=-1),
           dict(good, tint=[0.0, 0.5, 0.5], tint_distance=d), dict(good, tint=[1.1, 0.5, 0.5], tint_distance=d),
           dict(good, texture=0), dict(good, albedo=[0, 0, 0]), dict(good, fuzz=0.1), dict(good, index_of_refraction=1.5), dict(good, ior=1.5)]
    for k, m in enumerate(bad):
        with pytest.raises(rtmi.RtmiError) as e:
            rtmi.Scene.parse(with_material(m))
        assert e.value.status == RT_ERR_SCENE, (k, str(e.value))


def test_the_shipped_scene_and_the_cpp_wrapper(rtmi, tmp_path):
    sc = rtmi.Scene.load(os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "frosted_glass.json"))
    m, p = sc.materials(), sc.prims()
    glass = m[m["type"] == 6]
    assert len(glass) == 7 and (glass["albedo"] > 0).any(axis=1).sum() == 3 and sc.bump(7) is not None
    assert not sc.light_sampling  # (left to --nee, as in every shipped scene)
    sc.set_light_sampling(True)
    assert len(sc.lights()) == 1
    assert (p["type"] == 6).sum() == 6 and (p["type"] == R.TRIANGLE).sum() > 100 and sc.table_info().kernel_variant & 255 in (16, 36, 44)
    src = tmp_path / "w.cpp"
    src.write_text('#include "rtmi.hpp"\n#include <cstdio>\nint main() {\n'
                   "  rtmi::scene s(16, 9, 1, 3);\n"
                   "  s.add(rtmi::sphere(rtmi::point3(0, 0, 0), 1.0f, rtmi::rough_glass(1.4f, 0.25f, rtmi::color(0.5f, 0.0f, 2.0f))));\n"
                   "  s.add(rtmi::sphere(rtmi::point3(2, 0, 0), 1.0f, rtmi::rough_glass()));\n"
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
    assert mats[0] == {"type": "rough_glass", "ir": 1.4, "roughness": 0.25, "absorption": [0.5, 0, 2]}
    assert mats[1] == {"type": "rough_glass", "ir": 1.5, "roughness": 0.3, "absorption": [0, 0, 0]}


def test_the_packed_record(rtmi):
    """{kind 16, alpha = max(r^2, 1e-3), 1 / ir, r}{sigma.rgb, ir}{0, 0, 0, bump}: found in the packed image by the first record"""
    sc, ids = _two(rtmi)
    w = sc.table_image().reshape(-1)
    bits = w.view(np.int32)
    alpha = lambda r: max(np.float32(r) * np.float32(r), np.float32(1e-3))
    inv = lambda ir: np.float32(1) / np.float32(ir)
    at = [k for k in np.flatnonzero(bits[::4] == MK_ROUGH_GLASS) * 4 if k + 36 <= len(w) and w[k + 1] == alpha(0.3) and w[k + 2] == inv(1.5) and w[k + 3] == np.float32(0.3)
          and w[k + 7] == np.float32(1.5) and bits[k + 12] == MK_ROUGH_GLASS and w[k + 15] == np.float32(0.02)]
    assert len(at) == 1, at
    f = w[at[0]:at[0] + 36]
    assert list(f[4:7]) == [0, 0, 0] and list(f[8:12]) == [0, 0, 0, 0]
    assert f[13] == np.float32(1e-3) and f[14] == inv(1.33) and list(f[16:20]) == [np.float32(0.25), np.float32(0.5), np.float32(2.0), np.float32(1.33)]
    assert bits[at[0] + 24] == MK_ROUGH_GLASS
    # the spheres' cold records carry the kind too
    assert (bits[3::4] == MK_ROUGH_GLASS).sum() >= 3


def test_scenes_without_the_material_pack_as_before(rtmi, scenes_dir, golden_dir, tmp_path):
    """every scene and pack case recorded before the feature: the digests tests/golden/bump_off_pack_digests.json holds"""
    with open(os.path.join(golden_dir, "bump_off_pack_digests.json")) as f:
        want = json.load(f)
    cases = BS.digest_cases(rtmi, scenes_dir, str(tmp_path))
    assert set(cases) == set(want) and len(want) >= 20
    for name, build in cases.items():
        assert BS.digest(build()) == want[name], name


# --------------------------------------------------------------------------------------------- 2. fp32 code, fp64 statement
def test_the_fp32_code_against_the_fp64_statement(tmp_path):
    """Measured here: C++ 100.000 %, numpy float32 100.000 % of the same-branch records of seed 5; no branch differs in either."""
    exe, fin, fout = (str(tmp_path / n) for n in ("glass_host_driver", "in.bin", "out.bin"))
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "glass_host_driver.cpp"), "-lm"], check=True)
    rec = GS.records()
    assert rec.shape == (20000, GS.RECORD_WORDS)
    rec.tofile(fin)
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    got = np.fromfile(fout, np.float32).reshape(-1, GS.OUTPUT_WORDS).astype(np.float64)
    ref, ref32 = GS.statement(rec, np.float64), GS.statement(rec, np.float32)
    (code, code_flips), (numpy32, numpy_flips) = GS.share(got, ref), GS.share(ref32, ref)
    print(f"\nrt_glass.h on the host: within tolerance {100 * code:.3f} % of the same-branch records, branch differs on {100 * code_flips:.3f} %;"
          f" the numpy statement at float32 {100 * numpy32:.3f} %, {100 * numpy_flips:.3f} %")
    assert numpy_flips <= 0.005 and code_flips <= 0.005, (numpy_flips, code_flips)
    assert numpy32 >= 0.97, numpy32
    assert code >= numpy32 - 0.005, (code, numpy32)
    # the records cover every branch, both sides and the light sample's hemisphere
    branch = ref[:, 0]
    assert (branch == 0).mean() > 0.1 and (branch == 1).mean() > 0.3 and (branch == 3).sum() > 20 and (ref[:, 11] > 0).mean() > 0.3
    assert 0.4 < (rec[:, 8] != 0).mean() < 0.6 and (ref[:, 12:15] < 0.05).any() and (ref[:, 15] > 0).all()


# ------------------------------------------------------------------------------------------------------- 3. closed forms
def test_closed_forms():
    rng = np.random.default_rng(3)
    k = 2000
    ir = rng.uniform(1.1, 2.4, k)
    one = np.ones(k)
    # normal incidence, from both sides
    f0 = ((ir - 1) / (ir + 1)) ** 2
    assert np.allclose(GL.fresnel(1 / ir, one)[0], f0, rtol=1e-12) and np.allclose(GL.fresnel(ir, one)[0], f0, rtol=1e-12)
    # beyond the critical angle (from inside: eta = ir, sin > 1 / ir)
    F, ct, tir = GL.fresnel(ir, np.sqrt(1 - 1 / ir ** 2) * rng.uniform(0, 1 - 1e-9, k))
    assert tir.all() and (F == 1).all() and (ct == 0).all()
    assert not GL.fresnel(ir, np.sqrt(1 - 1 / ir ** 2) * (1 + 1e-9))[2].any() and not GL.fresnel(1 / ir, rng.uniform(0, 1, k))[2].any()
    # F(c; eta) = F(ct; 1 / eta)
    c = rng.uniform(0.01, 1, k)
    for eta in (1 / ir, ir):
        F, ct, tir = GL.fresnel(eta, c)
        ok = ~tir
        assert ok.sum() > k // 8
        assert np.allclose(GL.fresnel(1 / eta[ok], ct[ok])[0], F[ok], rtol=1e-9)
    # the refracted direction is unit, lies in the plane of wo and h and obeys Snell's law about h
    z, ph = rng.uniform(0.05, 1, k), rng.uniform(0, 2 * np.pi, k)
    wo = np.stack([np.sqrt(1 - z * z) * np.cos(ph), np.sqrt(1 - z * z) * np.sin(ph), z], axis=1)
    h = G.sample_h(np.full(k, 0.25), wo, rng.uniform(0, 1, k), rng.uniform(0, 1, k), T)
    c = G._dot(wo, h)
    for eta in (1 / ir, ir):
        F, ct, tir = GL.fresnel(eta, c)
        ok = ~tir & (c > 0)
        wi = GL.refract(wo, h, eta, c, ct)[ok]
        assert np.allclose(G._dot(wi, wi), 1, rtol=1e-12)
        sin_o, sin_i = np.sqrt(1 - c[ok] ** 2), np.sqrt(np.maximum(0, 1 - G._dot(wi, h[ok]) ** 2))
        assert np.allclose(sin_i, eta[ok] * sin_o, atol=1e-9) and (G._dot(wi, h[ok]) < 0).all()
        assert np.allclose(G._dot(np.cross(wo[ok], h[ok]), wi), 0, atol=1e-12)
    # Tr against exp
    sigma, dist = rng.uniform(0, 3, (k, 3)), rng.uniform(0, 4, k)
    assert np.allclose(GL.tint(sigma, dist, T), np.exp(-sigma * dist[:, None]), rtol=1e-15)
    assert (GL.tint(np.zeros((k, 3)), dist, T) == 1).all()


# ------------------------------------------------------------------------------------------- 4. the estimator against itself
GRID = [(z, r, front) for z in (0.1, 0.5, 0.95) for r in (0.1, 0.4, 0.9) for front in (True, False)]
IR = 1.5


def _vertex(woz, n):
    wo = np.array([np.sqrt(1 - woz * woz), 0.0, woz])
    return np.tile([0.0, 0.0, 1.0], (n, 1)), np.tile(-wo, (n, 1))


def _integrals(woz, r, eta, ns, nphi):
    """(integral of pdf_b, integral of f cos) over the reflection hemisphere by test_glossy.py's midpoint rule: (theta, phi) about
    the mirror direction, theta = pi s^3, phi over half the circle, twice; both are zero below the surface"""
    alpha = float(G.alpha_of(r))
    wo = np.array([np.sqrt(1 - woz * woz), 0.0, woz])
    m = np.array([[-wo[0], 0.0, wo[2]]])
    a, b = G.frame(m, T)
    s = (np.arange(ns) + 0.5) / ns
    th = np.pi * s ** 3
    w_th = np.sin(th) * 3 * np.pi * s * s / ns
    ph = (np.arange(nphi) + 0.5) / nphi * np.pi
    total = np.zeros(2)
    for i in range(0, ns, 64):
        t = th[i:i + 64][:, None]
        w = (w_th[i:i + 64][:, None] * (2 * np.pi / nphi) * np.ones(nphi)[None, :]).ravel()
        wi = ((np.sin(t) * np.cos(ph))[..., None] * a + (np.sin(t) * np.sin(ph))[..., None] * b + np.cos(t)[..., None] * m).reshape(-1, 3)
        k = len(wi)
        n, ud = _vertex(woz, k)
        fc, pdf = GL.glass_eval(n, ud, np.full(k, alpha), np.full(k, eta), np.ones((k, 3)), wi, T)
        total += (pdf * w).sum(), (fc[:, 0] * w).sum()
    return total


def _converged(woz, r, eta):
    """doubled until both integrals move by less than 1e-4 (asserted)"""
    ns = 64
    prev = _integrals(woz, r, eta, ns, ns)
    while ns < 4096:
        ns *= 2
        cur = _integrals(woz, r, eta, ns, ns)
        if np.abs(cur - prev).max() < 1e-4:
            return cur
        prev = cur
    raise AssertionError(f"the quadrature did not settle: {woz}, {r}, {eta}")


def _stratified(seed, n=256):
    """n^2 = 2^16 draws: (u1, u2) jittered on an n x n grid, uf jittered on n^2 strata in a random order"""
    rng = np.random.default_rng(seed)
    i, j = np.divmod(np.arange(n * n), n)
    return (rng.permutation(n * n) + rng.random(n * n)) / (n * n), (i + rng.random(n * n)) / n, (j + rng.random(n * n)) / n


def test_the_estimator_is_consistent_with_itself():
    worst = 0.0
    for woz, r, front in GRID:
        eta = 1 / IR if front else IR
        quad = _converged(woz, r, eta)
        uf, u1, u2 = _stratified(int(1000 * woz + 10 * r) + front)
        k = len(uf)
        n, ud = _vertex(woz, k)
        alpha = np.full(k, float(G.alpha_of(r)))
        wi, att, pdf, below, absorbed, refl = GL.glass_sample(n, ud, alpha, np.full(k, eta), np.ones((k, 3)), uf, u1, u2, T)
        assert not below.any()
        live = refl & ~absorbed
        # the integral of pdf_b over the reflection hemisphere is the share of the draws that reflect and survive
        p = live.mean()
        assert abs(quad[0] - p) < 1e-4 + 5 * np.sqrt(p * (1 - p) / k), (woz, r, front, quad[0], p)
        # the integral of the reflection's f cos is their mean attenuation (every other draw: zero)
        a = np.where(live, att[:, 0], 0)
        assert abs(a.mean() - quad[1]) < 5 * a.std() / np.sqrt(k) + 1e-4, (woz, r, front, a.mean(), quad[1])
        # a reflected direction's pdf_b and attenuation are what the evaluation gives for it; a refracted one carries -1
        fc, pw = GL.glass_eval(n[live], ud[live], alpha[live], np.full(live.sum(), eta), np.ones((live.sum(), 3)), wi[live], T)
        assert np.allclose(pw, pdf[live], rtol=1e-7) and np.allclose(fc / pw[:, None], att[live], rtol=1e-7, atol=1e-12)
        assert (pdf[~refl & ~absorbed] == -1).all() and (wi[~refl & ~absorbed] @ [0, 0, 1.0] < 0).all()
        # with sigma = 0 the material gives back no more than it receives
        assert att[:, 0].mean() <= 1, (woz, r, front, att[:, 0].mean())
        worst = max(worst, float(att[:, 0].mean()))
    print(f"\nlargest mean attenuation over the grid (sigma = 0, ir = {IR}): {worst:.4f}")


# -------------------------------------------------------------------------------------------------- 5. the fp64 path tracer
@pytest.mark.parametrize("name", ["light sampling", "environment", "medium"])
def test_installed_leaves_the_pinned_cases_alone(rtmi, golden_dir, name, monkeypatch):
    """test_glossy.py's three pinned cases with every entry point of the extensions' models replaced by one that
    raises: none of them is reached without its records in the scene, the draws and the signature are exact, the radiance within
    1e-9.  (Named for the wrappers these models once were installed by.)"""
    from test_glossy import _existing_cases

    def never(*a, **k):
        raise AssertionError("an extension's model was reached in a scene without it")
    for module, names in ((R.GL, ("glass_sample", "glass_eval")), (R.PB, ("choose",)), (R.NO, ("colour",)), (R.BU, ("gradient_of",)),
                          (R.NM, ("normal",)), (R.AL, ("sample",)), (R, ("sample_quad", "sample_triangle", "quad_t"))):
        for f in names:
            monkeypatch.setattr(module, f, never)
    pin = np.load(os.path.join(golden_dir, "ref64_trace_pin.npz"))
    sc, seed = _existing_cases(rtmi)[name]
    words = R.uniforms(rtmi, seed, NS.REF_W, NS.REF_H, 0, 1, NS.REF_DRAWS)
    S = R.RefScene(sc)
    for tag, dtype in (("64", np.float64), ("32", np.float32)):
        rgb, sig, draws = R.trace(S, words, dtype=dtype)
        assert np.array_equal(draws, pin[f"{name}/draws{tag}"]), (name, tag)
        assert hashlib.sha256(np.ascontiguousarray(sig).tobytes()).hexdigest() == str(pin[f"{name}/sig{tag}"]), (name, tag)
        assert np.allclose(rgb, pin[f"{name}/rgb{tag}"], rtol=1e-9, atol=1e-12), (name, tag)


@pytest.mark.parametrize("family", ["mesh_lights", "noise", "bump", "quads", "glass", "analytic_lights", "pbr", "normal_map"])
def test_the_extensions_trace_as_pinned(rtmi, golden_dir, family):
    """golden/ref64_ext_pin.npz holds what the reference returned on one case of each extension of DESIGN 7n-7u while each was a
    module of its own around ref64's functions (golden/make_ref64_ext_pin.py; the first sample of each pixel).  As the first pin
    is compared: the draws and the signature exact, the radiance at rtol 1e-9 -- the fp64 run's after rounding to float32, as
    it is stored; the fp32 run's by its bytes.  One exception, which the fold made on purpose: a point, spot or distant light's
    sample is stated at weight 1 directly, no longer through the power heuristic at a scaled density, and lands a few roundings
    from the pinned value; the analytic-light case's fp32 radiance is therefore held to 32 float32 epsilons."""
    import importlib
    import json
    pin = np.load(os.path.join(golden_dir, "ref64_ext_pin.npz"))
    cases = json.loads(str(pin["cases"]))
    at, rec = list(cases).index(family), cases[family]
    SC = importlib.import_module({"mesh_lights": "mesh_light_scenes", "quads": "quad_scenes", "analytic_lights": "analytic_light_scenes"}.get(family, family + "_scenes"))
    sc = SC.scene(rtmi, rec["case"])
    words = SC.inputs(rtmi, rec["case"])[0]
    S, sha = R.RefScene(sc), lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    for k, (tag, dtype) in enumerate((("64", np.float64), ("32", np.float32))):
        rgb, sig, draws = R.trace(S, words[:NS.REF_W * NS.REF_H], dtype=dtype)
        assert np.array_equal(draws, pin["draws"][k][at]) and sha(sig) == rec["sig" + tag], (family, tag)
        if tag == "64":
            assert np.allclose(rgb.astype(np.float32), pin["rgb64"][at], rtol=1e-9, atol=1e-12), (family, tag)
        elif family != "analytic_lights":
            assert sha(rgb) == rec["rgb32"], (family, tag)
        else:
            pinned = (pin["rgb64"][at].view(np.int32) + pin["analytic_rgb32_steps"]).view(np.float32)
            assert sha(pinned) == rec["rgb32"] and np.allclose(rgb, pinned, rtol=32 * np.finfo(np.float32).eps, atol=0), (family, tag)


@pytest.fixture(scope="module")
def references(rtmi):
    made = {}

    def of(name):
        if name not in made:
            sc = GS.scene(rtmi, name)
            words, shutter = GS.inputs(rtmi, name)
            S = R.RefScene(sc)
            made[name] = (sc, S, words, shutter, R.reference(S, words, shutter))
        return made[name]
    return of


@pytest.mark.parametrize("name", list(GS.CASES))
def test_the_cases_hold_what_they_are_there_for(rtmi, references, name):
    """every case: the reference stays within its draws, contains its vertices, and the fp32 reference alone meets criterion
    (a) with at most 1 % of the samples flipping a branch (the condition under which a scene was kept)"""
    sc, S, words, shutter, (ref, stable, draws, tally) = references(name)
    assert len(words) >= 16000 and draws.max() <= NS.REF_DRAWS
    GS.check_contents(name, tally)
    rgb32, _, _ = R.trace(S, words, shutter=shutter, dtype=np.float32)
    j = R.judge(rgb32, ref, stable)
    print("\n" + R.row(name + " (fp32 reference)", j))
    print("    " + ", ".join(f"{k[6:]} {v}" for k, v in tally.items() if k.startswith("glass_") and not isinstance(v, list)))
    assert j["flips"] <= 0.01 and j["share"] >= 0.97, j
    # the twin has the same geometry, dielectric of the same index where the case has rough glass
    twin, m = GS.plain_twin(rtmi, name), sc.materials()
    assert not (twin.materials()["type"] == GL.ROUGH_GLASS).any() and twin.prims().tobytes() == sc.prims().tobytes()
    g = m["type"] == GL.ROUGH_GLASS
    assert g.any() and (twin.materials()["type"][g] == R.DIELECTRIC).all() and (twin.materials()["ir"][g] == m["ir"][g]).all()


@pytest.mark.parametrize("name,mistake", GS.MISTAKES)
def test_the_perturbations_change_the_reference(references, name, mistake):
    sc, S, words, shutter, (ref, stable, _, _) = references(name)
    wrong, _, _ = R.trace(S, words, shutter=shutter, perturb=(mistake,))
    j = R.judge(wrong, ref, stable)
    print(f"\n{name}, {mistake}: the perturbed reference agrees with the reference on {100 * j['share']:.1f} % of the samples")
    assert j["share"] < 0.97, j
