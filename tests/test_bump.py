"""Bump mapping (a noise texture's scalar as a height field that tilts the shading normal) without a GPU:
  1. the interface -- C, Python, C++, JSON, every argument rule, the round trip, the unchanged ABI -- and the packed records; every
     scene shipped before the feature and every case of smooth_pack_cases.py packs to the digest the parent commit wrote;
  2. the gradient: the fp64 statement of ref64_bump.py against central differences of ref64_noise.value, zero where fbm and
     turbulence are clamped; csrc/rt_noise.h compiled by the host compiler against the fp64 statement on 20 000 seeded records per
     style (criterion (b)'s form: the C++ code's share within tolerance is at least the fp32 numpy statement's minus 0.5 points);
  3. the model: n' is unit, n' . n > 0, k -> -k mirrors Gt, a clamped texture leaves n;
  4. ref64_bump.trace: ref64.trace's results exactly on a case without bumps; a case holds its vertices and the deliberate
     mistakes change it.
test_gpu_bump.py holds the kernels to that reference."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import bump_scenes as BS
import nee_scenes as NS
import ref64 as R
import ref64_bump as B
import ref64_noise as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
RT_ERR_ARG, RT_ERR_SCENE = 1, 4
T = np.float64


# ------------------------------------------------------------------------------------------------------------ 1. interface
def _five(rtmi):
    """a sphere of every material that takes a bump and an emitter, two height textures and a solid one"""
    sc = rtmi.Scene.new(32, 18, 1, 4)
    sc.camera((0, 1, 6), (0, 0.5, 0), (0, 1, 0), 40.0)
    h = [sc.noise_texture((0, 0, 0), (1, 1, 1), style="fbm", scale=1.5, octaves=3, seed=7),
         sc.noise_texture((0.2, 0.1, 0.0), (1, 0.5, 0.25), style="marble", scale=2.5, octaves=2, seed=9, axis="z", distortion=2.0)]
    solid = sc.solid_color((0.5, 0.5, 0.5))
    ids = [sc.lambertian(h[1]), sc.metal((0.8, 0.8, 0.8), 0.1), sc.dielectric(1.5), sc.rough_metal((0.9, 0.7, 0.4), 0.3), sc.plastic(solid, 1.5, 0.3),
           sc.diffuse_light((4.0, 4.0, 4.0))]
    for k, m in enumerate(ids):
        sc.sphere((k - 2.5, 0.5, 0.0), 0.4, m)
    return sc, h, solid, ids


def test_python_sets_gets_removes_and_refuses(rtmi):
    sc, h, solid, ids = _five(rtmi)
    assert rtmi.MATERIAL_DTYPE.itemsize == 28 == rtmi.struct_size(3) and rtmi.abi_version() == 3
    before = sc.materials().tobytes()
    assert all(sc.bump(m) is None for m in ids)
    for k, m in enumerate(ids[:5]):
        sc.set_bump(m, h[k % 2], 0.1 * (k + 1) * (-1) ** k)
        assert sc.bump(m) == (h[k % 2], float(np.float32(0.1 * (k + 1) * (-1) ** k)))
    assert sc.materials().tobytes() == before  # (a side table: the material records do not change)
    assert sc.clone().bump(ids[3]) == sc.bump(ids[3])
    nan, inf = float("nan"), float("inf")
    for call in (lambda: sc.set_bump(99, h[0], 0.2), lambda: sc.set_bump(-1, h[0], 0.2), lambda: sc.set_bump(ids[5], h[0], 0.2),
                 lambda: sc.set_bump(ids[5], -1, 0.0), lambda: sc.set_bump(ids[0], solid, 0.2), lambda: sc.set_bump(ids[0], 99, 0.2),
                 lambda: sc.set_bump(ids[0], -2, 0.2), lambda: sc.set_bump(ids[0], h[0], nan), lambda: sc.set_bump(ids[0], h[0], inf),
                 lambda: sc.set_bump(ids[0], h[0], -inf), lambda: sc.set_bump(ids[0], -1, nan), lambda: sc.bump(99), lambda: sc.bump(-1)):
        with pytest.raises(rtmi.RtmiError) as e:
            call()
        assert e.value.status == RT_ERR_ARG, str(e.value)
    assert sc.bump(ids[0]) == (h[0], float(np.float32(0.1)))  # (a refused call changes nothing)
    sc.set_bump(ids[0], -1, 0.7)
    sc.set_bump(ids[1], h[1], 0.0)
    assert sc.bump(ids[0]) is None and sc.bump(ids[1]) is None and sc.bump(ids[2]) is not None
    for name in ("rt_scene_set_bump", "rt_scene_get_bump"):
        assert name in rtmi.C_SYMBOLS


def test_the_c_entry_points(rtmi):
    lib = ctypes.CDLL(rtmi.LIB_PATH)
    sc, h, solid, ids = _five(rtmi)
    lib.rt_scene_set_bump.argtypes, lib.rt_scene_set_bump.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float], ctypes.c_int
    lib.rt_scene_get_bump.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)]
    lib.rt_scene_get_bump.restype = ctypes.c_int
    lib.rt_last_error.restype = ctypes.c_char_p
    s = sc._h
    t, k = ctypes.c_int(5), ctypes.c_float(5)
    assert lib.rt_scene_get_bump(s, ids[2], ctypes.byref(t), ctypes.byref(k)) == 0 and (t.value, k.value) == (-1, 0.0)
    assert lib.rt_scene_set_bump(s, ids[2], h[0], 0.25) == 0
    assert lib.rt_scene_get_bump(s, ids[2], ctypes.byref(t), ctypes.byref(k)) == 0 and (t.value, k.value) == (h[0], 0.25)
    assert lib.rt_scene_get_bump(s, ids[2], None, None) == 0 and lib.rt_scene_get_bump(s, ids[2], ctypes.byref(t), None) == 0
    for call in (lambda: lib.rt_scene_set_bump(None, ids[2], h[0], 0.25), lambda: lib.rt_scene_set_bump(s, len(ids), h[0], 0.25),
                 lambda: lib.rt_scene_set_bump(s, ids[5], h[0], 0.25), lambda: lib.rt_scene_set_bump(s, ids[2], solid, 0.25),
                 lambda: lib.rt_scene_set_bump(s, ids[2], h[0], float("nan")), lambda: lib.rt_scene_get_bump(None, 0, None, None),
                 lambda: lib.rt_scene_get_bump(s, len(ids), ctypes.byref(t), ctypes.byref(k))):
        assert call() == RT_ERR_ARG and lib.rt_last_error()
    assert lib.rt_scene_set_bump(s, ids[2], -1, 0.0) == 0 and sc.bump(ids[2]) is None


def test_json_reads_writes_and_refuses(rtmi):
    sc, h, solid, ids = _five(rtmi)
    for k, m in enumerate(ids[:5]):
        sc.set_bump(m, h[k % 2], 0.125 * (k + 1))
    text = sc.to_json()
    mats = json.loads(text)["material"]["data"]
    assert [m.get("bump") for m in mats] == [{"texture": h[k % 2], "strength": 0.125 * (k + 1)} for k in range(5)] + [None]
    back = rtmi.Scene.parse(text)
    assert [back.bump(m) for m in ids] == [sc.bump(m) for m in ids]
    assert back.table_image().tobytes() == sc.table_image().tobytes()
    assert back.to_json() == text

    def with_material(i, x):
        d = json.loads(text)
        d["material"]["data"][i] = x
        return json.dumps(d)
    for i in range(5):
        rtmi.Scene.parse(with_material(i, mats[i]))
    bump = {"texture": h[0], "strength": 0.2}
    bad = [(5, dict(mats[5], bump=bump))]  # a diffuse_light
    for i in range(5):
        bad += [(i, dict(mats[i], bump=dict(bump, height=1))), (i, dict(mats[i], bump={"texture": h[0]})), (i, dict(mats[i], bump={"strength": 0.2})),
                (i, dict(mats[i], bump=dict(bump, texture=solid))), (i, dict(mats[i], bump=dict(bump, texture=99))), (i, dict(mats[i], bump=dict(bump, texture=1.5))),
                (i, dict(mats[i], bump=dict(bump, strength="x"))), (i, dict(mats[i], bump=[h[0], 0.2])), (i, dict(mats[i], bump=3))]
    for k, (i, x) in enumerate(bad):
        with pytest.raises(rtmi.RtmiError) as e:
            rtmi.Scene.parse(with_material(i, x))
        assert e.value.status == RT_ERR_SCENE, (k, str(e.value))
        assert "material %d" % i in str(e.value), str(e.value)
    # strength 0 in a file: no bump
    assert rtmi.Scene.parse(with_material(0, dict(mats[0], bump={"texture": h[0], "strength": 0}))).bump(0) is None


def test_the_shipped_scene_and_the_cpp_wrapper(rtmi, tmp_path):
    sc = rtmi.Scene.load(os.path.join(PKG, "scenes", "bumpy_pond.json"))
    m = sc.materials()
    bumped = {int(m[i]["type"]): sc.bump(i) for i in range(len(m)) if sc.bump(i) is not None}
    assert set(bumped) == {R.DIELECTRIC, R.ROUGH_METAL, R.PLASTIC, R.LAMBERTIAN}
    marble = [i for i in range(len(m)) if int(m[i]["type"]) == R.LAMBERTIAN and sc.bump(i) is not None][0]
    assert sc.bump(marble)[0] == int(m[marble]["texture"]) and sc.noise(sc.bump(marble)[0])["style"] == "marble"  # colour and relief: one texture
    assert not sc.light_sampling
    sc.set_light_sampling(True)  # (the file leaves it to --nee)
    assert len(sc.lights()) == 1
    assert rtmi.Scene.parse(sc.to_json()).table_image().tobytes() == sc.table_image().tobytes()
    # include/rtmi.hpp: bumped() carries the bump through the scene's build
    src = tmp_path / "w.cpp"
    src.write_text('#include "rtmi.hpp"\n#include <cstdio>\nint main() {\n'
                   "  rtmi::scene s(16, 9, 1, 3);\n"
                   "  auto h = rtmi::noise_texture(rtmi::color(0, 0, 0), rtmi::color(1, 1, 1), RT_NOISE_STYLE_FBM, 1.5f, 3, 7u);\n"
                   "  auto glass = rtmi::dielectric(1.5f);\n"
                   "  s.add(rtmi::sphere(rtmi::point3(0, 0, 0), 1.0f, rtmi::bumped(glass, h, 0.25f)));\n"
                   "  s.add(rtmi::sphere(rtmi::point3(2, 0, 0), 1.0f, glass));\n"
                   "  s.add(rtmi::sphere(rtmi::point3(4, 0, 0), 1.0f, rtmi::bumped(rtmi::lambertian(h), h, -0.5f)));\n"
                   "  int bad = 0;\n"
                   "  try { s.add(rtmi::sphere(rtmi::point3(6, 0, 0), 1.0f, rtmi::bumped(rtmi::diffuse_light(rtmi::color(1, 1, 1)), h, 0.1f))); }\n"
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
    assert doc["material"]["data"][:3] == [{"type": "dielectric", "index_of_refraction": 1.5, "bump": {"texture": 0, "strength": 0.25}},
                                          {"type": "dielectric", "index_of_refraction": 1.5},
                                          {"type": "lambertian", "texture": 0, "bump": {"texture": 0, "strength": -0.5}}]


def test_the_packed_records(rtmi):
    """a bumped material's word 11 (c1.w) holds the offset of its bump record {offset of the noise record (bits), k, 0, 0}; the
    bump records lie in material order behind the noise records; the material's other words are those of the unbumped scene"""
    sc, h, solid, ids = _five(rtmi)
    flat = sc.table_image().reshape(-1).copy()
    strength = {ids[4]: 0.3, ids[0]: -0.2, ids[2]: 0.45}
    height = {ids[4]: h[0], ids[0]: h[1], ids[2]: h[1]}
    for m in strength:
        sc.set_bump(m, height[m], strength[m])
    w = sc.table_image().reshape(-1)
    bits, fbits = w.view(np.int32), flat.view(np.int32)
    assert w.size == flat.size + 3 * 4 and sc.table_info().image_floats == w.size
    # the material table: found by the lambertian's kind (MK_LAMBERT_NOISE = 13) and its two colours
    at = [k for k in np.flatnonzero(bits[::4] == 13) * 4 if list(w[k + 4:k + 7]) == [np.float32(0.2), np.float32(0.1), np.float32(0.0)]]
    assert len(at) == 1, at
    rec = lambda i: at[0] + 12 * (i - ids[0])
    noise_of = {h[1]: int(bits[rec(ids[0]) + 7])}  # (7o: the offset of the texture's noise record rides in c0.w)
    noise_of[h[0]] = noise_of[h[1]] - 1
    offsets = []
    for m in ids:
        r = rec(m)
        other = [j for j in range(12) if j != 11]
        assert np.array_equal(bits[r:r + 12][other], fbits[r:r + 12][other]), m
        assert fbits[r + 11] == 0
        if m in strength:
            o = int(bits[r + 11])
            offsets.append((m, o))
            assert (int(bits[4 * o]), w[4 * o + 1], int(bits[4 * o + 2]), int(bits[4 * o + 3])) == (noise_of[height[m]], np.float32(strength[m]), 0, 0), m
        else:
            assert bits[r + 11] == 0, m
    order = [o for _, o in sorted(offsets)]
    assert order == list(range(order[0], order[0] + 3)) and order[0] == noise_of[h[1]] + 1 and 4 * (order[-1] + 1) == w.size
    # every other word of the image is the unbumped scene's
    same = np.ones(flat.size, bool)
    same[[rec(m) + 11 for m in strength]] = False
    assert np.array_equal(bits[:flat.size][same], fbits[same])
    # removing them gives the unbumped bytes back
    for m in strength:
        sc.set_bump(m, -1, 0.0)
    assert sc.table_image().tobytes() == flat.tobytes()
    # alone, a bump takes a sphere-only scene to the general kernels over the wide tables
    a = rtmi.Scene.new(32, 18, 1, 4)
    a.sphere((0, 0, 0), 1.0, a.metal((0.5, 0.5, 0.5), 0.0))
    assert a.table_info().kernel_variant in (2, 6) and a.table_info().grid_wide == 0
    t = a.noise_texture((0, 0, 0), (1, 1, 1))
    a.set_bump(0, t, 0.2)
    assert a.table_info().kernel_variant in (16, 36, 44) and a.table_info().grid_wide == 1


def test_scenes_without_a_bump_pack_as_before(rtmi, scenes_dir, golden_dir, tmp_path):
    """every scene shipped before the feature and every case of smooth_pack_cases.py: the digests the parent commit wrote"""
    with open(os.path.join(golden_dir, "bump_off_pack_digests.json")) as f:
        want = json.load(f)
    cases = BS.digest_cases(rtmi, scenes_dir, str(tmp_path))
    assert set(cases) == set(want) and len(want) >= 20
    for name, build in cases.items():
        assert BS.digest(build()) == want[name], name


# ------------------------------------------------------------------------------------------------------------- 2. the gradient
@pytest.mark.parametrize("style", [N.FBM, N.TURBULENCE, N.MARBLE], ids=["fbm", "turbulence", "marble"])
def test_the_fp64_gradient_against_central_differences(style):
    """20 000 points away from the clamps, h = 1e-6: the largest difference of a prototype was 3e-9 (fbm); asserted 1e-6.  A
    central difference that straddles a kink of the scalar -- |n_o| at n_o = 0, a clamp -- is no derivative: those points are
    left out (where the scalar's two one-sided differences disagree by more than 1e-3), and they are few."""
    rng = np.random.default_rng(17 + style)
    p = rng.uniform(-4, 4, (20000, 3))
    par = dict(scale=2.3, octaves=3, seed=7, axis=1, distortion=2.0)
    val = lambda q: N.value(q, style, par["scale"], par["octaves"], par["seed"], par["axis"], par["distortion"], T)
    g = B.value_gradient(p, style, par["scale"], par["octaves"], par["seed"], par["axis"], par["distortion"], T)
    h = 1e-6
    fd, kink = np.zeros_like(g), np.zeros(len(p), bool)
    centre = val(p)
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        up, down = val(p + e), val(p - e)
        fd[:, a] = (up - down) / (2 * h)
        kink |= np.abs((up - centre) - (centre - down)) / h > 1e-3
    err = np.abs(g - fd).max(axis=1)
    print(f"\nstyle {style}: max |analytic - central difference| {err[~kink].max():.2e} on {(~kink).sum()} points ({kink.sum()} at a kink left out), "
          f"largest |grad s| {np.abs(g).max():.2f}")
    assert kink.mean() < 0.002, kink.mean()
    assert err[~kink].max() <= 1e-6, err[~kink].max()
    assert np.abs(g).max() > 1.0  # (a gradient, not zeros)


def test_the_gradient_is_zero_where_the_scalar_is_clamped():
    rng = np.random.default_rng(3)
    p = rng.uniform(-4, 4, (20000, 3))
    # turbulence over 8 octaves at a large scale reaches A >= 1 at some points; fbm does not clamp by itself (|S| < 1 needs
    # |n| near 1 in every octave), so its clamp is met through the statement's own S: points are kept where 0.5 + 0.5 S leaves (0, 1)
    for style, scale, octaves in ((N.TURBULENCE, 2.7, 8), (N.FBM, 2.7, 8)):
        s = N.value(p, style, scale, octaves, 5, 0, 0.0, T)
        g = B.value_gradient(p, style, scale, octaves, 5, 0, 0.0, T)
        clamped = (s >= 1.0) | (s <= 0.0)
        assert np.all(g[clamped] == 0.0)
        assert (np.abs(g[~clamped]).max(axis=1) > 0).mean() > 0.99
        if style == N.TURBULENCE:
            assert clamped.sum() >= 1, clamped.sum()
    # a coordinate outside (-2^30, 2^30) or a NaN: that component of the lattice noise's gradient is 0
    q = np.array([(2.0 ** 31, 0.3, 0.4), (0.3, -2.0 ** 31, 0.4), (0.3, 0.4, np.nan), (0.3, 0.4, 0.5)])
    _, dn = B.noise_gradient(q, 7, T)
    assert dn[0, 0] == 0 and dn[1, 1] == 0 and dn[2, 2] == 0 and np.all(dn[3] != 0) and np.isfinite(dn).all()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/bump_host_driver.cpp built with the host compiler; run(records [n][16] uint32) -> (grad s [n][3], n' [n][3], accepted [n])"""
    d = tmp_path_factory.mktemp("bump_driver")
    exe = str(d / "bump_host_driver")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "bump_host_driver.cpp"), "-lm"], check=True)

    def run(rec, program=exe):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(rec, np.uint32).tofile(fin)
        p = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
        out = np.fromfile(fout, np.uint32).reshape(-1, BS.OUTPUT_WORDS)
        return out[:, 0:3].view(np.float32).astype(np.float64), out[:, 3:6].view(np.float32).astype(np.float64), out[:, 6] != 0
    run.dir = d
    return run


@pytest.mark.parametrize("style", [N.FBM, N.TURBULENCE, N.MARBLE], ids=["fbm", "turbulence", "marble"])
def test_the_fp32_code_against_the_fp64_statement(driver, style):
    """Measured here, share of the 20 000 records with every component of n' within 1e-4: C++ and numpy float32
    100.000 % in every style (largest difference: fbm 1.1e-5, turbulence 5.8e-6, marble 4.4e-6)."""
    rec = BS.records(style)
    assert rec.shape == (20000, BS.RECORD_WORDS)
    G, nb, ok = driver(rec)
    G64, n64, ok64 = BS.statement(rec, np.float64)
    _, n32, _ = BS.statement(rec, np.float32)
    code, numpy32 = BS.share(nb, n64), BS.share(n32, n64)
    print(f"\nrt_noise.h on the host, style {style}: n' within 1e-4 on {100 * code:.3f} % of {len(rec)} records, max {np.abs(nb - n64).max():.2e}; "
          f"the numpy statement at float32 {100 * numpy32:.3f} %, max {np.abs(n32 - n64).max():.2e}; max |grad s - fp64| {np.abs(G - G64).max():.2e}")
    assert numpy32 >= 0.97, numpy32
    assert code >= numpy32 - 0.005, (code, numpy32)
    # the records cover both sides, both signs of k, every octave count and both outcomes of the guards
    k = rec[:, 7].view(np.float32)
    assert 0.4 < (rec[:, 14] != 0).mean() < 0.6 and k.min() < -0.45 and k.max() > 0.45
    assert set(np.unique((rec[:, 6] >> 4) & 15)) == ({1, 2, 3, 4, 5} if style == N.FBM else {1, 2})
    assert 0.02 < (~ok64).mean() < 0.5 and (ok == ok64).mean() >= 0.999
    moved = np.abs(n64 - rec[:, 8:11].view(np.float32)).max(axis=1)
    assert np.median(moved[ok64]) > 0.02
    # and a deliberate mistake of the statement is seen by the same measure
    for mistake in ("bump_full_gradient", "bump_back_unsigned", "bump_cubic_fade_derivative"):
        assert BS.share(BS.statement(rec[:2000], np.float64, (mistake,))[1], n64[:2000]) < 0.9, mistake


# --------------------------------------------------------------------------------------------------------------- 3. the model
def test_sanity_of_the_model():
    rng = np.random.default_rng(11)
    n_pts = 5000
    n = rng.normal(size=(n_pts, 3))
    n /= np.sqrt((n * n).sum(axis=1))[:, None]
    d = rng.normal(size=(n_pts, 3))
    d = np.where(((d * n).sum(axis=1) > 0)[:, None], -d, d)
    G = rng.normal(size=(n_pts, 3)) * 3
    front = rng.integers(0, 2, n_pts) != 0
    k = rng.uniform(-0.5, 0.5, n_pts).astype(np.float32)
    nb, ok = B.bump(n, n, d, front, k, G, T)
    assert np.abs(np.sqrt((nb * nb).sum(axis=1)) - 1).max() < 1e-12           # unit
    assert ((nb * n).sum(axis=1) > 0).all()                                      # never below the surface it started from
    assert ((nb * d).sum(axis=1) < 0).all() and 0.5 < ok.mean() < 1.0           # faces the ray; some were kept by the guard
    assert np.array_equal(nb[~ok], n[~ok])
    # k -> -k mirrors Gt: b - n changes sign
    Gt = G - (G * n).sum(axis=1)[:, None] * n
    sigma = np.where(front, 1.0, -1.0)
    b_plus = n - (sigma * k.astype(T))[:, None] * Gt
    b_minus = n + (sigma * k.astype(T))[:, None] * Gt
    unit = lambda a: a / np.sqrt((a * a).sum(axis=1))[:, None]
    wide = np.zeros_like(d) - n  # (a direction along -n: the guards accept every tilt below 90 degrees)
    up, _ = B.bump(n, n, wide, front, k, G, T)
    down, _ = B.bump(n, n, wide, front, -k, G, T)
    assert np.abs(up - unit(b_plus)).max() < 1e-12 and np.abs(down - unit(b_minus)).max() < 1e-12
    assert np.abs((up - (up * n).sum(axis=1)[:, None] * n) + (down - (down * n).sum(axis=1)[:, None] * n)).max() < 1e-12
    # front and back of the same surface point see the same relief: the outward normal n_out tilts the same way
    f, _ = B.bump(n, n, wide, np.ones(n_pts, bool), k, G, T)
    bk, _ = B.bump(-n, -n, -wide, np.zeros(n_pts, bool), k, G, T)
    assert np.abs(f + bk).max() < 1e-12
    # a texture whose scalar is clamped everywhere has grad s = 0 and leaves n: turbulence of 8 octaves at scale 2.7 is >= 1
    # at some of these points (the statement itself says where)
    p = rng.uniform(-4, 4, (n_pts, 3))
    s = N.value(p, N.TURBULENCE, 2.7, 8, 5, 0, 0.0, T)
    g = B.value_gradient(p, N.TURBULENCE, 2.7, 8, 5, 0, 0.0, T)
    clamped = s >= 1.0
    assert clamped.any()
    same, _ = B.bump(n[clamped], n[clamped], d[clamped], front[clamped], 0.5, g[clamped], T)
    assert np.abs(same - n[clamped]).max() < 1e-15  # (b = n, normalised once more: a rounding of the last bit)
    # a NaN gradient (marble's phase at a non-finite point) keeps n
    kept, ok = B.bump(n[:4], n[:4], d[:4], front[:4], 0.5, np.full((4, 3), np.nan), T)
    assert np.array_equal(kept, n[:4]) and not ok.any()


# ------------------------------------------------------------------------------------------------------ 4. the cases on the CPU
def test_a_case_holds_its_vertices_and_the_mistakes_change_it(rtmi):
    """bump_prims at fp64 on the CPU (the other cases: test_gpu_bump.py): the vertices it is there for, the twin's first hits,
    and every deliberate mistake moves a tenth of the samples and more"""
    name = "bump_prims"
    words, shutter = BS.inputs(rtmi, name)
    words = words[:4 * NS.REF_W * NS.REF_H]
    sc = BS.scene(rtmi, name)
    S = R.RefScene(sc)
    log = R.new_log()
    rgb, sig, draws = R.trace(S, words, log=log)
    tally = R.tally(sig, S, log)
    assert tally["bump_share"] >= BS.MIN_BUMP_SHARE and min(tally[k] for k in BS.CASES[name][3]) >= 50, tally
    assert log["bump_bumped"] >= tally["bump_vertices"]
    twin = BS.scene(rtmi, name, bump=False)
    rgb_t, sig_t, _ = R.trace(R.RefScene(twin), words)
    assert np.array_equal(sig[:, R.SAMPLE_COLUMNS + R.C_PRIM], sig_t[:, R.SAMPLE_COLUMNS + R.C_PRIM])  # (the geometry is the twin's)
    far = lambda a, b: (np.abs(a - b).max(axis=1) > 1e-4 * np.maximum(1, np.abs(b).max(axis=1))).mean()
    assert far(rgb_t, rgb) > 0.15
    off, _, _ = R.trace(S, words, perturb=("bump_off",))
    assert np.array_equal(off, rgb_t)  # (bump_off IS the twin)
    for mistake in B.PERTURBATIONS:
        wrong, _, _ = R.trace(S, words, perturb=(mistake,))
        moved = far(wrong, rgb)
        print(f"{name}, {mistake}: {100 * moved:.1f} % of the samples move")
        assert moved > 0.10, (mistake, moved)
