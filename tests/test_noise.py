"""The noise textures (fBm, turbulence and marble over hashed-lattice gradient noise) without a GPU:
  1. the model: known answers of an independent fp64 prototype (the fp64 statement of ref64_noise.py within 1e-12, csrc/rt_noise.h
     compiled by the host compiler within 6.1e-8, the hashes exactly); zero on the lattice, continuity across lattice planes, range,
     independence of seeds;
  2. csrc/rt_noise.h on the host against the fp64 statement on 20 000 seeded records per style (criterion (b)'s form: the C++
     code's share within tolerance is at least the fp32 numpy statement's minus 0.5 points), and the same program built with
     -fsanitize=undefined,address on coordinates no scene should hold;
  3. the interface -- C, Python, C++, JSON, every argument rule, the round trip, the packed records, the table sizes -- and that a
     scene without a noise texture packs to the bytes of its twin built without the feature's entry points;
  4. the cases of noise_scenes.py: each holds the vertices it is there for, and ref64_noise's deliberate mistakes change them.
test_gpu_noise.py holds the kernels to that reference."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import nee_scenes as NS
import noise_scenes as NSC
import ref64 as R
import ref64_noise as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
RT_ERR_ARG, RT_ERR_SCENE = 1, 4
MK_LAMBERT_NOISE, MK_LIGHT_NOISE, MK_PLASTIC_NOISE = 13, 14, 15
T = np.float64

# ---------------------------------------------------------------------------------------------------------- 1. the model
POINTS = np.array([(0.5, 0.5, 0.5), (0.25, -1.75, 3.125), (-0.375, 0.625, -2.5), (10.0625, -7.1875, 0.03125), (1, 2, 3)], np.float64)
HASHES = {(0, 0, 0): 0x18c9aec4, (1, 2, 3): 0xe7962d5e, (-1, -1, -1): 0x70f00f45, (12345, -678, 9): 0xb5ad083f}
N_SEED0 = (0.125, 0.202912919834489, 0.132566929096356, -0.119920772015989, 0.0)
N_SEED7 = (0.125, -0.301615087111713, 0.209463323699310, 0.107479550989604, 0.0)
STYLED = {N.FBM: (0.481566622853279, 0.367102234406342, 0.538961298676745, 0.642366085198865, 0.3125),
          N.TURBULENCE: (0.286866754293442, 0.559384938940050, 0.229556258128168, 0.401421667783323, 0.375),
          N.MARBLE: (0.908808203396879, 0.966243735843646, 0.243200541268468, 0.942759362410101, 0.545842874245089)}
KNOWN = dict(scale=1.5, octaves=3, seed=7, axis=2, distortion=5.0)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/noise_host_driver.cpp built with the host compiler; run(records [n][8] uint32) -> (n(p, seed), s, hash) per record"""
    d = tmp_path_factory.mktemp("noise_driver")
    exe = str(d / "noise_host_driver")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "noise_host_driver.cpp"), "-lm"], check=True)

    def run(rec, program=exe):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(rec, np.uint32).tofile(fin)
        p = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
        out = np.fromfile(fout, np.uint32).reshape(-1, NSC.OUTPUT_WORDS)
        return out[:, 0].view(np.float32).astype(np.float64), out[:, 1].view(np.float32).astype(np.float64), out[:, 2].copy()
    run.dir = d
    return run


def _records(p, style=0, scale=1.0, octaves=1, seed=0, axis=0, distortion=0.0):
    p = np.asarray(p, np.float32).reshape(-1, 3)
    rec = np.zeros((len(p), NSC.RECORD_WORDS), np.uint32)
    rec[:, 0:3] = p.view(np.uint32)
    rec[:, 3], rec[:, 4] = np.float32(scale).view(np.uint32), np.float32(distortion).view(np.uint32)
    rec[:, 5], rec[:, 6] = np.uint32(seed), np.uint32(style | axis << 2 | octaves << 4)
    return rec


def test_known_answers_of_the_fp64_statement():
    for (i, j, k), h in HASHES.items():
        assert int(N.lattice_hash(i, j, k, 7)) == h, (i, j, k)
    assert np.abs(N.noise(POINTS, 0, T) - N_SEED0).max() <= 1e-12
    assert np.abs(N.noise(POINTS, 7, T) - N_SEED7).max() <= 1e-12
    for style, want in STYLED.items():
        got = N.value(POINTS, style, KNOWN["scale"], KNOWN["octaves"], KNOWN["seed"], KNOWN["axis"], KNOWN["distortion"], T)
        assert np.abs(got - want).max() <= 1e-12, (style, got)


def test_known_answers_of_the_fp32_code(driver):
    lattice = np.array(list(HASHES), np.float32)
    assert [int(h) for h in driver(_records(lattice, seed=7))[2]] == list(HASHES.values())
    assert np.abs(driver(_records(POINTS, seed=0))[0] - N_SEED0).max() <= 6.1e-8
    assert np.abs(driver(_records(POINTS, seed=7))[0] - N_SEED7).max() <= 6.1e-8
    for style, want in STYLED.items():
        s = driver(_records(POINTS, style, 1.5, 3, 7, 2, 5.0))[1]
        assert np.abs(s - want).max() <= 6.1e-8, (style, s)


def test_zero_on_the_lattice_continuous_bounded_and_seeds_independent(driver):
    rng = np.random.default_rng(1)
    lattice = rng.integers(-1000, 1000, (2000, 3)).astype(np.float64)
    assert np.all(N.noise(lattice, 5, T) == 0) and np.all(driver(_records(lattice, seed=5))[0] == 0)
    # across random integer planes: |n(p + eps) - n(p - eps)| <= slope x 2 eps.  The slope of n is bounded by the gradients' (each
    # component of a gradient is 0 or +-1: |grad . t|' <= 2) plus the fade's 1.875 times the corner values' spread (< 4): 10
    p = rng.uniform(-50, 50, (20000, 3))
    axis = rng.integers(0, 3, len(p))
    p[np.arange(len(p)), axis] = rng.integers(-50, 50, len(p))
    eps = 1e-6
    step = np.zeros_like(p)
    step[np.arange(len(p)), axis] = eps
    jump = np.abs(N.noise(p + step, 9, T) - N.noise(p - step, 9, T))
    assert jump.max() <= 10 * 2 * eps, jump.max()
    # range and mean on 200 000 points (the prototype: mean -1e-4, sd 0.27, range +-0.97)
    q = rng.uniform(-100, 100, (200000, 3))
    n = N.noise(q, 0, T)
    assert abs(n.mean()) < 0.01 and -1 < n.min() and n.max() < 1 and 0.2 < n.std() < 0.35, (n.mean(), n.std(), n.min(), n.max())
    n32 = driver(_records(q, seed=0))[0]
    assert abs(n32.mean()) < 0.01 and -1 < n32.min() and n32.max() < 1
    # two seeds: uncorrelated (200 000 independent pairs: |r| of a few 1 / sqrt(n) = 2.2e-3)
    r = np.corrcoef(n, N.noise(q, 1, T))[0, 1]
    assert abs(r) < 0.01, r
    # the marble, fbm and turbulence scalars stay in [0, 1]
    for style in (N.FBM, N.TURBULENCE, N.MARBLE):
        s = N.value(q[:20000], style, 2.5, 8, 4, 1, 7.0, T)
        assert s.min() >= 0 and s.max() <= 1


# --------------------------------------------------------------------------------------------- 2. fp32 code, fp64 statement
@pytest.mark.parametrize("style", [N.FBM, N.TURBULENCE, N.MARBLE], ids=["fbm", "turbulence", "marble"])
def test_the_fp32_code_against_the_fp64_statement(driver, style):
    """Measured here, share of the 20 000 records within 1e-4: C++ and numpy float32 100.000 % in every style."""
    rec = NSC.records(style)
    assert rec.shape == (20000, NSC.RECORD_WORDS)
    got = driver(rec)[1]
    ref, ref32 = NSC.statement(rec, np.float64), NSC.statement(rec, np.float32)
    code, numpy32 = NSC.share(got, ref), NSC.share(ref32, ref)
    print(f"\nrt_noise.h on the host, style {style}: within tolerance {100 * code:.3f} % of {len(rec)} records, max {np.abs(got - ref).max():.2e}; "
          f"the numpy statement at float32 {100 * numpy32:.3f} %, max {np.abs(ref32 - ref).max():.2e}")
    assert numpy32 >= 0.97, numpy32
    assert code >= numpy32 - 0.005, (code, numpy32)
    # the records cover the value range and every octave count
    assert ref.min() < 0.2 and ref.max() > 0.8 and set(np.unique((rec[:, 6] >> 4) & 15)) == {1, 2, 3, 4}
    # and a deliberate mistake of the statement is seen by the same measure
    assert NSC.share(NSC.statement(rec[:2000], np.float64, ("noise_cubic_fade",)), ref[:2000]) < 0.5


def test_coordinates_no_scene_should_hold_under_the_sanitizers(driver):
    """the driver built once more, a stand-alone program with -fsanitize=undefined,address: NaN, +-inf, +-1e30 and +-2^31
    coordinates report nothing and return finite values in [0, 1] (n in (-1, 1))"""
    exe = str(driver.dir / "noise_host_driver_san")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "noise_host_driver.cpp"), "-lm"], check=True)
    odd = [np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 31, -2.0 ** 31, 2.0 ** 30, -2.0 ** 30, 0.5]
    p = np.array([(a, b, c) for a in odd for b in odd for c in odd], np.float32)
    with np.errstate(all="ignore"):
        for style in (N.FBM, N.TURBULENCE, N.MARBLE):
            for axis in (0, 1, 2):
                n, s, _ = driver(_records(p, style, 3.0, 8, 0xFFFFFFFE, axis, 5.0), program=exe)
                assert np.isfinite(n).all() and np.isfinite(s).all(), style
                assert (np.abs(n) < 1).all() and s.min() >= 0 and s.max() <= 1, (style, s.min(), s.max())


# ------------------------------------------------------------------------------------------------------------ 3. interface
def _four(rtmi, noise=True):
    """a texture of every style under every material that takes one, on a sphere each"""
    sc = rtmi.Scene.new(32, 18, 1, 4)
    sc.camera((0, 1, 5), (0, 0.5, 0), (0, 1, 0), 40.0)
    tex = NSC._Tex(sc, noise)
    t = [tex((0.1, 0.2, 0.3), (0.9, 0.8, 0.7), style="fbm", scale=2.0, octaves=3, seed=7),
         tex((0.0, 0.0, 0.0), (1.0, 0.5, 0.25), style="turbulence", scale=0.5, octaves=8, seed=4294967295),
         tex((0.9, 0.9, 0.9), (0.2, 0.2, 0.3), style="marble", scale=3.0, octaves=4, seed=11, axis="z", distortion=-2.5),
         tex((1.5, 1.25, 1.0), (3.0, 2.5, 2.0), style="marble", scale=1.0, octaves=1, seed=0, axis="x", distortion=0.0)]
    ids = [sc.lambertian(t[0]), sc.lambertian(t[1]), sc.plastic(t[2], 1.5, 0.4), sc.diffuse_light(t[3])]
    for k, m in enumerate(ids):
        sc.sphere((k - 1.5, 0.5, 0.0), 0.4, m)
    return sc, t, ids


def test_constructors_tables_and_sizes(rtmi):
    sc, t, ids = _four(rtmi)
    assert rtmi.TEXTURE_DTYPE.itemsize == 28 == rtmi.struct_size(4) and rtmi.abi_version() == 3
    assert rtmi.struct_size(24) == ctypes.sizeof(rtmi.Noise) == 24

    class Mirror(ctypes.Structure):  # rt_noise, field by field
        _fields_ = [("style", ctypes.c_int32), ("octaves", ctypes.c_int32), ("seed", ctypes.c_uint32), ("axis", ctypes.c_int32),
                    ("scale", ctypes.c_float), ("distortion", ctypes.c_float)]
    assert ctypes.sizeof(Mirror) == 24
    tex = sc.textures()
    assert [int(tex[i]["type"]) for i in t] == [N.NOISE] * 4
    assert list(tex[t[0]]["c0"]) == [np.float32(0.1), np.float32(0.2), np.float32(0.3)] and list(tex[t[3]]["c1"]) == [3.0, 2.5, 2.0]
    assert sc.noise(t[0]) == dict(style="fbm", scale=2.0, octaves=3, seed=7, axis="x", distortion=0.0)  # (axis, distortion: marble's alone)
    assert sc.noise(t[1]) == dict(style="turbulence", scale=0.5, octaves=8, seed=4294967295, axis="x", distortion=0.0)
    assert sc.noise(t[2]) == dict(style="marble", scale=3.0, octaves=4, seed=11, axis="z", distortion=-2.5)
    plain = sc.solid_color((0.5, 0.5, 0.5))
    for bad in (plain, -1, 99):
        with pytest.raises(rtmi.RtmiError) as e:
            sc.noise(bad)
        assert e.value.status == RT_ERR_ARG
    # such a scene runs the general kernels over the wide tables, spheres only as it is; its emitter is no sampled light
    assert sc.table_info().kernel_variant in (16, 36, 44)
    sc.set_light_sampling(True)
    assert len(sc.lights()) == 0
    # a clone carries the parameters
    assert sc.clone().noise(t[2]) == sc.noise(t[2]) if hasattr(sc, "clone") else True


def test_the_c_entry_points_and_their_argument_rules(rtmi):
    lib = ctypes.CDLL(rtmi.LIB_PATH)
    lib.rt_scene_new.restype = ctypes.c_void_p
    lib.rt_scene_new.argtypes = [ctypes.c_int] * 4
    f3 = ctypes.c_float * 3
    fp = ctypes.POINTER(ctypes.c_float)
    lib.rt_scene_add_noise_texture.argtypes, lib.rt_scene_add_noise_texture.restype = [ctypes.c_void_p, fp, fp, ctypes.POINTER(rtmi.Noise)], ctypes.c_int
    lib.rt_scene_get_noise.argtypes, lib.rt_scene_get_noise.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(rtmi.Noise)], ctypes.c_int
    lib.rt_scene_add_plastic.argtypes, lib.rt_scene_add_plastic.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float], ctypes.c_int
    lib.rt_scene_add_lambertian.argtypes = lib.rt_scene_add_diffuse_light.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.rt_scene_free.argtypes, lib.rt_scene_free.restype = [ctypes.c_void_p], None
    lib.rt_last_error.restype = ctypes.c_char_p
    s = lib.rt_scene_new(8, 8, 1, 2)
    nan, inf = float("nan"), float("inf")
    a, b = f3(0.1, 0.2, 0.3), f3(2.0, 0.0, 1.0)
    ok = lambda **kw: rtmi.Noise(**dict(dict(style=2, octaves=3, seed=5, axis=1, scale=2.0, distortion=4.0), **kw))
    add = lambda c0, c1, n, scene=None: lib.rt_scene_add_noise_texture(s if scene is None else scene, c0, c1, ctypes.byref(n) if n is not None else None)
    try:
        assert add(a, b, ok()) == 0 and add(a, b, ok(style=0, axis=77, distortion=nan)) == 1  # (not marble: neither field is read)
        out = rtmi.Noise()
        assert lib.rt_scene_get_noise(s, 1, ctypes.byref(out)) == 0 and (out.style, out.axis, out.distortion, out.octaves) == (0, 0, 0.0, 3)
        assert lib.rt_scene_get_noise(s, 0, ctypes.byref(out)) == 0 and (out.style, out.axis, out.distortion, out.seed, out.scale) == (2, 1, 4.0, 5, 2.0)
        # every material that takes a texture takes it
        assert lib.rt_scene_add_lambertian(s, 0) == 0 and lib.rt_scene_add_plastic(s, 0, 1.5, 0.3) == 1 and lib.rt_scene_add_diffuse_light(s, 1) == 2
        bad = [lambda: add(f3(-0.1, 0.2, 0.3), b, ok()), lambda: add(a, f3(0.5, nan, 0.5), ok()), lambda: add(a, f3(0.5, inf, 0.5), ok()),
               lambda: add(None, b, ok()), lambda: add(a, None, ok()), lambda: add(a, b, None), lambda: add(a, b, ok(), scene=ctypes.c_void_p()),
               lambda: add(a, b, ok(scale=0.0)), lambda: add(a, b, ok(scale=-1.0)), lambda: add(a, b, ok(scale=nan)), lambda: add(a, b, ok(scale=inf)),
               lambda: add(a, b, ok(octaves=0)), lambda: add(a, b, ok(octaves=9)), lambda: add(a, b, ok(octaves=-3)),
               lambda: add(a, b, ok(style=3)), lambda: add(a, b, ok(style=-1)),
               lambda: add(a, b, ok(axis=3)), lambda: add(a, b, ok(axis=-1)), lambda: add(a, b, ok(distortion=nan)), lambda: add(a, b, ok(distortion=inf))]
        for k, call in enumerate(bad):
            assert call() == -RT_ERR_ARG, k
            assert lib.rt_last_error(), k
        assert lib.rt_scene_get_noise(s, 2, ctypes.byref(out)) == RT_ERR_ARG and lib.rt_scene_get_noise(s, 0, None) == RT_ERR_ARG
        assert lib.rt_scene_get_noise(None, 0, ctypes.byref(out)) == RT_ERR_ARG
    finally:
        lib.rt_scene_free(s)
    # the same rules through Python
    sc = rtmi.Scene.new(8, 8, 1, 2)
    for call in (lambda: sc.noise_texture((0.5, 0.5, 0.5), (1, 1, 1), scale=0.0), lambda: sc.noise_texture((0.5, 0.5, 0.5), (1, 1, 1), octaves=9),
                 lambda: sc.noise_texture((0.5, -0.5, 0.5), (1, 1, 1)), lambda: sc.noise_texture((0.5, 0.5, 0.5), (1, 1, 1), "marble", distortion=inf)):
        with pytest.raises(rtmi.RtmiError) as e:
            call()
        assert e.value.status == RT_ERR_ARG
    for call in (lambda: sc.noise_texture((0, 0, 0), (1, 1, 1), style="wood"), lambda: sc.noise_texture((0, 0, 0), (1, 1, 1), axis="w")):
        with pytest.raises(ValueError):
            call()
    assert sc.noise_texture((0, 0, 0), (1, 1, 1)) == 0 and sc.noise(0) == dict(style="fbm", scale=1.0, octaves=1, seed=0, axis="x", distortion=0.0)
    assert sc.noise(sc.noise_texture((0, 0, 0), (1, 1, 1), "marble")) == dict(style="marble", scale=1.0, octaves=1, seed=0, axis="y", distortion=5.0)


def test_json_reads_writes_and_refuses(rtmi):
    sc, t, ids = _four(rtmi)
    text = sc.to_json()
    texs = json.loads(text)["texture"]["data"]
    assert texs[t[0]] == {"type": "noise", "style": "fbm", "color0": [0.1, 0.2, 0.3], "color1": [0.9, 0.8, 0.7], "scale": 2, "octaves": 3, "seed": 7}
    assert texs[t[1]]["seed"] == 4294967295 and set(texs[t[1]]) == {"type", "style", "color0", "color1", "scale", "octaves", "seed"}
    assert texs[t[2]] == {"type": "noise", "style": "marble", "color0": [0.9, 0.9, 0.9], "color1": [0.2, 0.2, 0.3], "scale": 3, "octaves": 4,
                          "seed": 11, "axis": "z", "distortion": -2.5}
    back = rtmi.Scene.parse(text)
    assert back.textures().tobytes() == sc.textures().tobytes() and back.materials().tobytes() == sc.materials().tobytes()
    assert [back.noise(i) for i in t] == [sc.noise(i) for i in t]
    assert back.table_image().tobytes() == sc.table_image().tobytes()
    assert back.to_json() == text

    def with_texture(x):
        d = json.loads(text)
        d["texture"]["data"][t[0]] = x
        return json.dumps(d)
    fbm = {"type": "noise", "style": "fbm", "color0": [0.1, 0.2, 0.3], "color1": [0.9, 0.8, 0.7], "scale": 2.0, "octaves": 3, "seed": 7}
    marble = dict(fbm, style="marble", axis="y", distortion=5.0)
    rtmi.Scene.parse(with_texture(fbm))
    rtmi.Scene.parse(with_texture(marble))
    without = lambda d, k: {a: b for a, b in d.items() if a != k}
    bad = [dict(fbm, axis="y"), dict(fbm, distortion=5.0), dict(fbm, style="turbulence", axis="x"), dict(fbm, colour0=[0, 0, 0]),
           dict(fbm, style="wood"), dict(fbm, style=1), without(fbm, "style"), without(fbm, "seed"), without(fbm, "octaves"), without(fbm, "scale"),
           without(fbm, "color1"), dict(fbm, scale=0), dict(fbm, scale=-2), dict(fbm, octaves=0), dict(fbm, octaves=9), dict(fbm, octaves=2.5),
           dict(fbm, seed=-1), dict(fbm, seed=4294967296), dict(fbm, seed=1.5), dict(fbm, color0=[-0.1, 0, 0]), dict(fbm, color0=[0, 0]),
           without(marble, "axis"), without(marble, "distortion"), dict(marble, axis="w"), dict(marble, axis=1), dict(marble, axis="xy"),
           dict(marble, distortion="x"), dict(marble, frequency=2)]
    for k, x in enumerate(bad):
        with pytest.raises(rtmi.RtmiError) as e:
            rtmi.Scene.parse(with_texture(x))
        assert e.value.status == RT_ERR_SCENE, (k, str(e.value))
        assert "texture" in str(e.value), str(e.value)


def test_the_shipped_scene_and_the_cpp_wrapper(rtmi, tmp_path):
    sc = rtmi.Scene.load(os.path.join(PKG, "scenes", "marble_hall.json"))
    m, tex = sc.materials(), sc.textures()
    noisy = [i for i in range(len(tex)) if int(tex[i]["type"]) == N.NOISE]
    assert sorted(sc.noise(i)["style"] for i in noisy) == ["fbm", "fbm", "marble", "turbulence"]
    by_style = {(int(x["type"]), sc.noise(int(x["texture"]))["style"]) for x in m if int(x["texture"]) in noisy}
    assert by_style == {(R.PLASTIC, "marble"), (R.LAMBERTIAN, "turbulence"), (R.LAMBERTIAN, "fbm"), (R.DIFFUSE_LIGHT, "fbm")}
    sc.set_light_sampling(True)  # (the file leaves it to --nee)
    assert len(sc.lights()) == 1  # the solid emitter alone: the mottled panel is hit, never sampled
    # include/rtmi.hpp: the descriptor registers its texture through the C entry point
    src = tmp_path / "w.cpp"
    src.write_text('#include "rtmi.hpp"\n#include <cstdio>\nint main() {\n'
                   "  rtmi::scene s(16, 9, 1, 3);\n"
                   "  auto marble = rtmi::noise_texture(rtmi::color(0.9f, 0.9f, 0.8f), rtmi::color(0.1f, 0.2f, 0.3f), RT_NOISE_STYLE_MARBLE, 3.0f, 4, 11u, 2, 6.0f);\n"
                   "  s.add(rtmi::sphere(rtmi::point3(0, 0, 0), 1.0f, rtmi::plastic(marble, 1.4f, 0.5f)));\n"
                   "  s.add(rtmi::sphere(rtmi::point3(2, 0, 0), 1.0f, rtmi::lambertian(rtmi::noise_texture(rtmi::color(0, 0, 0), rtmi::color(1, 1, 1)))));\n"
                   "  s.add(rtmi::sphere(rtmi::point3(4, 0, 0), 1.0f, rtmi::diffuse_light(marble)));\n"
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
    assert doc["texture"]["data"] == [
        {"type": "noise", "style": "marble", "color0": [0.9, 0.9, 0.8], "color1": [0.1, 0.2, 0.3], "scale": 3, "octaves": 4, "seed": 11, "axis": "z",
         "distortion": 6},
        {"type": "noise", "style": "fbm", "color0": [0, 0, 0], "color1": [1, 1, 1], "scale": 1, "octaves": 1, "seed": 0}]  # (one marble, shared)
    assert [x["type"] for x in doc["material"]["data"]] == ["plastic", "lambertian", "diffuse_light"]


def test_the_packed_records(rtmi):
    """kind, the two colours, the offset of the noise record in c0.w and the record {scale, distortion, seed, style | axis << 2 |
    octaves << 4}, found in the packed image by the first material's colours; the records lie in texture order behind the
    material table (a scene without image textures: directly behind it)"""
    sc, t, ids = _four(rtmi)
    w = sc.table_image().reshape(-1)
    bits = w.view(np.int32)
    at = [k for k in np.flatnonzero(bits[::4] == MK_LAMBERT_NOISE) * 4
          if list(w[k + 4:k + 7]) == [np.float32(0.1), np.float32(0.2), np.float32(0.3)] and list(w[k + 8:k + 11]) == [np.float32(0.9), np.float32(0.8), np.float32(0.7)]]
    assert len(at) == 1, at
    rec = lambda i: (w[at[0] + 12 * (i - ids[0]):][:12], bits[at[0] + 12 * (i - ids[0]):][:12])
    want = [(MK_LAMBERT_NOISE, 2.0, 0.0, 7, 0 | 0 << 2 | 3 << 4), (MK_LAMBERT_NOISE, 0.5, 0.0, -1, 1 | 0 << 2 | 8 << 4),
            (MK_PLASTIC_NOISE, 3.0, -2.5, 11, 2 | 2 << 2 | 4 << 4), (MK_LIGHT_NOISE, 1.0, 0.0, 0, 2 | 0 << 2 | 1 << 4)]
    offsets = []
    for i, (kind, scale, dist, seed, packed) in zip(ids, want):
        f, b = rec(i)
        assert b[0] == kind, (i, b[0])
        offsets.append(int(b[7]))
        n = 4 * b[7]
        assert (w[n], w[n + 1], bits[n + 2], bits[n + 3]) == (np.float32(scale), np.float32(dist), seed, packed), (i, w[n:n + 2], bits[n + 2:n + 4])
        assert b[11] == 0
    assert offsets == list(range(offsets[0], offsets[0] + 4)) and 4 * offsets[0] == at[0] + 12 * len(sc.materials())
    f, b = rec(ids[2])
    r0 = ((np.float32(1.5) - np.float32(1)) / (np.float32(1.5) + np.float32(1))) ** 2
    assert f[1] == np.float32(0.4) * np.float32(0.4) and f[2] == r0 and f[3] == np.float32(0.4)  # plastic's p0..p2, untouched
    assert list(f[4:7]) == [np.float32(0.9)] * 3 and list(f[8:11]) == [np.float32(0.2), np.float32(0.2), np.float32(0.3)]
    # the spheres' cold records carry the kinds too
    kinds = sorted(int(k) for k in bits[3::4][np.isin(bits[3::4], (13, 14, 15))])
    assert kinds[:4] == [13, 13, 14, 15]


def test_a_scene_without_noise_packs_as_before(rtmi):
    """the twin of _four -- the same calls with solid colours in place of the noise textures -- packs to the bytes it packed to
    before the noise textures existed (the digest was taken from the parent commit's library), holds none of the new kinds, and
    is shorter than the noise scene by the four records"""
    import hashlib
    sc, _, _ = _four(rtmi)
    twin, _, _ = _four(rtmi, noise=False)
    assert not np.isin(twin.textures()["type"], (N.NOISE,)).any()
    image = twin.table_image()
    assert image.size == 364 and hashlib.sha256(image.tobytes()).hexdigest() == "1a4dd8d0a6724b86c3e856f847a8f47b65f8f079156adfc5823aee47fc5fecbc"
    bits = image.reshape(-1).view(np.int32)
    assert not np.isin(bits[3::4][:twin.table_info().ns], (13, 14, 15)).any()
    assert sc.table_info().image_floats == twin.table_info().image_floats + 4 * 4
    assert sc.table_info().kernel_variant == twin.table_info().kernel_variant  # (both general: the twin for its plastic)
    # and alone, a noise texture takes a sphere-only scene to the general kernels, as an image texture does
    a, b = rtmi.Scene.new(32, 18, 1, 4), rtmi.Scene.new(32, 18, 1, 4)
    a.sphere((0, 0, 0), 1.0, a.lambertian(a.noise_texture((0, 0, 0), (1, 1, 1))))
    b.sphere((0, 0, 0), 1.0, b.lambertian((0.5, 0.5, 0.5)))
    assert b.table_info().kernel_variant in (2, 6) and b.table_info().grid_wide == 0
    assert a.table_info().kernel_variant in (16, 36, 44) and a.table_info().grid_wide == 1


# ------------------------------------------------------------------------------------------------------ 4. the cases on the CPU
def test_a_case_holds_its_vertices_and_the_mistakes_change_it(rtmi):
    """noise_lights at fp64 on the CPU (the other cases: test_gpu_noise.py): the vertices it is there for, the twin's first
    hits, and every deliberate mistake moves a fifth of the samples and more"""
    name = "noise_lights"
    words, shutter = NSC.inputs(rtmi, name)
    words = words[:4 * NS.REF_W * NS.REF_H]
    sc = NSC.scene(rtmi, name)
    S = R.RefScene(sc)
    rgb, sig, draws = R.trace(S, words)
    tally = R.tally(sig, S)
    assert tally["noise_share"] >= NSC.MIN_NOISE_SHARE and min(tally[k] for k in NSC.CASES[name][3]) >= 100, tally
    twin = NSC.scene(rtmi, name, noise=False)
    rgb_t, sig_t, _ = R.trace(R.RefScene(twin), words)
    # (the geometry is the twin's: the first vertex is the same primitive; later branches may differ, plastic picks its lobe by rho)
    assert np.array_equal(sig[:, R.SAMPLE_COLUMNS + R.C_PRIM], sig_t[:, R.SAMPLE_COLUMNS + R.C_PRIM]) and (np.abs(rgb - rgb_t).max(axis=1) > 1e-4).mean() > 0.15
    for mistake in N.PERTURBATIONS:
        wrong, wsig, _ = R.trace(S, words, perturb=(mistake,))
        moved = (np.abs(wrong - rgb).max(axis=1) > 1e-4 * np.maximum(1, np.abs(rgb).max(axis=1))).mean()
        assert moved > 0.15, (mistake, moved)
