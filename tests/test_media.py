"""Homogeneous participating media, host side (no GPU): the scene interface, JSON, the packed tables, the host
evaluation of the device's interval formula against an fp64 derivation, and the C++ descriptor."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import media_scenes as MS
import ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SCENE, ERR_LIMIT = 1, 4, 6


def base(rtmi):
    return rtmi.Scene.load(os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "three_sphere.json"))


def status_of(rtmi, call):
    with pytest.raises(rtmi.RtmiError) as e:
        call()
    return e.value.status


def test_struct_and_symbols(rtmi):
    assert rtmi.struct_size(17) == rtmi.MEDIUM_DTYPE.itemsize == 44 and rtmi.struct_size(11) == 0
    for name in ("rt_scene_add_medium_sphere", "rt_scene_add_medium_box", "rt_scene_get_media", "rt_scene_clear_media", "rt_medium_interval"):
        assert name in rtmi.C_SYMBOLS
    assert rtmi.abi_version() == 3


def test_add_get_clear_clone(rtmi):
    sc = base(rtmi)
    n_prims = len(sc.prims())
    assert len(sc.media()) == 0
    assert sc.add_medium_sphere((1, 2, 3), 0.5, 2.0, (0.1, 0.2, 0.3)) == 0
    assert sc.add_medium_box((-1, -2, -3), (1, 2, 3), 0.0, (1, 1, 1)) == 1
    m = sc.media()
    assert list(m["shape"]) == [rtmi.MEDIUM_SPHERE, rtmi.MEDIUM_BOX]
    assert list(m["f"][0]) == [1, 2, 3, 0.5, 0, 0] and list(m["f"][1]) == [-1, -2, -3, 1, 2, 3]
    assert list(m["density"]) == [2.0, 0.0] and np.allclose(m["albedo"][0], (0.1, 0.2, 0.3))
    assert len(sc.prims()) == n_prims  # media are not primitives
    clone = sc.clone()
    assert clone.media().tobytes() == m.tobytes()
    sc.clear_media()
    assert len(sc.media()) == 0 and len(clone.media()) == 2


def test_argument_errors_and_the_limit(rtmi):
    sc = base(rtmi)
    lib = C.CDLL(rtmi.LIB_PATH)
    f3 = (C.c_float * 3)(0, 0, 0)
    one = (C.c_float * 3)(1, 1, 1)
    for fn, args in ((lib.rt_scene_add_medium_sphere, (None, f3, C.c_float(1), C.c_float(1), one)),
                     (lib.rt_scene_add_medium_sphere, (sc._h, None, C.c_float(1), C.c_float(1), one)),
                     (lib.rt_scene_add_medium_sphere, (sc._h, f3, C.c_float(1), C.c_float(1), None)),
                     (lib.rt_scene_add_medium_box, (sc._h, None, one, C.c_float(1), one)),
                     (lib.rt_scene_add_medium_box, (sc._h, f3, None, C.c_float(1), one)),
                     (lib.rt_scene_add_medium_box, (sc._h, f3, one, C.c_float(1), None)),
                     (lib.rt_scene_get_media, (None, None, 0))):
        assert fn(*args) == -ERR_ARG
    assert lib.rt_scene_clear_media(None) == ERR_ARG
    assert lib.rt_medium_interval(None, f3, one, C.c_float(1), None, None) == -ERR_ARG
    bad = [lambda: sc.add_medium_sphere((0, 0, 0), 1.0, -0.1), lambda: sc.add_medium_sphere((0, 0, 0), 1.0, float("nan")),
           lambda: sc.add_medium_sphere((0, 0, 0), 1.0, float("inf")), lambda: sc.add_medium_sphere((0, 0, 0), 0.0, 1.0),
           lambda: sc.add_medium_sphere((0, 0, 0), -1.0, 1.0), lambda: sc.add_medium_sphere((0, 0, 0), 1.0, 1.0, (1.1, 0.5, 0.5)),
           lambda: sc.add_medium_sphere((0, 0, 0), 1.0, 1.0, (0.5, -0.1, 0.5)), lambda: sc.add_medium_box((0, 0, 0), (1, 0, 1), 1.0),
           lambda: sc.add_medium_box((0, 0, 2), (1, 1, 1), 1.0), lambda: sc.add_medium_box((0, 0, 0), (1, 1, 1), 1.0, (0.5, 0.5, float("nan")))]
    for call in bad:
        assert status_of(rtmi, call) == ERR_SCENE
    assert len(sc.media()) == 0
    for i in range(16):
        assert sc.add_medium_sphere((i, 0, 0), 1.0, 0.1) == i
    assert status_of(rtmi, lambda: sc.add_medium_sphere((0, 0, 0), 1.0, 0.1)) == ERR_LIMIT
    assert status_of(rtmi, lambda: sc.add_medium_box((0, 0, 0), (1, 1, 1), 0.1)) == ERR_LIMIT
    assert len(sc.media()) == 16


def test_json_round_trip(rtmi):
    sc = base(rtmi)
    sc.add_medium_sphere((0.25, 1.5, -2), 0.75, 3.5, (0.5, 0.25, 0.125))
    sc.add_medium_box((-1, 0, -4), (1, 2.5, 0.5), 0.0625, (1, 1, 1))
    text = sc.to_json()
    j = json.loads(text)
    assert j["media"]["data"][0] == {"type": "sphere", "center": [0.25, 1.5, -2], "radius": 0.75, "density": 3.5, "albedo": [0.5, 0.25, 0.125]}
    assert j["media"]["data"][1] == {"type": "box", "min": [-1, 0, -4], "max": [1, 2.5, 0.5], "density": 0.0625, "albedo": [1, 1, 1]}
    back = rtmi.Scene.parse(text)
    assert back.media().tobytes() == sc.media().tobytes() and back.to_json() == text
    assert "media" not in json.loads(base(rtmi).to_json())
    j["media"]["data"][0]["type"] = "cone"
    assert status_of(rtmi, lambda: rtmi.Scene.parse(json.dumps(j))) == ERR_SCENE
    j["media"]["data"][0] = {"type": "sphere", "center": [0, 0, 0], "radius": 1, "density": -1, "albedo": [1, 1, 1]}
    assert status_of(rtmi, lambda: rtmi.Scene.parse(json.dumps(j))) == ERR_SCENE
    j["media"]["data"] = [{"type": "box", "min": [0, 0, 0], "max": [1, 1, 1], "density": 1, "albedo": [1, 1, 1]}] * 17
    with pytest.raises(rtmi.RtmiError, match="at most 16 media"):  # (a parse that fails returns no scene: the message says why)
        rtmi.Scene.parse(json.dumps(j))


def test_shipped_fog_room(rtmi):
    sc = rtmi.Scene.load(os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "fog_room.json"))
    m = sc.media()
    assert len(m) == 3 and list(m["shape"]) == [rtmi.MEDIUM_BOX, rtmi.MEDIUM_SPHERE, rtmi.MEDIUM_SPHERE]
    assert sc.table_info().kernel_variant & MS.MEDIA
    assert rtmi.Scene.parse(sc.to_json()).media().tobytes() == m.tobytes()


@pytest.mark.parametrize("build", [MS.three_spheres, MS.mixed_scene], ids=["three spheres", "mixed"])
def test_tables(rtmi, build):
    sc = build(rtmi)
    info0, image0 = sc.table_info(), sc.table_image().copy()
    assert info0.kernel_variant & MS.MEDIA == 0
    sc.clear_media()  # (nothing to clear: the scene stays the scene it was)
    assert sc.table_image().tobytes() == image0.tobytes()
    sc.add_medium_sphere((0, 50, 0), 1.0, 1.0, (0.5, 0.5, 0.5))
    sc.add_medium_box((0, 60, 0), (1, 61, 2), 0.5, (0.25, 0.5, 0.75))
    info, image = sc.table_info(), sc.table_image()
    assert info.kernel_variant & MS.MEDIA and info.kernel_variant & 255 in (16, 36, 44) and info.grid_wide == 1
    # the MEDIA part: the last 2 x 3 records of the image; the camera block says how many and where
    w = image.reshape(-1)
    off_cam = info.off_tri_hot + 5 * info.nt
    n, off = w.view(np.int32)[4 * (off_cam + 1) + 3], w.view(np.int32)[4 * (off_cam + 2) + 3]
    assert n == 2 and 4 * (off + 3 * n) == w.size
    rec = w[4 * off:].reshape(2, 12)
    assert list(rec[0][:8]) == [0, 50, 0, 1, 0.5, 0.5, 0.5, 1.0] and rec[0].view(np.int32)[10] == 0
    assert list(rec[1][:10]) == [0, 60, 0, 1, 0.25, 0.5, 0.75, 0.5, 61, 2] and rec[1].view(np.int32)[10] == 1
    # the primitive counts stay; cleared, the scene packs to the bytes it had
    assert (info.ns, info.nr, info.nc, info.nt) == (info0.ns, info0.nr, info0.nc, info0.nt)
    sc.clear_media()
    assert sc.table_image().tobytes() == image0.tobytes() and sc.table_info().kernel_variant == info0.kernel_variant


def test_json_errors_name_the_medium(rtmi):
    j = json.loads(base(rtmi).to_json())
    ok = {"type": "box", "min": [0, 0, 0], "max": [1, 1, 1], "density": 1, "albedo": [1, 1, 1]}
    j["media"] = {"data": [ok, dict(ok, density=-2)]}
    with pytest.raises(rtmi.RtmiError, match=r"medium 1: .*density"):
        rtmi.Scene.parse(json.dumps(j))
    j["media"] = {"data": [dict(ok, max=[1, 0, 1])]}
    with pytest.raises(rtmi.RtmiError, match=r"medium 0: .*min"):
        rtmi.Scene.parse(json.dumps(j))


def test_interval_refuses_an_unknown_shape(rtmi):
    rec = np.zeros(1, rtmi.MEDIUM_DTYPE)[0]
    rec["shape"], rec["f"] = 2, [-1, -1, -1, 1, 1, 1]
    assert status_of(rtmi, lambda: rtmi.medium_interval(rec, (0, 0, -5), (0, 0, 1))) == ERR_ARG


def test_buried_media_are_unreachable(rtmi):
    """the premise of the GPU pin test (test_gpu_media.py, 1), held on the scenes as they are built"""
    sc = MS.mixed_scene(rtmi)
    MS.bury_medium_mixed(sc)
    MS.check_buried_mixed(rtmi, sc)
    sc = MS.three_spheres(rtmi)
    MS.bury_medium_three_spheres(sc)
    MS.check_buried_three_spheres(rtmi, sc)


def test_reference_branch_flip_rate_of_every_case(rtmi):
    """ref64 alone, no kernel: on every case of the per-sample GPU comparison the share of samples whose event signature
    differs between the reference's fp32 and fp64 runs is at most 1 %, the reference stays inside the draws it requested, medium
    events occur (some on paths with later surface vertices), and leaving the free-flight draw out is noticed"""
    words = R.uniforms(rtmi, MS.REF_SEED, MS.REF_W, MS.REF_H, 0, MS.REF_K, MS.REF_DRAWS)
    print()
    for name, build in MS.ref_cases().items():
        sc = build(rtmi)
        S = R.RefScene(sc)
        r64, sig64, draws = R.trace(S, words)
        r32, sig32, _ = R.trace(S, words, dtype=np.float32)
        stable = R.same_signature(sig64, sig32)
        flips, tally = 1 - stable.mean(), {k: v for k, v in R.tally(sig64).items() if k in R.MEDIA_KEYS}
        j = R.judge(r32, r64, stable)
        print(f"{name:32s} flips {100 * flips:.3f} %   fp32 within {100 * j['share']:.3f} %   draws <= {draws.max()}   {tally}")
        assert flips <= 0.01 and j["share"] >= 0.97, (name, flips, j["share"])
        assert draws.max() <= MS.REF_DRAWS
        assert tally["medium_events"] > 0 and tally["medium_then_surface"] >= 1
        assert tally["media_with_events"] == list(range(len(sc.media())))
    S = R.RefScene(MS.ref_cases()["camera inside thin fog"](rtmi))
    r32, sig32, _ = R.trace(S, words, dtype=np.float32)
    r64, sig64, _ = R.trace(S, words)
    wrong, _, _ = R.trace(S, words, perturb=("skip_flight",))
    assert R.judge(r32, wrong, R.same_signature(sig64, sig32))["share"] < 0.97
    # without media the statement is the plain integrator's: the media=False view is the scene with its media cleared
    sc = MS.ref_cases()["dense sphere"](rtmi)
    a, _, da = R.trace(R.RefScene(sc, media=False), words[:4000])
    sc.clear_media()
    b, sig, db = R.trace(R.RefScene(sc), words[:4000])
    assert np.array_equal(a, b) and np.array_equal(da, db) and R.tally(sig)["medium_events"] == 0


# ---- rt_medium_interval against an fp64 derivation --------------------------------------------------------------------
def _interval64(m, o, d, t_max):
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    f = m["f"].astype(np.float64)
    if m["shape"] == 0:
        oc = o - f[:3]
        A, hb, cc = d @ d, oc @ d, oc @ oc - f[3] ** 2
        disc = hb * hb - A * cc
        if disc <= 0:
            return None, disc / max(hb * hb, A * abs(cc), 1e-300)
        a, b = (-hb - np.sqrt(disc)) / A, (-hb + np.sqrt(disc)) / A
        margin = disc / max(hb * hb, A * abs(cc), 1e-300)
    else:
        a, b = -np.inf, np.inf
        for k in range(3):
            if d[k] == 0:
                if not (f[k] < o[k] < f[3 + k]):
                    return None, (0.0 if o[k] in (f[k], f[3 + k]) else 1.0)
                continue
            t0, t1 = (f[k] - o[k]) / d[k], (f[3 + k] - o[k]) / d[k]
            a, b = max(a, min(t0, t1)), min(b, max(t0, t1))
        margin = 1.0
    a, b = max(a, 0.001), min(b, t_max)
    return ((a, b) if a < b else None), margin * (abs(b - a) / max(abs(a), abs(b), 1e-300) if np.isfinite(b) else 1.0)


@pytest.mark.parametrize("shape", ["sphere", "box"])
def test_interval_against_fp64(rtmi, shape):
    """hit or miss and both ends, on random rays: origins outside and inside, rays aimed at the rim (tangent), and for the box
    axis-parallel rays.  A verdict is only compared where the fp64 derivation is not itself on the fence (a relative margin of
    1e-4 in the discriminant or in the interval's length); the ends within 2e-5 relative + 1e-5 absolute of fp32 inputs."""
    rng = np.random.default_rng(11 if shape == "sphere" else 12)
    rec = np.zeros(1, rtmi.MEDIUM_DTYPE)[0]
    checked = hits = inside = parallel = 0
    for i in range(4000):
        c = rng.uniform(-3, 3, 3).astype(np.float32)
        if shape == "sphere":
            r = np.float32(rng.uniform(0.2, 2.0))
            rec["shape"], rec["f"] = 0, [c[0], c[1], c[2], r, 0, 0]
            half = np.array([r, r, r])
        else:
            half = rng.uniform(0.2, 2.0, 3).astype(np.float32)
            rec["shape"], rec["f"] = 1, list(c - half) + list(c + half)
        mode = i % 4
        if mode == 0:    # an origin inside
            o = c + rng.uniform(-0.5, 0.5, 3) * half * (0.57 if shape == "sphere" else 1.0)
            d = rng.normal(size=3)
        elif mode == 1:  # aimed at the rim: tangent rays and corner grazes
            o = c + rng.normal(size=3) * 6
            rim = rng.normal(size=3)
            rim = rim / np.linalg.norm(rim) * half if shape == "sphere" else np.sign(rim) * half
            d = (c + rim * rng.uniform(0.98, 1.02)) - o
        elif mode == 2 and shape == "box":  # axis-parallel
            o = c + rng.uniform(-1.5, 1.5, 3) * half
            d = np.zeros(3)
            d[rng.integers(3)] = rng.choice([-1.0, 1.0]) * rng.uniform(0.1, 3)
            if rng.integers(2):
                d[rng.integers(3)] = rng.uniform(-2, 2)
            parallel += 1
        else:
            o = c + rng.normal(size=3) * 5
            d = (c + rng.uniform(-1.2, 1.2, 3) * half) - o
        d = d * rng.uniform(0.2, 4)  # (directions are not normalised)
        o, d = o.astype(np.float32), d.astype(np.float32)
        t_max = float(np.float32(rng.choice([np.inf, rng.uniform(0.1, 3)])))
        hit, a, b = rtmi.medium_interval(rec, o, d, t_max)
        want, margin = _interval64(rec, o, d, t_max)
        if abs(margin) < 1e-4:
            continue
        checked += 1
        assert hit == (want is not None), (i, shape, o, d, t_max, (hit, a, b), want)
        if hit:
            hits += 1
            inside += a == np.float32(0.001)
            for got, ref in ((a, want[0]), (b, want[1])):
                assert abs(got - ref) <= 2e-5 * abs(ref) + 1e-5, (i, shape, o, d, (a, b), want)
    assert checked > 3000 and hits > 1000 and inside > 500 and checked - hits > 300, (checked, hits, inside)
    assert shape == "sphere" or parallel > 500


def test_interval_special_rays(rtmi):
    box = np.zeros(1, rtmi.MEDIUM_DTYPE)[0]
    box["shape"], box["f"] = 1, [-1, -1, -1, 1, 1, 1]
    assert rtmi.medium_interval(box, (0, 0, -5), (0, 0, 1)) == (True, 4.0, 6.0)
    assert rtmi.medium_interval(box, (0, 0, -5), (0, 0, 2), 2.5) == (True, 2.0, 2.5)
    assert rtmi.medium_interval(box, (0, 2, -5), (0, 0, 1))[0] is False       # parallel, outside the slab
    assert rtmi.medium_interval(box, (0, 0, -5), (-0.0, 0.0, 1))[0] is True   # signed zeros
    assert rtmi.medium_interval(box, (0, 0, 0), (0, 0, -1), 0.5) == (True, np.float32(0.001), 0.5)
    assert rtmi.medium_interval(box, (0, 0, 5), (0, 0, 1))[0] is False        # behind the origin
    ball = np.zeros(1, rtmi.MEDIUM_DTYPE)[0]
    ball["shape"], ball["f"] = 0, [0, 0, 0, 1, 0, 0]
    assert rtmi.medium_interval(ball, (0, 0, -3), (0, 0, 1)) == (True, 2.0, 4.0)
    assert rtmi.medium_interval(ball, (0, 0, -3), (0, 0, 1), 1.5)[0] is False  # the surface hit comes first
    assert rtmi.medium_interval(ball, (0, 1, -3), (0, 0, 1))[0] is False       # tangent: disc = 0 is no interval
    assert rtmi.medium_interval(ball, (0, 0, 0), (0, 0, 0.5)) == (True, np.float32(0.001), 2.0)


# ---- the C++ descriptor ------------------------------------------------------------------------------------------------
CPP = r'''
#include <cstdio>
#include "rtmi.hpp"
int main() {
    rtmi::scene sc(64, 36, 4, 8);
    sc.add(rtmi::sphere({0, 0, -1}, 0.5f, rtmi::lambertian(rtmi::color(0.1f, 0.2f, 0.5f))));
    const int a = sc.add(rtmi::constant_medium(rtmi::point3(0, 1, -1), 0.75f, 2.0f, rtmi::color(0.5f, 0.5f, 0.5f)));
    const int b = sc.add(rtmi::constant_medium(rtmi::point3(-4, 0, -4), rtmi::point3(4, 3, 4), 0.125f, rtmi::color(1, 1, 1)));
    if (a != 0 || b != 1 || sc.media().size() != 2) return 2;
    fputs(sc.to_json().c_str(), stdout);
    try { sc.add(rtmi::constant_medium(rtmi::point3(0, 0, 0), -1.0f, 1.0f, rtmi::color(1, 1, 1))); } catch (const rtmi::error &e) { fprintf(stderr, "caught: %s\n", e.what()); return 0; }
    return 1;
}
'''


def test_cpp_constant_medium(rtmi, tmp_path):
    pkg = os.path.dirname(rtmi.LIB_PATH)
    src, exe = tmp_path / "m.cpp", tmp_path / "m"
    src.write_text(CPP)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", pkg, "-lrtmi", f"-Wl,-rpath,{pkg}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "radius" in r.stderr, (r.returncode, r.stderr)
    m = rtmi.Scene.parse(r.stdout).media()
    assert list(m["shape"]) == [0, 1] and list(m["f"][0][:4]) == [0, 1, -1, 0.75] and list(m["f"][1]) == [-4, 0, -4, 4, 3, 4]
    assert list(m["density"]) == [2.0, 0.125]
