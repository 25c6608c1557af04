"""Anisotropic media, host side (no GPU): the interface of a medium's asymmetry g through C, C++ and Python, JSON, the
packed tables, the host evaluations of the device's phase function (csrc/rt_phase.h) against fp64, the fp64 statement
(ref64.trace with ref64_phase.py's model) against what it returned before the phase function joined its loop where every g = 0,
and the premises of the GPU comparison (test_gpu_phase.py) from the reference alone.

The tolerances of rt_phase_hg_sample, per |g|: the committed fp32 sequence measured on the CPU over the fixed inputs of
sample_inputs() (MEASURED below; DESIGN 7y has the table), asserted at 4 x the measured maximum.  The inverse's numerator
1 + g^2 - s^2 cancels as g -> 0 (s -> 1) and the quotient by 2 g amplifies what is left, so the error of cos t grows like
2^-24 / |g| towards the snap at 1e-3; at |g| = 0.99 the distribution function is steep (the density reaches 1584 per steradian),
so a cos t good to a few 1e-6 is a u1 good to a few 1e-4."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import media_nee_scenes as MN
import media_scenes as MS
import per_sample as PS
import phase_scenes as PH
import ref64 as R
import ref64_phase as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SCENE = 1, 4
G_VALUES = (1e-3, -1e-3, 0.01, -0.01, 0.1, -0.1, 0.3, -0.3, 0.5, 0.76, 0.9, -0.9, 0.95, 0.99, -0.99)
# |g| -> (max |cos t (fp32) - cos t (fp64)|, max |F_g(cos t (fp32)) - u1|) as measured on the CPU with the committed text over
# sample_inputs(); the test asserts 4 x these
MEASURED = {1e-3: (1.15e-4, 5.73e-5), 0.01: (1.12e-5, 5.52e-6), 0.1: (1.33e-6, 6.45e-7), 0.3: (7.45e-7, 5.49e-7), 0.5: (2.59e-7, 4.67e-7),
            0.76: (3.06e-7, 2.70e-6), 0.9: (2.70e-7, 1.56e-5), 0.95: (3.64e-7, 7.19e-5), 0.99: (2.73e-7, 1.57e-3)}
# unit length and the frame: a direction is three fused sums of three products of values that are each a few roundings of 2^-24
# from exact, below 1 in size: 16 x 2^-24 bounds the length's and every inner product's departure with room to spare
FRAME_TOL = 16 * 2.0 ** -24


def base(rtmi):
    return rtmi.Scene.load(os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "three_sphere.json"))


def status_of(rtmi, call):
    with pytest.raises(rtmi.RtmiError) as e:
        call()
    return e.value.status


# ---- the interface ---------------------------------------------------------------------------------------------------------
def test_symbols_and_the_abi(rtmi):
    for name in ("rt_scene_set_medium_phase", "rt_scene_get_medium_phase", "rt_phase_hg_sample", "rt_phase_hg_eval"):
        assert name in rtmi.C_SYMBOLS
    assert rtmi.abi_version() == 3 and rtmi.struct_size(17) == rtmi.MEDIUM_DTYPE.itemsize == 44


def test_range_snap_getter_clone_and_clear(rtmi):
    sc = base(rtmi)
    a = sc.add_medium_sphere((0, 0, 0), 1.0, 1.0)
    b = sc.add_medium_box((0, 0, 0), (1, 1, 1), 1.0, (0.5, 0.5, 0.5), g=-0.4)
    assert (a, b) == (0, 1) and sc.medium_phase(a) == 0.0 and sc.medium_phase(b) == np.float32(-0.4)
    for g in (0.99, -0.99, 0.5, 1e-3, -1e-3):
        sc.set_medium_phase(a, g)
        assert sc.medium_phase(a) == np.float32(g)
    for g in (5e-4, -5e-4, 9.99e-4, 0.0, -0.0):  # |g| < 1e-3 is stored as exactly +0
        sc.set_medium_phase(a, 0.5)
        sc.set_medium_phase(a, g)
        assert sc.medium_phase(a) == 0.0 and np.signbit(np.float32(sc.medium_phase(a))) == False  # noqa: E712
    sc.set_medium_phase(a, 0.7)
    for g in (0.991, -0.991, 1.0, -1.0, 2.0, float("nan"), float("inf"), -float("inf")):
        assert status_of(rtmi, lambda: sc.set_medium_phase(a, g)) == ERR_SCENE
    with pytest.raises(rtmi.RtmiError, match="g .*0.99"):
        sc.set_medium_phase(a, 1.5)
    assert sc.medium_phase(a) == np.float32(0.7)  # (a refused set changes nothing)
    for bad in (-1, 2, 16, 1 << 20):
        assert status_of(rtmi, lambda: sc.set_medium_phase(bad, 0.1)) == ERR_ARG
        assert status_of(rtmi, lambda: sc.medium_phase(bad)) == ERR_ARG
    assert status_of(rtmi, lambda: sc.add_medium_sphere((0, 0, 0), 1.0, 1.0, g=1.2)) == ERR_SCENE
    media = sc.media()
    clone = sc.clone()
    assert [clone.medium_phase(i) for i in range(len(clone.media()))] == [np.float32(0.7), np.float32(-0.4), 0.0]  # (the refused add's medium stays, isotropic)
    clone.set_medium_phase(0, -0.2)
    assert sc.medium_phase(0) == np.float32(0.7) and sc.media().tobytes() == media.tobytes()  # (rt_medium holds no g)
    sc.clear_media()
    assert len(sc.media()) == 0 and status_of(rtmi, lambda: sc.medium_phase(0)) == ERR_ARG
    assert sc.add_medium_sphere((0, 0, 0), 1.0, 1.0) == 0 and sc.medium_phase(0) == 0.0  # (cleared with the media)
    assert clone.medium_phase(0) == np.float32(-0.2)


def test_c_interface_errors(rtmi):
    lib = C.CDLL(rtmi.LIB_PATH)
    lib.rt_phase_hg_eval.restype = C.c_float
    sc = base(rtmi)
    sc.add_medium_sphere((0, 0, 0), 1.0, 1.0)
    g = C.c_float(7.0)
    assert lib.rt_scene_set_medium_phase(None, 0, C.c_float(0.5)) == ERR_ARG
    assert lib.rt_scene_get_medium_phase(None, 0, C.byref(g)) == ERR_ARG
    assert lib.rt_scene_get_medium_phase(sc._h, 0, None) == ERR_ARG
    assert lib.rt_scene_get_medium_phase(sc._h, 1, C.byref(g)) == ERR_ARG and g.value == 7.0
    assert lib.rt_scene_set_medium_phase(sc._h, 0, C.c_float(5e-4)) == 0
    assert lib.rt_scene_get_medium_phase(sc._h, 0, C.byref(g)) == 0 and g.value == 0.0
    assert lib.rt_scene_set_medium_phase(sc._h, 0, C.c_float(1.0)) == ERR_SCENE
    f3, out = (C.c_float * 3)(0, 0, 1), (C.c_float * 3)()
    assert lib.rt_phase_hg_sample(C.c_float(0.5), None, C.c_float(0.5), C.c_float(0.5), out) == ERR_ARG
    assert lib.rt_phase_hg_sample(C.c_float(0.5), f3, C.c_float(0.5), C.c_float(0.5), None) == ERR_ARG
    for bad in (0.0, 1.0, -1.0, float("nan")):
        assert lib.rt_phase_hg_sample(C.c_float(bad), f3, C.c_float(0.5), C.c_float(0.5), out) == ERR_ARG
    assert lib.rt_phase_hg_sample(C.c_float(0.5), f3, C.c_float(0.5), C.c_float(0.5), out) == 0
    assert status_of(rtmi, lambda: rtmi.phase_hg_sample(0.0, (0, 0, 1), 0.5, 0.5)) == ERR_ARG


def test_the_stored_value_decides_what_the_tables_hold(rtmi):
    """what a version bump shows on the host: the tables follow a set of a different stored value at once, and a set of the
    value already stored leaves them the bytes they were"""
    sc = MS.three_spheres(rtmi)
    sc.add_medium_sphere((0, 50, 0), 1.0, 1.0, (0.5, 0.5, 0.5))
    image0 = sc.table_image().copy()
    sc.set_medium_phase(0, 0.25)
    image1 = sc.table_image().copy()
    assert image1.tobytes() != image0.tobytes()
    sc.set_medium_phase(0, 0.25)
    assert sc.table_image().tobytes() == image1.tobytes()
    sc.set_medium_phase(0, 2e-4)
    assert sc.table_image().tobytes() == image0.tobytes()


CPP = r'''
#include <cstdio>
#include <cmath>
#include "rtmi.hpp"
int main() {
    rtmi::scene sc(64, 36, 4, 8);
    sc.add(rtmi::sphere({0, 0, -1}, 0.5f, rtmi::lambertian(rtmi::color(0.1f, 0.2f, 0.5f))));
    const int a = sc.add(rtmi::constant_medium({0, 0, -1}, 2.0f, 0.5f, rtmi::color(0.9f, 0.9f, 0.9f), 0.8f));
    const int b = sc.add(rtmi::constant_medium({-1, -1, -1}, {1, 1, 1}, 0.25f, rtmi::color(0.5f, 0.5f, 0.5f)));
    if (a != 0 || b != 1 || sc.medium_phase(a) != 0.8f || sc.medium_phase(b) != 0.0f) return 2;
    sc.set_medium_phase(b, -0.4f);
    sc.set_medium_phase(a, 5e-4f);
    if (sc.medium_phase(a) != 0.0f || sc.medium_phase(b) != -0.4f) return 3;
    int caught = 0;
    try { sc.set_medium_phase(a, 1.0f); } catch (const rtmi::error &e) { caught += 1; }
    try { sc.set_medium_phase(7, 0.1f); } catch (const rtmi::error &e) { caught += 1; }
    try { sc.medium_phase(-1); } catch (const rtmi::error &e) { caught += 1; }
    try { sc.add(rtmi::constant_medium({0, 0, 0}, 1.0f, 1.0f, rtmi::color(1, 1, 1), 1.5f)); } catch (const rtmi::error &e) { caught += 1; }
    try { rtmi::phase_hg_sample(0.0f, {0, 0, 1}, 0.5f, 0.5f); } catch (const rtmi::error &e) { caught += 1; }
    if (caught != 5) return 4;
    const rtmi::vec3 w = rtmi::phase_hg_sample(0.8f, {0, 0, 3}, 0.999f, 0.25f);
    if (std::fabs(std::sqrt(w.x() * w.x() + w.y() * w.y() + w.z() * w.z()) - 1.0f) > 1e-5f || !(w.z() > 0.9f)) return 5;
    if (std::fabs(rtmi::phase_hg_eval(0.5f, 1.0f) - 0.75f / (4.0f * 3.14159265f * 0.125f)) > 1e-5f) return 6;
    sc.clear_media();
    sc.add(rtmi::constant_medium({0, 0, -1}, 2.0f, 0.5f, rtmi::color(0.9f, 0.9f, 0.9f), -0.3f));
    fputs(sc.to_json().c_str(), stdout);
    return 0;
}
'''


def test_cpp_wrappers(rtmi, tmp_path):
    pkg = os.path.dirname(rtmi.LIB_PATH)
    src, exe = tmp_path / "t.cpp", tmp_path / "t"
    src.write_text(CPP)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", pkg, "-lrtmi", f"-Wl,-rpath,{pkg}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = rtmi.Scene.parse(r.stdout)
    assert len(got.media()) == 1 and got.medium_phase(0) == np.float32(-0.3)


# ---- JSON ------------------------------------------------------------------------------------------------------------------
def test_json_round_trip(rtmi):
    sc = base(rtmi)
    sc.add_medium_sphere((0.25, 1.5, -2), 0.75, 3.5, (0.5, 0.25, 0.125))
    sc.add_medium_box((-1, 0, -4), (1, 2.5, 0.5), 0.0625, (1, 1, 1))
    before = sc.to_json()
    assert '"g"' not in before
    sc.set_medium_phase(0, 0.0)
    sc.set_medium_phase(1, 4e-4)
    assert sc.to_json() == before  # (a scene whose media are isotropic writes the text it always wrote)
    sc.set_medium_phase(1, 0.75)
    text = sc.to_json()
    j = json.loads(text)
    assert "g" not in j["media"]["data"][0]
    assert j["media"]["data"][1] == {"type": "box", "min": [-1, 0, -4], "max": [1, 2.5, 0.5], "density": 0.0625, "albedo": [1, 1, 1], "g": 0.75}
    back = rtmi.Scene.parse(text)
    assert back.media().tobytes() == sc.media().tobytes() and back.to_json() == text
    assert (back.medium_phase(0), back.medium_phase(1)) == (0.0, 0.75)
    sc.set_medium_phase(1, -0.123456789)
    again = rtmi.Scene.parse(sc.to_json())
    assert again.medium_phase(1) == sc.medium_phase(1) == np.float32(-0.123456789)
    assert rtmi.Scene.parse(before).to_json() == before and rtmi.Scene.parse(before).medium_phase(1) == 0.0
    j["media"]["data"][0]["g"] = 5e-4
    assert rtmi.Scene.parse(json.dumps(j)).medium_phase(0) == 0.0
    for bad in (1.0, -2.0, "0.5"):
        j["media"]["data"][0]["g"] = bad
        assert status_of(rtmi, lambda: rtmi.Scene.parse(json.dumps(j))) == ERR_SCENE
    j["media"]["data"][0]["g"] = 1.5
    with pytest.raises(rtmi.RtmiError, match=r"medium 0: .*g"):
        rtmi.Scene.parse(json.dumps(j))


def test_shipped_fog_halo(rtmi):
    sc = rtmi.Scene.load(os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "fog_halo.json"))
    g = RP.stored_g(sc)
    assert len(g) == 3 and g[0] >= 0.7 and g[1] < -0.3 and g[2] > 0.5
    assert sc.table_info().kernel_variant & MS.MEDIA
    back = rtmi.Scene.parse(sc.to_json())
    assert back.media().tobytes() == sc.media().tobytes() and np.array_equal(RP.stored_g(back), g)


# ---- packing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", [MS.three_spheres, MS.mixed_scene], ids=["three spheres", "mixed"])
def test_tables(rtmi, build):
    def with_media():
        sc = build(rtmi)
        sc.add_medium_sphere((0, 50, 0), 1.0, 1.0, (0.5, 0.5, 0.5))
        sc.add_medium_box((0, 60, 0), (1, 61, 2), 0.5, (0.25, 0.5, 0.75))
        return sc
    untouched = with_media().table_image()
    sc = with_media()
    sc.set_medium_phase(0, 0.0)
    sc.set_medium_phase(1, 0.0)
    assert sc.table_image().tobytes() == untouched.tobytes()
    sc.set_medium_phase(0, 0.6)
    sc.set_medium_phase(1, 0.6)
    image, info = sc.table_image(), sc.table_info()
    a, b = untouched.reshape(-1).view(np.uint32), image.reshape(-1).view(np.uint32)
    differ = np.flatnonzero(a != b)
    off_cam = info.off_tri_hot + 5 * info.nt
    n, off = int(b.view(np.int32)[4 * (off_cam + 1) + 3]), int(b.view(np.int32)[4 * (off_cam + 2) + 3])
    assert n == 2 and list(differ) == [4 * (off + 3 * m + 2) + 3 for m in range(n)]  # .w of record 2 of each medium
    assert (a[differ] == 0).all() and (image.reshape(-1)[differ] == np.float32(0.6)).all()


# ---- rt_phase_hg_sample against fp64 ---------------------------------------------------------------------------------------
def sample_inputs():
    """the fixed inputs: (dir [n][3], k1 [n], k2 [n]) with u = k 2^-24 -- both ends of the lattice, its neighbours, and seeded
    points; unit directions (the axes and the poles of the frame among them) and directions of other lengths"""
    rng = np.random.default_rng(20240607)
    top = (1 << 24) - 1
    ends = np.array([0, 1, 2, 1 << 12, 1 << 23, top - 2, top - 1, top], np.int64)
    k1 = np.concatenate([ends, rng.integers(0, 1 << 24, 120)])
    dirs = rng.normal(size=(len(k1), 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    dirs[:6] = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0], [1e-4, 0, -1], [0.6, 0, 0.8]]
    dirs[len(k1) // 2:] *= rng.uniform(1e-3, 1e3, (len(k1) - len(k1) // 2, 1))
    k2 = np.concatenate([rng.integers(0, 1 << 24, len(k1) - len(ends)), ends])
    return dirs.astype(np.float32), k1, k2


def measure_sample(rtmi, report=False):
    """{g: dict of the maxima over sample_inputs()}: |len - 1|, the frame's departure from orthonormal, |cos t - cos t (fp64)|
    and |F_g(cos t) - u1|.  The frame is read off four samples a quarter turn of u2 apart (exact on the lattice):
    (a0 - a2) / 2 = sin t t1, (a1 - a3) / 2 = sin t t2, (a0 + a2) / 2 = cos t w."""
    dirs, k1, k2 = sample_inputs()
    w = dirs.astype(np.float64) / np.linalg.norm(dirs.astype(np.float64), axis=1)[:, None]
    u1 = k1 * 2.0 ** -24
    out = {}
    for g in G_VALUES:
        g32 = float(np.float32(g))
        a = np.array([[rtmi.phase_hg_sample(g, d, x, ((int(k) + q * (1 << 22)) % (1 << 24)) * 2.0 ** -24) for q in range(4)]
                      for d, x, k in zip(dirs, u1, k2)], np.float64)
        length = np.abs(np.linalg.norm(a, axis=2) - 1).max()
        ct = (a @ w[:, :, None])[:, :, 0]  # [n][4]: cos t of each sample, in fp64 from the fp32 output
        want = RP.hg_cos(g32, u1)
        cdf = np.abs(RP.hg_cdf(g32, np.clip(ct, -1, 1)) - u1[:, None]).max()
        # (sin t is taken from the four samples themselves: near the poles it is the root of a small difference, and a cos t
        #  that is right to 1e-7 says nothing about it)
        e1, e2, e3 = (a[:, 0] - a[:, 2]) / 2, (a[:, 1] - a[:, 3]) / 2, (a[:, 0] + a[:, 2]) / 2
        n1, n2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
        along = (e3 * w).sum(axis=1)
        frame = max(np.abs((e1 * e2).sum(axis=1)).max(), np.abs((e1 * w).sum(axis=1)).max(), np.abs((e2 * w).sum(axis=1)).max(),
                    np.abs(n1 - n2).max(), np.abs(n1 * n1 + along * along - 1).max(),
                    np.abs(e3 - along[:, None] * w).max(),
                    np.abs(np.cross(e1, e2) - (n1 * n2)[:, None] * w).max())  # (right-handed: t1 x t2 = w)
        out[g] = dict(length=length, frame=frame, cos=np.abs(ct - want[:, None]).max(), cdf=cdf)
        if report:
            print(f"g {g:+.3f}: |len - 1| {length:.2e}  frame {frame:.2e}  |d cos| {out[g]['cos']:.2e}  |F - u1| {cdf:.2e}")
    return out


def test_sample_against_fp64(rtmi):
    got = measure_sample(rtmi, report=True)
    for g, m in got.items():
        cos_max, cdf_max = MEASURED[abs(g)]
        assert m["length"] <= FRAME_TOL and m["frame"] <= FRAME_TOL, (g, m)
        assert m["cos"] <= 4 * cos_max, (g, m["cos"], cos_max)
        assert m["cdf"] <= 4 * cdf_max, (g, m["cdf"], cdf_max)


def test_sample_ends_and_direction(rtmi):
    """u1 = 0 is straight back, the last u1 of the lattice all but straight on; a non-unit direction of travel gives what its unit vector gives"""
    for g in G_VALUES:
        back = np.array(rtmi.phase_hg_sample(g, (0, 0, 2), 0.0, 0.3))
        on = np.array(rtmi.phase_hg_sample(g, (0, 0, 2), 1 - 2.0 ** -24, 0.3))
        last = float(RP.hg_cos(float(np.float32(g)), 1 - 2.0 ** -24))  # (g < 0 is flat there: 1 - 4.7e-5 at -0.99)
        assert back[2] <= -1 + 4 * MEASURED[abs(g)][0] and abs(on[2] - last) <= 4 * MEASURED[abs(g)][0] and last > 0.9999, (g, back, on, last)
    assert rtmi.phase_hg_sample(0.6, (0, 0, 1), 0.4, 0.7) == rtmi.phase_hg_sample(0.6, (0, 0, 4), 0.4, 0.7)
    # forward means along the direction of travel: the mean cosine of the samples is g
    u = (np.arange(512) + 0.5) / 512
    for g in (0.8, -0.5):
        mean = np.mean([rtmi.phase_hg_sample(g, (0.6, 0, 0.8), x, 0.1)[0] * 0.6 + rtmi.phase_hg_sample(g, (0.6, 0, 0.8), x, 0.1)[2] * 0.8 for x in u])
        assert abs(mean - g) < 1e-3, (g, mean)


# ---- rt_phase_hg_eval ------------------------------------------------------------------------------------------------------
def test_eval_against_the_closed_form_and_its_quadrature(rtmi):
    """density per steradian to relative 1e-5 on a fixed grid of cos t; and 2 pi times its Gauss-Legendre quadrature over
    cos t in [-1, 1] on 2048 fixed nodes, in fp64 from the fp32 values, is 1 within 1e-4 (the integrand's nearest singularity, at
    cos t = (1 + g^2) / (2 g), is 5e-5 outside the interval at |g| = 0.99: the rule converges like 1.01^-4096 there)"""
    x, wq = np.polynomial.legendre.leggauss(2048)
    assert abs(wq.sum() - 2) < 1e-12
    nodes = x.astype(np.float32)
    grid = np.concatenate([np.linspace(-1, 1, 257), [1 - 2.0 ** -24, -1 + 2.0 ** -24, 0.999, -0.999]]).astype(np.float32)
    assert rtmi.phase_hg_eval(0.0, 0.3) == np.float32(1 / (4 * np.pi))
    for g in G_VALUES:
        g32 = float(np.float32(g))
        got = np.array([rtmi.phase_hg_eval(g, float(c)) for c in grid], np.float64)
        want = RP.hg_density(g32, grid.astype(np.float64))
        assert np.abs(got / want - 1).max() <= 1e-5, (g, np.abs(got / want - 1).max())
        vals = np.array([rtmi.phase_hg_eval(g, float(c)) for c in nodes], np.float64)
        # (the nodes as fp32 hands them to the function: the weights are the fp64 rule's, the abscissae move by 2^-25 at most,
        #  which the integrand's slope times the weight keeps far below 1e-4 except at |g| = 0.99, where the fp64 closed form at the
        #  same fp32 nodes says what the rule gives)
        integral = 2 * np.pi * (wq * vals).sum()
        at_nodes = 2 * np.pi * (wq * RP.hg_density(g32, nodes.astype(np.float64))).sum()
        assert abs(integral - 1) <= 1e-4, (g, integral, at_nodes)


# ---- the phase step in ref64.trace: pinned where every g = 0, inert there, and the premises of the GPU comparison -------------------
@pytest.fixture(scope="module")
def words(rtmi):
    return R.uniforms(rtmi, PH.REF_SEED, PH.REF_W, PH.REF_H, 0, PH.REF_K, PH.REF_DRAWS)


@pytest.mark.parametrize("name", list(PH.ref_cases()))
def test_with_every_g_zero_the_statement_is_ref64s(rtmi, golden_dir, name):
    """... as ref64.trace stated it before the phase function joined its loop: the twins are held to golden/ref64_media_pin.npz"""
    sc = PH.isotropic_twin(PH.ref_cases()[name](rtmi))
    assert not RP.stored_g(sc).any()
    S, words, got, tally = PS.check_media_pin(rtmi, golden_dir, "twin/" + name, sc)
    assert not S.media_g.any() and tally["anisotropic_events"] == 0 and tally["isotropic_events"] == tally["medium_events"] > 0
    # and a mistake of the phase step changes nothing where no vertex takes it
    for mistake in RP.PERTURBATIONS:
        assert np.array_equal(R.trace(S, words[:3000], perturb=(mistake,))[0], got[:3000])


def test_the_phase_block_is_inert_where_every_g_is_zero(rtmi, monkeypatch):
    """on the pinned glossy-free cases, an isotropic twin and a media case with light samples whose g is 0, neither the
    Henyey-Greenstein direction nor its density is ever called"""
    from test_glossy import _existing_cases

    def never(*a, **k):
        raise AssertionError("the phase function was evaluated in a scene whose media are isotropic")
    assert R.PH is RP
    direction = RP.hg_direction
    monkeypatch.setattr(RP, "hg_direction", never)
    monkeypatch.setattr(RP, "hg_density", never)
    fog = MN.scene(rtmi, "camera inside thin fog")
    assert len(fog.lights()) and not RP.stored_g(fog).any()
    scenes = dict(_existing_cases(rtmi), twin=(PH.isotropic_twin(PH.scene(rtmi, PH.OVERLAP)), PH.REF_SEED), lit=(fog, MN.REF_SEED))
    for name, (sc, seed) in scenes.items():
        words = R.uniforms(rtmi, seed, PH.REF_W, PH.REF_H, 0, 1, PH.REF_DRAWS)
        rgb, sig, _ = R.trace(R.RefScene(sc), words)
        assert rgb.any(), name
    assert R.tally(sig)["medium_light_samples"] > 0
    with pytest.raises(AssertionError, match="phase function"):  # ... and the swap does reach the tracer: the direction
        R.trace(R.RefScene(PH.scene(rtmi, PH.OVERLAP)), words)
    monkeypatch.setattr(RP, "hg_direction", direction)
    with pytest.raises(AssertionError, match="phase function"):  # ... and, with the direction back, a light sample's density
        R.trace(R.RefScene(MN.scene(rtmi, "thin fog, g = 0.7")), words)


@pytest.mark.parametrize("name", list(PH.ref_cases()))
def test_premises_of_the_gpu_comparison(rtmi, words, name):
    assert len(words) >= 16000
    sc = PH.ref_cases()[name](rtmi)
    S = R.RefScene(sc)
    assert np.array_equal(S.media_g, RP.stored_g(sc)) and S.media_g.any()
    ref, stable, draws, tally = R.reference(S, words)
    r32, _, _ = R.trace(S, words, dtype=np.float32)
    print(f"\n{name:44s} flips {100 * (1 - stable.mean()):.3f} %   draws <= {draws.max()}   " + str({k: tally[k] for k in PH.TALLY_KEYS}))
    assert 1 - stable.mean() <= 0.01
    assert tally["anisotropic_events"] >= 200 and tally["surface_after_anisotropic"] >= 50, tally
    assert tally["media_with_events"] == list(range(len(S.media))), tally
    if name == PH.OVERLAP:
        assert tally["both_on_one_path"] >= 50 and tally["isotropic_events"] >= 200, tally
    assert draws.max() <= PH.REF_DRAWS
    assert R.judge(r32, ref, stable)["share"] >= 0.97
    for mistake in RP.PERTURBATIONS:
        wrong, _, _ = R.trace(S, words, perturb=(mistake,))
        share = R.judge(r32, wrong, stable)["share"]
        print(f"    {mistake:22s} agrees on {100 * share:.2f} %")
        assert share < 0.97, (name, mistake, share)
