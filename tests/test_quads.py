"""Quads and boxes without a GPU: the constructors through C / Python, C++ and JSON with their argument rules, the
record words, a box's outward normals, rotate-then-translate against the fp64 matrix, the JSON round trip, the light list and
its records; ref64's quads pinned to its rectangles on axis-aligned scenes; csrc/rt_quad.h on the host against the
fp64 statement on random rays (test_primitives_fuzz.py's tolerances and its rule for rays near an edge or near grazing); the
light's density integrated over the quad's solid angle; the per-sample cases' fp32 NumPy reference; the shipped scene."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import nee_scenes as NS
import quad_scenes as Q
import ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
RT_ERR_ARG, RT_ERR_SCENE = 1, 4


def _scene(rtmi):
    sc = rtmi.Scene.new(16, 9, 1, 4)
    sc.camera((0, 1, 5), (0, 0, 0), (0, 1, 0), 40.0)
    return sc, sc.lambertian((0.5, 0.5, 0.5))


def _derived(Q3, u, v):
    """(n, A, B) in fp64 from the fp32 Q, u, v, rounded once"""
    u, v = np.asarray(u, np.float32).astype(np.float64), np.asarray(v, np.float32).astype(np.float64)
    c = np.cross(u, v)
    w = c / (c @ c)
    return (c / np.sqrt(c @ c)).astype(np.float32), np.cross(v, w).astype(np.float32), np.cross(w, u).astype(np.float32)


def _rodrigues(axis, deg):
    """the cylinder's rotation (vec3.cuh:396-418), element by element in fp64 with libm's sin and cos, from the fp32 axis and
    angle the C interface takes"""
    a = [float(np.float32(x)) for x in axis]
    deg = float(np.float32(deg))
    ln = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    a = [x / ln for x in a]
    th = deg / 180.0 * math.acos(-1.0)
    sn, cs = math.sin(th), math.cos(th)
    return [[a[0] * a[0] + (1 - a[0] * a[0]) * cs, a[0] * a[1] * (1 - cs) - a[2] * sn, a[0] * a[2] * (1 - cs) + a[1] * sn],
            [a[0] * a[1] * (1 - cs) + a[2] * sn, a[1] * a[1] + (1 - a[1] * a[1]) * cs, a[1] * a[2] * (1 - cs) - a[0] * sn],
            [a[0] * a[2] * (1 - cs) - a[1] * sn, a[1] * a[2] * (1 - cs) + a[0] * sn, a[2] * a[2] + (1 - a[2] * a[2]) * cs]]


def _apply(Rm, t, x):
    x = [float(np.float32(c)) for c in x]
    return np.array([Rm[i][0] * x[0] + Rm[i][1] * x[1] + Rm[i][2] * x[2] + t[i] for i in range(3)], np.float64).astype(np.float32)


# ---------------------------------------------------------------------------------------------- constructors and packing
def test_quad_record_words(rtmi):
    sc, m = _scene(rtmi)
    q, u, v = (0.3, -0.2, 0.7), (1.5, 0.2, -0.4), (-0.3, 1.1, 0.25)
    i = sc.quad(q, u, v, m)
    p = sc.prims()[i]
    assert p["type"] == rtmi.PRIM_QUAD == 6 and p["material"] == m
    assert np.array_equal(p["m"][0:9], np.array(q + u + v, np.float32))
    n, A, B = _derived(q, u, v)
    assert np.array_equal(p["m"][9:12], n) and np.array_equal(p["m_inv"][0:3], A) and np.array_equal(p["m_inv"][3:6], B)
    assert not p["f"].any() and not p["m_inv"][6:].any()
    # A and B turn p - Q into the quad's coordinates
    for a, b in ((0, 0), (1, 0), (0.25, 0.75), (1, 1)):
        r = a * np.array(u) + b * np.array(v)
        assert abs(A.astype(np.float64) @ r - a) < 1e-6 and abs(B.astype(np.float64) @ r - b) < 1e-6
    assert rtmi.abi_version() == 3 and sc.prims().dtype.itemsize == 128


def test_argument_rules(rtmi):
    sc, m = _scene(rtmi)
    bad = [lambda: sc.quad((0, 0, 0), (1, 0, 0), (2, 0, 0), m),              # parallel edges: |c|^2 = 0
           lambda: sc.quad((0, 0, 0), (0, 0, 0), (0, 1, 0), m),
           lambda: sc.quad((0, 0, 0), (1e-30, 0, 0), (0, 1e-30, 0), m),      # |c|^2 underflows to a denormal: 1 / |c| is not finite in fp32
           lambda: sc.quad((0, 0, 0), (1e30, 0, 0), (0, 1e30, 0), m),        # |c| beyond fp32
           lambda: sc.quad((float("nan"), 0, 0), (1, 0, 0), (0, 1, 0), m),
           lambda: sc.quad((0, 0, 0), (float("inf"), 0, 0), (0, 1, 0), m),
           lambda: sc.quad((0, 0, 0), (1, 0, 0), (0, 1, 0), m, rotate=((0, 0, 0), 30.0)),
           lambda: sc.quad((0, 0, 0), (1, 0, 0), (0, 1, 0), m, translate=(float("nan"), 0, 0)),
           lambda: sc.quad((0, 0, 0), (1, 0, 0), (0, 1, 0), 99),
           lambda: sc.box((0, 0, 0), (1, 1, 0), m),                             # min < max on every axis
           lambda: sc.box((0, 0, 0), (1, -1, 1), m),
           lambda: sc.box((0, 0, 0), (1, float("nan"), 1), m),
           lambda: sc.box((0, 0, 0), (1, 1, 1), m, rotate=((0, 0, 0), 1.0)),
           lambda: sc.box((0, 0, 0), (1, 1, 1), 99)]
    for call in bad:
        with pytest.raises(rtmi.RtmiError) as e:
            call()
        assert e.value.status == RT_ERR_SCENE, str(e.value)
    assert len(sc.prims()) == 0  # a refused box leaves none of its faces
    assert sc.box((0, 0, 0), (1, 1, 1), m) == 0 and sc.quad((0, 0, 0), (1, 0, 0), (0, 1, 0), m) == 6 and sc.box((0, 0, 0), (1, 2, 3), m) == 7
    assert len(sc.prims()) == 13


def test_box_faces_point_outward(rtmi):
    for rotate, translate in ((None, None), (((1, 2, 3), 37.0), (-0.4, 0.5, 0.1)), (((0, 1, 0), -120.0), None), (None, (3, 2, 1))):
        sc, m = _scene(rtmi)
        first = sc.box((-0.5, 0.1, 0.2), (0.7, 0.9, 1.6), m, rotate, translate)
        P = sc.prims()[first:first + 6].copy()
        assert (P["type"] == rtmi.PRIM_QUAD).all()
        M = P["m"].astype(np.float64)
        centre = (M[:, 0:3] + 0.5 * M[:, 3:6] + 0.5 * M[:, 6:9])
        box_centre = centre.mean(axis=0)
        out = ((centre - box_centre) * M[:, 9:12]).sum(axis=1)
        assert (out > 0.3).all(), out
        # u x v along the stored normal, six distinct directions, the faces close the box
        assert (np.einsum("ij,ij->i", np.cross(M[:, 3:6], M[:, 6:9]), M[:, 9:12]) > 0).all()
        assert np.allclose(M[:, 9:12].sum(axis=0), 0, atol=1e-6)
        if rotate is None and translate is None:
            assert np.array_equal(M[:, 9:12], np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], float))


@pytest.mark.parametrize("axis,deg,off", [((0, 1, 0), 15.0, (265, 0.5, 295)), ((1, 2, 3), 37.0, (-0.4, 0.5, 0.1)), ((0.1, 1, 0.05), 41.0, None),
                                          (None, 0.0, (0.25, -3.0, 7.5))])
def test_rotate_then_translate_is_the_fp64_matrix_rounded_once(rtmi, axis, deg, off):
    sc, m = _scene(rtmi)
    q, u, v = (0.3, -0.2, 0.7), (1.5, 0.2, -0.4), (-0.3, 1.1, 0.25)
    sc.quad(q, u, v, m, (axis, deg) if axis else None, off)
    first = sc.box((-0.5, 0.1, 0.2), (0.7, 0.9, 1.6), m, (axis, deg) if axis else None, off)
    Rm = _rodrigues(axis, deg) if axis else [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]
    t = [float(np.float32(x)) for x in off] if off else [0.0, 0.0, 0.0]  # (the C interface takes fp32)
    P = sc.prims()
    want = np.concatenate([_apply(Rm, t, q), _apply(Rm, [0, 0, 0], u), _apply(Rm, [0, 0, 0], v)])
    assert np.array_equal(P[0]["m"][0:9], want), (P[0]["m"][0:9], want)
    n, A, B = _derived(want[0:3], want[3:6], want[6:9])
    assert np.array_equal(P[0]["m"][9:12], n) and np.array_equal(P[0]["m_inv"][0:6], np.concatenate([A, B]))
    # the box's +x face: Q = (x1, y0, z0), u = (0, dy, 0), v = (0, 0, dz), the extents fp64 differences of the fp32 bounds
    lo, hi = np.array((-0.5, 0.1, 0.2), np.float32).astype(np.float64), np.array((0.7, 0.9, 1.6), np.float32).astype(np.float64)
    d = hi - lo
    f = P[first + 2]["m"]
    ap = lambda x, tt: np.array([Rm[i][0] * x[0] + Rm[i][1] * x[1] + Rm[i][2] * x[2] + tt[i] for i in range(3)]).astype(np.float32)
    assert np.array_equal(f[0:3], ap([hi[0], lo[1], lo[2]], t)) and np.array_equal(f[3:6], ap([0.0, d[1], 0.0], [0, 0, 0])) \
        and np.array_equal(f[6:9], ap([0.0, 0.0, d[2]], [0, 0, 0]))


SCENE_JSON = {
    "width": 32, "height": 18, "samples_per_pixel": 1, "max_depth": 4, "background": [0.1, 0.1, 0.1],
    "camera": {"lookfrom": [0, 1, 5], "lookat": [0, 0, 0], "vup": [0, 1, 0], "vfov": 40, "aperture": 0},
    "object": {"data": []},
    "material": {"data": [{"type": "lambertian", "texture": 0}, {"type": "diffuse_light", "texture": 1}]},
    "texture": {"data": [{"type": "solid_color", "color": [0.5, 0.5, 0.5]}, {"type": "checker", "even": [4, 3, 2], "odd": [1, 2, 3]}]},
}


def _parse(rtmi, objects):
    return rtmi.Scene.parse(json.dumps(dict(SCENE_JSON, object={"data": objects})))


def test_json_in_out_and_the_round_trip(rtmi):
    quad = {"type": "quad", "q": [0.3, -0.2, 0.7], "u": [1.5, 0.2, -0.4], "v": [-0.3, 1.1, 0.25], "material": 0}
    box = {"type": "box", "min": [-0.5, 0.1, 0.2], "max": [0.7, 0.9, 1.6], "material": 0}
    turn = {"rotate": {"axis": [1, 2, 3], "angle": 37}, "translate": [-0.375, 0.5, 0.125]}  # (fp32 values: JSON carries doubles)
    light = {"type": "quad", "q": [-1, 3, -1], "u": [2, 0, 0], "v": [0, 0, 2], "material": 1}
    sc = _parse(rtmi, [quad, dict(quad, **turn), box, dict(box, **turn), light])
    P = sc.prims()
    assert len(P) == 15 and (P["type"] == rtmi.PRIM_QUAD).all()
    # the same scene through the Python constructors
    py, m = _scene(rtmi)
    py.quad(quad["q"], quad["u"], quad["v"], m)
    py.quad(quad["q"], quad["u"], quad["v"], m, ((1, 2, 3), 37.0), (-0.375, 0.5, 0.125))
    py.box(box["min"], box["max"], m)
    py.box(box["min"], box["max"], m, ((1, 2, 3), 37.0), (-0.375, 0.5, 0.125))
    assert P[:14].tobytes() == py.prims().tobytes()
    # the writer emits quads: a box comes back as six, a turned quad as the quad it became, and packs to the same bytes
    text = sc.to_json()
    objs = json.loads(text)["object"]["data"]
    assert [o["type"] for o in objs] == ["quad"] * 15 and all(set(o) == {"type", "q", "u", "v", "material"} for o in objs)
    back = rtmi.Scene.parse(text)
    assert back.prims().tobytes() == P.tobytes()
    for on in (False, True):
        sc.set_light_sampling(on), back.set_light_sampling(on)
        assert np.array_equal(back.table_image().view(np.uint32), sc.table_image().view(np.uint32))
    assert back.to_json() == rtmi.Scene.parse(back.to_json()).to_json()
    # a field the type does not have, a missing one, a bad transform; "torus" stays unknown
    for wrong in (dict(quad, min=[0, 0, 0]), dict(box, q=[0, 0, 0]), dict(quad, radius=1), {k: x for k, x in quad.items() if k != "v"},
                  dict(quad, rotate={"axis": [0, 1, 0], "angle": 1, "order": 2}), dict(quad, rotate=3), dict(box, rotate={"axis": [0, 0, 0], "angle": 1}),
                  dict(box, max=[0.7, 0.0, 1.6]), dict(quad, v=[3.0, 0.4, -0.8]), dict(quad, type="torus")):
        with pytest.raises(rtmi.RtmiError) as e:
            _parse(rtmi, [wrong])
        assert e.value.status == RT_ERR_SCENE, (wrong, str(e.value))


CPP = r'''
#include <cstdio>
#include "rtmi.hpp"
int main() {
    rtmi::scene sc(32, 18, 1, 4);
    auto grey = rtmi::lambertian(rtmi::color(0.5f, 0.5f, 0.5f));
    if (sc.add(rtmi::quad(rtmi::point3(0.3f, -0.2f, 0.7f), rtmi::vec3(1.5f, 0.2f, -0.4f), rtmi::vec3(-0.3f, 1.1f, 0.25f), grey)) != 0) return 2;
    rtmi::hittable b = rtmi::box(rtmi::point3(-0.5f, 0.1f, 0.2f), rtmi::point3(0.7f, 0.9f, 1.6f), grey);
    b.rotate(rtmi::vec3(0, 1, 0), 0.5f);
    b.translate(rtmi::vec3(1, 2, 3));
    if (sc.add(b) != 1) return 3;
    rtmi::hittable q = rtmi::quad(rtmi::point3(0, 0, 0), rtmi::vec3(1, 0, 0), rtmi::vec3(0, 1, 0), grey);
    q.translate(rtmi::vec3(0, 0, -1));
    if (sc.add(q) != 7) return 4;
    try {
        sc.add(rtmi::quad(rtmi::point3(0, 0, 0), rtmi::vec3(1, 0, 0), rtmi::vec3(2, 0, 0), grey));
        return 5;
    } catch (const rtmi::error &) {
    }
    try {
        rtmi::hittable s = rtmi::sphere(rtmi::point3(0, 0, 0), 1.0f, grey);
        s.translate(rtmi::vec3(1, 0, 0));
        return 6;
    } catch (const std::logic_error &) {
    }
    fputs(sc.to_json().c_str(), stdout);
    return 0;
}
'''


def test_quad_and_box_in_cpp(rtmi, tmp_path):
    src, exe = tmp_path / "t.cpp", tmp_path / "t"
    src.write_text(CPP)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", PKG, "-lrtmi", f"-Wl,-rpath,{PKG}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    objs = json.loads(r.stdout)["object"]["data"]
    assert [o["type"] for o in objs] == ["quad"] * 8 and objs[7]["q"] == [0, 0, -1]
    sc, m = _scene(rtmi)
    sc.quad((0.3, -0.2, 0.7), (1.5, 0.2, -0.4), (-0.3, 1.1, 0.25), m)
    sc.box((-0.5, 0.1, 0.2), (0.7, 0.9, 1.6), m, ((0, 1, 0), float(np.float32(np.float32(0.5) * np.float32(180.0) / np.float32(math.pi)))), (1, 2, 3))
    got = rtmi.Scene.parse(r.stdout).prims()
    assert got[:7]["m"].tobytes() == sc.prims()["m"].tobytes()


def test_c_symbols_and_null_arguments(rtmi):
    import ctypes as C
    assert {"rt_scene_add_quad", "rt_scene_add_box"} <= set(rtmi.C_SYMBOLS)
    lib = C.CDLL(os.path.join(PKG, "librtmi.so"))
    f3 = (C.c_float * 3)
    for fn, args in ((lib.rt_scene_add_quad, (None, f3(0, 0, 0), f3(1, 0, 0), f3(0, 1, 0), 0, None, C.c_float(0), None)),
                     (lib.rt_scene_add_box, (None, f3(0, 0, 0), f3(1, 1, 1), 0, None, C.c_float(0), None))):
        fn.restype = C.c_int
        assert fn(*args) == -RT_ERR_ARG
    sc, m = _scene(rtmi)
    lib.rt_scene_add_quad.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_float, C.c_void_p]
    assert lib.rt_scene_add_quad(sc._h, None, f3(1, 0, 0), f3(0, 1, 0), m, None, 0.0, None) == -RT_ERR_ARG
    lib.rt_scene_add_box.argtypes = [C.c_void_p] + [C.c_void_p] * 2 + [C.c_int, C.c_void_p, C.c_float, C.c_void_p]
    assert lib.rt_scene_add_box(sc._h, f3(0, 0, 0), None, m, None, 0.0, None) == -RT_ERR_ARG


def test_packed_records_lights_and_layouts(rtmi):
    sc, m = _scene(rtmi)
    sc.sphere((0, -100, 0), 100, m)
    t0 = sc.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), m)
    li = sc.diffuse_light(sc.checker_texture((4, 3, 2), (1, 2, 3)))
    q0 = sc.quad((-1, 3, -1), (2, 0, 0.5), (0.25, 0, 2), li)
    q1 = sc.quad((0.3, -0.2, 0.7), (1.5, 0.2, -0.4), (-0.3, 1.1, 0.25), m, ((0, 1, 0), 30.0))
    sc.quad((0, 2, 0), (1, 0, 0), (0, 0, 1), sc.diffuse_light(sc.image_texture(np.zeros((2, 2, 3), np.uint8) + 200)))  # no sampled light
    info = sc.table_info()
    assert info.grid_wide == 1 and info.kernel_variant in (16, 36, 44) and info.nt == 1
    img = sc.table_image().reshape(-1, 4)
    bits = img.view(np.int32)
    P = sc.prims()
    for k, pi in enumerate((q0, q1)):  # (small scene: nothing listed, the tables are in list order)
        hot = img[info.off_tri_hot + 5 * (info.nt + k):][:5]
        p = P[pi]
        assert np.array_equal(hot[0], np.append(p["m"][0:3], p["m"][9])) and np.array_equal(hot[1], np.append(p["m_inv"][0:3], p["m"][10]))
        assert np.array_equal(hot[2], np.append(p["m_inv"][3:6], p["m"][11]))
        M = p["m"].astype(np.float64)
        corners = np.array([M[0:3], M[0:3] + M[3:6], M[0:3] + M[3:6] + M[6:9], M[0:3] + M[6:9]])
        assert (hot[3, :3] <= corners.min(axis=0)).all() and (hot[4, :3] >= corners.max(axis=0)).all()
        assert (corners.min(axis=0) - hot[3, :3] < 1e-3).all() and (hot[4, :3] - corners.max(axis=0) < 1e-3).all()
        cold = bits[info.off_tri_cold + 2 * (info.nt + k)]
        assert cold[0] == p["material"] and cold[1] == pi
    # the light list: the checker quad alone, |u x v| its area
    L = sc.lights()
    assert len(L) == 1 and L[0]["prim"] == q0 and L[0]["shape"] == rtmi.PRIM_QUAD
    area = np.linalg.norm(np.cross((2, 0, 0.5), (0.25, 0, 2)))
    assert abs(L[0]["area"] - area) < 1e-6 and abs(L[0]["probability"] - 1) < 1e-7
    assert tuple(L[0]["emission"]) == (4, 3, 2) and tuple(L[0]["emission_odd"]) == (1, 2, 3)
    # ... and its record: shape 5, selection, 1 / area, the colours, then Q, u, v, n
    sc.set_light_sampling(True)
    img = sc.table_image().reshape(-1, 4)
    assert sc.table_info().kernel_variant & 256
    at = [i for i in range(len(img) - 7) if img[i].view(np.int32)[0] == 5 and img[i, 2] == 1.0 and np.array_equal(img[i + 1, :3], (4, 3, 2))]
    assert len(at) == 1
    rec = img[at[0]:at[0] + 7]
    assert abs(rec[0, 3] - 1 / area) < 1e-7 and rec[1].view(np.int32)[3] == 1 and np.array_equal(rec[2, :3], (1, 2, 3))
    p = P[q0]
    assert np.array_equal(rec[3:7, :3].reshape(-1), p["m"])
    # layouts 2 and 6 (the sphere-only kernels' compact tables) refuse a scene with a quad before they touch a device ... where
    # there is one; here the refusal of the table format is what can be seen
    sc.set_light_sampling(False)
    assert sc.table_info().grid_wide == 1


def test_a_grid_lists_quads(rtmi):
    """enough small quads for a grid: every quad is listed in a cell or among the always-tested ones, the room's wall is not listed"""
    sc, m = _scene(rtmi)
    rng = np.random.default_rng(3)
    for _ in range(40):
        c = rng.uniform(-3, 3, 3)
        sc.quad(tuple(c), tuple(rng.uniform(-0.3, 0.3, 3)), tuple(rng.uniform(-0.3, 0.3, 3)), m)
    sc.quad((-50, -4, -50), (0, 0, 100), (100, 0, 0), m)
    info = sc.table_info()
    assert info.grid_cells > 0 and info.grid_wide == 1
    img = sc.table_image().reshape(-1, 4)
    cells = img[info.off_grid_cells:info.off_grid_items].view(np.uint32).reshape(-1)[:2 * info.grid_cells].reshape(-1, 2)
    items = img[info.off_grid_items:].view(np.uint32).reshape(-1)
    listed = set()
    for first, h in cells:
        n_all, n_other = (h >> 10) & 1023, h >> 20
        listed.update(int(x) for x in items[first + n_all:first + n_all + n_other])
    base = info.ns + info.nr + info.nc + info.nt
    ids = sorted(x - base for x in listed)
    assert ids and ids[0] >= 1 and ids[-1] == 40 and len(ids) == 40  # the wall (always tested) leads the table; the 40 are listed
    wall = img[info.off_tri_hot + 5 * info.nt][:3]
    assert tuple(wall) == (-50, -4, -50)


# --------------------------------------------------------------------------- the wrapper pinned to the unedited yardstick
def _pair(rtmi, quads, nee, checker):
    sc = rtmi.Scene.new(24, 14, 1, 6)
    sc.set_background((0.02, 0.02, 0.03), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    fl = sc.lambertian(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.4, 0.2)) if checker else (0.6, 0.5, 0.4))
    li = sc.diffuse_light(sc.checker_texture((6, 5, 4), (1, 2, 6)) if checker else (6.0, 5.0, 4.0))
    wall, pic = sc.metal((0.8, 0.7, 0.6), 0.3), sc.lambertian(sc.image_texture(np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3) * 2))
    if quads:  # Q = (x0, y0, k) and the edges along the axes, in the rect's (first, second) order: (a, b) is the rect's (u, v)
        sc.quad((-20, NS.LIFT, -20), (40, 0, 0), (0, 0, 40), fl)
        sc.quad((-1, 3.0, -1), (2, 0, 0), (0, 0, 2), li)
        sc.quad((-3, NS.LIFT, -3), (6, 0, 0), (0, 4, 0), wall)
        sc.quad((-3, NS.LIFT, -3), (0, 4, 0), (0, 0, 5), pic)
    else:
        sc.xz_rect(-20, 20, -20, 20, NS.LIFT, fl)
        sc.xz_rect(-1, 1, -1, 1, 3.0, li)
        sc.xy_rect(-3, 3, NS.LIFT, 4 + NS.LIFT, -3, wall)
        sc.yz_rect(NS.LIFT, 4 + NS.LIFT, -3, 2, -3, pic)
    sc.sphere((0.5, 0.65 + NS.LIFT, 0.3), 0.6, sc.dielectric(1.5))
    sc.set_light_sampling(nee)
    return sc


@pytest.mark.parametrize("nee,checker", [(False, False), (True, False), (False, True), (True, True)])
def test_wrappers_give_the_rects_answers(rtmi, nee, checker):
    """(named for the wrappers ref64's quads once were: now ref64's own quad code, held to its rectangles on axis-aligned scenes)"""
    words = R.uniforms(rtmi, NS.REF_SEED, 24, 14, 0, 4, NS.REF_DRAWS)
    rects, quads = _pair(rtmi, False, nee, checker), _pair(rtmi, True, nee, checker)
    ra, sa, da = R.trace(R.RefScene(rects), words)
    rb, sb, db = R.trace(R.RefScene(quads), words)
    assert R.same_signature(sa, sb).all() and np.array_equal(da, db)
    assert np.abs(ra - rb).max() <= 1e-9, np.abs(ra - rb).max()
    t = R.tally(sb, R.RefScene(quads))
    assert t["image_vertices"] > 20
    if nee:
        assert t["quad_picks"] > 500


# ---------------------------------------------------------------------------------------- rt_quad.h on the host, random rays
QUADS = [((-0.9, -0.6, 0.1), (1.9, 0.2, -0.4), (0.3, 1.5, 0.3), None, 0.0, None),
         ((-0.8, -0.5, 0.25), (1.9, 0, 0), (0, 1.4, 0), (1, 2, 3), 37.0, (-0.4, 0.5, 0.1)),
         ((-0.7, 0.2, -0.6), (1.2, 0, 0.9), (-0.5, 0.1, 1.1), (0, 1, 0), -120.0, (0.0, 0.3, -0.2))]


def _rays(rng, n, reach=4.0):
    """test_primitives_fuzz._rays: origins in a box around the primitive, directions towards a jittered point near it"""
    o = rng.uniform(-reach, reach, (n, 3))
    target = rng.normal(0.0, 0.7, (n, 3))
    d = (target - o) * rng.uniform(0.2, 3.0, (n, 1))
    return o.astype(np.float32), d.astype(np.float32)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("quad") / "quad_host_driver")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "quad_host_driver.cpp"), "-lm"], check=True)
    return exe


@pytest.mark.parametrize("case", range(len(QUADS)))
def test_the_fp32_code_against_the_fp64_statement(rtmi, driver, tmp_path, case):
    q, u, v, axis, deg, off = QUADS[case]
    sc, m = _scene(rtmi)
    sc.quad(q, u, v, m, (axis, deg) if axis else None, off)
    p = sc.prims()[0]
    rng = np.random.default_rng(50 + case)
    n = 4000
    o, d = _rays(rng, n)
    rec = np.concatenate([np.tile(p["m"], (n, 1)), np.tile(p["m_inv"][0:6], (n, 1)), o, d, rng.random((n, 2)).astype(np.float32)], axis=1)
    assert rec.shape == (n, 26)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    rec.astype(np.float32).tofile(fin)
    subprocess.run([driver, fin, fout], check=True, timeout=120)
    got = np.fromfile(fout, np.float32).reshape(n, 16).astype(np.float64)
    # the fp64 statement, from the stored Q, u, v alone (n, A, B derived here, unrounded)
    M = p["m"].astype(np.float64)
    Q3, U, V = M[0:3], M[3:6], M[6:9]
    c = np.cross(U, V)
    nrm, w = c / np.linalg.norm(c), c / (c @ c)
    A, B = np.cross(V, w), np.cross(w, U)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    den = d64 @ nrm
    with np.errstate(all="ignore"):
        t64 = ((Q3 - o64) @ nrm) / den
    pt = o64 + t64[:, None] * d64
    a, b = (pt - Q3) @ A, (pt - Q3) @ B
    hit64 = np.isfinite(t64) & (t64 >= 1e-3) & (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
    # test_primitives_fuzz's rule: rays within 2e-3 of an edge, of t_min (x 10) or of grazing (x 10) are set aside, and are few
    margin = np.minimum(np.minimum(np.abs(a), np.abs(1 - a)), np.minimum(np.abs(b), np.abs(1 - b)))
    margin = np.minimum(margin, np.abs(t64 - 1e-3) * 10)
    margin = np.minimum(margin, np.abs(den) / np.linalg.norm(d64, axis=1) * 10)
    margin = np.nan_to_num(margin)
    decided = margin > 2e-3
    assert decided.mean() > 0.9, decided.mean()
    hit32 = got[:, 0] != 0
    assert not (decided & (hit32 != hit64)).any()
    both = decided & hit64
    assert both.sum() > 50 and ((den > 0) & both).sum() > 30 and ((den < 0) & both).sum() > 30
    rel = np.abs(got[both, 1] - t64[both]) / np.maximum(1.0, np.abs(t64[both]))
    assert rel.max() < 2e-5, rel.max()
    assert np.abs(got[both, 2] - a[both]).max() < 1e-5 and np.abs(got[both, 3] - b[both]).max() < 1e-5
    assert (np.abs(got[both, 4:7] - pt[both]).max(axis=1) < 1e-5 * np.maximum(1.0, np.abs(pt[both]).max(axis=1))).all()
    turned = np.where((den < 0)[:, None], nrm, -nrm)
    assert np.abs(got[both, 7:10] - turned[both]).max() < 2e-5
    assert np.array_equal(got[both, 10] != 0, den[both] < 0)
    # the light sample: y = Q + u1 u + u2 v, and its density from the ray's origin
    u1, u2 = rec[:, 24].astype(np.float64), rec[:, 25].astype(np.float64)
    y = Q3 + u1[:, None] * U + u2[:, None] * V
    assert np.abs(got[:, 11:14] - y).max() < 1e-5
    ld = y - o64
    d2 = (ld * ld).sum(axis=1)
    cosl = np.abs(ld @ nrm) / np.sqrt(d2)
    ok = cosl > 2e-3
    assert ok.mean() > 0.95
    assert (np.abs(got[ok, 14] - d2[ok] / cosl[ok]) / (d2[ok] / cosl[ok])).max() < 1e-3


def test_uniformly_drawn_rays_stay_under_the_cap():
    """the share of rays the rule sets aside, on uniformly drawn rays (uniform origins in the box, uniform directions): below the
    10 % the comparison allows"""
    rng = np.random.default_rng(7)
    n = 20000
    o = rng.uniform(-4, 4, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    Q3, U, V = (np.array(x, float) for x in QUADS[0][:3])
    c = np.cross(U, V)
    nrm, w = c / np.linalg.norm(c), c / (c @ c)
    den = d @ nrm
    t = ((Q3 - o) @ nrm) / den
    pt = o + t[:, None] * d
    a, b = (pt - Q3) @ np.cross(V, w), (pt - Q3) @ np.cross(w, U)
    margin = np.minimum(np.minimum(np.abs(a), np.abs(1 - a)), np.minimum(np.abs(b), np.abs(1 - b)))
    margin = np.minimum(np.minimum(margin, np.abs(t - 1e-3) * 10), np.abs(den) * 10)
    assert (np.nan_to_num(margin) > 2e-3).mean() > 0.9


# --------------------------------------------------------------------------------------------------------- the light sample
@pytest.mark.parametrize("vertex", [(0.2, 0.0, 0.3), (2.5, 1.0, -1.0), (-0.4, 2.2, 0.9), (0.3, 4.0, 0.2)])
def test_the_density_integrates_to_one_over_the_solid_angle(rtmi, vertex):
    """integral of p_l over the directions towards the quad = integral over the quad of p_l cos / dist^2 dA = 1, by midpoint
    quadrature in (u1, u2); and the points of sample_quad cover the quad uniformly"""
    sc, m = _scene(rtmi)
    sc.quad((-1, 3, -1), (2, 0.3, 0.5), (0.25, -0.2, 2), sc.diffuse_light((4.0, 3.0, 2.0)))
    sc.sphere((0, 0, 0), 0.5, m)
    sc.set_light_sampling(True)
    S = R.RefScene(sc)
    assert len(S.lights) == 1
    k = 400
    g = (np.arange(k) + 0.5) / k
    u1, u2 = (x.reshape(-1) for x in np.meshgrid(g, g, indexing="ij"))
    p = np.tile(np.array(vertex, np.float64), (len(u1), 1))
    ld, pl, rad, _, delta = R.sample_light(S, 0, p, u1, u2, np.float64)
    assert not delta
    Q3, U, V, nrm, _, _ = R.quad_record(S.prims[0], np.float64)
    area = np.linalg.norm(np.cross(U, V))
    d2 = (ld * ld).sum(axis=1)
    cosl = np.abs(ld @ nrm) / np.sqrt(d2)
    # d omega = cos / dist^2 dA, dA = area du1 du2
    total = (pl * cosl / d2).sum() * area / (k * k)
    assert abs(total - 1.0) < 1e-6, total
    assert np.allclose(p + ld, Q3 + u1[:, None] * U + u2[:, None] * V) and np.array_equal(rad, np.tile((4.0, 3.0, 2.0), (len(p), 1)))
    # from the hit's side: a ray from the vertex that hits the quad at the sampled point has the same density
    back = R.light_pdf_of_hit(S, 0, p, ld, np.ones(len(p)), np.tile(nrm, (len(p), 1)), np.float64)
    assert np.allclose(back, pl, rtol=1e-12)
    half = R.sample_light(S, 0, p, u1, u2, np.float64, ("quad_light_half_area",))[1]
    assert np.allclose(half, 2 * pl)


# ------------------------------------------------------------------------------------------- the per-sample cases on the CPU
@pytest.fixture(scope="module")
def inputs(rtmi):
    made = {}

    def of(name):
        key = Q.seed_of(name), Q.family(name) == Q.MOTION
        if key not in made:
            made[key] = Q.inputs(rtmi, name)
        return made[key]
    return of


@pytest.mark.parametrize("name", list(Q.CASES))
def test_fp32_reference_meets_criterion_a(rtmi, inputs, name):
    """Measured here (DESIGN 7q holds the rows): the fp32 NumPy reference within tolerance of the fp64 one on >= 97 % of the
    samples with at most 1 % flipping a branch, and the case holds what it is there for"""
    sc = Q.scene(rtmi, name)
    S = R.RefScene(sc)
    words, shutter = inputs(name)
    ref, stable, draws, tally = R.reference(S, words, shutter)
    assert draws.max() <= NS.REF_DRAWS
    r32, _, _ = R.trace(S, words, shutter=shutter, dtype=np.float32)
    j = R.judge(r32, ref, stable)
    print("\n" + R.row(name + " (fp32 NumPy)", j) + "\n    " + ", ".join(f"{k} {tally[k]}" for k in Q.CASES[name][3]))
    assert j["share"] >= 0.97 and j["flips"] <= 0.01, j
    Q.check_contents(name, tally)


def test_a_mistake_changes_the_reference(rtmi, inputs):
    """each deliberate mistake moves the fp64 reference itself on its case (the GPU test holds the kernel against both)"""
    for name, mistake in Q.MISTAKES:
        sc = Q.scene(rtmi, name)
        S = R.RefScene(sc)
        words, shutter = inputs(name)
        ref, stable, _, _ = R.reference(S, words, shutter)
        wrong, _, _ = R.trace(S, words, shutter=shutter, perturb=(mistake,))
        assert R.judge(wrong, ref, stable)["share"] < 0.97, (name, mistake)


# ------------------------------------------------------------------------------------------------------- the shipped scene
def test_the_shipped_scene(rtmi, scenes_dir):
    sc = rtmi.Scene.load(os.path.join(scenes_dir, "cornell_box.json"))
    assert not sc.light_sampling  # (--nee switches it on)
    P = sc.prims()
    assert len(P) == 18 and (P["type"] == rtmi.PRIM_QUAD).all()
    L = sc.lights()
    assert len(L) == 1 and L[0]["shape"] == rtmi.PRIM_QUAD and abs(L[0]["area"] - 130 * 105) < 1e-2
    assert sc.materials()["type"][P["material"][6]] == R.ROUGH_METAL
    info = sc.table_info()
    assert info.kernel_variant in (16, 36, 44) and info.grid_wide == 1
    sc.set_light_sampling(True)
    assert sc.table_info().kernel_variant & 256
    # both boxes stand inside the room, turned
    for first in (6, 12):
        M = P[first:first + 6]["m"].astype(np.float64)
        corners = np.concatenate([M[:, 0:3], M[:, 0:3] + M[:, 3:6] + M[:, 6:9]])
        assert corners.min() > 0 and corners.max() < 555 and abs(M[2, 9]) < 0.999
