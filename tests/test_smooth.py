"""Smooth shading without a GPU: the API and its errors, OBJ vertex normals, generated normals, and the packed
tables (unchanged for a scene without vertex normals; the NORMALS part for one with)."""
import hashlib
import json
import os

import numpy as np
import pytest

import ref64 as R
import smooth_pack_cases as PC
import smooth_scenes as SS

V = ((0.0, 0.0, 0.0), (2.0, 0.0, 0.5), (0.5, 1.5, 0.0))
N = ((0.0, 0.2, 1.0), (0.3, 0.0, 2.0), (-0.1, 0.1, 0.7))  # not unit: the scene normalises


def unit(a):
    a = np.asarray(a, np.float64)
    return a / np.sqrt((a * a).sum(axis=-1))[..., None]


def tris(sc):
    p = sc.prims()
    return p[p["type"] == 5]


def new(rtmi):
    sc = rtmi.Scene.new(16, 9, 1, 4)
    return sc, sc.lambertian((0.5, 0.5, 0.5))


# ---------------------------------------------------------------------------------------------------------------- API
def test_round_trip_through_prims_and_json(rtmi, tmp_path):
    sc, mat = new(rtmi)
    sc.triangle(*V, mat, (0.1, 0.2), (0.3, 0.4), (0.5, 0.6), normals=N)
    sc.triangle(*V, mat)
    smooth, flat = tris(sc)
    got = R.prim_normals(smooth)
    # normalised in fp64, rounded once
    assert np.array_equal(got, unit(np.asarray(N, np.float32)).astype(np.float32))  # (the interface takes fp32)
    assert np.abs(np.sqrt((got.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() <= 1e-7
    assert np.array_equal(smooth["m_inv"][9:12], np.zeros(3, np.float32))
    assert np.array_equal(smooth["m_inv"][:6], np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6], np.float32))
    # a flat triangle: nine zeros, and the geometry words are the same with and without normals
    assert not R.has_normals(flat) and np.array_equal(R.prim_normals(flat), np.zeros((3, 3), np.float32))
    assert np.array_equal(smooth["m"], flat["m"])
    # JSON: the normals are written and read back bit for bit; a flat triangle has no n1
    text = sc.to_json()
    path = tmp_path / "scene.json"
    path.write_text(text)
    back = rtmi.Scene.load(str(path))
    assert back.prims().tobytes() == sc.prims().tobytes()
    assert back.to_json() == text
    assert text.count('"n1"') == 1 and text.count('"n3"') == 1


def test_sizes_and_abi_version_are_unchanged(rtmi):
    assert rtmi.abi_version() == 3
    assert rtmi.PRIM_DTYPE.itemsize == 128 and rtmi._lib.rt_struct_size(2) == 128


def test_argument_errors_each_give_a_message(rtmi, tmp_path):
    sc, mat = new(rtmi)
    for bad in ((0.0, 0.0, 0.0), (float("nan"), 0.0, 1.0), (float("inf"), 0.0, 0.0)):
        for slot in range(3):
            n = [N[0], N[1], N[2]]
            n[slot] = bad
            with pytest.raises(rtmi.RtmiError) as e:
                sc.triangle(*V, mat, normals=n)
            assert e.value.status == 1 and "normal" in str(e.value)
    assert len(sc.prims()) == 0  # nothing was added
    with pytest.raises(ValueError):
        sc.triangle(*V, mat, normals=(N[0], N[1]))
    # a null normal through the C interface
    f3 = lambda v: (rtmi.C.c_float * 3)(*v)
    rc = rtmi._lib.rt_scene_add_triangle_normals(sc._h, f3(V[0]), f3(V[1]), f3(V[2]), f3(N[0]), None, f3(N[2]), None, None, None, mat)
    assert rc == -1 and b"normal is null" in rtmi._lib.rt_last_error()
    # the mesh: mode and crease angle
    obj = tmp_path / "t.obj"
    obj.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    with pytest.raises(ValueError):
        sc.add_obj(str(obj), mat, normals="round")
    for mode, crease, word in ((3, 10.0, "mode"), (-1, 10.0, "mode"), (2, -1.0, "crease"), (2, 181.0, "crease"), (2, float("nan"), "crease")):
        rc = rtmi._lib.rt_scene_add_obj_normals(sc._h, os.fsencode(str(obj)), mat, 1.0, None, None, mode, crease)
        assert rc == -1 and word.encode() in rtmi._lib.rt_last_error(), (mode, crease, rtmi._lib.rt_last_error())
    # JSON: all three normals or none; a mesh's "normals" is one of three words
    base = json.loads(sc.to_json())
    for obj_json, word in (({"type": "triangle", "v1": V[0], "v2": V[1], "v3": V[2], "n1": N[0], "material": 0}, "come together"),
                           ({"type": "mesh", "file": str(obj), "normals": "round", "material": 0}, "normals")):
        doc = dict(base, object={"data": [obj_json]})
        p = tmp_path / "bad.json"
        p.write_text(json.dumps(doc))
        with pytest.raises(rtmi.RtmiError) as e:
            rtmi.Scene.load(str(p))
        assert word in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------------------------- OBJ
QUAD_OBJ = """v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0.25 0.75
vn 0 0 1
vn 1 0 1
vn 0 2 2
f 1//1 2//2 3//3
f 1/1/3 3/1/2 4/1/1
f 1 2//2 3/1
"""


def test_obj_vn_lines_and_corner_forms(rtmi, tmp_path):
    obj = tmp_path / "q.obj"
    obj.write_text(QUAD_OBJ)
    vn = unit([(0, 0, 1), (1, 0, 1), (0, 2, 2)]).astype(np.float32)
    face = np.array([0, 0, 1], np.float32)
    sc, mat = new(rtmi)
    assert sc.add_obj(str(obj), mat, normals="file") == 3
    t = tris(sc)
    assert np.array_equal(R.prim_normals(t[0]), vn[[0, 1, 2]])          # a//n
    assert np.array_equal(R.prim_normals(t[1]), vn[[2, 1, 0]])          # a/t/n
    assert np.array_equal(t[1]["m_inv"][:6], np.array([0.25, 0.75] * 3, np.float32))
    assert np.array_equal(R.prim_normals(t[2]), np.array([face, vn[1], face]))  # corners without n: the face normal
    # rt_scene_add_obj and normals="flat": n ignored, as before
    for kw in ({}, {"normals": "flat"}):
        fl, m2 = new(rtmi)
        assert fl.add_obj(str(obj), m2, **kw) == 3
        assert not any(R.has_normals(p) for p in tris(fl))
        assert np.array_equal(tris(fl)["m"], t["m"])
    # an n out of range (0 and negative included) is an error
    for corner in ("1//4", "1//0", "1//-1"):
        bad = tmp_path / "bad.obj"
        bad.write_text(QUAD_OBJ.replace("f 1//1 2//2 3//3", "f %s 2//2 3//3" % corner))
        s2, m2 = new(rtmi)
        with pytest.raises(rtmi.RtmiError) as e:
            s2.add_obj(str(bad), m2, normals="file")
        assert "normal" in str(e.value)
        assert s2.add_obj(str(bad), m2) == 3  # flat: still ignored


def test_obj_normals_go_through_the_inverse_transpose(rtmi, tmp_path):
    """a non-uniform, sheared matrix with a negative scale: a normal stays perpendicular to its placed tangents"""
    v, n = SS.uv_sphere((0.0, 0.0, 0.0), 1.0, 4, 6)
    obj = tmp_path / "s.obj"
    SS.write_obj(str(obj), v, n, "a//n")
    M = np.array([[2.0, 0.3, 0.0], [0.0, 0.5, 0.1], [0.4, 0.0, 1.5]])
    for scale in (1.7, -0.6):
        sc, mat = new(rtmi)
        assert sc.add_obj(str(obj), mat, scale, M.reshape(9), (0.5, -1.0, 2.0), normals="file") == len(v)
        A = scale * M
        want = unit(n.reshape(-1, 3) @ np.linalg.inv(A)).reshape(-1, 3, 3)  # rows: (A^-T n)^T = n^T A^-1
        got = np.array([R.prim_normals(p) for p in tris(sc)], np.float64)
        # bound: the product and the normalisation in fp64, one rounding to fp32 (2^-24 per component)
        assert np.abs(got - want).max() <= 1e-7, np.abs(got - want).max()
        # and it is NOT the matrix itself applied to the normal
        wrong = unit(n.reshape(-1, 3) @ A.T).reshape(-1, 3, 3)
        assert np.abs(got - wrong).max() > 0.1


# ------------------------------------------------------------------------------------------------------ generated normals
CUBE_V = [(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]  # index 4 ix + 2 iy + iz
CUBE_FACES = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # outward quads


def cube_obj(path, cut):
    """cut[f] = 0: quad (a, b, c, d) as (a, b, c) + (a, c, d); 1: as (b, c, d) + (b, d, a)"""
    with open(path, "w") as f:
        for p in CUBE_V:
            f.write("v %d %d %d\n" % p)
        for k, (a, b, c, d) in enumerate(CUBE_FACES):
            for tri in (((a, b, c), (a, c, d)) if cut[k] == 0 else ((b, c, d), (b, d, a))):
                f.write("f %d %d %d\n" % tuple(i + 1 for i in tri))


@pytest.mark.parametrize("cut", [(0,) * 6, (1,) * 6, (0, 1, 1, 0, 1, 0)])
def test_cube_normals_do_not_depend_on_the_triangulation(rtmi, tmp_path, cut):
    """crease 180: every corner (+-1, +-1, +-1) / sqrt 3, whichever way each face is cut -- what angle weights are for (area or
    uniform weights give a corner with one triangle of a face on one side and two on another a leaning normal); crease 30:
    the face normals"""
    obj = tmp_path / "cube.obj"
    cube_obj(str(obj), cut)
    sc, mat = new(rtmi)
    assert sc.add_obj(str(obj), mat, 0.75, None, (3.0, 1.0, -2.0), normals="smooth", crease_angle=180.0) == 12
    for p in tris(sc):
        corners = (p["m"][:9].reshape(3, 3).astype(np.float64) - (3.0, 1.0, -2.0)) / 0.75
        want = (corners / np.sqrt(3.0)).astype(np.float32)
        got = R.prim_normals(p)
        assert np.abs(got - want).max() <= 2.0 ** -24, (got, want)  # to fp32 rounding of 0.577...
    sharp, m2 = new(rtmi)
    assert sharp.add_obj(str(obj), m2, normals="smooth", crease_angle=30.0) == 12
    for p in tris(sharp):
        assert np.array_equal(R.prim_normals(p), np.tile(p["m"][9:12], (3, 1)))


def test_generated_normals_of_a_uv_sphere_are_radial(rtmi, tmp_path):
    """16 rings x 24 segments: the angle-weighted normal of a vertex leans from the radial direction by the asymmetry of the
    rings above and below it.  Measured 0.0078 (max component difference); the bound 0.02 is the
    angle between neighbouring rings (pi / 16 = 0.196) times a tenth: a normal that took one neighbouring face's direction
    would be off by half that angle, 0.098."""
    v, n = SS.uv_sphere((0.0, 0.0, 0.0), 1.0, 16, 24)
    obj = tmp_path / "s.obj"
    SS.write_obj(str(obj), v, None, "a")
    sc, mat = new(rtmi)
    assert sc.add_obj(str(obj), mat, normals="smooth") == len(v)
    got = np.array([R.prim_normals(p) for p in tris(sc)], np.float64)
    dev = np.abs(got - n).max()
    print("uv sphere generated normals: max deviation from radial", dev)
    assert dev <= 0.02
    assert np.abs(np.sqrt((got * got).sum(axis=-1)) - 1.0).max() <= 1e-7


# ---------------------------------------------------------------------------------------------------------------- packing
def test_scenes_without_normals_pack_to_the_parents_bytes(rtmi, scenes_dir, golden_dir, tmp_path):
    with open(os.path.join(golden_dir, "smooth_pack_digests.json")) as f:
        golden = json.load(f)
    cases = PC.cases(rtmi, scenes_dir, str(tmp_path))
    assert sorted(cases) == sorted(golden)
    for name, build in cases.items():
        assert PC.digest(build()) == golden[name], name


def test_the_normals_part(rtmi):
    """a scene with vertex normals: the flat scene's image, then three records per triangle in table order, found through the
    .w of the camera block's last record; a flat triangle's records are zeros"""
    sc, flat = SS.query_scene(rtmi, True), SS.query_scene(rtmi, False)
    a, b = sc.table_image().reshape(-1, 4), flat.table_image().reshape(-1, 4)
    ti, tf = sc.table_info(), flat.table_info()
    nt = ti.nt
    assert nt == tf.nt == 87 and len(a) == len(b) + 3 * nt
    assert ti.kernel_variant == tf.kernel_variant
    off_cam = ti.off_tri_hot + 5 * nt  # behind the triangles' hot records (device_scene.h)
    word = a[off_cam + 5].view(np.int32)[3]
    assert word == len(b) and b[off_cam + 5].view(np.int32)[3] == 0
    head = a[:len(b)].copy()
    head[off_cam + 5, 3] = 0.0
    assert head.tobytes() == b.tobytes()
    part = a[len(b):].reshape(nt, 3, 4)
    cold = a[ti.off_tri_cold:ti.off_tri_cold + 2 * nt].reshape(nt, 2, 4)
    prims = sc.prims()
    n_smooth = 0
    for k in range(nt):
        p = prims[cold[k, 0].view(np.int32)[1]]  # the triangle's list index
        assert np.array_equal(part[k, :, :3], R.prim_normals(p))
        assert part[k, 0].view(np.int32)[3] == (1 if R.has_normals(p) else 0) and part[k, 1, 3] == 0 and part[k, 2, 3] == 0
        n_smooth += R.has_normals(p)
    assert n_smooth == 83
