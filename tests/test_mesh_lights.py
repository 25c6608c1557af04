"""Mesh lights (rt_scene_set_mesh_lights) on the host, no GPU needed: the switch through every interface, what it
lists, what it leaves alone, the packed record of a triangle light, and the references of the per-sample cases of
test_gpu_mesh_lights.py (the fp64 statement against the same formulas at fp32, and the counts each case pins)."""
import json
import os
import subprocess

import numpy as np
import pytest

import ext_scenes as X
import mesh_light_scenes as ML
import nee_scenes as NS
import ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
RTMI = os.path.join(PKG, "rtmi")
RT_ERR_ARG = 1


def lum(c):
    c = np.asarray(c, np.float64)
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


# ---- the switch --------------------------------------------------------------------------------------------------------
def test_switch_in_c_and_python(rtmi):
    lib = rtmi._lib
    sc = X._unlisted(rtmi)
    assert sc.mesh_lights is False and lib.rt_scene_get_mesh_lights(sc._h) == 0  # the default
    assert lib.rt_scene_set_mesh_lights(sc._h, 1) == 0 and lib.rt_scene_get_mesh_lights(sc._h) == 1 and sc.mesh_lights is True
    assert lib.rt_scene_set_mesh_lights(sc._h, 7) == 0 and sc.mesh_lights is True  # (any nonzero value)
    sc.set_mesh_lights(False)
    assert sc.mesh_lights is False
    sc.set_mesh_lights()
    assert sc.mesh_lights is True
    assert lib.rt_scene_set_mesh_lights(None, 1) == RT_ERR_ARG and lib.rt_scene_get_mesh_lights(None) == -RT_ERR_ARG
    for name in ("rt_scene_set_mesh_lights", "rt_scene_get_mesh_lights"):
        assert name in rtmi.C_SYMBOLS
    assert rtmi.abi_version() == 3  # the ABI version stays
    assert sc.clone().mesh_lights is True


def test_switch_repacks_the_tables(rtmi):
    """the setter bumps the scene's version: the next table_image() is packed anew, with the triangles' records"""
    sc = X._unlisted(rtmi)
    before = sc.table_image()
    sc.set_mesh_lights(True)
    after = sc.table_image()
    assert after.shape[0] == before.shape[0] + 2 * (7 + 1)  # two more lights: 7 records and 1 alias entry each
    sc.set_mesh_lights(False)
    assert sc.table_image().tobytes() == before.tobytes()  # (bytes: integer words read as floats are NaNs)


def test_switch_in_json(rtmi, scenes_dir):
    doc = json.loads(rtmi.Scene.load(os.path.join(scenes_dir, "three_sphere.json")).to_json())
    assert "mesh_lights" not in doc  # written only when on
    assert rtmi.Scene.parse(json.dumps(doc)).mesh_lights is False
    doc["mesh_lights"] = True
    sc = rtmi.Scene.parse(json.dumps(doc))
    assert sc.mesh_lights is True
    again = json.loads(sc.to_json())
    assert again["mesh_lights"] is True
    assert rtmi.Scene.parse(json.dumps(again)).to_json() == sc.to_json()  # JSON -> scene -> JSON is a fixed point
    doc["mesh_lights"] = False
    sc = rtmi.Scene.parse(json.dumps(doc))
    assert sc.mesh_lights is False and "mesh_lights" not in json.loads(sc.to_json())
    for bad in (1, 0, "true", None, [True]):
        doc["mesh_lights"] = bad
        with pytest.raises(rtmi.RtmiError):
            rtmi.Scene.parse(json.dumps(doc))
    # a scene built through the API writes the key too
    sc = X._unlisted(rtmi)
    sc.set_mesh_lights(True)
    assert json.loads(sc.to_json())["mesh_lights"] is True


def test_shipped_scene(rtmi, scenes_dir):
    sc = rtmi.Scene.load(os.path.join(scenes_dir, "mesh_light.json"))
    assert sc.mesh_lights is True and sc.light_sampling is False  # (light sampling is left to --nee)
    L = sc.lights()
    assert len(L) == 576 and (L["shape"] == R.TRIANGLE).all()
    sc.set_mesh_lights(False)
    assert len(sc.lights()) == 0


CPP = r'''
#include <cstdio>
#include "rtmi.hpp"
int main() {
    rtmi::scene sc(64, 36, 1, 4);
    sc.add(rtmi::xz_rect(-1, 1, -2, 2, 0.5f, rtmi::lambertian(rtmi::color(0.5f, 0.5f, 0.5f))));
    if (sc.mesh_lights()) return 2;
    sc.set_mesh_lights(true);
    if (!sc.mesh_lights()) return 3;
    fputs(sc.to_json().c_str(), stdout);
    sc.set_mesh_lights(false);
    return sc.mesh_lights() ? 4 : 0;
}
'''


def test_switch_in_cpp(rtmi, tmp_path):
    src, exe = tmp_path / "t.cpp", tmp_path / "t"
    src.write_text(CPP)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", PKG, "-lrtmi", f"-Wl,-rpath,{PKG}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert json.loads(r.stdout)["mesh_lights"] is True


def test_switch_in_the_cli(scenes_dir, tmp_path):
    """--mesh-lights is a flag: the dumped scene carries the key (what follows the dump needs a GPU and may fail without one)"""
    sample = os.path.join(scenes_dir, "three_sphere.json")
    for flags, want in ((["--mesh-lights"], True), (["--nee", "--mesh-lights"], True), ([], None)):
        out = tmp_path / "scene.json"
        p = subprocess.run([RTMI, "-f", sample, "-w", "16", "-h", "9", "-spp", "1", *flags, "--dump-json", str(out),
                            "-o", str(tmp_path / "x.ppm"), "--no-png"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
        assert p.returncode != 2, p.stderr
        assert json.loads(out.read_text()).get("mesh_lights") is want
    p = subprocess.run([RTMI, "--mesh-lights=1"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 2 and "--mesh-lights" in p.stderr


# ---- off: nothing changes ------------------------------------------------------------------------------------------------
def test_switch_off_keeps_lights_and_tables_of_the_parent(rtmi, scenes_dir, golden_dir):
    """lights() and the packed image of every scene shipped before the feature, with and without light sampling, and of the
    "unlisted emitters" case: the digests the commit before the feature wrote"""
    with open(os.path.join(golden_dir, "mesh_lights_off_digests.json")) as f:
        want = json.load(f)
    cases = ML.digest_cases(rtmi, scenes_dir)
    assert sorted(cases) == sorted(want)
    for name, make in cases.items():
        sc = make()
        assert sc.mesh_lights is False
        assert ML.digest(sc) == want[name], name
        # with light sampling off the switch changes no table
        if not sc.light_sampling:
            sc.set_mesh_lights(True)
            assert ML.digest(sc)["image"] == want[name]["image"], name


# ---- on: what is listed --------------------------------------------------------------------------------------------------
def test_unlisted_emitters_with_the_switch_on(rtmi):
    sc = X.scene(rtmi, "unlisted emitters")  # (asserts the premise: one light while the switch is off)
    P, M, T = sc.prims(), sc.materials(), sc.textures()
    sc.set_mesh_lights(True)
    L = sc.lights()
    tris = [i for i in range(len(P)) if P["type"][i] == R.TRIANGLE and M["type"][P["material"][i]] == R.DIFFUSE_LIGHT]
    assert len(tris) == 2
    assert list(L["prim"]) == [2] + tris and list(L["shape"]) == [R.XZ_RECT, R.TRIANGLE, R.TRIANGLE]  # list order
    # the image-textured rectangle emitter still is no light
    img = [i for i in range(len(P)) if M["type"][P["material"][i]] == R.DIFFUSE_LIGHT and T["type"][M["texture"][P["material"][i]]] == R.IMAGE]
    assert len(img) == 1 and img[0] not in L["prim"]
    # area and probability against fp64
    area = np.array([1.0] + [R.triangle_area(P[i]) for i in tris])
    power = area * np.array([lum((6.0, 5.0, 4.0))] + [lum((2.0, 1.5, 1.0))] * 2)
    np.testing.assert_allclose(L["area"], area, rtol=1e-6)
    np.testing.assert_allclose(L["probability"], power / power.sum(), rtol=1e-6)
    assert abs(float(L["probability"].astype(np.float64).sum()) - 1.0) <= 3 * 2.0 ** -24
    assert np.array_equal(L["emission"][1], (2.0, 1.5, 1.0)) and np.array_equal(L["emission_odd"][1], (2.0, 1.5, 1.0))


def _slivers(rtmi, emitter=True):
    sc = ML._frame(rtmi)
    sc.xz_rect(-5, 5, -5, 5, 0.0, sc.lambertian((0.5, 0.5, 0.5)))
    e = sc.diffuse_light((3.0, 3.0, 3.0))
    sc.triangle((0, 1, 0), (1, 1, 0), (0, 1, 1), e)                # area 0.5: a light
    sc.triangle((0, 2, 0), (1e-25, 2, 0), (0, 2, 1e-25), e)        # area 5e-51: zero as the record's fp32 word
    sc.triangle((0, 3, 0), (1e-20, 3, 0), (0, 3, 1e-20), e)        # area 5e-41: 1 / area is not finite in fp32
    sc.triangle((0, 4, 0), (1, 4, 0), (0, 4, 1), sc.diffuse_light((0.0, 0.0, 0.0)))  # no power
    return sc


def test_degenerate_triangles_are_skipped(rtmi):
    sc = _slivers(rtmi)
    sc.set_mesh_lights(True)
    sc.set_light_sampling(True)
    L = sc.lights()
    assert list(L["prim"]) == [1] and L["probability"][0] == 1.0 and L["area"][0] == 0.5
    image = sc.table_image()  # packs: no error, and every word of the one record is finite
    thr, alias = R.find_alias_table(image, L)
    assert list(alias) == [0]


def test_an_emissive_mesh_is_one_light_per_triangle(rtmi):
    sc = ML._frame(rtmi)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.5, 0.5, 0.5)))
    sc.xz_rect(-1, 1, -1, 1, 4.0, sc.diffuse_light((2.0, 2.0, 2.0)))
    n = sc.add_obj(os.path.join(PKG, "meshes", "torus.obj"), sc.diffuse_light(sc.checker_texture((5.0, 1.0, 1.0), (1.0, 1.0, 5.0))), 0.4,
                   translate=(0.0, 1.5, 0.0), normals="smooth")
    assert n == 576
    assert len(sc.lights()) == 1
    sc.set_mesh_lights(True)
    sc.set_light_sampling(True)
    L = sc.lights()
    assert len(L) == 1 + n and (L["shape"][1:] == R.TRIANGLE).all() and list(L["prim"][1:]) == list(range(2, 2 + n))
    P = sc.prims()
    area = np.array([4.0] + [R.triangle_area(P[i]) for i in L["prim"][1:]])
    np.testing.assert_allclose(L["area"], area, rtol=1e-6)
    power = area * 0.5 * (lum(L["emission"]) + lum(L["emission_odd"]))
    np.testing.assert_allclose(L["probability"], power / power.sum(), rtol=1e-6)
    assert abs(float(L["probability"].astype(np.float64).sum()) - 1.0) <= len(L) * 2.0 ** -24
    # the alias table is found by content, and implies the probabilities (test_nee_reference.test_alias_table's bound)
    thr, alias = R.find_alias_table(sc.table_image(), L)
    assert alias.min() >= 0 and alias.max() < len(L) and thr.min() >= 0 and thr.max() <= 1
    bound = len(L) * 2.0 ** -24
    assert np.abs(R.implied_alias_probability(thr, alias) - L["probability"]).max() <= bound
    # a scene whose only sampled emitters are triangles gets the light part and the wide tables as well
    only = ML.lone(rtmi)
    only.set_light_sampling(True)
    small = only.table_image().shape[0]
    only.set_mesh_lights(True)
    assert only.table_image().shape[0] > small and only.table_info().grid_wide >= 1


# ---- the packed record -----------------------------------------------------------------------------------------------------
def test_packed_record_of_a_triangle_light(rtmi):
    """The 7 records of each light of the checker quad's two triangles, word for word: {4, grouped id, probability, 1 / area} {even, checker}
    {odd, 0} {v1, 0} {e1, 0} {e2, 0} {n, 0}; and the light slot of its grouped id"""
    sc = ML.checker_quad(rtmi)
    sc.set_light_sampling(True)
    sc.set_mesh_lights(True)
    L, P, info = sc.lights(), sc.prims(), sc.table_info()
    assert len(L) == 2
    w = np.ascontiguousarray(sc.table_image(), np.float32).reshape(-1)
    bits = w.view(np.int32)
    starts = [k for k in np.flatnonzero(w[2::4] == L["probability"][0]) * 4
              if bits[k] == 4 and np.array_equal(w[k + 4:k + 7], L["emission"][0])]
    at = starts[0]
    assert starts == [at, at + 28]  # (the quad's two halves have the same area: both records match, one stride apart)
    base = info.ns + info.nr + info.nc  # triangles follow the spheres, rects and cylinders in the grouped ids
    for i in range(2):
        rec, ib = w[at + 28 * i:at + 28 * (i + 1)], bits[at + 28 * i:at + 28 * (i + 1)]
        pr = P[L["prim"][i]]
        v1, e1, e2, n = R.triangle_light_record(pr)
        want = np.zeros(28, np.float32)
        want[2], want[3] = L["probability"][i], np.float32(1.0 / R.triangle_area(pr))
        want[4:7], want[8:11] = (6.0, 1.0, 0.5), (0.5, 2.0, 6.0)
        want[12:15], want[16:19], want[20:23], want[24:27] = v1, e1, e2, n
        wb = want.view(np.int32).copy()
        wb[0], wb[1], wb[7] = 4, base + i, 1  # shape code, grouped id (the packer's triangle order: list order here), checker
        assert np.array_equal(ib, wb), (i, ib, wb)
        np.testing.assert_allclose(rec[24:27], np.cross(e1.astype(np.float64), e2) / np.linalg.norm(np.cross(e1.astype(np.float64), e2)), atol=1e-6)
    # the alias table follows the records, the slot table follows it: one word per grouped id, -1 but for the two triangles
    slot = bits[at + 28 * 2 + 4 * 2:][:base + info.nt]
    assert list(slot[:base]) == [-1] * base and list(slot[base:]) == [0, 1]


# ---- the references of the per-sample cases ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def words(rtmi):
    return ML.inputs(rtmi, ML.MIXED)[0]


def test_refscene_builds_and_the_wrapper_is_removed(rtmi, words):
    """(the wrapper that once held the triangle lights is gone for good: ref64.sample_light samples them itself)"""
    sc = ML.scene(rtmi, ML.MIXED)
    S = R.RefScene(sc)
    assert len(S.lights) == 18 and (S.lights["shape"] == R.TRIANGLE).sum() == 16 and len(S.light_of_prim) == 18
    # the density of a sampled point equals the density ref64 states from the hit's side (geometric normal on both)
    rng = np.random.default_rng(1)
    li = int(np.flatnonzero(S.lights["shape"] == R.TRIANGLE)[3])
    p = rng.uniform(-1, 1, (50, 3)) + (0.0, 0.2, 2.5)
    ld, pl, _, _, _ = R.sample_light(S, li, p, rng.random(50), rng.random(50), np.float64)
    n = np.repeat(S.prims[S.lights[li]["prim"]]["m"][9:12].astype(np.float64)[None, :], 50, axis=0)
    np.testing.assert_allclose(R.light_pdf_of_hit(S, li, p, ld, np.ones(50), n, np.float64), pl, rtol=1e-12)


@pytest.mark.parametrize("name", list(ML.CASES))
def test_fp32_statement_clears_the_share_and_the_case_holds_its_vertices(rtmi, words, name):
    """on the CPU, before any kernel: the same formulas at fp32 against fp64 meet criterion (a) with at most 1 % of the samples
    flipping a branch, and the reference's signatures hold the pinned counts"""
    sc = ML.scene(rtmi, name)
    S = R.RefScene(sc)
    ref, stable, draws, tally = R.reference(S, words)
    assert draws.max() <= NS.REF_DRAWS
    r32, _, _ = R.trace(S, words, dtype=np.float32)
    j = R.judge(r32, ref, stable)
    print("\n" + R.row(name + " (fp32 NumPy)", j))
    assert j["share"] >= 0.97 and j["flips"] <= 0.01 and j["bias_ok"], j
    ML.check_contents(name, tally)
