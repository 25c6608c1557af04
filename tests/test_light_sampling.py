"""Light sampling (rt_scene_set_light_sampling): the scene switch, its JSON key, the list of sampled emitters and the device
tables it adds -- everything the host does, no GPU needed."""
import glob
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes")
GOLDEN = os.path.join(ROOT, "tests", "golden", "scenes_as_shipped")


@pytest.fixture(scope="module")
def rtmi():
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


def lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def test_switch_and_json_round_trip(rtmi):
    sc = rtmi.Scene.load(os.path.join(SCENES, "mixed_emissive.json"))
    assert not sc.light_sampling and "light_sampling" not in json.loads(sc.to_json())
    sc.set_light_sampling(True)
    assert sc.light_sampling and json.loads(sc.to_json())["light_sampling"] is True
    assert rtmi.Scene.parse(sc.to_json()).light_sampling
    assert sc.clone().light_sampling and rtmi.Scene.dna(10.0, sc).light_sampling
    sc.override(32, 18, 2)
    assert sc.light_sampling
    sc.set_light_sampling(False)
    assert "light_sampling" not in json.loads(sc.to_json())
    j = json.loads(sc.to_json())
    for bad in (1, "yes", None):
        j["light_sampling"] = bad
        with pytest.raises(rtmi.RtmiError):
            rtmi.Scene.parse(json.dumps(j))
    j["light_sampling"] = False
    assert not rtmi.Scene.parse(json.dumps(j)).light_sampling


def test_lights_of_mixed_emissive(rtmi):
    sc = rtmi.Scene.load(os.path.join(SCENES, "mixed_emissive.json"))
    prims, mats, texs = sc.prims(), sc.materials(), sc.textures()
    L = sc.lights()
    emitters = [i for i, p in enumerate(prims) if mats[p["material"]]["type"] == rtmi.MAT_DIFFUSE_LIGHT]
    assert sorted(L["prim"]) == emitters and len(L) == 3
    assert sorted(L["shape"]) == [rtmi.PRIM_XZ_RECT, rtmi.PRIM_CYLINDER, rtmi.PRIM_CYLINDER]
    checker = [l for l in L if texs[mats[prims[l["prim"]]["material"]]["texture"]]["type"] == rtmi.TEX_CHECKER]
    assert len(checker) == 1 and not np.array_equal(checker[0]["emission"], checker[0]["emission_odd"])
    power = L["area"] * 0.5 * (lum(L["emission"]) + lum(L["emission_odd"]))
    assert abs(L["probability"].sum() - 1.0) < 1e-6
    np.testing.assert_allclose(L["probability"], power / power.sum(), rtol=1e-5)
    rect = L[L["shape"] == rtmi.PRIM_XZ_RECT][0]
    f = prims[rect["prim"]]["f"]
    assert rect["area"] == pytest.approx((f[1] - f[0]) * (f[3] - f[2]), rel=1e-6)
    for c in L[L["shape"] == rtmi.PRIM_CYLINDER]:
        f = prims[c["prim"]]["f"]
        assert c["area"] == pytest.approx(2 * np.pi * abs(f[0]) * (f[2] - f[1]), rel=1e-6)


def test_lights_of_hand_built_scenes(rtmi):
    sc = rtmi.Scene.load(os.path.join(SCENES, "mixed_emissive.json"))
    before = sc.lights()
    s1 = sc.sphere((0, 3, 0), -0.5, sc.diffuse_light((2.0, 1.0, 0.5)))  # (|r| counts)
    sc.sphere((1, 3, 0), 0.5, sc.diffuse_light((0.0, 0.0, 0.0)))  # no power
    sc.sphere((2, 3, 0), 0.5, sc.diffuse_light(sc.image_texture(np.full((2, 2, 3), 255, np.uint8))))
    sc.triangle((0, 4, 0), (1, 4, 0), (0, 4, 1), sc.diffuse_light((5.0, 5.0, 5.0)))
    L = sc.lights()
    assert len(L) == len(before) + 1 and s1 in L["prim"]
    sph = L[L["prim"] == s1][0]
    assert sph["shape"] == rtmi.PRIM_SPHERE and sph["area"] == pytest.approx(4 * np.pi * 0.25, rel=1e-6)
    power = L["area"] * 0.5 * (lum(L["emission"]) + lum(L["emission_odd"]))
    np.testing.assert_allclose(L["probability"], power / power.sum(), rtol=1e-5)
    assert abs(L["probability"].sum() - 1.0) < 1e-6
    assert len(rtmi.Scene.rtiow(7, 32, 18, 1, 4).lights()) == 0


def _all_scenes():
    return sorted(glob.glob(os.path.join(SCENES, "*.json")) + glob.glob(os.path.join(GOLDEN, "*.json")))


@pytest.mark.parametrize("path", _all_scenes(), ids=os.path.basename)
def test_tables_unchanged_when_off_and_grown_when_on(rtmi, path):
    try:
        sc = rtmi.Scene.load(path)
    except rtmi.RtmiError:
        pytest.skip("scene needs files that are not shipped")
    img, info = sc.table_image().copy(), sc.table_info()
    sc.set_light_sampling(True)
    on, info_on = sc.table_image().copy(), sc.table_info()
    if len(sc.lights()) == 0:
        assert np.array_equal(on.view(np.uint32), img.view(np.uint32)) and info_on.kernel_variant == info.kernel_variant
    else:
        assert on.shape[0] > img.shape[0] and info_on.kernel_variant & 256
        assert info_on.kernel_variant & 255 in (16, 36, 44)
    sc.set_light_sampling(False)
    assert np.array_equal(sc.table_image().view(np.uint32), img.view(np.uint32))
    assert sc.table_info().kernel_variant == info.kernel_variant


def test_sphere_only_scene_with_a_light_gets_the_wide_tables(rtmi):
    sc = rtmi.Scene.load(os.path.join(SCENES, "three_sphere.json"))
    assert sc.table_info().kernel_variant in (2, 6)
    sc.sphere((0, 3, 0), 0.5, sc.diffuse_light((4.0, 4.0, 4.0)))
    v_off = sc.table_info().kernel_variant
    sc.set_light_sampling(True)
    assert sc.table_info().kernel_variant & 255 in (16, 36, 44) and sc.table_info().kernel_variant & 256 and v_off in (2, 6)
