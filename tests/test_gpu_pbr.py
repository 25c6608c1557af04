"""The metallic-roughness material on the MI355X, against the fp64 statement of ref64.py and ref64_pbr.py, sample by
sample on the same draws: criteria (a) - (d) of test_gpu_nee_reference.py with per_sample's thresholds, on the four cases of
pbr_scenes.py (48 x 27 x 13 one-sample frames each).  The (b) baseline is the plain kernel on the case's twin -- every pbr
material replaced by a lambertian of its base texture, light sampling off -- against the twin's reference.  Each case asserts
from the wrapper's log that it contains the vertices it is about.

(d): a reference with one of the four deliberate mistakes of ref64_pbr is far from 97 % against the kernel.

Then the independent twin (m = 0 against UNMODIFIED ref64 on the plastic twin), known answers (m = 1 against the rough_metal
twin, linearity in m8, a checker ORM map against its two constant materials), and what every feature keeps: the same bytes in
every layout, through a sample split and from the product library; the albedo feature; ray queries; the media and motion
families; the command line on the shipped scene.

Every case prints one row of figures (pytest -s); DESIGN 7t holds the rows measured on the MI355X."""
import numpy as np
import pytest

import nee_scenes as NS
import pbr_scenes as PBS
import per_sample as PS
import ref64 as R
import ref64_pbr as RP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    return PS.input_cache(rtmi, PBS)


@pytest.fixture(scope="module")
def words(inputs):
    return inputs("room")[0]


@pytest.fixture(scope="module")
def cases(rtmi, inputs):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)): rendered and traced once, shared by the tests"""
    return PS.case_cache(rtmi, PBS, inputs)


@pytest.mark.parametrize("name", list(PBS.CASES))
def test_kernel_against_fp64(rtmi, inputs, cases, name):
    PS.check_kernel_against_fp64(rtmi, PBS, inputs, cases, name)
    print("    " + ", ".join(f"{k[4:]} {v}" for k, v in cases(name)[3][3].items() if k.startswith("pbr_") and v))


@pytest.mark.parametrize("name,mistake", PBS.MISTAKES)
def test_a_mistake_fails_the_agreement(inputs, cases, name, mistake):
    PS.check_a_mistake_fails_the_agreement(inputs, cases, name, mistake)


def test_m0_against_unmodified_ref64_on_the_plastic_twin(rtmi, words):
    """with m = 0, no map, base colour and roughness on the 8-bit grid, the kernel's samples of the pbr scene are held per sample to
    ref64 as it stands on the scene whose materials are plastic(c, ior, r): no new reference code is involved.  (The two kernels'
    frames are the same bytes as well: the draws and every operation coincide.)"""
    sc, twin = PBS.grid_scene(rtmi, "pbr0"), PBS.grid_scene(rtmi, "plastic")
    got = PS.kernel_samples(rtmi, sc, NS.REF_SEED, NS.REF_K, PBS.FAMILIES, PBS.NEE)
    ref, stable, draws, tally = R.reference(R.RefScene(twin), words)
    assert draws.max() <= NS.REF_DRAWS and tally["glossy_light_samples"] >= 100 and tally["smooth_glossy_vertices"] >= 50
    of_twin = PS.kernel_samples(rtmi, twin, NS.REF_SEED, NS.REF_K, PBS.FAMILIES, PBS.NEE)
    PS.assert_agreement("pbr at m = 0 against ref64 on plastic", R.judge(got, ref, stable), R.judge(of_twin, ref, stable))
    assert np.array_equal(got, of_twin)


def _frame_means(rtmi, sc, seeds=4):
    return np.array([sc.render(rtmi.Opts(seed=100 + s)).astype(np.float64).mean() / sc.spp for s in range(seeds)])


def _equal_means(tag, a, b):
    """test_gpu_light_sampling.test_analytic_known_answer's criterion: within 3 standard errors + 1e-4, standard errors from 4 seeds"""
    se = np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    print(f"\n{tag}: {a.mean():.6f} against {b.mean():.6f}, standard error {se:.2e}")
    assert abs(a.mean() - b.mean()) < 3 * se + 1e-4, (tag, a.mean(), b.mean(), se)


def test_known_answer_m1_is_the_rough_metal(rtmi):
    """with m = 1 the frame mean of the pbr scene equals the rough_metal(c, r) twin's (the draws differ: pbr takes ul as well)"""
    a = _frame_means(rtmi, PBS.grid_scene(rtmi, "pbr1", w=64, h=36, spp=256))
    b = _frame_means(rtmi, PBS.grid_scene(rtmi, "rough_metal", w=64, h=36, spp=256))
    _equal_means("pbr at m = 1 against rough_metal", a, b)


def test_known_answer_linearity_in_the_metalness(rtmi):
    """one convex pbr sphere on a black background under one quad light, 64 x 36 x 256: at most one pbr vertex per path, so the
    mean at m8 = 128 is (128 / 255) mean(m = 1) + (127 / 255) mean(m = 0)"""
    m0, m128, m255 = (_frame_means(rtmi, PBS.linearity_scene(rtmi, m8)) for m8 in (0, 128, 255))
    assert m0.mean() > 1e-3 and abs(m255.mean() - m0.mean()) > 20 * np.sqrt(m0.var(ddof=1) / 4 + m255.var(ddof=1) / 4)  # (the ends differ)
    _equal_means("m8 = 128 against the blend of the ends", m128, (128 / 255) * m255 + (127 / 255) * m0)


def test_known_answer_a_checker_map_is_its_two_constant_materials(rtmi):
    """A checker ORM map with bytes (G, B) alternating (255, 0) / (26, 255) on a floor quad.  The checker's tiles are cells of a 3-D
    sine lattice (pi / 10 wide), which a pair of quads does not express: so the pixels whose footprint lies wholly inside tiles of
    one class are held to the frame of the constant pbr material of that class on the same quad, by the criterion above (the
    floor is flat and the light absorbs: a path meets the material once, so a pixel depends on its own tile's material alone)."""
    frames = {}
    for which in ("map", "even", "odd"):
        sc = PBS.checker_map_scene(rtmi, which)
        frames[which] = np.stack([sc.render(rtmi.Opts(seed=100 + s)).astype(np.float64).mean(axis=2) / sc.spp for s in range(4)])
    sc = PBS.checker_map_scene(rtmi, "map")
    cam = sc.get_camera()
    org, ll, hor, ver = (np.array(getattr(cam, k)[:], np.float64) for k in ("origin", "lower_left", "horizontal", "vertical"))
    W, H = sc.width, sc.height
    xi = np.array([0.0, 1.0])
    u = (np.arange(W)[None, :, None, None] + xi[None, None, :, None]) / (W - 1)
    v = (np.arange(H)[:, None, None, None] + xi[None, None, None, :]) / (H - 1)
    d = ll + u[..., None] * hor + v[..., None] * ver - org
    t = (PBS.LIFT - org[1]) / d[..., 1]
    p = org + t[..., None] * d
    cell = np.floor(p * 10 / np.pi).astype(np.int64)
    flat = cell.reshape(H, W, 4, 3)
    one_tile = (t > 0).reshape(H, W, 4).all(axis=2) & (flat == flat[:, :, :1]).all(axis=(2, 3)) & (np.abs(p[..., [0, 2]]).reshape(H, W, -1) < 1.95).all(axis=2)
    odd = (flat[:, :, 0].sum(axis=-1) & 1) == 1
    for name, mask in (("even", one_tile & ~odd), ("odd", one_tile & odd)):
        assert mask.sum() >= 150, (name, mask.sum())
        _equal_means(f"checker map, {mask.sum()} pixels of the {name} tiles", frames["map"][:, mask].mean(axis=1), frames[name][:, mask].mean(axis=1))
    # ... and the two classes are different materials: the test could fail
    assert abs(frames["even"][:, one_tile].mean() - frames["odd"][:, one_tile].mean()) > 0.01


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    PS.check_same_bytes(rtmi, PBS, ("room", "maps under an environment"), tmp_path)
    PS.check_compact_layouts_refuse(rtmi, lambda: PBS.scene(rtmi, "room"))


def test_the_albedo_feature_shows_the_bytes(rtmi, words):
    """a one-sample albedo pass of `maps` against the reference's first vertex of sample 0 of every pixel: c8 / 255 (in
    fp32) to the pixel sums' 2^-24 on every pixel that is pbr at both precisions -- image, solid and noise-mapped materials"""
    name = "maps"
    sc = PBS.scene(rtmi, name)
    n = NS.REF_W * NS.REF_H
    probe, probe32 = {}, {}
    R.trace(R.RefScene(sc), words[:n], probe=probe)
    R.trace(R.RefScene(sc), words[:n], dtype=np.float32, probe=probe32)
    albedo = sc.render_feature(rtmi.FEATURE_ALBEDO, rtmi.Opts(seed=NS.REF_SEED, sample_first=0, sample_count=1)).reshape(-1, 3)
    on = probe["glossy"] & probe32["glossy"] & (probe["albedo"] == probe32["albedo"]).all(axis=1)
    assert on.sum() >= 100, on.sum()
    want = probe["albedo"][on].astype(np.float32)  # (a pbr row: c8 / 255 in fp32)
    c8 = np.rint(want.astype(np.float64) * 255)
    assert np.array_equal((c8.astype(np.float32) / np.float32(255)), want)
    assert np.abs(albedo[on].astype(np.float64) - want).max() <= 2.0 ** -24, float(np.abs(albedo[on] - want).max())
    assert len(np.unique(c8, axis=0)) >= 20  # (many texels and the solid colour)


def test_ray_queries_are_unchanged_by_swapping_plastic_for_pbr(rtmi):
    sc, twin = PBS.grid_scene(rtmi, "pbr0"), PBS.grid_scene(rtmi, "plastic")
    a, hit = PS.check_ray_queries_of_twins(sc, twin, lambda prims: [p for p in prims if int(p["type"]) != R.XZ_RECT])
    assert RP.PBR in set(np.unique(sc.materials()["type"][a["material"][hit]]))


@pytest.mark.parametrize("family", ["media", "motion"])
def test_a_pbr_scene_renders_in_the_media_and_motion_families(rtmi, family):
    """one finite frame each, light sampling off, the family's bit in rt_stats.kernel_variant"""
    sc = PBS.scene(rtmi, "plain, bumped")
    if family == "media":
        sc.add_medium_box((-4, 0, -4), (4, 3, 4), 0.15, (0.9, 0.9, 0.9))
    else:
        mapped = int(np.flatnonzero(sc.materials()["type"] == RP.PBR)[1])  # (image base and image map: a mover's (u, v))
        sc.add_moving_sphere((-1.5, 2.4, 1.0), (-1.2, 2.6, 1.0), 0.4, mapped)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=3, sample_count=4), st)
    assert st.kernel_variant & (PBS.MEDIA if family == "media" else PBS.MOTION) and not st.kernel_variant & PBS.NEE, st.kernel_variant
    assert np.isfinite(img).all() and img.mean() > 0


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_the_cli_renders_the_shipped_scene(rtmi, tmp_path, nee):
    PS.check_cli(rtmi, tmp_path, "pbr_wear.json", nee, PBS.NEE)