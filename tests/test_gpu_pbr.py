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
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import nee_scenes as NS
import pbr_scenes as PBS
import per_sample as PS
import ref64 as R
import ref64_pbr as RP

pytestmark = pytest.mark.gpu
ROOT = PS.ROOT
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
GENERAL_LAYOUTS = (16, 36, 44)  # a scene with a pbr material runs the general (EXT) builds: never the compact layouts 2 / 6


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def words(rtmi):
    return PBS.inputs(rtmi)


@pytest.fixture(scope="module")
def cases(rtmi, words):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)): rendered and traced once, shared by the tests"""
    made = {}

    def of(name):
        if name not in made:
            sc = PBS.scene(rtmi, name)
            S = R.RefScene(sc)
            st = rtmi.Stats()
            sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=1), st)
            assert st.kernel_variant & ~PBS.FAMILIES in GENERAL_LAYOUTS and st.kernel_variant & PBS.FAMILIES == PBS.family(name), st.kernel_variant
            got = PS.kernel_samples(rtmi, sc, NS.REF_SEED, NS.REF_K, PBS.FAMILIES, PBS.family(name))
            made[name] = (sc, S, got, R.reference(S, words))
        return made[name]
    return of


@pytest.mark.parametrize("name", list(PBS.CASES))
def test_kernel_against_fp64(rtmi, words, cases, name):
    assert len(words) >= 16000
    sc, S, got, (ref, stable, draws, tally) = cases(name)
    assert draws.max() <= NS.REF_DRAWS, draws.max()                                        # (d)
    PBS.check_contents(name, tally)
    plain = PBS.plain_twin(rtmi, name)
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    b = R.judge(PS.kernel_samples(rtmi, plain, NS.REF_SEED, NS.REF_K, PBS.FAMILIES, 0), bref, bstable)
    PS.assert_agreement(name, R.judge(got, ref, stable), b)                                # (a), (b), (c)
    print("    " + ", ".join(f"{k[4:]} {v}" for k, v in tally.items() if k.startswith("pbr_") and v))


@pytest.mark.parametrize("name,mistake", PBS.MISTAKES)
def test_a_mistake_fails_the_agreement(words, cases, name, mistake):
    """(d): against the kernel, a reference with one deliberate mistake of the model is far from 97 %"""
    sc, S, got, (ref, stable, _, _) = cases(name)
    wrong, _, _ = R.trace(S, words, perturb=(mistake,))
    good, bad = R.judge(got, ref, stable), R.judge(got, wrong, stable)
    print(f"\n{name}, {mistake}: within tolerance {100 * good['share']:.2f} % -> {100 * bad['share']:.2f} %")
    PS.assert_perturbation_noticed(good, bad)


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


_PRODUCT = textwrap.dedent("""
    import os, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, os.path.join(%r, "tests"))
    from __graft_entry__ import load_package
    rtmi = load_package()
    assert not rtmi.has_ablations()
    import pbr_scenes as PBS, nee_scenes as NS
    for name in ("room", "maps under an environment"):
        st = rtmi.Stats()
        img = PBS.scene(rtmi, name).render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
        assert st.kernel_variant & PBS.FAMILIES == PBS.family(name), st.kernel_variant
        np.save(os.path.join(sys.argv[1], name.replace(" ", "_") + ".npy"), img)
""") % (ROOT, ROOT)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    env = dict(os.environ, RTMI_LIB=os.path.join(PKG, "librtmi_product.so"))
    p = subprocess.run([sys.executable, "-c", _PRODUCT, str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    for name in ("room", "maps under an environment"):
        sc, fam, seed, st = PBS.scene(rtmi, name), PBS.family(name), NS.REF_SEED, rtmi.Stats()
        ref = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K), st)
        assert st.kernel_variant & PBS.FAMILIES == fam and st.kernel_variant & ~PBS.FAMILIES in GENERAL_LAYOUTS
        for variant in GENERAL_LAYOUTS:
            got = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K, variant=variant), st)
            assert st.kernel_variant == variant | fam, (variant, st.kernel_variant)
            assert np.array_equal(got, ref), (name, variant, float(np.abs(got - ref).max()))
        acc, _ = sc.accumulate(None, rtmi.Opts(seed=seed, sample_first=0, sample_count=5), st)
        assert st.kernel_variant & PBS.FAMILIES == fam
        acc, img = sc.accumulate(acc, rtmi.Opts(seed=seed, sample_first=5, sample_count=NS.REF_K - 5), st)
        assert np.array_equal(img, ref), (name, float(np.abs(img - ref).max()))
        assert np.array_equal(np.load(str(tmp_path / (name.replace(" ", "_") + ".npy"))), ref), name
    # the compact layouts list spheres for the sphere-only kernels, which carry no pbr material: refused
    for variant in (2, 6):
        with pytest.raises(rtmi.RtmiError):
            PBS.scene(rtmi, "room").render(rtmi.Opts(variant=variant))


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
    import trace_cases as TC
    sc, twin = PBS.grid_scene(rtmi, "pbr0"), PBS.grid_scene(rtmi, "plastic")
    boxes = [TC.prim_box(p) for p in sc.prims() if int(p["type"]) != R.XZ_RECT]
    lo, hi = np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)
    o, d = TC.make_rays(lo, hi)
    a, b = sc.trace(o, d), twin.trace(o, d)
    assert (a["prim"] >= 0).sum() >= 500 and a.tobytes() == b.tobytes()
    assert RP.PBR in set(np.unique(sc.materials()["type"][a["material"][a["prim"] >= 0]]))


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
    out = str(tmp_path / "wear.ppm")
    p = subprocess.run([os.path.join(PKG, "rtmi"), "-f", os.path.join(PKG, "scenes", "pbr_wear.json"), "-w", "64", "-h", "36", "-spp", "4",
                        "-o", out, "--no-png"] + (["--nee"] if nee else []), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    sc = rtmi.Scene.load(os.path.join(PKG, "scenes", "pbr_wear.json"))
    sc.override(64, 36, 4)
    sc.set_light_sampling(nee)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(), st)
    assert bool(st.kernel_variant & PBS.NEE) == nee and np.isfinite(img).all() and img.mean() > 0
    tokens = open(out).read().split()  # the reference's text PPM: P3, width, height, 255, then the 8-bit values
    assert tokens[:4] == ["P3", "64", "36", "255"] and len(tokens) == 4 + 64 * 36 * 3
    values = np.array(tokens[4:], np.int64)
    assert values.min() >= 0 and values.max() <= 255 and values.max() > 0
