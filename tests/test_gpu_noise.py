"""The noise textures (fBm, turbulence, marble) in every render family, against the fp64 statement of ref64.py with
ref64_noise.py installed, sample by sample on the same draws: criteria (a) - (d) of test_gpu_nee_reference.py with per_sample's
thresholds, on the six cases of noise_scenes.py.  The (b) baseline is the plain kernel on the case's twin -- every noise texture
replaced by a solid colour, light sampling off, environment, media and movers cleared -- against the twin's reference.  Each case
asserts from the reference's signatures that it contains the vertices it is there for and that 15 % of its samples touch a noise
texture.

(d): the reference's draws stay within REF_DRAWS, and a reference with a deliberate mistake -- the cubic fade, every octave on one
seed, marble's phase along another axis -- is far from 97 % against the kernel.  These tests fail without the feature and with a
wrong hash, fade or octave rule in the kernel.

Then what every feature keeps: the same bytes in every layout, through a sample split and from the product library; the feature
buffers; ray queries; the command line on the shipped scene; and light sampling against the plain estimator.

Every case prints one row of figures (pytest -s); DESIGN 7o holds the rows measured on the MI355X."""
import numpy as np
import pytest

import nee_scenes as NS
import noise_scenes as NSC
import per_sample as PS
import ref64 as R
import ref64_noise as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    return PS.input_cache(rtmi, NSC)


@pytest.fixture(scope="module")
def cases(rtmi, inputs):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)): rendered and traced once, shared by the tests"""
    return PS.case_cache(rtmi, NSC, inputs, nested=("noise_nested",))


@pytest.mark.parametrize("name", list(NSC.CASES))
def test_kernel_against_fp64(rtmi, inputs, cases, name):
    PS.check_kernel_against_fp64(rtmi, NSC, inputs, cases, name)
    print("    " + ", ".join(f"{k} {v}" for k, v in cases(name)[3][3].items() if k.startswith("noise_") and v))


@pytest.mark.parametrize("name,mistake", [("noise_sky", "noise_cubic_fade"), ("noise_sky", "noise_same_seed"), ("noise_lights", "noise_wrong_axis")])
def test_a_mistake_fails_the_agreement(inputs, cases, name, mistake):
    PS.check_a_mistake_fails_the_agreement(inputs, cases, name, mistake)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    PS.check_same_bytes(rtmi, NSC, ("noise_sky", "noise_lights"), tmp_path)
    # the nested clump: its own layout against the flat wide-table walk of the same scene
    sc, st = NSC.scene(rtmi, "noise_nested"), rtmi.Stats()
    nested = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant == NSC.NESTED_LAYOUT
    sc.set_nested_grid(False)
    flat = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant in PS.GENERAL_LAYOUTS and np.array_equal(nested, flat)
    PS.check_compact_layouts_refuse(rtmi, lambda: NSC.scene(rtmi, "noise_sky"))


def test_feature_buffers_show_the_first_vertex(rtmi, inputs):
    """one-sample feature passes of noise_sky: the albedo against the texture values the reference read at its FIRST vertex of
    sample 0 of every pixel (trace()'s probe["texture_value"]), within 1e-4 per channel -- the per-sample tolerance -- on at least 99 % of the noise pixels;
    normal and depth are the twin's, byte for byte"""
    name = "noise_sky"
    sc, twin = NSC.scene(rtmi, name), NSC.scene(rtmi, name, noise=False)
    words, _ = inputs(name)
    n = NS.REF_W * NS.REF_H
    S, probe = R.RefScene(sc), {}
    _, sig, _ = R.trace(S, words[:n], probe=probe)
    prim = sig[:, R.SAMPLE_COLUMNS + R.C_PRIM]
    mtype = np.where(prim >= 0, S.mats["type"][S.prims["material"][np.clip(prim, 0, None)]], -1)
    tex_of = np.where(prim >= 0, S.mats["texture"][S.prims["material"][np.clip(prim, 0, None)]], -1)
    want = np.where(np.isin(mtype, (R.DIFFUSE_LIGHT, R.LAMBERTIAN, R.PLASTIC))[:, None], probe["texture_value"], np.nan)
    noisy = (tex_of >= 0) & (S.texs["type"][np.clip(tex_of, 0, None)] == N.NOISE) & np.isin(mtype, (R.LAMBERTIAN, R.PLASTIC, R.DIFFUSE_LIGHT))
    assert noisy.sum() >= 300 and set(np.unique(mtype[noisy])) == {R.LAMBERTIAN, R.PLASTIC}, noisy.sum()
    o = rtmi.Opts(seed=NSC.seed_of(name), sample_first=0, sample_count=1)
    albedo = sc.render_feature(rtmi.FEATURE_ALBEDO, o).reshape(-1, 3).astype(np.float64)
    err = np.abs(albedo[noisy] - want[noisy]).max(axis=1)
    print(f"\nfeature pass of {name}: {noisy.sum()} noise pixels, max |albedo - fp64| {err.max():.2e}, within 1e-4: {100 * (err <= 1e-4).mean():.2f} %")
    assert (err <= 1e-4).mean() >= 0.99, float((err <= 1e-4).mean())
    assert np.ptp(albedo[noisy], axis=0).min() > 0.3  # (the texture shows: no single colour)
    for feature in (rtmi.FEATURE_NORMAL, rtmi.FEATURE_DEPTH):
        assert sc.render_feature(feature, o).tobytes() == twin.render_feature(feature, o).tobytes(), feature


def test_ray_queries_report_the_twins_records(rtmi):
    """Scene.trace on noise_sky returns the records of its solid-colour twin: a query never looks at a texture"""
    sc, twin = NSC.scene(rtmi, "noise_sky"), NSC.scene(rtmi, "noise_sky", noise=False)
    a, hit = PS.check_ray_queries_of_twins(sc, twin, lambda prims: prims[1:])  # (every primitive but the far floor)
    tex = sc.textures()["type"][sc.materials()["texture"][a["material"][hit]]]
    assert (tex == N.NOISE).sum() >= 300 and not (twin.textures()["type"] == N.NOISE).any()


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_the_cli_renders_the_shipped_scene(rtmi, tmp_path, nee):
    PS.check_cli(rtmi, tmp_path, "marble_hall.json", nee, NSC.NEE)


def test_light_sampling_is_unbiased_against_the_plain_estimator(rtmi):
    """noise_lights at 64 x 36 x 256 spp with and without light sampling: equal frame and block means, by the test
    test_gpu_light_sampling.py uses (8 seeds each; c_max: the brightest emission -- the sphere light's 7.0, above the emitter
    panel's larger colour -- over the roulette's survival probability)"""
    from test_gpu_light_sampling import compare, seeds_of
    sc = NSC.lights(rtmi, w=64, h=36, spp=256)
    c_max = max(7.0, max(NSC.EMITTER_COLOURS[1])) / 0.9
    compare(seeds_of(rtmi, sc), seeds_of(rtmi, sc, nee=True), "noise_lights", c_max=c_max)
