"""Rough glass (GGX transmission with a Beer-Lambert tint) in every render family, against the fp64 statement of
ref64.py and ref64_glass.py, sample by sample on the same draws: criteria (a) - (d) of test_gpu_nee_reference.py with per_sample's
thresholds, on the six cases of glass_scenes.py.  The (b) baseline is the plain kernel on the case's twin -- every rough_glass
replaced by dielectric of the same ir, light sampling off, environment, media and movers cleared -- against the twin's
reference: the precision baseline for refractive paths.  Each case asserts from the reference's signatures (and the wrapper's
log) that it contains the vertices it is there for.

(d): the reference's draws stay within REF_DRAWS, and a reference with one of the five deliberate mistakes of ref64_glass is
far from 97 % against the kernel.

Then a known answer (a camera at the centre of a tinted ball), and what every feature keeps: the same bytes in every layout,
through a sample split and from the product library; the feature buffers; ray queries; the command line on the shipped scene;
and light sampling against the plain estimator.

Every case prints one row of figures (pytest -s); DESIGN 7r holds the rows measured on the MI355X."""
import numpy as np
import pytest

import glass_scenes as GS
import nee_scenes as NS
import per_sample as PS
import ref64 as R
import ref64_glass as GL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    return PS.input_cache(rtmi, GS)


@pytest.fixture(scope="module")
def cases(rtmi, inputs):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)): rendered and traced once, shared by the tests"""
    return PS.case_cache(rtmi, GS, inputs)


@pytest.mark.parametrize("name", list(GS.CASES))
def test_kernel_against_fp64(rtmi, inputs, cases, name):
    PS.check_kernel_against_fp64(rtmi, GS, inputs, cases, name)
    print("    " + ", ".join(f"{k[6:]} {v}" for k, v in cases(name)[3][3].items() if k.startswith("glass_") and not isinstance(v, list) and v))


@pytest.mark.parametrize("name,mistake", GS.MISTAKES)
def test_a_mistake_fails_the_agreement(inputs, cases, name, mistake):
    PS.check_a_mistake_fails_the_agreement(inputs, cases, name, mistake)


def test_known_answer_from_the_centre_of_a_tinted_ball(rtmi):
    """A camera at the centre of a tinted ball of radius 2 (r = 0, ir = 1.5, constant background B, max_depth 2), 32 x 18 x 64:
    every camera ray meets the ball from inside at normal incidence after the distance 2.  It refracts with probability
    1 - F0 and then leaves with Tr B G2 / G1; reflected, it meets the ball again and ends black at depth 0.  The frame mean is
    (1 - F0) exp(-sigma 2) B G2 / G1, within 4 standard errors of the binomial choice (alpha = 1e-3 tilts h by ~1e-3: c = 1 to
    1e-6).  F0 and G2 / G1 (= 1: Lambda vanishes along the normal) come from the fp64 model at normal incidence."""
    ir, radius, sigma, B, spp = 1.5, 2.0, np.array([0.1, 0.3, 0.6]), np.array([0.8, 0.9, 1.0]), 64
    sc = rtmi.Scene.new(32, 18, spp, 2)
    sc.set_background(tuple(B), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0, 1, 0), 40.0)
    sc.sphere((0.0, 0.0, 0.0), radius, sc.rough_glass(ir, 0.0, tuple(sigma)))
    img = sc.render(rtmi.Opts(seed=11)).reshape(-1, 3).astype(np.float64) / spp
    one = np.ones(1)
    F0 = float(GL.fresnel(np.array([ir]), one)[0][0])
    up, down = np.array([[0.0, 0.0, 1.0]]), np.array([[0.0, 0.0, -1.0]])
    lo, li = GL.G.ggx_lambda(np.array([1e-3]), up), GL.G.ggx_lambda(np.array([1e-3]), down)
    ratio = float(((1 + lo) / (1 + lo + li))[0])
    value = np.exp(-sigma.astype(np.float32).astype(np.float64) * radius) * B.astype(np.float32).astype(np.float64) * ratio
    n = 32 * 18 * spp
    want, se = (1 - F0) * value, value * np.sqrt(F0 * (1 - F0) / n)
    got = img.mean(axis=0)
    print(f"\ntinted ball from inside: frame mean {got}, expected {want}, in standard errors {(got - want) / se}")
    assert ratio == 1.0 and (np.abs(got - want) <= 4 * se).all(), (got, want, se)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    PS.check_same_bytes(rtmi, GS, ("glass_sky", "glass_lights"), tmp_path)
    PS.check_compact_layouts_refuse(rtmi, lambda: GS.scene(rtmi, "glass_sky"))


def test_feature_buffers_show_the_first_vertex(rtmi, inputs):
    """one-sample feature passes of glass_mesh against the reference's first vertex of sample 0 of every pixel: albedo exactly 1
    on the glass pixels, the normal = the bumped, interpolated shading normal within 1e-4 per component on every pixel that is
    glass at both precisions (measured: 1.9e-5 at most)"""
    name = "glass_mesh"
    sc = GS.scene(rtmi, name)
    words, _ = inputs(name)
    n = NS.REF_W * NS.REF_H
    probe, probe32 = {}, {}
    R.trace(R.RefScene(sc), words[:n], probe=probe)
    R.trace(R.RefScene(sc), words[:n], dtype=np.float32, probe=probe32)
    o = rtmi.Opts(seed=GS.seed_of(name), sample_first=0, sample_count=1)
    albedo = sc.render_feature(rtmi.FEATURE_ALBEDO, o).reshape(-1, 3).astype(np.float64)
    normal = sc.render_feature(rtmi.FEATURE_NORMAL, o).reshape(-1, 3).astype(np.float64)
    on = probe["glossy"] & probe32["glossy"]  # (the torus: the only glossy surface)
    assert on.sum() >= 100, on.sum()
    assert (albedo[on] == 1.0).all()
    err = np.abs(normal[on] - probe["normal"][on]).max(axis=1)
    print(f"\nfeature pass of {name}: {on.sum()} glass pixels, albedo 1 on all, max |normal - fp64| {err.max():.2e}, "
          f"within 1e-4 on {100 * (err <= 1e-4).mean():.2f} %")
    assert (err <= 1e-4).all(), float(err.max())


def test_ray_queries_report_the_twins_records(rtmi):
    """Scene.trace on glass_mesh and glass_sky returns the records of the dielectric twin: a query never looks at what a
    material does"""
    for name in ("glass_mesh", "glass_sky"):
        sc, twin = GS.scene(rtmi, name), GS.scene(rtmi, name, glass=False)
        a, hit = PS.check_ray_queries_of_twins(sc, twin, lambda prims: [p for p in prims if int(p["type"]) not in (R.XZ_RECT, 6)])
        kinds = sc.materials()["type"][a["material"][hit]]
        assert GL.ROUGH_GLASS in set(np.unique(kinds)) and not (twin.materials()["type"] == GL.ROUGH_GLASS).any()


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_the_cli_renders_the_shipped_scene(rtmi, tmp_path, nee):
    PS.check_cli(rtmi, tmp_path, "frosted_glass.json", nee, GS.NEE)


def test_light_sampling_is_unbiased_against_the_plain_estimator(rtmi):
    """glass_lights at 64 x 36 x 256 spp with and without light sampling: equal frame and block means, by the test
    test_gpu_light_sampling.py uses (8 seeds each; c_max: the brightest emission over the roulette's survival probability)"""
    from test_gpu_light_sampling import compare, seeds_of
    sc = GS.lights(rtmi, w=64, h=36, spp=256)
    compare(seeds_of(rtmi, sc), seeds_of(rtmi, sc, nee=True), "glass_lights", c_max=14.0 / 0.9)
