"""The glossy materials (GGX rough metal, coated plastic) in every render family, against the fp64 statement of
ref64.py and ref64_glossy.py, sample by sample on the same draws: criteria (a) - (d) of test_gpu_nee_reference.py with per_sample's
thresholds, on the six cases of glossy_scenes.py.  The (b) baseline is the plain kernel on the case's twin -- every glossy
material replaced by lambertian of the same texture (or of F0), light sampling off, environment, media and movers cleared --
against the twin's reference.  Each case asserts from the reference's signatures that it contains the vertices it is there for.

(d): the reference's draws stay within REF_DRAWS, and a reference with a deliberate mistake -- the attenuation without G2 / G1,
plastic's lobe draw taken last, the light sample's f cos taken as albedo x pdf_b -- is far from 97 % against the kernel.

Then what every feature keeps: the same bytes in every layout, through a sample split and from the product library; the feature
buffers; ray queries; the command line on the shipped scene; and light sampling against the plain estimator.

Every case prints one row of figures (pytest -s); DESIGN 7m holds the rows measured on the MI355X."""
import numpy as np
import pytest

import glossy_scenes as GS
import nee_scenes as NS
import per_sample as PS
import ref64 as R
import ref64_glossy as G

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
    tally = cases(name)[3][3]
    print("    " + ", ".join(f"{k} {tally[k]}" for k in G.GLOSSY_KEYS if tally[k]))


@pytest.mark.parametrize("name,mistake", [("glossy_sky", "g1_for_g2"), ("glossy_sky", "lobe_draw_last"), ("glossy_lights", "nee_albedo_pdf")])
def test_a_mistake_fails_the_agreement(inputs, cases, name, mistake):
    PS.check_a_mistake_fails_the_agreement(inputs, cases, name, mistake)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    PS.check_same_bytes(rtmi, GS, ("glossy_sky", "glossy_lights"), tmp_path)
    PS.check_compact_layouts_refuse(rtmi, lambda: GS.scene(rtmi, "glossy_sky"))


def test_feature_buffers_show_the_first_vertex(rtmi, inputs):
    """one-sample feature passes of glossy_mesh against the reference's first vertex of sample 0 of every pixel: albedo = F0 /
    rho exactly (through the 2^-24 quantisation of a pixel sum), the normal = the interpolated shading normal within 1e-4 per
    component (the per-sample tolerance: the fp32 interpolation carries the plane point's error, a few 1e-6 at these sizes)"""
    name = "glossy_mesh"
    sc = GS.scene(rtmi, name)
    words, _ = inputs(name)
    n = NS.REF_W * NS.REF_H
    probe, probe32 = {}, {}
    R.trace(R.RefScene(sc), words[:n], probe=probe)
    R.trace(R.RefScene(sc), words[:n], dtype=np.float32, probe=probe32)
    o = rtmi.Opts(seed=GS.seed_of(name), sample_first=0, sample_count=1)
    albedo = sc.render_feature(rtmi.FEATURE_ALBEDO, o).reshape(-1, 3).astype(np.float64)
    normal = sc.render_feature(rtmi.FEATURE_NORMAL, o).reshape(-1, 3).astype(np.float64)
    on = probe["glossy"] & probe32["glossy"]
    assert on.sum() >= 200, on.sum()
    quant = lambda v: np.rint(v.astype(np.float32).astype(np.float64) * 2.0 ** 24) / 2.0 ** 24
    # (where both precisions read the same texel: a (u, v) on a texel's border may fall either way)
    same = on & (probe["albedo"].astype(np.float32) == probe32["albedo"]).all(axis=1)
    assert same.sum() >= 0.98 * on.sum(), (same.sum(), on.sum())
    assert np.array_equal(albedo[same], quant(probe["albedo"][same]))
    err = np.abs(normal[on] - probe["normal"][on]).max(axis=1)
    print(f"\nfeature pass of {name}: {on.sum()} glossy pixels, albedo exact on {same.sum()}, max |normal - fp64| {err.max():.2e}")
    assert (err <= 1e-4).mean() >= 0.99, float((err <= 1e-4).mean())


def test_ray_queries_report_the_twins_records(rtmi):
    """Scene.trace on glossy_mesh returns the records of its lambertian twin: a query never looks at what a material does"""
    sc, twin = GS.scene(rtmi, "glossy_mesh"), GS.scene(rtmi, "glossy_mesh", glossy=False)
    a, hit = PS.check_ray_queries_of_twins(sc, twin, lambda prims: [p for p in prims if int(p["type"]) != R.XZ_RECT])
    kinds = sc.materials()["type"][a["material"][hit]]
    assert set(np.unique(kinds)) >= {G.ROUGH_METAL, G.PLASTIC}, np.unique(kinds)
    assert not np.isin(twin.materials()["type"], (G.ROUGH_METAL, G.PLASTIC)).any()


def test_the_cli_renders_the_shipped_scene(rtmi, tmp_path):
    PS.check_cli(rtmi, tmp_path, "glossy_balls.json", True, GS.NEE)


def test_light_sampling_is_unbiased_against_the_plain_estimator(rtmi):
    """glossy_lights at 64 x 36 x 256 spp with and without light sampling: equal frame and block means, by the test
    test_gpu_light_sampling.py uses (8 seeds each; c_max: the brightest emission over the roulette's survival probability)"""
    from test_gpu_light_sampling import compare, seeds_of
    sc = GS.lights(rtmi, w=64, h=36, spp=256)
    compare(seeds_of(rtmi, sc), seeds_of(rtmi, sc, nee=True), "glossy_lights", c_max=7.0 / 0.9)
