"""Bump mapping in every render family, against the fp64 statement of ref64.py with ref64_bump.py installed, sample by
sample on the same draws: criteria (a) - (d) of test_gpu_nee_reference.py with per_sample's thresholds, on the six cases of
bump_scenes.py.  The (b) baseline is the plain kernel on the case's twin -- every bump removed, light sampling off, environment,
media and movers cleared -- against the twin's reference.  Each case asserts from ref64_bump.tally that it contains the vertices
it is there for and that 15 % of its samples touch a bumped vertex.

(d): the reference's draws stay within REF_DRAWS, and a reference with a deliberate mistake -- no perturbation, the full gradient
in place of its tangential part, an unsigned back face, the cubic fade's derivative -- is far from 97 % against the kernel.  These
tests fail without the feature and with a wrong gradient or rule in the kernel.

Then what every feature keeps: the same bytes in every layout, through a sample split and from the product library; the
refusals; the nested grid; the feature buffers; ray queries; the command line on the shipped scene; and light sampling against
the plain estimator.

Every case prints one row of figures (pytest -s); DESIGN 7p holds the rows measured on the MI355X."""
import numpy as np
import pytest

import bump_scenes as BS
import nee_scenes as NS
import per_sample as PS
import ref64 as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    return PS.input_cache(rtmi, BS)


@pytest.fixture(scope="module")
def cases(rtmi, inputs):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)): rendered and traced once, shared by the tests"""
    return PS.case_cache(rtmi, BS, inputs)


@pytest.mark.parametrize("name", list(BS.CASES))
def test_kernel_against_fp64(rtmi, inputs, cases, name):
    PS.check_kernel_against_fp64(rtmi, BS, inputs, cases, name)
    bump_tally = {k: v for k, v in cases(name)[3][3].items() if k.startswith("bump_")}
    print("    " + ", ".join(f"{k} {v if isinstance(v, int) else round(v, 3)}" for k, v in bump_tally.items() if v))


@pytest.mark.parametrize("name,mistake", BS.MISTAKES)
def test_a_mistake_fails_the_agreement(inputs, cases, name, mistake):
    PS.check_a_mistake_fails_the_agreement(inputs, cases, name, mistake)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    PS.check_same_bytes(rtmi, BS, ("bump_sky", "bump_lights"), tmp_path, twin=lambda name: BS.scene(rtmi, name, bump=False))


def test_refusals(rtmi):
    # the compact layouts list spheres for the sphere-only kernels, which know no bump: refused
    for variant in (2, 6):
        with pytest.raises(rtmi.RtmiError):
            BS.scene(rtmi, "bump_sky").render(rtmi.Opts(variant=variant))
    # a bumped mover: the relief would swim through the ball
    sc = BS.scene(rtmi, "bump_motion")
    mover_material = int(sc.moving_spheres()["material"][0])
    height = sc.noise_texture((0, 0, 0), (1, 1, 1), **BS.H_FBM)
    sc.set_bump(mover_material, height, 0.2)
    assert "moving sphere" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(sample_count=1)))
    sc.set_bump(mover_material, -1, 0.0)
    sc.render(rtmi.Opts(sample_count=1))


def test_the_nested_grid_renders_the_same_bytes(rtmi):
    """bump_prims with set_nested_grid() has no cell that nests (its tables stay flat: the same kernel, the same bytes), so the
    nested-grid kernel gets a fixture that does: bump_scenes.nested, a bumped smooth clump.  Layout 52 gives the bytes of the flat
    wide-table walk of the same scene, which is the code test_kernel_against_fp64 holds to fp64 per sample"""
    sc, st = BS.scene(rtmi, "bump_prims"), rtmi.Stats()
    flat = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    sc.set_nested_grid(True)
    assert sc.nested_info().cells == 0
    assert np.array_equal(sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st), flat) and st.kernel_variant in PS.GENERAL_LAYOUTS
    sc = BS.nested(rtmi)
    assert sc.nested_info().cells > 0
    nested = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant == PS.NESTED_LAYOUT
    twin = BS.nested(rtmi, bump=False).render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert not np.array_equal(nested, twin)  # (the bumps show)
    sc.set_nested_grid(False)
    flat = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant in PS.GENERAL_LAYOUTS and np.array_equal(nested, flat)


def test_feature_buffers_show_the_bumped_normal(rtmi, inputs):
    """one-sample feature passes of bump_prims: the normal buffer against the reference's first-vertex n' (probe["normal"]) within
    1e-4 per component -- the per-sample tolerance -- on at least 99 % of the bumped pixels (a guard may fall either way where
    n' . d is within rounding of 0), and it is not the twin's; albedo and depth are the twin's, byte for byte"""
    name = "bump_prims"
    sc, twin = BS.scene(rtmi, name), BS.scene(rtmi, name, bump=False)
    words, _ = inputs(name)
    n = NS.REF_W * NS.REF_H
    S, probe = R.RefScene(sc), {}
    _, sig, _ = R.trace(S, words[:n], probe=probe)
    prim = sig[:, R.SAMPLE_COLUMNS + R.C_PRIM]
    mat = np.where(prim >= 0, S.prims["material"][np.clip(prim, 0, None)], -1)
    bumped = np.isin(mat, [m for m in range(len(S.mats)) if sc.bump(m) is not None])
    assert bumped.sum() >= 300, bumped.sum()
    o = rtmi.Opts(seed=BS.seed_of(name), sample_first=0, sample_count=1)
    normal = sc.render_feature(rtmi.FEATURE_NORMAL, o).reshape(-1, 3).astype(np.float64)
    flat = twin.render_feature(rtmi.FEATURE_NORMAL, o).reshape(-1, 3).astype(np.float64)
    err = np.abs(normal[bumped] - probe["normal"][bumped]).max(axis=1)
    moved = np.abs(normal[bumped] - flat[bumped]).max(axis=1)
    print(f"\nfeature pass of {name}: {bumped.sum()} bumped pixels, max |normal - fp64| {err.max():.2e}, within 1e-4: {100 * (err <= 1e-4).mean():.2f} %, "
          f"median |normal - twin's| {np.median(moved):.3f}")
    assert (err <= 1e-4).mean() >= 0.99, float((err <= 1e-4).mean())
    assert np.median(moved) > 0.01
    assert np.abs(normal[~bumped] - flat[~bumped]).max() == 0
    for feature in (rtmi.FEATURE_ALBEDO, rtmi.FEATURE_DEPTH):
        assert sc.render_feature(feature, o).tobytes() == twin.render_feature(feature, o).tobytes(), feature


def test_ray_queries_report_the_twins_records(rtmi):
    """Scene.trace on bump_prims returns the records of its unbumped twin: queries are for geometry"""
    sc, twin = BS.scene(rtmi, "bump_prims"), BS.scene(rtmi, "bump_prims", bump=False)
    a, hit = PS.check_ray_queries_of_twins(sc, twin, lambda prims: prims[1:])  # (every primitive but the far floor)
    assert sum(sc.bump(int(m)) is not None for m in a["material"][hit]) >= 300


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_the_cli_renders_the_shipped_scene(rtmi, tmp_path, nee):
    PS.check_cli(rtmi, tmp_path, "bumpy_pond.json", nee, BS.NEE)


def test_light_sampling_is_unbiased_against_the_plain_estimator(rtmi):
    """bump_lights at 64 x 36 x 256 spp with and without light sampling: equal frame and block means, by the test and the bounds
    test_gpu_light_sampling.py uses (8 seeds each; c_max: the brightest emission, the sphere light's 7.0, over the roulette's
    survival probability)"""
    from test_gpu_light_sampling import compare, seeds_of
    sc = BS.lights(rtmi, w=64, h=36, spp=256)
    compare(seeds_of(rtmi, sc), seeds_of(rtmi, sc, nee=True), "bump_lights", c_max=7.0 / 0.9)
