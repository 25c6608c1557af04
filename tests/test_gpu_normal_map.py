"""Tangent-space normal maps in every render family, against the fp64 statement of ref64.py with
ref64_normal_map.py installed, sample by sample on the same draws: criteria (a) - (d) of test_gpu_nee_reference.py with
per_sample's thresholds, on the six cases of normal_map_scenes.py.  The (b) baseline is the plain kernel on the case's twin --
every map removed, light sampling off, environment, media, movers and analytic lights cleared -- against the twin's reference.
Each case asserts from ref64_normal_map.tally that it contains the vertices it is there for and that 15 % of its samples touch
a mapped vertex.

(d): the reference's draws stay within REF_DRAWS, and a reference with a deliberate mistake -- no perturbation, T and B swapped,
an unsigned back face, the frame not re-orthogonalised about a smooth triangle's n, glTF's 2c - 1 decoding -- is far from 97 %
against the kernel.  These tests fail without the feature and with a wrong frame or rule in the kernel.

A known answer that does not rest on the fp64 statement: with every map a constant (128, 128, 255) image -- the texel that
leaves n untouched -- the mapped path (the (u, v), the texel fetch, the branch) runs and the frame is the twin's, byte for byte.

Then what every feature keeps: the same bytes in every layout, through a sample split and from the product library; the
refusals; the nested grid; the feature buffers; ray queries; the command line on the shipped scene; and light sampling against
the plain estimator.

Every case prints one row of figures (pytest -s); DESIGN 7u holds the rows measured on the MI355X."""
import numpy as np
import pytest

import nee_scenes as NS
import normal_map_scenes as NMS
import per_sample as PS
import ref64 as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    return PS.input_cache(rtmi, NMS)


@pytest.fixture(scope="module")
def cases(rtmi, inputs):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)): rendered and traced once, shared by the tests"""
    return PS.case_cache(rtmi, NMS, inputs)


@pytest.mark.parametrize("name", list(NMS.CASES))
def test_kernel_against_fp64(rtmi, inputs, cases, name):
    map_tally = {k: v for k, v in cases(name)[3][3].items() if k.startswith("nm_")}
    print("\n    " + ", ".join(f"{k} {v if isinstance(v, int) else round(v, 3)}" for k, v in map_tally.items() if v))
    PS.check_kernel_against_fp64(rtmi, NMS, inputs, cases, name)


@pytest.mark.parametrize("name,mistake", NMS.MISTAKES)
def test_a_mistake_fails_the_agreement(inputs, cases, name, mistake):
    PS.check_a_mistake_fails_the_agreement(inputs, cases, name, mistake)


@pytest.mark.parametrize("name", ["nm_sky", "nm_lights"])
def test_a_constant_map_renders_the_twins_bytes(rtmi, name):
    """every map replaced by a constant (128, 128, 255) image: such a texel leaves n untouched, so the frame is the twin's in
    every general layout -- and the maps were read: the material word is set, the scene packs to other bytes"""
    still, twin = NMS.scene(rtmi, name, maps="flat"), NMS.scene(rtmi, name, maps=False)
    assert sum(still.normal_map(m) is not None for m in range(len(still.materials()))) >= 4
    assert still.table_image().tobytes() != twin.table_image().tobytes()
    st = rtmi.Stats()
    for variant in PS.GENERAL_LAYOUTS:
        o = rtmi.Opts(seed=NMS.seed_of(name), sample_count=NS.REF_K, variant=variant)
        a = still.render(o, st)
        assert st.kernel_variant == variant | NMS.family(name), (variant, st.kernel_variant)
        b = twin.render(o, st)
        assert st.kernel_variant == variant | NMS.family(name), (variant, st.kernel_variant)
        assert a.tobytes() == b.tobytes(), (name, variant, float(np.abs(a - b).max()))
    assert not np.array_equal(NMS.scene(rtmi, name).render(rtmi.Opts(seed=NMS.seed_of(name), sample_count=NS.REF_K), st), b)  # (a relief shows)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    PS.check_same_bytes(rtmi, NMS, ("nm_sky", "nm_lights"), tmp_path)


def test_refusals(rtmi):
    # the compact layouts list spheres for the sphere-only kernels, which know no map: refused
    for variant in (2, 6):
        with pytest.raises(rtmi.RtmiError):
            NMS.scene(rtmi, "nm_sky").render(rtmi.Opts(variant=variant))
    # a mapped mover: the relief would swim through the ball
    sc = NMS.scene(rtmi, "nm_motion")
    mover_material = int(sc.moving_spheres()["material"][0])
    sc.set_normal_map(mover_material, sc.image_texture(NMS.relief(**NMS.M_WAVES)), 1.0)
    assert "moving sphere" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(sample_count=1)))
    sc.set_normal_map(mover_material, -1, 0.0)
    sc.render(rtmi.Opts(sample_count=1))


def test_the_nested_grid_renders_the_same_bytes(rtmi):
    """normal_map_scenes.nested, a mapped smooth clump whose cell nests: layout 52 gives the bytes of the flat wide-table walk
    of the same scene, which is the code test_kernel_against_fp64 holds to fp64 per sample"""
    st = rtmi.Stats()
    sc = NMS.nested(rtmi)
    assert sc.nested_info().cells > 0
    nested = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant == PS.NESTED_LAYOUT
    twin = NMS.nested(rtmi, maps=False).render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert not np.array_equal(nested, twin)  # (the maps show)
    sc.set_nested_grid(False)
    flat = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant in PS.GENERAL_LAYOUTS and np.array_equal(nested, flat)


def test_feature_buffers_show_the_mapped_normal(rtmi, inputs):
    """one-sample feature passes of nm_prims: the normal buffer against the reference's first-vertex n' (probe["normal"]) within
    1e-4 per component -- the per-sample tolerance -- on EVERY mapped pixel, and it is not the twin's.  The one exception is a
    guard that falls the other way in fp32 (n' . d or n' . g within rounding of 0): such a pixel must then show exactly the twin's
    unmapped normal, the guard having kept n.  (Measured: all 544 mapped pixels within 1e-4, largest 2.4e-5, no exception used.)
    Albedo and depth are the twin's, byte for byte"""
    name = "nm_prims"
    sc, twin = NMS.scene(rtmi, name), NMS.scene(rtmi, name, maps=False)
    words, _ = inputs(name)
    n = NS.REF_W * NS.REF_H
    S, probe = R.RefScene(sc), {}
    _, sig, _ = R.trace(S, words[:n], probe=probe)
    prim = sig[:, R.SAMPLE_COLUMNS + R.C_PRIM]
    mat = np.where(prim >= 0, S.prims["material"][np.clip(prim, 0, None)], -1)
    mapped = np.isin(mat, [m for m in range(len(S.mats)) if sc.normal_map(m) is not None])
    assert mapped.sum() >= 300, mapped.sum()
    o = rtmi.Opts(seed=NMS.seed_of(name), sample_first=0, sample_count=1)
    normal = sc.render_feature(rtmi.FEATURE_NORMAL, o).reshape(-1, 3).astype(np.float64)
    flat = twin.render_feature(rtmi.FEATURE_NORMAL, o).reshape(-1, 3).astype(np.float64)
    err = np.abs(normal[mapped] - probe["normal"][mapped]).max(axis=1)
    moved = np.abs(normal[mapped] - flat[mapped]).max(axis=1)
    print(f"\nfeature pass of {name}: {mapped.sum()} mapped pixels, max |normal - fp64| {err.max():.2e}, within 1e-4: {100 * (err <= 1e-4).mean():.2f} %, "
          f"median |normal - twin's| {np.median(moved):.3f}")
    out = err > 1e-4
    kept = (normal[mapped] == flat[mapped]).all(axis=1)
    print(f"outside 1e-4: {out.sum()}, of them showing the twin's normal: {(out & kept).sum()}")
    assert not (out & ~kept).any(), (int(out.sum()), float(err[out & ~kept].max()))
    assert np.median(moved) > 0.01
    assert np.abs(normal[~mapped] - flat[~mapped]).max() == 0
    for feature in (rtmi.FEATURE_ALBEDO, rtmi.FEATURE_DEPTH):
        assert sc.render_feature(feature, o).tobytes() == twin.render_feature(feature, o).tobytes(), feature


def test_ray_queries_report_the_twins_records(rtmi):
    """Scene.trace on nm_prims returns the records of its twin without maps: queries are for geometry"""
    sc, twin = NMS.scene(rtmi, "nm_prims"), NMS.scene(rtmi, "nm_prims", maps=False)
    # (every primitive but the far floor; the box's faces lie among them)
    a, hit = PS.check_ray_queries_of_twins(sc, twin, lambda prims: [p for p in prims[1:] if int(p["type"]) != 6])
    assert sum(sc.normal_map(int(m)) is not None for m in a["material"][hit]) >= 300


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_the_cli_renders_the_shipped_scene(rtmi, tmp_path, nee):
    PS.check_cli(rtmi, tmp_path, "normal_map_wall.json", nee, NMS.NEE,
                 loaded=lambda sc: sum(sc.normal_map(m) is not None for m in range(len(sc.materials()))) >= 5)


def test_light_sampling_is_unbiased_against_the_plain_estimator(rtmi):
    """nm_lights' area light at 64 x 36 x 256 spp with and without light sampling: equal frame and block means, by the test and
    the bounds test_gpu_light_sampling.py uses (8 seeds each; c_max: the brightest emission, 6.0, over the roulette's survival
    probability).  The point light is taken out: the plain estimator cannot see a light without area"""
    from test_gpu_light_sampling import compare, seeds_of
    sc = NMS.lights(rtmi, w=64, h=36, spp=256)
    sc.clear_analytic_lights()
    compare(seeds_of(rtmi, sc), seeds_of(rtmi, sc, nee=True), "nm_lights", c_max=6.0 / 0.9)
