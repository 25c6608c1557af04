"""Alpha cutouts in every general render family, against the fp64 statement of ref64.py (its opaque_hit is the query
trace() makes), sample by sample on the same draws: criteria (a) - (d) of test_gpu_nee_reference.py with per_sample's
thresholds, on the five cases of alpha_scenes.py.  The (b) baseline is the plain kernel on the case's twin -- every mask
removed, light sampling off, environment, movers and analytic lights cleared -- against the twin's reference.  Each case
asserts its contents from the reference's tally alone (alpha_scenes.check_contents).

(d): the reference's draws stay within REF_DRAWS, and a reference with a deliberate mistake -- masks ignored, the comparison
inverted, the mask read with (u, v) swapped, opaque shadow rays, a pass that uses up a bounce -- is far from 97 % against the
kernel.  These tests fail without the feature.

Known answers that do not rest on the fp64 statement, in every general layout (16, 36, 44): all-opaque masks give the twin's
frame byte for byte while the packed tables differ; all-transparent masks on a set of primitives give the frame of the scene
with those primitives deleted -- deleting changes the tables (other cells, other ids: the tie rule and the walk's order of
roundings stay, but a kernel variant may be chosen differently), so this one is compared per sample at the per-sample
tolerance, not byte for byte; the 70-quad stack shows the 65th quad in its centre pixel.

Then what every feature keeps: the same bytes in every layout, through a sample split and from the product library; the nested
grid; the feature buffers; ray queries; the refusals; the command line on the shipped scene; light sampling against the plain
estimator.

None of the five cases of alpha_scenes.CASES has a grid in its tables: the alpha instances' grid walk, resumed behind a hole,
is held to their linear scan in tests/test_gpu_walk_families.py.

Every case prints one row of figures (pytest -s)."""

import numpy as np
import pytest

import alpha_scenes as AS
import nee_scenes as NS
import per_sample as PS
import ref64 as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    return PS.input_cache(rtmi, AS)


@pytest.fixture(scope="module")
def cases(rtmi, inputs):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)): rendered and traced once, shared by the tests"""
    return PS.case_cache(rtmi, AS, inputs)


@pytest.mark.parametrize("name", list(AS.CASES))
def test_kernel_against_fp64(rtmi, inputs, cases, name):
    print("\n    " + ", ".join(f"{k} {v if isinstance(v, int) else round(v, 3)}" for k, v in cases(name)[3][3].items() if k.startswith("alpha_")))
    PS.check_kernel_against_fp64(rtmi, AS, inputs, cases, name)


@pytest.mark.parametrize("name,mistake", AS.MISTAKES)
def test_a_mistake_fails_the_agreement(inputs, cases, name, mistake):
    PS.check_a_mistake_fails_the_agreement(inputs, cases, name, mistake)


@pytest.mark.parametrize("name", ["al_sky", "al_lights", "al_motion"])
def test_opaque_masks_render_the_twins_bytes(rtmi, name):
    """every mask's plane all 255: no hit is a hole, so the frame is the twin's in every general layout -- and the masks were
    read: the scene packs to other bytes (the mask records)"""
    still, twin = AS.scene(rtmi, name, masks="opaque"), AS.scene(rtmi, name, masks=False)
    assert sum(still.alpha(m) is not None for m in range(len(still.materials()))) >= 2
    assert still.table_image().tobytes() != twin.table_image().tobytes()
    st = rtmi.Stats()
    for variant in PS.GENERAL_LAYOUTS:
        o = rtmi.Opts(seed=AS.seed_of(name), sample_count=NS.REF_K, variant=variant)
        a = still.render(o, st)
        assert st.kernel_variant == variant | AS.family(name), (variant, st.kernel_variant)
        b = twin.render(o, st)
        assert st.kernel_variant == variant | AS.family(name), (variant, st.kernel_variant)
        assert a.tobytes() == b.tobytes(), (name, variant, float(np.abs(a - b).max()))
    assert not np.array_equal(AS.scene(rtmi, name).render(rtmi.Opts(seed=AS.seed_of(name), sample_count=NS.REF_K), st), b)  # (holes show)


@pytest.mark.parametrize("name", ["al_sky", "al_layers", "al_lights"])
def test_clear_masks_render_the_scene_without_those_primitives(rtmi, name):
    """every mask's plane all 0: every masked hit is a hole, so each sample is the sample of the scene with those primitives
    deleted.  Deleting them changes the packed tables (cells, ids, the boxes' extent), and with them the order in which a walk
    meets its candidates: compared per sample at the per-sample tolerance (share within 1e-4 max(1, |ref|) >= 97 %, no bias),
    in every general layout, not byte for byte"""
    clear, gone = AS.scene(rtmi, name, masks="clear"), AS.scene(rtmi, name, masks="deleted")
    assert len(gone.prims()) < len(clear.prims())
    fam, seed = AS.family(name), AS.seed_of(name)
    want = PS.kernel_samples(rtmi, gone, seed, 4, AS.FAMILIES, fam)
    for variant in PS.GENERAL_LAYOUTS:
        got = PS.kernel_samples(rtmi, clear, seed, 4, AS.FAMILIES, fam, variant=variant)
        j = R.judge(got, want, np.ones(len(want), bool))
        print(f"\n{name}, layout {variant}: within {100 * j['share']:.3f} %, max |mean diff| {np.abs(j['mean_diff']).max():.1e}")
        assert j["share"] >= 0.97 and j["bias_ok"], j


def test_the_cap_shows_the_65th_quad(rtmi):
    """70 stacked all-transparent quads in front of a wall under a white background: the centre pixel's camera ray passes
    through 64 and stops on the 65th, whose lambertian colour the frame then shows (its scattered ray leaves through the 64 in
    front, which a new query may pass).  Without the cap it would show the wall"""
    sc = AS.stack(rtmi)
    st = rtmi.Stats()
    for variant in PS.GENERAL_LAYOUTS:
        img = sc.render(rtmi.Opts(seed=5, sample_count=1, variant=variant), st)
        assert st.kernel_variant == variant
        px = img[4, 4].astype(np.float64)
        print(f"\nlayout {variant}: centre pixel {px}")
        assert np.abs(px - np.array(AS.stack_colour(R.CAP))).max() < 1e-4, (variant, px)
        assert np.abs(px - np.array(AS.STACK_WALL)).max() > 0.1
    few = AS.stack(rtmi, n=R.CAP).render(rtmi.Opts(seed=5, sample_count=1), st)[4, 4]
    assert np.abs(few - np.array(AS.STACK_WALL)).max() < 1e-4, few  # (64 quads: all passed, the wall shows)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    PS.check_same_bytes(rtmi, AS, ("al_sky", "al_lights"), tmp_path)


def test_refusals(rtmi):
    # the compact layouts list spheres for the sphere-only kernels, which know no mask
    for variant in (2, 6):
        assert "compact" in PS.refused(rtmi, lambda: AS.scene(rtmi, "al_sky").render(rtmi.Opts(variant=variant)))
    # the counting kernels carry no masks
    assert "counting" in PS.refused(rtmi, lambda: AS.scene(rtmi, "al_sky").count(rtmi.Opts(sample_count=1)))
    # a masked mover: the holes would swim through the ball
    sc = AS.scene(rtmi, "al_motion")
    mover_material = int(sc.moving_spheres()["material"][0])
    mask = sc.image_texture(AS.colours(AS.PLANES["two"]), alpha=AS.PLANES["two"])
    sc.set_alpha(mover_material, mask, 0.5)
    assert "moving sphere" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(sample_count=1)))
    sc.set_alpha(mover_material, -1)
    sc.render(rtmi.Opts(sample_count=1))
    # masks with media: the media kernels draw one free-flight distance per query
    sc = AS.scene(rtmi, "al_sky")
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9))
    assert "media" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(sample_count=1)))
    sc.clear_media()
    sc.render(rtmi.Opts(sample_count=1))


def test_the_nested_grid_renders_the_same_bytes(rtmi):
    """alpha_scenes.nested, a masked clump whose cell nests: layout 52 gives the bytes of the flat wide-table walk of the same
    scene, which is the code test_kernel_against_fp64 holds to fp64 per sample"""
    st = rtmi.Stats()
    sc = AS.nested(rtmi)
    assert sc.nested_info().cells > 0
    tally = AS.nested_tally(rtmi)
    print("\n    " + ", ".join(f"{k} {v if isinstance(v, int) else round(v, 3)}" for k, v in tally.items() if k.startswith("alpha_")))
    AS.check_contents("al_nested", tally)  # (the clump's queries meet masked hits, with both verdicts)
    nested = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant == PS.NESTED_LAYOUT
    twin = AS.nested(rtmi, masks=False).render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert not np.array_equal(nested, twin)  # (the holes show)
    sc.set_nested_grid(False)
    flat = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant in PS.GENERAL_LAYOUTS and np.array_equal(nested, flat)


def test_feature_buffers_show_the_first_opaque_hit(rtmi, inputs):
    """one-sample feature passes of al_layers: depth against the reference's first query (the total t from the camera) and the
    normal against its probe, within 1e-4 (the depth: relative to max(1, t)) on EVERY pixel whose first opaque winner is the
    same primitive in the fp32 and the fp64 reference (at least 99 % of the hit pixels); the pixels that look through a hole
    differ from the twin's"""
    name = "al_layers"
    sc, twin = AS.scene(rtmi, name), AS.scene(rtmi, name, masks=False)
    words, _ = inputs(name)
    n = NS.REF_W * NS.REF_H
    S, probe, p32 = R.RefScene(sc), {}, {}
    R.trace(S, words[:n], probe=probe)
    R.trace(S, words[:n], dtype=np.float32, probe=p32)
    hit = probe["first_idx"] >= 0
    same = hit & (probe["first_idx"] == p32["first_idx"])  # (the pixels whose first opaque winner does not depend on the precision)
    o = rtmi.Opts(seed=AS.seed_of(name), sample_first=0, sample_count=1)
    depth = sc.render_feature(rtmi.FEATURE_DEPTH, o).reshape(-1, 3).astype(np.float64)
    normal = sc.render_feature(rtmi.FEATURE_NORMAL, o).reshape(-1, 3).astype(np.float64)
    flat_d = twin.render_feature(rtmi.FEATURE_DEPTH, o).reshape(-1, 3).astype(np.float64)
    assert (depth[same, 1] == 1).all()  # (coverage: 1 on a hit)
    err_t = np.abs(depth[same, 0] - probe["first_t"][same]) / np.maximum(1.0, probe["first_t"][same])
    err_n = np.abs(normal[same] - probe["normal"][same]).max(axis=1)
    through = hit & (np.abs(depth[:, 0] - flat_d[:, 0]) > 1e-3)
    print(f"\nfeature passes of {name}: {hit.sum()} hit pixels, {same.sum()} with one winner at both precisions: max depth error "
          f"{err_t.max():.2e}, max normal error {err_n.max():.2e}; {through.sum()} pixels look through a hole")
    assert same.sum() >= 0.99 * hit.sum(), (int(same.sum()), int(hit.sum()))
    assert err_t.max() <= 1e-4 and err_n.max() <= 1e-4, (float(err_t.max()), float(err_n.max()))
    assert through.sum() >= 200, through.sum()
    assert sc.render_feature(rtmi.FEATURE_ALBEDO, o).tobytes() != twin.render_feature(rtmi.FEATURE_ALBEDO, o).tobytes()


def test_ray_queries_report_the_twins_records(rtmi):
    """Scene.trace on al_layers returns the records of its twin without masks: queries are for geometry"""
    sc, twin = AS.scene(rtmi, "al_layers"), AS.scene(rtmi, "al_layers", masks=False)
    a, hit = PS.check_ray_queries_of_twins(sc, twin, lambda prims: prims[2:])  # (every primitive but the floor and the wall)
    assert sum(sc.alpha(int(m)) is not None for m in a["material"][hit]) >= 300


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_the_cli_renders_the_shipped_scene(rtmi, tmp_path, nee):
    PS.check_cli(rtmi, tmp_path, "cutout_garden.json", nee, AS.NEE,
                 loaded=lambda sc: sum(sc.alpha(m) is not None for m in range(len(sc.materials()))) >= 4)


def test_light_sampling_is_unbiased_against_the_plain_estimator(rtmi):
    """al_lights' quad light at 64 x 36 x 256 spp with and without light sampling: equal frame and block means, by the test and
    the bounds test_gpu_light_sampling.py uses (8 seeds each; c_max: the brightest emission, 14.0, over the roulette's survival
    probability).  The point light is taken out: the plain estimator cannot see a light without area"""
    from test_gpu_light_sampling import compare, seeds_of
    sc = AS.lights(rtmi, w=64, h=36, spp=256)
    sc.clear_analytic_lights()
    compare(seeds_of(rtmi, sc), seeds_of(rtmi, sc, nee=True), "al_lights", c_max=14.0 / 0.9)
