"""Anisotropic media on the GPU: a medium vertex with a Henyey-Greenstein asymmetry g != 0 in the media kernels.

  1. g = 0 set explicitly renders the bytes of the scene never touched, through every layout;
  2. an anisotropic medium no ray can reach gives the plain kernel's bytes (media_scenes.bury_medium_*): no interval, no draw, so
     everything else in the media kernel is still the oracle-pinned computation;
  3. the sample weight is exactly the albedo: exact powers of 1/2 inside a closed emitter;
  4. per-sample agreement with the fp64 statement (ref64.trace), criteria (a)-(c) of test_gpu_nee_reference.py with the
     plain kernel on the plain twin as the baseline (per_sample.assert_agreement);
  5. (d): each of the statement's three deliberate mistakes is noticed by the kernel's samples;
  6. the exact composition of layouts, a sample split, row shards and the product library; the shipped fog_halo scene;
  7. the refusals are those of the isotropic media.

Rows of test 4 measured on the MI355X: DESIGN 2.  The premises of 4 and 5 (events, draws, what a mistake changes) are held on
the reference alone in tests/test_phase.py."""
import os

import numpy as np
import pytest

import media_scenes as MS
import per_sample as PS
import phase_scenes as PH
import ref64 as R
import ref64_phase as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MEDIA = PH.MEDIA
SEED = 37


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


def fog_scene(rtmi, g=None):
    """media_scenes.room in thin fog around a smoke ball, 96 x 54 x 4; g: the two media's asymmetries, None: never set"""
    sc = MS.room(rtmi, w=96, h=54, spp=4)
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9))
    sc.add_medium_sphere((-0.2, 1.6, 1.5), 0.7, 3.0, (0.8, 0.6, 0.4))
    for i, v in enumerate(() if g is None else g):
        sc.set_medium_phase(i, v)
    return sc


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
def test_g_zero_set_explicitly_gives_the_untouched_bytes(rtmi):
    untouched, zero, snapped, forward = fog_scene(rtmi), fog_scene(rtmi, (0.0, 0.0)), fog_scene(rtmi, (5e-4, -9e-4)), fog_scene(rtmi, (0.8, 0.0))
    st = rtmi.Stats()
    for variant in (0, 16, 36, 44):
        ref = untouched.render(rtmi.Opts(seed=SEED, variant=variant), st)
        assert st.kernel_variant & MEDIA and (variant == 0 or st.kernel_variant & 255 == variant)
        assert np.array_equal(zero.render(rtmi.Opts(seed=SEED, variant=variant), st), ref), variant
        assert np.array_equal(snapped.render(rtmi.Opts(seed=SEED, variant=variant), st), ref), variant
        assert not np.array_equal(forward.render(rtmi.Opts(seed=SEED, variant=variant), st), ref), variant  # (and g shows)
    # a scene that has rendered follows a set of another stored value, and comes back to its bytes with the first
    ref = untouched.render(rtmi.Opts(seed=SEED))
    untouched.set_medium_phase(0, 0.8)
    assert np.array_equal(untouched.render(rtmi.Opts(seed=SEED)), forward.render(rtmi.Opts(seed=SEED)))
    untouched.set_medium_phase(0, 0.0)
    assert np.array_equal(untouched.render(rtmi.Opts(seed=SEED)), ref)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three spheres", "mixed"])
def test_unreachable_anisotropic_medium_gives_the_plain_bytes(rtmi, name):
    build, bury = {"three spheres": (MS.three_spheres, MS.bury_medium_three_spheres), "mixed": (MS.mixed_scene, MS.bury_medium_mixed)}[name]
    plain, sc = build(rtmi), build(rtmi)
    st = rtmi.Stats()
    ref = plain.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MEDIA == 0
    sc.set_medium_phase(bury(sc), 0.8)
    assert sc.medium_phase(0) == np.float32(0.8)
    (MS.check_buried_three_spheres if name == "three spheres" else MS.check_buried_mixed)(rtmi, sc)  # (the premise: no ray reaches it)
    for variant in (0, 16, 36, 44):
        got = sc.render(rtmi.Opts(seed=SEED, variant=variant), st)
        assert st.kernel_variant & MEDIA and (variant == 0 or st.kernel_variant & 255 == variant), (variant, st.kernel_variant)
        assert np.array_equal(got, ref), (name, variant, float(np.abs(got - ref).max()))


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def test_exact_powers_of_the_albedo(rtmi):
    """the scene of test_gpu_media.test_exact_powers_of_the_albedo with g = 0.7: the direction is drawn with the phase function's
    own density, so a vertex multiplies by the albedo 1/2 and by nothing else"""
    depth = 8
    sc = rtmi.Scene.new(64, 36, 1, depth)
    sc.set_background((0, 0, 0), sky_gradient=False, defocus_blur=False)
    sc.camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0)
    sc.sphere((0, 0, 0), 50.0, sc.diffuse_light((1, 1, 1)))
    sc.add_medium_sphere((0, 0, 0), 4.0, 0.5, (0.5, 0.5, 0.5), g=0.7)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MEDIA
    assert (img[..., 0] == img[..., 1]).all() and (img[..., 0] == img[..., 2]).all()
    v = img[..., 0].ravel()
    powers = 2.0 ** -np.arange(depth + 1)
    assert np.isin(v, np.concatenate([powers, [0.0]])).all(), np.unique(v)
    seen = [k for k in range(depth + 1) if (v == powers[k]).any()]
    assert len(seen) >= 4 and 0 in seen, seen


# ---- 4, 5 ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def words(rtmi):
    return R.uniforms(rtmi, PH.REF_SEED, PH.REF_W, PH.REF_H, 0, PH.REF_K, PH.REF_DRAWS)


@pytest.fixture(scope="module")
def cases(rtmi, words):
    """of(name) -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)), rendered and traced once"""
    made = {}

    def of(name):
        if name not in made:
            sc = PH.scene(rtmi, name)
            S = R.RefScene(sc)
            made[name] = (sc, S, PS.kernel_samples(rtmi, sc, PH.REF_SEED, PH.REF_K, MEDIA, MEDIA), R.reference(S, words))
        return made[name]
    return of


@pytest.mark.parametrize("name", list(PH.ref_cases()))
def test_media_kernel_against_fp64(rtmi, words, cases, name):
    assert len(words) >= 16000
    sc, S, got, (ref, stable, draws, tally) = cases(name)
    assert draws.max() <= PH.REF_DRAWS, draws.max()
    assert tally["anisotropic_events"] >= 200 and tally["surface_after_anisotropic"] >= 50, tally
    assert tally["media_with_events"] == list(range(len(S.media))), tally
    if name == PH.OVERLAP:
        assert tally["both_on_one_path"] >= 50, tally
    plain = PH.plain_twin(sc)
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    b = R.judge(PS.kernel_samples(rtmi, plain, PH.REF_SEED, PH.REF_K, MEDIA, 0), bref, bstable)
    PS.assert_agreement(name, R.judge(got, ref, stable), b)                                 # (a), (b), (c)
    print("    " + ", ".join(f"{k} {tally[k]}" for k in PH.TALLY_KEYS))


@pytest.mark.parametrize("mistake", RP.PERTURBATIONS)
@pytest.mark.parametrize("name", list(PH.ref_cases()))
def test_a_mistake_of_the_phase_step_fails_the_agreement(words, cases, name, mistake):
    PS.check_a_mistake_fails_the_agreement(lambda name: (words, None), cases, name, mistake)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    PS.check_same_bytes(rtmi, PH, [PH.OVERLAP, "russian roulette"], tmp_path, twin=lambda name: PH.isotropic_twin(PH.scene(rtmi, name)))


def test_row_shards_give_the_same_bytes(rtmi):
    sc = fog_scene(rtmi, (0.8, -0.5))
    st = rtmi.Stats()
    ref = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MEDIA
    full = np.zeros_like(ref)
    for r in range(2):
        o = rtmi.Opts(seed=SEED, tile_first=r, tile_stride=2, tile_rows=4)
        sc.scatter_rows(o, sc.render(o, st), full)
        assert st.kernel_variant & MEDIA
    assert np.array_equal(full, ref)


def test_shipped_fog_halo_renders(rtmi):
    sc = rtmi.Scene.load(os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "fog_halo.json"))
    sc.override(width=64, height=36, spp=4)
    assert RP.stored_g(sc).all()
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MEDIA and np.isfinite(img).all() and img.sum() > 0
    twin = PH.isotropic_twin(sc)
    assert not np.array_equal(twin.render(rtmi.Opts(seed=SEED), st), img) and st.kernel_variant & MEDIA


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_refusals_are_the_isotropic_ones(rtmi):
    sc = fog_scene(rtmi, (0.8, -0.5))
    sc.set_light_sampling(True)
    assert len(sc.lights()) >= 1
    assert "light sampling" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED)))
    sc.set_light_sampling(False)
    sc.set_environment(np.ones((4, 8, 3), np.float32))
    assert "environment" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED)))
    sc.set_environment(None)
    assert "counting" in PS.refused(rtmi, lambda: sc.count(rtmi.Opts(seed=SEED)))
    assert "variant 6" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED, variant=6)))
    st = rtmi.Stats()
    sc.render(rtmi.Opts(seed=SEED), st)  # (and on its own it renders)
    assert st.kernel_variant & MEDIA
