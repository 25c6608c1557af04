"""Light sampling in participating media (media_nee_kernel) on the GPU.

  1. routing: the switch, light sampling and media together run the new kernels (kernel_variant & 2048 and & 256); without the
     switch the scene is refused as before; with the switch and light sampling off the plain media kernel renders its bytes;
  2. neutrality: a medium no ray can reach (media_scenes.bury_medium_mixed) gives, in every layout, the bytes of the
     light-sampling kernel on the scene without it -- no interval, no draw, tau = 0, T = 1;
  3. inside a closed sphere emitter every one-sample pixel is exactly 2^-k or 0, though the light draws are consumed;
  4. the white furnace: every pixel's expectation is exactly 1;
  5. per-sample agreement with the fp64 statement (ref64.trace), criteria (a)-(d) of test_gpu_nee_reference.py, and
     each of the statement's four deliberate mistakes noticed;
  6. the same estimator as the plain media kernel, by frame means;
  7. it pays on the showcase's lamp: the median per-pixel variance ratio plain / sampled is above 1;
  8. the exact composition of layouts, a sample split, row shards, an adaptive pass and the product library;
  9. the refusals; the showcase renders.

Measured on the MI355X: DESIGN 7z."""
import os

import numpy as np
import pytest

import media_nee_scenes as MN
import media_scenes as MS
import per_sample as PS
import ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NEE, MEDIA = MN.NEE, MN.MEDIA
SEED = 37


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
def test_routing(rtmi):
    sc = MN.thin_fog(rtmi)
    st = rtmi.Stats()
    plain = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MEDIA and not st.kernel_variant & NEE
    sc.set_media_light_sampling(True)  # (light sampling off: inert)
    assert np.array_equal(sc.render(rtmi.Opts(seed=SEED), st), plain)
    assert st.kernel_variant & MEDIA and not st.kernel_variant & NEE
    sc.set_light_sampling(True)
    assert len(sc.lights()) >= 1
    img = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MEDIA and st.kernel_variant & NEE and st.kernel_variant & 255 in PS.GENERAL_LAYOUTS
    assert sc.table_info().kernel_variant == st.kernel_variant
    assert np.isfinite(img).all() and not np.array_equal(img, plain)
    sc.set_media_light_sampling(False)
    msg = PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED)))
    assert "light sampling" in msg and "media_light_sampling" in msg


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
def test_unreachable_medium_gives_the_light_sampling_kernels_bytes(rtmi):
    plain, sc = MS.mixed_scene(rtmi), MS.mixed_scene(rtmi)
    plain.set_light_sampling(True)
    st = rtmi.Stats()
    ref = plain.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & NEE and not st.kernel_variant & MEDIA
    MS.bury_medium_mixed(sc)
    MS.check_buried_mixed(rtmi, sc)  # (the premise: no ray reaches it)
    MN.switch_on(sc)
    for variant in (16, 36, 44, 0):
        got = sc.render(rtmi.Opts(seed=SEED, variant=variant), st)
        assert st.kernel_variant & MN.FAMILIES == MN.FAMILIES and (variant == 0 or st.kernel_variant & 255 == variant), (variant, st.kernel_variant)
        assert np.array_equal(got, ref), (variant, float(np.abs(got - ref).max()))


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [0.0, 0.7])
def test_exact_powers_of_the_albedo_inside_a_closed_emitter(rtmi, g):
    """a vertex inside a sphere light takes no sample of it and a hit from inside keeps full weight"""
    sc = MN.switch_on(MN.closed_emitter(rtmi, g))
    depth = sc.info.max_depth
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MN.FAMILIES == MN.FAMILIES
    assert (img[..., 0] == img[..., 1]).all() and (img[..., 0] == img[..., 2]).all()
    v = img[..., 0].ravel()
    powers = 2.0 ** -np.arange(depth + 1)
    assert np.isin(v, np.concatenate([powers, [0.0]])).all(), np.unique(v)
    seen = [k for k in range(depth + 1) if (v == powers[k]).any()]
    assert len(seen) >= 4 and 0 in seen, seen
    # the light draws are consumed: the paths are not the plain media kernel's
    sc.set_light_sampling(False)
    assert not np.array_equal(sc.render(rtmi.Opts(seed=SEED)), img)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", MN.FURNACE_G)
def test_white_furnace(rtmi, g):
    """|frame mean - 1| <= 5 std(pixel means) / sqrt(pixels): the frame's own standard error (tests/test_media_nee.py shows on
    the CPU that a missing T, a wrong phase density or a wrong weight moves the mean by far more)"""
    sc = MN.switch_on(MN.furnace(rtmi, g))
    MN.check_furnace_closed(sc)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED), st).astype(np.float64)
    assert st.kernel_variant & MN.FAMILIES == MN.FAMILIES
    assert np.array_equal(img[..., 0], img[..., 1]) and np.array_equal(img[..., 0], img[..., 2])
    px = img[..., 0].ravel() / sc.spp  # (a frame holds sums over its samples)
    se = px.std() / np.sqrt(px.size)
    print(f"\nwhite furnace, g = {g}: frame mean {px.mean():.6f}, standard error {se:.6f}, pixel means in [{px.min():.3f}, {px.max():.3f}]")
    assert abs(px.mean() - 1) <= 5 * se, (px.mean(), se)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def words(rtmi):
    return R.uniforms(rtmi, MN.REF_SEED, MN.REF_W, MN.REF_H, 0, MN.REF_K, MN.REF_DRAWS)


@pytest.fixture(scope="module")
def cases(rtmi, words):
    """of(name) -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)), rendered and traced once"""
    made = {}

    def of(name):
        if name not in made:
            sc = MN.scene(rtmi, name)
            got = PS.kernel_samples(rtmi, sc, MN.REF_SEED, MN.REF_K, MN.FAMILIES, MN.FAMILIES)
            made[name] = (sc, R.RefScene(sc), got, R.reference(R.RefScene(sc), words))
        return made[name]
    return of


TALLY_KEYS = ("medium_events", "medium_light_samples", "clear_through_media", "occluded_through_media", "medium_then_emitter", "medium_then_emitter_mis")


@pytest.mark.parametrize("name", list(MN.ref_cases()))
def test_kernel_against_fp64(rtmi, words, cases, name):
    assert len(words) >= 16000
    sc, S, got, (ref, stable, draws, tally) = cases(name)
    assert draws.max() <= MN.REF_DRAWS, draws.max()                                         # (d)
    assert tally["medium_events"] > 0 and tally["medium_light_samples"] > 0, tally
    if name == "medium inside a glass shell":
        # (any surface occludes: the glass stops every shadow ray of a vertex inside the shell, which gets nothing from the sample)
        assert tally["occluded_through_media"] > 0, tally
    else:
        assert tally["clear_through_media"] > 0 and tally["medium_samples_clear"] > 0, tally
    j = R.judge(got, ref, stable)
    # the baseline row: the light-sampling kernel on the same scene without media
    plain = MN.ref_cases()[name](rtmi)
    plain.clear_media()
    plain.set_light_sampling(True)
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    b = R.judge(PS.kernel_samples(rtmi, plain, MN.REF_SEED, MN.REF_K, MN.FAMILIES, NEE), bref, bstable)
    PS.assert_agreement(name, j, b)                                                         # (a), (b), (c)
    print("    " + ", ".join(f"{k} {tally[k]}" for k in TALLY_KEYS))


def test_the_cases_together_cover_the_new_vertices(rtmi, words, cases):
    total = {k: 0 for k in TALLY_KEYS + ("anisotropic_events",)}
    for name in MN.ref_cases():
        tally = cases(name)[3][3]
        for k in total:
            total[k] += tally[k]
    print("\n" + ", ".join(f"{k} {v}" for k, v in total.items()))
    assert all(v > 0 for v in total.values()), total


@pytest.mark.parametrize("mistake", list(MN.MISTAKES))
def test_a_mistake_fails_the_agreement(rtmi, words, cases, mistake):
    """(d): against the kernel, the statement with one deliberate mistake is far from 97 %"""
    PS.check_a_mistake_fails_the_agreement(lambda name: (words, None), cases, MN.MISTAKES[mistake], mistake)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_same_estimator_as_the_plain_media_kernel(rtmi):
    """frame means of REF_K one-sample frames each, with the switch and through the plain media kernel: within 5 combined
    standard errors"""
    sampled, plain = MN.switch_on(MN.thin_fog(rtmi)), MN.thin_fog(rtmi)
    a = PS.kernel_samples(rtmi, sampled, SEED, MN.REF_K, MN.FAMILIES, MN.FAMILIES).reshape(MN.REF_K, -1).mean(axis=1)
    b = PS.kernel_samples(rtmi, plain, SEED, MN.REF_K, MN.FAMILIES, MEDIA).reshape(MN.REF_K, -1).mean(axis=1)
    se = np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    print(f"\nthin fog: frame mean sampled {a.mean():.5f}, plain {b.mean():.5f}, combined standard error {se:.5f}")
    assert abs(a.mean() - b.mean()) <= 5 * se, (a.mean(), b.mean(), se)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_it_pays_on_the_showcase_lamp(rtmi):
    sampled = MN.beams(rtmi, lamp_only=True)
    plain = MN.beams(rtmi, lamp_only=True)
    plain.set_light_sampling(False)
    st = rtmi.Stats()
    frames = {}
    for key, sc, fam in (("sampled", sampled, MN.FAMILIES), ("plain", plain, MEDIA)):
        out = []
        for seed in range(4):
            out.append(sc.render(rtmi.Opts(seed=100 + seed), st).astype(np.float64))
            assert st.kernel_variant & MN.FAMILIES == fam
        frames[key] = np.stack(out)
    var = {k: v.var(axis=0, ddof=1).sum(axis=-1).ravel() for k, v in frames.items()}
    both = (var["sampled"] > 0) & (var["plain"] > 0)
    ratio = float(np.median(var["plain"][both] / var["sampled"][both]))
    print(f"\nfog_beams' lamp, 64 x 36 x 64 spp, 4 seeds: median per-pixel variance ratio plain / sampled {ratio:.2f} over {int(both.sum())} pixels")
    assert both.sum() >= 0.5 * both.size and ratio > 1.0, ratio


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    PS.check_same_bytes(rtmi, MN, ["two overlapping media", "thin fog, g = 0.7"], tmp_path)


def test_row_shards_and_an_adaptive_pass(rtmi):
    sc = MN.switch_on(MN.thin_fog(rtmi, 0.7))
    sc.override(width=64, height=36, spp=24)
    st = rtmi.Stats()
    ref = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MN.FAMILIES == MN.FAMILIES
    full = np.zeros_like(ref)
    for r in range(2):
        o = rtmi.Opts(seed=SEED, tile_first=r, tile_stride=2, tile_rows=4)
        sc.scatter_rows(o, sc.render(o, st), full)
        assert st.kernel_variant & MN.FAMILIES == MN.FAMILIES
    assert np.array_equal(full, ref)
    img, spp, _ = sc.render_adaptive(0.05, min_spp=4, max_spp=24, opts=rtmi.Opts(seed=SEED))
    for n in np.unique(spp):
        at_n = sc.render(rtmi.Opts(seed=SEED, sample_count=int(n)))
        assert np.array_equal(img[spp == n], at_n[spp == n]), n


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(rtmi):
    def fog():
        sc = MN.thin_fog(rtmi)
        sc.override(width=32, height=18, spp=2)
        return MN.switch_on(sc)
    sc = fog()
    sc.set_projection("orthographic", 4.0)
    assert "projection" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED)))
    sc = fog()
    sc.set_environment(np.ones((4, 8, 3), np.float32))
    assert "environment" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED)))
    sc = fog()
    assert "counting" in PS.refused(rtmi, lambda: sc.count(rtmi.Opts(seed=SEED)))
    assert "variant 6" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED, variant=6)))
    sc.add_moving_sphere((0, 1, 0), (0.2, 1, 0), 0.3, sc.lambertian((0.5, 0.5, 0.5)))
    assert "moving spheres" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED)))
    sc = fog()
    rgba = np.full((4, 4, 4), 255, np.uint8)
    rgba[::2, ::2, 3] = 0
    tex = sc.image_texture(rgba)
    m = sc.lambertian(tex)
    sc.set_alpha(m, tex, 0.5)
    sc.sphere((0, 2, 0), 0.3, m)
    assert "alpha mask" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED)))
    from test_nested_grid import clump
    nested = clump(rtmi)
    nested.set_nested_grid(True)
    nested.sphere((0, 6, 0), 0.5, nested.diffuse_light((4, 4, 4)))
    nested.add_medium_sphere((0, 0, 0), 1.0, 0.5, (0.5, 0.5, 0.5))
    MN.switch_on(nested)
    assert nested.nested_info().cells > 0
    assert "nested" in PS.refused(rtmi, lambda: nested.render(rtmi.Opts(seed=SEED)))
    # a feature pass goes on ignoring media (and light sampling)
    sc = fog()
    clear = fog()
    clear.clear_media()
    assert np.array_equal(sc.render_feature(rtmi.FEATURE_NORMAL, rtmi.Opts(seed=SEED)), clear.render_feature(rtmi.FEATURE_NORMAL, rtmi.Opts(seed=SEED)))
    sc.render(rtmi.Opts(seed=SEED))  # (and on its own it renders)


def test_the_showcase_renders(rtmi):
    sc = MN.beams(rtmi, w=96, h=54, spp=8)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MN.FAMILIES == MN.FAMILIES and np.isfinite(img).all() and img.sum() > 0
    # its shafts exist only through light samples: without them the two spotlights light nothing
    dark = MN.beams(rtmi, w=96, h=54, spp=8)
    dark.set_light_sampling(False)
    plain = dark.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MN.FAMILIES == MEDIA and not np.array_equal(plain, img)
