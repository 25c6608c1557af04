"""The media kernels (render_media_kernel) on the GPU.

  1. pinned to the plain kernels: a scene with a medium no ray can reach (media_scenes.bury_medium_*) renders, through the media
     kernels of every layout, the bytes of the same scene without media -- no interval, no draw, so everything else in the
     media kernel is the oracle-pinned computation;
  2. the exact composition of layouts, spp chunks, sample splits, row shards and adaptive tiles;
  3. exact powers of the albedo inside a closed emitter;
  4. Beer-Lambert transmittance within the binomial bound of the samples' own fp64 transmittances;
  5. per-sample agreement with the fp64 statement (ref64.py), criteria (a)-(d) of test_gpu_nee_reference.py;
  6. the refusals.

Rows of test 5 measured on the MI355X: DESIGN 2.

These cases pack to tables without a grid (layouts 36 and 44 run the scan's loops on them): the media kernels' grid walk is
held to their linear scan in tests/test_gpu_walk_families.py."""
import os

import numpy as np
import pytest

import media_scenes as MS
import ref64 as R
import per_sample as PS
from test_nested_grid import clump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MEDIA = MS.MEDIA
SEED = 31


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three spheres", "mixed"])
def test_unreachable_medium_gives_the_plain_bytes(rtmi, name):
    build, bury = {"three spheres": (MS.three_spheres, MS.bury_medium_three_spheres), "mixed": (MS.mixed_scene, MS.bury_medium_mixed)}[name]
    plain, sc = build(rtmi), build(rtmi)
    st = rtmi.Stats()
    ref = plain.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MEDIA == 0
    if name == "three spheres":
        assert plain.table_info().grid_wide == 0  # (compact tables without media)
    bury(sc)
    (MS.check_buried_three_spheres if name == "three spheres" else MS.check_buried_mixed)(rtmi, sc)  # (the premise: no ray reaches it)
    assert sc.table_info().grid_wide == 1
    for variant in (0, 16, 36, 44):
        got = sc.render(rtmi.Opts(seed=SEED, variant=variant), st)
        assert st.kernel_variant & MEDIA and (variant == 0 or st.kernel_variant & 255 == variant), (variant, st.kernel_variant)
        assert np.array_equal(got, ref), (name, variant, float(np.abs(got - ref).max()))


# ---- 2 ---------------------------------------------------------------------------------------------------------------
def fog_scene(rtmi, spp=48):
    sc = MS.room(rtmi, w=64, h=36, spp=spp)
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9))
    sc.add_medium_sphere((-0.2, 1.6, 1.5), 0.7, 3.0, (0.8, 0.6, 0.4))
    return sc


def test_layouts_chunks_splits_shards_and_adaptive(rtmi):
    sc = fog_scene(rtmi)
    st = rtmi.Stats()
    ref = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MEDIA
    plain = fog_scene(rtmi)
    plain.clear_media()
    assert not np.array_equal(plain.render(rtmi.Opts(seed=SEED)), ref)  # (the fog is seen)
    for variant in (16, 36, 44):
        assert np.array_equal(sc.render(rtmi.Opts(seed=SEED, variant=variant), st), ref), variant
        assert st.kernel_variant == variant | MEDIA
    assert np.array_equal(sc.render(rtmi.Opts(seed=SEED, spp_chunk=8)), ref) and np.array_equal(sc.render(rtmi.Opts(seed=SEED, spp_chunk=48)), ref)
    acc = None
    for first, n in ((0, 20), (20, 11), (31, 17)):
        acc, img = sc.accumulate(acc, rtmi.Opts(seed=SEED, sample_first=first, sample_count=n), st)
        assert st.kernel_variant & MEDIA
    assert np.array_equal(img, ref)
    full = np.zeros_like(ref)
    for r in range(3):
        o = rtmi.Opts(seed=SEED, tile_first=r, tile_stride=3, tile_rows=4)
        sc.scatter_rows(o, sc.render(o), full)
    assert np.array_equal(full, ref)
    assert np.array_equal(sc.render_tiles(None, rtmi.Opts(seed=SEED), st, n=1), ref)
    img, spp, _ = sc.render_adaptive(0.05, min_spp=4, max_spp=48, opts=rtmi.Opts(seed=SEED))
    for n in np.unique(spp):
        at_n = sc.render(rtmi.Opts(seed=SEED, sample_count=int(n)))
        assert np.array_equal(img[spp == n], at_n[spp == n]), n


def test_shipped_fog_room_renders(rtmi):
    sc = rtmi.Scene.load(os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "fog_room.json"))
    sc.override(width=96, height=54, spp=8)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MEDIA and np.isfinite(img).all() and img.sum() > 0
    sc.clear_media()
    clear = sc.render(rtmi.Opts(seed=SEED), st)
    assert not st.kernel_variant & MEDIA and not np.array_equal(clear, img)


# ---- 3 ---------------------------------------------------------------------------------------------------------------
def test_exact_powers_of_the_albedo(rtmi):
    depth = 8
    sc = rtmi.Scene.new(64, 36, 1, depth)
    sc.set_background((0, 0, 0), sky_gradient=False, defocus_blur=False)
    sc.camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0)
    sc.sphere((0, 0, 0), 50.0, sc.diffuse_light((1, 1, 1)))
    sc.add_medium_sphere((0, 0, 0), 4.0, 0.5, (0.5, 0.5, 0.5))
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MEDIA
    assert (img[..., 0] == img[..., 1]).all() and (img[..., 0] == img[..., 2]).all()
    v = img[..., 0].ravel()
    powers = 2.0 ** -np.arange(depth + 1)
    assert np.isin(v, np.concatenate([powers, [0.0]])).all(), np.unique(v)
    seen = [k for k in range(depth + 1) if (v == powers[k]).any()]
    assert len(seen) >= 4 and 0 in seen, seen


# ---- 4 ---------------------------------------------------------------------------------------------------------------
def test_beer_lambert(rtmi):
    W, H, spp, sigma, z0, z1 = 64, 36, 32, 0.8, -2.0, -1.0
    sc = rtmi.Scene.new(W, H, spp, 4)
    sc.set_background((1, 1, 1), sky_gradient=False, defocus_blur=False)
    sc.camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 70.0)
    sc.sphere((0, 0, 60), 1.0, sc.lambertian((0.5, 0.5, 0.5)))  # (behind the camera: no ray meets it)
    sc.add_medium_box((-100, -100, z0), (100, 100, z1), sigma, (0, 0, 0))
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MEDIA
    # each sample's own camera ray, in fp64, from the jitter of its stream
    cam = sc.get_camera()
    org, ll, hor, ver = (np.array(getattr(cam, k)[:], np.float64) for k in ("origin", "lower_left", "horizontal", "vertical"))
    p = np.empty((spp, H * W))
    for k in range(spp):
        w = np.stack([rtmi.sample_stream(SEED, pix, k, 2) for pix in range(H * W)])
        xi = (w >> 8).astype(np.float64) * 2.0 ** -24
        pix = np.arange(H * W)
        u, v = ((pix % W) + xi[:, 0]) / (W - 1), ((pix // W) + xi[:, 1]) / (H - 1)
        d = ll + u[:, None] * hor + v[:, None] * ver - org
        length = (z1 - z0) * np.sqrt((d * d).sum(axis=1)) / np.abs(d[:, 2])  # world length of the ray's stay in the slab
        p[k] = np.exp(-sigma * length)
    N = p.size
    mean_p, bound = p.mean(), 5.0 * np.sqrt((p * (1 - p)).sum()) / N
    got = float(img[..., 0].astype(np.float64).sum() / N)
    print(f"\nBeer-Lambert: mean transmittance {got:.6f}, fp64 {mean_p:.6f}, bound {bound:.6f}")
    assert 0.2 < mean_p < 0.8
    assert set(np.unique(img)) <= set(np.arange(spp + 1, dtype=np.float32))  # (every sample is 0 or 1)
    assert abs(got - mean_p) <= bound, (got, mean_p, bound)


# ---- 5 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def words(rtmi):
    return R.uniforms(rtmi, MS.REF_SEED, MS.REF_W, MS.REF_H, 0, MS.REF_K, MS.REF_DRAWS)


def kernel_samples(rtmi, sc, family):
    return PS.kernel_samples(rtmi, sc, MS.REF_SEED, MS.REF_K, MEDIA, family)


@pytest.mark.parametrize("name", list(MS.ref_cases()))
def test_media_kernel_against_fp64(rtmi, words, name):
    assert len(words) >= 16000
    sc = MS.ref_cases()[name](rtmi)
    ref, stable, draws, tally = R.reference(R.RefScene(sc), words)
    assert draws.max() <= MS.REF_DRAWS, draws.max()                                         # (d)
    assert tally["medium_events"] > 0 and tally["medium_then_surface"] >= 1, tally
    assert tally["media_with_events"] == list(range(len(sc.media()))), tally
    if name == "medium inside a glass shell":
        assert tally["medium_behind_glass"] == tally["medium_events"], tally
    j = R.judge(kernel_samples(rtmi, sc, MEDIA), ref, stable)
    plain = MS.ref_cases()[name](rtmi)
    plain.clear_media()
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    b = R.judge(kernel_samples(rtmi, plain, 0), bref, bstable)
    PS.assert_agreement(name, j, b)                                                         # (a), (b), (c)
    print("    " + ", ".join(f"{k} {tally[k]}" for k in R.MEDIA_KEYS))


def test_a_skipped_free_flight_draw_fails_the_agreement(rtmi, words):
    """(d): a reference that leaves the free-flight draw out of the order of draws is far from 97 %"""
    sc = MS.ref_cases()["camera inside thin fog"](rtmi)
    S = R.RefScene(sc)
    got = kernel_samples(rtmi, sc, MEDIA)
    ref, stable, _, _ = R.reference(S, words)
    wrong, _, _ = R.trace(S, words, perturb=("skip_flight",))
    good, bad = R.judge(got, ref, stable), R.judge(got, wrong, stable)
    print(f"\nskipped free-flight draw: within tolerance {100 * good['share']:.2f} % -> {100 * bad['share']:.2f} %")
    PS.assert_perturbation_noticed(good, bad)


# ---- 6 ---------------------------------------------------------------------------------------------------------------
def test_refusals(rtmi):
    sc = fog_scene(rtmi, spp=2)
    sc.set_light_sampling(True)
    assert len(sc.lights()) >= 1
    assert "light sampling" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED)))
    sc.set_light_sampling(False)
    sc.set_environment(np.ones((4, 8, 3), np.float32))
    assert "environment" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED)))
    sc.set_environment(None)
    assert "counting" in PS.refused(rtmi, lambda: sc.count(rtmi.Opts(seed=SEED)))
    assert "variant 6" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED, variant=6)))
    sc.render(rtmi.Opts(seed=SEED))  # (and on its own it renders)
    nested = clump(rtmi)
    nested.set_nested_grid(True)
    assert nested.nested_info().cells > 0
    nested.add_medium_sphere((0, 0, 0), 1.0, 0.5, (0.5, 0.5, 0.5))
    assert nested.nested_info().cells > 0
    assert "nested" in PS.refused(rtmi, lambda: nested.render(rtmi.Opts(seed=SEED)))
    # a light-sampling switch with nothing to sample is no obstacle
    dark = rtmi.Scene.new(32, 18, 2, 4)
    dark.sphere((0, 0, -3), 1.0, dark.lambertian((0.5, 0.5, 0.5)))
    dark.add_medium_sphere((0, 0, -3), 2.0, 0.5, (0.5, 0.5, 0.5))
    dark.set_light_sampling(True)
    st = rtmi.Stats()
    dark.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MEDIA and not st.kernel_variant & 256
