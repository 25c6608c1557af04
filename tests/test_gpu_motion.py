"""The motion kernels (render_motion_kernel) on the GPU.

  1. pinned to the plain kernels: a scene with a mover no ray can reach (motion_scenes.bury_mover_*) renders, through the motion
     kernels of every layout, the bytes of the same scene without it -- the shutter time takes nothing from the sample's
     stream, so everything else in the motion kernel is the oracle-pinned computation;
  2. the exact composition of layouts, spp chunks, sample splits, row shards, tiles and adaptive tiles;
  3. coverage: a black mover before a white background, every sample decided in fp64 from its own jitter and shutter time;
  4. per-sample agreement with the fp64 statement (ref64.py), criteria (a)-(d) of test_gpu_media.py;
  5. the comparison can fail: a reference that puts every sample at s = 0.5;
  6. the refusals;
  7. the shipped scene.

Rows of test 4 measured on the MI355X: DESIGN 2.

These cases pack to tables without a grid (layouts 36 and 44 run the scan's loops on them): the motion kernels' grid walk is
held to their linear scan in tests/test_gpu_walk_families.py."""
import os

import numpy as np
import pytest

import media_scenes as MS
import motion_scenes as MO
import ref64 as R
import per_sample as PS
from test_nested_grid import clump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MOTION = MO.MOTION
SEED = 31


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three spheres", "mixed"])
def test_unreachable_mover_gives_the_plain_bytes(rtmi, name):
    build, bury, check = {"three spheres": (MS.three_spheres, MO.bury_mover_three_spheres, MO.check_buried_three_spheres),
                          "mixed": (MS.mixed_scene, MO.bury_mover_mixed, MO.check_buried_mixed)}[name]
    plain, sc = build(rtmi), build(rtmi)
    st = rtmi.Stats()
    ref = plain.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MOTION == 0
    if name == "three spheres":
        assert plain.table_info().grid_wide == 0  # (compact tables without a mover)
    bury(sc)
    check(rtmi, sc)  # (the premise: no ray reaches it)
    assert sc.table_info().grid_wide == 1
    for variant in (0, 16, 36, 44):
        got = sc.render(rtmi.Opts(seed=SEED, variant=variant), st)
        assert st.kernel_variant & MOTION and (variant == 0 or st.kernel_variant & 255 == variant), (variant, st.kernel_variant)
        assert np.array_equal(got, ref), (name, variant, float(np.abs(got - ref).max()))


# ---- 2 ---------------------------------------------------------------------------------------------------------------
def test_layouts_chunks_splits_shards_tiles_and_adaptive(rtmi):
    sc = MO.two_movers(rtmi)
    st = rtmi.Stats()
    ref = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MOTION
    plain = MO.two_movers(rtmi)
    plain.clear_moving_spheres()
    assert not np.array_equal(plain.render(rtmi.Opts(seed=SEED), st), ref) and not st.kernel_variant & MOTION  # (the movers are seen)
    for variant in (16, 36, 44):
        assert np.array_equal(sc.render(rtmi.Opts(seed=SEED, variant=variant), st), ref), variant
        assert st.kernel_variant == variant | MOTION
    assert np.array_equal(sc.render(rtmi.Opts(seed=SEED, spp_chunk=8)), ref) and np.array_equal(sc.render(rtmi.Opts(seed=SEED, spp_chunk=48)), ref)
    acc = None
    for first, n in ((0, 20), (20, 11), (31, 17)):
        acc, img = sc.accumulate(acc, rtmi.Opts(seed=SEED, sample_first=first, sample_count=n), st)
        assert st.kernel_variant & MOTION
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


# ---- 3 ---------------------------------------------------------------------------------------------------------------
def test_coverage_of_a_black_mover(rtmi):
    sc = MO.coverage_scene(rtmi)
    hit64, rel, s = MO.coverage_reference(rtmi, sc)
    st = rtmi.Stats()
    got = np.stack([sc.render(rtmi.Opts(seed=MO.COV_SEED, sample_first=k, sample_count=1), st) for k in range(MO.COV_SPP)])
    assert st.kernel_variant & MOTION
    assert set(np.unique(got)) <= {0.0, 1.0}  # (every sample is exactly 0 or 1)
    assert (got[..., 0] == got[..., 1]).all() and (got[..., 0] == got[..., 2]).all()
    hit = got[..., 0].reshape(MO.COV_SPP, -1) == 0.0
    near = np.abs(rel) < MO.COV_CAP
    differ = hit != hit64
    print(f"\ncoverage: {hit.mean():.4f} of the samples covered (fp64 {hit64.mean():.4f}), {int(differ.sum())} differ, "
          f"{int(near.sum())} of {near.size} within the cap ({100 * near.mean():.4f} %)")
    assert near.mean() < 0.005, near.mean()
    assert not (differ & ~near).any(), int((differ & ~near).sum())
    MO.assert_motion_is_seen(hit, s)
    total = sc.render(rtmi.Opts(seed=MO.COV_SEED))  # (and the frame is the sum of its samples)
    assert np.array_equal(total, got.sum(axis=0))


# ---- 4 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def words(rtmi):
    return R.uniforms(rtmi, MS.REF_SEED, MS.REF_W, MS.REF_H, 0, MS.REF_K, MS.REF_DRAWS)


@pytest.fixture(scope="module")
def shutter(rtmi):
    return MO.shutter_times(rtmi, MS.REF_SEED, MS.REF_W, MS.REF_H, 0, MS.REF_K)


def kernel_samples(rtmi, sc, family):
    return PS.kernel_samples(rtmi, sc, MS.REF_SEED, MS.REF_K, MOTION, family)


@pytest.mark.parametrize("name", list(MO.ref_cases()))
def test_motion_kernel_against_fp64(rtmi, words, shutter, name):
    assert len(words) >= 16000 and len(shutter) == len(words)
    sc = MO.ref_cases()[name](rtmi)
    ref, stable, draws, tally = R.reference(R.RefScene(sc), words, shutter)
    assert draws.max() <= MS.REF_DRAWS, draws.max()                                         # (d)
    assert tally["movers_hit"] == list(range(len(sc.moving_spheres()))), tally
    if name != "an emissive mover over the floor":  # (an emitter ends its path: nothing comes after it)
        assert tally["mover_then_static"] >= 1, tally
    assert tally["static_then_mover"] >= 1, tally
    got = kernel_samples(rtmi, sc, MOTION)
    j = R.judge(got, ref, stable)
    plain = MO.ref_cases()[name](rtmi)
    plain.clear_moving_spheres()
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    b = R.judge(kernel_samples(rtmi, plain, 0), bref, bstable)
    PS.assert_agreement(name, j, b)                                                         # (a), (b), (c)
    print("    " + ", ".join(f"{k} {tally[k]}" for k in R.MOTION_KEYS))
    if name == "a zero-velocity mover":
        twin = kernel_samples(rtmi, MO.static_twin(rtmi), 0)
        print(f"    one-sample pixels bit-equal to the static twin's: {100 * (twin == got).all(axis=1).mean():.3f} %")


# ---- 5 ---------------------------------------------------------------------------------------------------------------
def test_a_reference_without_the_shutter_time_fails_the_agreement(rtmi, words, shutter):
    """a reference that puts every sample at s = 0.5 is far from 97 %"""
    sc = MO.ref_cases()[MO.IN_FRONT](rtmi)
    S = R.RefScene(sc)
    got = kernel_samples(rtmi, sc, MOTION)
    ref, stable, _, _ = R.reference(S, words, shutter)
    wrong, _, _ = R.trace(S, words, shutter=shutter, perturb=("half_time",))
    good, bad = R.judge(got, ref, stable), R.judge(got, wrong, stable)
    print(f"\nevery sample at s = 0.5: within tolerance {100 * good['share']:.2f} % -> {100 * bad['share']:.2f} %")
    PS.assert_perturbation_noticed(good, bad)


# ---- 6 ---------------------------------------------------------------------------------------------------------------
def test_refusals(rtmi):
    sc = MO.two_movers(rtmi, spp=2)
    sc.set_light_sampling(True)
    assert len(sc.lights()) >= 1
    assert "light sampling" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED)))
    sc.set_light_sampling(False)
    sc.set_environment(np.ones((4, 8, 3), np.float32))
    assert "environment" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED)))
    sc.set_environment(None)
    sc.add_medium_sphere((0, 1, 0), 1.0, 0.5, (0.5, 0.5, 0.5))
    assert "media" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED)))
    sc.clear_media()
    assert "counting" in PS.refused(rtmi, lambda: sc.count(rtmi.Opts(seed=SEED)))
    assert "feature pass" in PS.refused(rtmi, lambda: sc.render_feature(0, rtmi.Opts(seed=SEED)))
    assert "variant 6" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=SEED, variant=6)))
    st = rtmi.Stats()
    sc.render(rtmi.Opts(seed=SEED), st)  # (and on its own it renders)
    assert st.kernel_variant & MOTION
    nested = clump(rtmi)
    nested.set_nested_grid(True)
    assert nested.nested_info().cells > 0
    nested.add_moving_sphere((0, 0, 0), (1, 0, 0), 1.0, 0)
    assert nested.nested_info().cells > 0
    assert "nested" in PS.refused(rtmi, lambda: nested.render(rtmi.Opts(seed=SEED)))
    # a light-sampling switch with nothing to sample is no obstacle
    dark = rtmi.Scene.new(32, 18, 2, 4)
    dark.sphere((0, 0, -3), 1.0, dark.lambertian((0.5, 0.5, 0.5)))
    dark.add_moving_sphere((-1, 0, -3), (1, 0, -3), 0.5, 0)
    dark.set_light_sampling(True)
    dark.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MOTION and not st.kernel_variant & 256


# ---- 7 ---------------------------------------------------------------------------------------------------------------
def test_shipped_motion_balls_renders(rtmi):
    sc = rtmi.Scene.load(os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "motion_balls.json"))
    sc.override(width=96, height=54, spp=8)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & MOTION and np.isfinite(img).all() and img.sum() > 0
    sc.clear_moving_spheres()
    still = sc.render(rtmi.Opts(seed=SEED), st)
    assert not st.kernel_variant & MOTION and not np.array_equal(still, img)
