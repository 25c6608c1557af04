"""Analytic lights (point, spot and distant lights) on the GPU, against the fp64 statement of ref64.py with
ref64_analytic_lights' three samples, sample by sample on the same draws: criteria (a) - (c) of test_gpu_nee_reference.py with
per_sample's thresholds on the five cases of analytic_light_scenes.py.  The (b) baseline is the plain kernel on the case's plain
twin (light sampling off, so the analytic lights are in no table; environment cleared; glossy materials and rough glass replaced)
against the twin's reference.  Each case asserts from the reference's signatures and the wrapper's log that it holds what it is
there for, and prints the share of the same formulas at fp32 in NumPy beside the kernel's.

Then: a reference with one of the four deliberate mistakes is noticed; known answers on a lambertian floor under one light; the
refusals with media, moving spheres and the nested grid; and what every feature keeps -- the same bytes in every layout, through
a sample split and from the product library, the compact layouts refuse, with light sampling off the frame of the scene without
the lights, ray queries and feature passes unchanged, and the command line renders the shipped scene.

Every case prints one row of figures (pytest -s); DESIGN 7s holds the rows measured on the MI355X."""
import os
import subprocess

import numpy as np
import pytest

import analytic_light_scenes as AL
import nee_scenes as NS
import per_sample as PS
import ref64 as R
import smooth_scenes as SM

pytestmark = pytest.mark.gpu
NEE = AL.NEE


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    return PS.input_cache(rtmi, AL)


@pytest.fixture(scope="module")
def cases(rtmi, inputs):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)): rendered and traced once, shared by the tests"""
    return PS.case_cache(rtmi, AL, inputs)


@pytest.mark.parametrize("name", list(AL.CASES))
def test_kernel_against_fp64(rtmi, inputs, cases, name):
    sc, S, got, (ref, stable, draws, tally) = cases(name)
    r32, _, _ = R.trace(S, inputs(name)[0], dtype=np.float32)
    assert len(AL.plain_twin(rtmi, name).analytic_lights()) == len(sc.analytic_lights())
    shown = [k for k in tally if k in AL.CASES[name][2] or k.endswith("_picks")]
    print(f"\n    fp32 NumPy within {100 * R.judge(r32, ref, stable)['share']:.3f} %; " + ", ".join(f"{k} {tally[k]}" for k in shown))
    PS.check_kernel_against_fp64(rtmi, AL, inputs, cases, name)


@pytest.mark.parametrize("name,mistake", AL.MISTAKES)
def test_a_wrong_reference_is_noticed(inputs, cases, name, mistake):
    PS.check_a_mistake_fails_the_agreement(inputs, cases, name, mistake)


# ---------------------------------------------------------------------------------------------------------- known answers
def _mean3(sc, img):
    return img.astype(np.float64) / sc.spp


def test_point_light_known_answer(rtmi):
    """a lambertian floor under one point light, max_depth 2, black background: rho I cos(theta) / (pi d^2) -- the frame mean
    within 3 standard errors (4 seeds) + 1e-4, the per-pixel RMS relative error below 5 % at 64 x 36 x 256 (the criteria of
    test_gpu_light_sampling.test_analytic_known_answer)"""
    sc = AL.floor_scene(rtmi)
    sc.point_light(AL.POINT_X, AL.POINT_I)
    exp = AL.point_expected(sc)[..., 1]
    ok = np.isfinite(exp) & (exp > 1e-3)
    assert ok.mean() > 0.9
    st = rtmi.Stats()
    on = [_mean3(sc, sc.render(rtmi.Opts(seed=s), st))[..., 1] for s in range(4)]
    assert st.kernel_variant & NEE
    pm = np.array([p[ok].mean() for p in on])
    se = pm.std(ddof=1) / np.sqrt(len(pm))
    rel = np.sqrt(np.mean(((on[0] - exp) / exp)[ok] ** 2))
    print(f"\npoint light over a floor: frame mean {pm.mean():.6f} against {exp[ok].mean():.6f}, standard error {se:.2e}; RMS relative "
          f"error per pixel at 256 spp {rel:.5f}")
    assert abs(pm.mean() - exp[ok].mean()) < 3 * se + 1e-4, (pm.mean(), exp[ok].mean(), se)
    assert rel < 0.05, rel


def test_distant_light_known_answers(rtmi):
    """alpha = 0: every floor pixel is rho E cos(theta0) / pi within 1e-5 relative; alpha = 10 degrees: the frame mean within 3
    standard errors over 4 seeds"""
    want = AL.sun_expected()
    sc = AL.floor_scene(rtmi, spp=16)
    sc.distant_light(AL.SUN_DIR, AL.SUN_E, 0.0)
    pts, _, _ = AL.floor_points(sc, corners=True)
    floor = np.isfinite(pts).all(axis=(2, 3, 4))
    assert floor.mean() > 0.9
    img = _mean3(sc, sc.render(rtmi.Opts(seed=3)))
    err = np.abs(img[floor] / want - 1).max()
    print(f"\ndistant light, alpha = 0: largest relative error of a floor pixel {err:.2e}")
    assert err < 1e-5, err
    sc = AL.floor_scene(rtmi)
    sc.distant_light(AL.SUN_DIR, AL.SUN_E, 10.0)
    pm = np.array([_mean3(sc, sc.render(rtmi.Opts(seed=s)))[floor][:, 1].mean() for s in range(4)])
    se = pm.std(ddof=1) / np.sqrt(len(pm))
    print(f"distant light, alpha = 10: frame mean {pm.mean():.7f} against {want[1]:.7f}, standard error {se:.2e}")
    assert abs(pm.mean() - want[1]) < 3 * se, (pm.mean(), want[1], se)


def test_outside_the_cone_and_in_the_umbra_is_exactly_black(rtmi):
    """a spot: pixels whose footprint lies wholly outside the outer cone are exactly 0; a ball under a point light: pixels whose
    footprint lies wholly in its umbra (and that do not see the ball) are exactly 0"""
    sc = AL.floor_scene(rtmi, spp=64)
    sc.spot_light(AL.SPOT_X, AL.SPOT_DIR, (20.0, 20.0, 20.0), *AL.SPOT_ANGLES)
    pts, _, _ = AL.floor_points(sc, corners=True)
    x, a = np.array(AL.SPOT_X), np.array(AL.SPOT_DIR) / np.linalg.norm(AL.SPOT_DIR)
    v = pts - x
    cosine = (v @ a) / np.sqrt((v * v).sum(axis=-1))
    floor = np.isfinite(pts).all(axis=(2, 3, 4))
    with np.errstate(invalid="ignore"):
        outside = floor & (cosine < np.cos(np.radians(AL.SPOT_ANGLES[1] + 0.5))).all(axis=(2, 3))
        inside = floor & (cosine > np.cos(np.radians(AL.SPOT_ANGLES[0]))).all(axis=(2, 3))
    img = sc.render(rtmi.Opts(seed=5))
    print(f"\nspot: {outside.sum()} pixels wholly outside the outer cone, {inside.sum()} wholly inside the inner one")
    assert outside.sum() > 200 and inside.sum() > 20
    assert not img[outside].any() and (img[inside] > 0).all()
    # the umbra of a ball under a point light
    sc = AL.floor_scene(rtmi, spp=64)
    sc.point_light(AL.POINT_X, AL.POINT_I)
    c, r = np.array(AL.BALL[0]), AL.BALL[1]
    sc.sphere(AL.BALL[0], r, sc.lambertian((0.5, 0.5, 0.5)))
    pts, org, d = AL.floor_points(sc, corners=True)

    def nearest(o, w):
        """the distance from c to the segment o + s w, s in [0, 1]"""
        s = np.clip(((c - o) * w).sum(axis=-1) / (w * w).sum(axis=-1), 0, 1)
        return np.sqrt((((o + s[..., None] * w) - c) ** 2).sum(axis=-1))
    with np.errstate(invalid="ignore"):
        sees_ball = (nearest(np.broadcast_to(org, pts.shape), pts - org) < 1.1 * r).any(axis=(2, 3))
        umbra = floor & ~sees_ball & (nearest(pts, np.array(AL.POINT_X) - pts) < 0.9 * r).all(axis=(2, 3))
        lit = floor & ~sees_ball & (nearest(pts, np.array(AL.POINT_X) - pts) > 1.1 * r).all(axis=(2, 3))
    img = sc.render(rtmi.Opts(seed=5))
    print(f"point light over a ball: {umbra.sum()} pixels wholly in the umbra, {lit.sum()} wholly lit")
    assert umbra.sum() > 5 and lit.sum() > 500
    assert not img[umbra].any() and (img[lit] > 0).all()


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals_are_light_samplings(rtmi):
    """with media, with moving spheres and with the nested grid a scene whose only light is a point light refuses exactly as a
    scene with an emissive sphere does: the same status, the same message"""
    def room(analytic):
        sc = AL.lone_point(rtmi)
        if not analytic:
            sc.clear_analytic_lights()
            sc.sphere((0.2, 2.6, 1.0), 0.1, sc.diffuse_light((12.0, 11.0, 10.0)))
        sc.set_light_sampling(True)
        return sc

    def nested(analytic):
        sc = SM.nested_scene(rtmi, w=48, h=27)
        if analytic:
            sc.point_light((0.0, 3.0, 0.0), (5.0, 5.0, 5.0))
        else:
            sc.sphere((0.0, 3.0, 0.0), 0.1, sc.diffuse_light((5.0, 5.0, 5.0)))
        sc.set_light_sampling(True)
        return sc
    tail = lambda msg: msg.split("): ", 1)[-1]
    for what, spoil, build in (("media", lambda sc: sc.add_medium_sphere((0, 1, 0), 1.0, 0.5, (0.9, 0.9, 0.9)), room),
                               ("moving spheres", lambda sc: sc.add_moving_sphere((0, 1, 0), (1, 1, 0), 0.3, 0), room),
                               ("nested grid", lambda sc: None, nested)):
        said = []
        for analytic in (True, False):
            sc = build(analytic)
            spoil(sc)
            said.append(tail(PS.refused(rtmi, lambda: sc.render(rtmi.Opts(seed=1)))))
        assert said[0] == said[1] and "light sampling" in said[0], (what, said)
    # and the compact layouts, which list spheres for the sphere-only kernels
    for variant in (2, 6):
        PS.refused(rtmi, lambda: AL.scene(rtmi, "point light alone").render(rtmi.Opts(variant=variant)))


# ---------------------------------------------------------------------------------------------------------- what stays
def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    PS.check_same_bytes(rtmi, AL, ("two spots + quad + sphere", "sun + environment"), tmp_path)


def test_light_sampling_off_renders_the_scene_without_the_lights(rtmi):
    opts = lambda: rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K)
    for name in ("two spots + quad + sphere", "point light alone", "sun + environment"):
        sc, st = AL.scene(rtmi, name), rtmi.Stats()
        on = sc.render(opts(), st)
        assert st.kernel_variant & NEE
        bare = AL.scene(rtmi, name)
        bare.clear_analytic_lights()
        lit = bare.render(opts(), st)
        # (with other emitters the cleared scene still samples them; alone, nothing is left to sample)
        assert bool(st.kernel_variant & NEE) == (len(bare.lights()) > 0) and not np.array_equal(lit, on)
        sc.set_light_sampling(False)
        bare.set_light_sampling(False)
        off = sc.render(opts(), st)
        assert not st.kernel_variant & NEE
        assert np.array_equal(off, bare.render(opts(), st)) and not st.kernel_variant & NEE, name


def test_ray_queries_and_feature_passes_ignore_the_lights(rtmi):
    sc = AL.scene(rtmi, "two spots + quad + sphere")
    bare = AL.scene(rtmi, "two spots + quad + sphere")
    bare.clear_analytic_lights()
    rng = np.random.default_rng(2)
    o = np.tile(np.array([0.0, 2.5, 6.0], np.float32), (4096, 1))
    d = (np.array([0.0, -2.0, -6.0]) + rng.uniform(-2, 2, (4096, 3))).astype(np.float32)
    assert sc.trace(o, d).tobytes() == bare.trace(o, d).tobytes()
    assert sc.trace(o, d, occluded=True).tobytes() == bare.trace(o, d, occluded=True).tobytes()
    for feature in (rtmi.FEATURE_ALBEDO, rtmi.FEATURE_NORMAL, rtmi.FEATURE_DEPTH):
        a = sc.render_feature(feature, rtmi.Opts(seed=3, sample_count=4))
        assert np.array_equal(a, bare.render_feature(feature, rtmi.Opts(seed=3, sample_count=4))), feature


def test_the_command_line_renders_the_shipped_scene(rtmi, tmp_path):
    out = str(tmp_path / "spot_stage.png")
    scene = os.path.join(PS.PKG, "scenes", "spot_stage.json")
    size = ["-w", "96", "-h", "54", "-spp", "8"]
    p = subprocess.run([os.path.join(PS.PKG, "rtmi"), "-f", scene, "-o", out, "--nee"] + size, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert os.path.getsize(out) > 1000 and "light sampling is off" not in p.stderr
    # the file leaves light sampling to --nee, as every shipped scene does: without it the lights light nothing, and rtmi says
    # so in one line on stderr
    assert '"light_sampling": false' in open(scene).read()
    p = subprocess.run([os.path.join(PS.PKG, "rtmi"), "-f", scene, "-o", out] + size, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stderr.count("light sampling is off") == 1
