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
import sys
import textwrap

import numpy as np
import pytest

import analytic_light_scenes as AL
import nee_scenes as NS
import per_sample as PS
import ref64 as R
import smooth_scenes as SM

pytestmark = pytest.mark.gpu
ROOT = PS.ROOT
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
GENERAL_LAYOUTS = (16, 36, 44)
NEE = AL.NEE


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def words(rtmi):
    return AL.inputs(rtmi)


@pytest.fixture(scope="module")
def cases(rtmi, words):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)): rendered and traced once"""
    made = {}

    def of(name):
        if name not in made:
            sc = AL.scene(rtmi, name)
            S = R.RefScene(sc)
            st = rtmi.Stats()
            sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=1), st)
            assert st.kernel_variant & ~AL.FAMILIES in GENERAL_LAYOUTS and st.kernel_variant & AL.FAMILIES == AL.family(name), st.kernel_variant
            got = PS.kernel_samples(rtmi, sc, NS.REF_SEED, NS.REF_K, AL.FAMILIES, AL.family(name))
            made[name] = (sc, S, got, R.reference(S, words))
        return made[name]
    return of


@pytest.mark.parametrize("name", list(AL.CASES))
def test_kernel_against_fp64(rtmi, words, cases, name):
    assert len(words) >= 16000
    sc, S, got, (ref, stable, draws, tally) = cases(name)
    assert draws.max() <= NS.REF_DRAWS, draws.max()
    AL.check_contents(name, tally)
    plain = AL.plain_twin(rtmi, name)
    assert len(plain.analytic_lights()) == len(sc.analytic_lights())
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    b = R.judge(PS.kernel_samples(rtmi, plain, NS.REF_SEED, NS.REF_K, AL.FAMILIES, 0), bref, bstable)
    r32, _, _ = R.trace(S, words, dtype=np.float32)
    fp32 = f"fp32 NumPy within {100 * R.judge(r32, ref, stable)['share']:.3f} %"
    shown = [k for k in tally if k in AL.CASES[name][2] or k.endswith("_picks")]
    print(f"\n    {fp32}; " + ", ".join(f"{k} {tally[k]}" for k in shown))
    PS.assert_agreement(name, R.judge(got, ref, stable), b)                                # (a), (b), (c)


@pytest.mark.parametrize("name,mistake", AL.MISTAKES)
def test_a_wrong_reference_is_noticed(words, cases, name, mistake):
    """against the kernel, a reference with one deliberate mistake of the analytic lights is far from 97 %"""
    sc, S, got, (ref, stable, _, _) = cases(name)
    wrong, _, _ = R.trace(S, words, perturb=(mistake,))
    good, bad = R.judge(got, ref, stable), R.judge(got, wrong, stable)
    print(f"\n{name}, {mistake}: within tolerance {100 * good['share']:.2f} % -> {100 * bad['share']:.2f} %")
    PS.assert_perturbation_noticed(good, bad)


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
_BYTES_CASES = ("two spots + quad + sphere", "sun + environment")
_PRODUCT = textwrap.dedent("""
    import os, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, os.path.join(%r, "tests"))
    from __graft_entry__ import load_package
    rtmi = load_package()
    assert not rtmi.has_ablations()
    import analytic_light_scenes as AL, nee_scenes as NS
    for name in %r:
        st = rtmi.Stats()
        img = AL.scene(rtmi, name).render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
        assert st.kernel_variant & AL.FAMILIES == AL.family(name), st.kernel_variant
        np.save(os.path.join(sys.argv[1], name.replace(" ", "_") + ".npy"), img)
""") % (ROOT, ROOT, _BYTES_CASES)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    env = dict(os.environ, RTMI_LIB=os.path.join(PKG, "librtmi_product.so"))
    p = subprocess.run([sys.executable, "-c", _PRODUCT, str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    for name in _BYTES_CASES:
        sc, fam, seed, st = AL.scene(rtmi, name), AL.family(name), NS.REF_SEED, rtmi.Stats()
        ref = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K), st)
        assert st.kernel_variant & AL.FAMILIES == fam and st.kernel_variant & ~AL.FAMILIES in GENERAL_LAYOUTS
        for variant in GENERAL_LAYOUTS:
            got = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K, variant=variant), st)
            assert st.kernel_variant == variant | fam, (variant, st.kernel_variant)
            assert np.array_equal(got, ref), (name, variant, float(np.abs(got - ref).max()))
        acc, _ = sc.accumulate(None, rtmi.Opts(seed=seed, sample_first=0, sample_count=5), st)
        assert st.kernel_variant & AL.FAMILIES == fam
        acc, img = sc.accumulate(acc, rtmi.Opts(seed=seed, sample_first=5, sample_count=NS.REF_K - 5), st)
        assert np.array_equal(img, ref), (name, float(np.abs(img - ref).max()))
        assert np.array_equal(np.load(str(tmp_path / (name.replace(" ", "_") + ".npy"))), ref), name


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
    scene = os.path.join(PKG, "scenes", "spot_stage.json")
    size = ["-w", "96", "-h", "54", "-spp", "8"]
    p = subprocess.run([os.path.join(PKG, "rtmi"), "-f", scene, "-o", out, "--nee"] + size, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert os.path.getsize(out) > 1000 and "light sampling is off" not in p.stderr
    # the file leaves light sampling to --nee, as every shipped scene does: without it the lights light nothing, and rtmi says
    # so in one line on stderr
    assert '"light_sampling": false' in open(scene).read()
    p = subprocess.run([os.path.join(PKG, "rtmi"), "-f", scene, "-o", out] + size, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stderr.count("light sampling is off") == 1
