"""The noise textures (fBm, turbulence, marble) in every render family, against the fp64 statement of ref64.py with
ref64_noise.py installed, sample by sample on the same draws: criteria (a) - (d) of test_gpu_nee_reference.py with per_sample's
thresholds, on the six cases of noise_scenes.py.  The (b) baseline is the plain kernel on the case's twin -- every noise texture
replaced by a solid colour, light sampling off, environment, media and movers cleared -- against the twin's reference.  Each case
asserts from the reference's signatures that it contains the vertices it is there for and that 15 % of its samples touch a noise
texture.

(d): the reference's draws stay within REF_DRAWS, and a reference with a deliberate mistake -- the cubic fade, every octave on one
seed, marble's phase along another axis -- is far from 97 % against the kernel.  These tests fail without the feature and with a
wrong hash, fade or octave rule in the kernel.

Then what every feature keeps: the same bytes in every layout, through a sample split and from the product library; the feature
buffers; ray queries; the command line on the shipped scene; and light sampling against the plain estimator.

Every case prints one row of figures (pytest -s); DESIGN 7o holds the rows measured on the MI355X."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import nee_scenes as NS
import noise_scenes as NSC
import per_sample as PS
import ref64 as R
import ref64_noise as N

pytestmark = pytest.mark.gpu
ROOT = PS.ROOT
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
GENERAL_LAYOUTS = (16, 36, 44)  # a scene with a noise texture runs the general (EXT) builds: never the compact layouts 2 / 6


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    made = {}

    def of(name):
        key = (NSC.seed_of(name), NSC.family(name) == NSC.MOTION)
        if key not in made:
            made[key] = NSC.inputs(rtmi, name)
        return made[key]
    return of


@pytest.fixture(scope="module")
def cases(rtmi, inputs):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally), noise tally): rendered and traced once, shared"""
    made = {}

    def of(name):
        if name not in made:
            words, shutter = inputs(name)
            sc = NSC.scene(rtmi, name)
            S = R.RefScene(sc)
            st = rtmi.Stats()
            sc.render(rtmi.Opts(seed=NSC.seed_of(name), sample_count=1), st)
            layouts = (NSC.NESTED_LAYOUT,) if name == "noise_nested" else GENERAL_LAYOUTS
            assert st.kernel_variant & ~NSC.FAMILIES in layouts and st.kernel_variant & NSC.FAMILIES == NSC.family(name), st.kernel_variant
            got = PS.kernel_samples(rtmi, sc, NSC.seed_of(name), NS.REF_K, NSC.FAMILIES, NSC.family(name))
            ref = R.reference(S, words, shutter)
            made[name] = (sc, S, got, ref, {k: v for k, v in ref[3].items() if k.startswith("noise_")})
        return made[name]
    return of


@pytest.mark.parametrize("name", list(NSC.CASES))
def test_kernel_against_fp64(rtmi, inputs, cases, name):
    words, shutter = inputs(name)
    assert len(words) >= 16000
    sc, S, got, (ref, stable, draws, tally), noise_tally = cases(name)
    assert draws.max() <= NS.REF_DRAWS, draws.max()                                        # (d)
    NSC.check_contents(name, noise_tally)
    plain = NSC.plain_twin(rtmi, name)
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    b = R.judge(PS.kernel_samples(rtmi, plain, NSC.seed_of(name), NS.REF_K, NSC.FAMILIES, 0), bref, bstable)
    PS.assert_agreement(name, R.judge(got, ref, stable), b)                                # (a), (b), (c)
    print("    " + ", ".join(f"{k} {v}" for k, v in noise_tally.items() if v))


@pytest.mark.parametrize("name,mistake", [("noise_sky", "noise_cubic_fade"), ("noise_sky", "noise_same_seed"), ("noise_lights", "noise_wrong_axis")])
def test_a_mistake_fails_the_agreement(inputs, cases, name, mistake):
    """(d): against the kernel, a reference with one deliberate mistake of the model is far from 97 %"""
    words, shutter = inputs(name)
    sc, S, got, (ref, stable, _, _), _ = cases(name)
    wrong, _, _ = R.trace(S, words, shutter=shutter, perturb=(mistake,))
    good, bad = R.judge(got, ref, stable), R.judge(got, wrong, stable)
    print(f"\n{name}, {mistake}: within tolerance {100 * good['share']:.2f} % -> {100 * bad['share']:.2f} %")
    PS.assert_perturbation_noticed(good, bad)


_PRODUCT = textwrap.dedent("""
    import os, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, os.path.join(%r, "tests"))
    from __graft_entry__ import load_package
    rtmi = load_package()
    assert not rtmi.has_ablations()
    import noise_scenes as NSC, nee_scenes as NS
    for name in ("noise_sky", "noise_lights"):
        st = rtmi.Stats()
        img = NSC.scene(rtmi, name).render(rtmi.Opts(seed=NSC.seed_of(name), sample_count=NS.REF_K), st)
        assert st.kernel_variant & NSC.FAMILIES == NSC.family(name), st.kernel_variant
        np.save(os.path.join(sys.argv[1], name + ".npy"), img)
""") % (ROOT, ROOT)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    env = dict(os.environ, RTMI_LIB=os.path.join(PKG, "librtmi_product.so"))
    p = subprocess.run([sys.executable, "-c", _PRODUCT, str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    for name in ("noise_sky", "noise_lights"):
        sc, fam, seed, st = NSC.scene(rtmi, name), NSC.family(name), NSC.seed_of(name), rtmi.Stats()
        ref = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K), st)
        assert st.kernel_variant & NSC.FAMILIES == fam and st.kernel_variant & ~NSC.FAMILIES in GENERAL_LAYOUTS
        for variant in GENERAL_LAYOUTS:
            got = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K, variant=variant), st)
            assert st.kernel_variant == variant | fam, (variant, st.kernel_variant)
            assert np.array_equal(got, ref), (name, variant, float(np.abs(got - ref).max()))
        acc, _ = sc.accumulate(None, rtmi.Opts(seed=seed, sample_first=0, sample_count=5), st)
        assert st.kernel_variant & NSC.FAMILIES == fam
        acc, img = sc.accumulate(acc, rtmi.Opts(seed=seed, sample_first=5, sample_count=NS.REF_K - 5), st)
        assert np.array_equal(img, ref), (name, float(np.abs(img - ref).max()))
        assert np.array_equal(np.load(str(tmp_path / (name + ".npy"))), ref), name
    # the nested clump: its own layout against the flat wide-table walk of the same scene
    sc, st = NSC.scene(rtmi, "noise_nested"), rtmi.Stats()
    nested = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant == NSC.NESTED_LAYOUT
    sc.set_nested_grid(False)
    flat = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant in GENERAL_LAYOUTS and np.array_equal(nested, flat)
    # the compact layouts list spheres for the sphere-only kernels, which know no noise texture: refused
    for variant in (2, 6):
        with pytest.raises(rtmi.RtmiError):
            NSC.scene(rtmi, "noise_sky").render(rtmi.Opts(variant=variant))


def test_feature_buffers_show_the_first_vertex(rtmi, inputs):
    """one-sample feature passes of noise_sky: the albedo against the texture values the reference read at its FIRST vertex of
    sample 0 of every pixel (trace()'s probe["texture_value"]), within 1e-4 per channel -- the per-sample tolerance -- on at least 99 % of the noise pixels;
    normal and depth are the twin's, byte for byte"""
    name = "noise_sky"
    sc, twin = NSC.scene(rtmi, name), NSC.scene(rtmi, name, noise=False)
    words, _ = inputs(name)
    n = NS.REF_W * NS.REF_H
    S, probe = R.RefScene(sc), {}
    _, sig, _ = R.trace(S, words[:n], probe=probe)
    prim = sig[:, R.SAMPLE_COLUMNS + R.C_PRIM]
    mtype = np.where(prim >= 0, S.mats["type"][S.prims["material"][np.clip(prim, 0, None)]], -1)
    tex_of = np.where(prim >= 0, S.mats["texture"][S.prims["material"][np.clip(prim, 0, None)]], -1)
    want = np.where(np.isin(mtype, (R.DIFFUSE_LIGHT, R.LAMBERTIAN, R.PLASTIC))[:, None], probe["texture_value"], np.nan)
    noisy = (tex_of >= 0) & (S.texs["type"][np.clip(tex_of, 0, None)] == N.NOISE) & np.isin(mtype, (R.LAMBERTIAN, R.PLASTIC, R.DIFFUSE_LIGHT))
    assert noisy.sum() >= 300 and set(np.unique(mtype[noisy])) == {R.LAMBERTIAN, R.PLASTIC}, noisy.sum()
    o = rtmi.Opts(seed=NSC.seed_of(name), sample_first=0, sample_count=1)
    albedo = sc.render_feature(rtmi.FEATURE_ALBEDO, o).reshape(-1, 3).astype(np.float64)
    err = np.abs(albedo[noisy] - want[noisy]).max(axis=1)
    print(f"\nfeature pass of {name}: {noisy.sum()} noise pixels, max |albedo - fp64| {err.max():.2e}, within 1e-4: {100 * (err <= 1e-4).mean():.2f} %")
    assert (err <= 1e-4).mean() >= 0.99, float((err <= 1e-4).mean())
    assert np.ptp(albedo[noisy], axis=0).min() > 0.3  # (the texture shows: no single colour)
    for feature in (rtmi.FEATURE_NORMAL, rtmi.FEATURE_DEPTH):
        assert sc.render_feature(feature, o).tobytes() == twin.render_feature(feature, o).tobytes(), feature


def test_ray_queries_report_the_twins_records(rtmi):
    """Scene.trace on noise_sky returns the records of its solid-colour twin: a query never looks at a texture"""
    import trace_cases as TC
    sc, twin = NSC.scene(rtmi, "noise_sky"), NSC.scene(rtmi, "noise_sky", noise=False)
    boxes = [TC.prim_box(p) for p in sc.prims()[1:]]  # (every primitive but the far floor)
    lo, hi = np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)
    o, d = TC.make_rays(lo, hi)
    a, b = sc.trace(o, d), twin.trace(o, d)
    assert (a["prim"] >= 0).sum() >= 500
    assert a.tobytes() == b.tobytes()
    tex = sc.textures()["type"][sc.materials()["texture"][a["material"][a["prim"] >= 0]]]
    assert (tex == N.NOISE).sum() >= 300 and not (twin.textures()["type"] == N.NOISE).any()


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_the_cli_renders_the_shipped_scene(rtmi, tmp_path, nee):
    out = str(tmp_path / "marble.ppm")
    p = subprocess.run([os.path.join(PKG, "rtmi"), "-f", os.path.join(PKG, "scenes", "marble_hall.json"), "-w", "64", "-h", "36", "-spp", "4",
                        "-o", out, "--no-png"] + (["--nee"] if nee else []), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    sc = rtmi.Scene.load(os.path.join(PKG, "scenes", "marble_hall.json"))
    sc.override(64, 36, 4)
    sc.set_light_sampling(nee)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(), st)
    assert bool(st.kernel_variant & NSC.NEE) == nee and np.isfinite(img).all() and img.mean() > 0
    tokens = open(out).read().split()  # the reference's text PPM: P3, width, height, 255, then the 8-bit values
    assert tokens[:4] == ["P3", "64", "36", "255"] and len(tokens) == 4 + 64 * 36 * 3
    values = np.array(tokens[4:], np.int64)
    assert values.min() >= 0 and values.max() <= 255 and values.max() > 0


def test_light_sampling_is_unbiased_against_the_plain_estimator(rtmi):
    """noise_lights at 64 x 36 x 256 spp with and without light sampling: equal frame and block means, by the test
    test_gpu_light_sampling.py uses (8 seeds each; c_max: the brightest emission -- the sphere light's 7.0, above the emitter
    panel's larger colour -- over the roulette's survival probability)"""
    from test_gpu_light_sampling import compare, seeds_of
    sc = NSC.lights(rtmi, w=64, h=36, spp=256)
    c_max = max(7.0, max(NSC.EMITTER_COLOURS[1])) / 0.9
    compare(seeds_of(rtmi, sc), seeds_of(rtmi, sc, nee=True), "noise_lights", c_max=c_max)
