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
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import bump_scenes as BS
import nee_scenes as NS
import per_sample as PS
import ref64 as R

pytestmark = pytest.mark.gpu
ROOT = PS.ROOT
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
GENERAL_LAYOUTS = (16, 36, 44)  # a scene with a bump runs the general (EXT) builds: never the compact layouts 2 / 6
NESTED_LAYOUT = 52


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    made = {}

    def of(name):
        key = (BS.seed_of(name), BS.family(name) == BS.MOTION)
        if key not in made:
            made[key] = BS.inputs(rtmi, name)
        return made[key]
    return of


@pytest.fixture(scope="module")
def cases(rtmi, inputs):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally), bump tally): rendered and traced once, shared"""
    made = {}

    def of(name):
        if name not in made:
            words, shutter = inputs(name)
            sc = BS.scene(rtmi, name)
            S = R.RefScene(sc)
            st = rtmi.Stats()
            sc.render(rtmi.Opts(seed=BS.seed_of(name), sample_count=1), st)
            assert st.kernel_variant & ~BS.FAMILIES in GENERAL_LAYOUTS and st.kernel_variant & BS.FAMILIES == BS.family(name), st.kernel_variant
            got = PS.kernel_samples(rtmi, sc, BS.seed_of(name), NS.REF_K, BS.FAMILIES, BS.family(name))
            ref = R.reference(S, words, shutter)
            made[name] = (sc, S, got, ref, {k: v for k, v in ref[3].items() if k.startswith("bump_")})
        return made[name]
    return of


@pytest.mark.parametrize("name", list(BS.CASES))
def test_kernel_against_fp64(rtmi, inputs, cases, name):
    words, shutter = inputs(name)
    assert len(words) >= 16000
    sc, S, got, (ref, stable, draws, tally), bump_tally = cases(name)
    assert draws.max() <= NS.REF_DRAWS, draws.max()                                        # (d)
    BS.check_contents(name, bump_tally)
    plain = BS.plain_twin(rtmi, name)
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    b = R.judge(PS.kernel_samples(rtmi, plain, BS.seed_of(name), NS.REF_K, BS.FAMILIES, 0), bref, bstable)
    PS.assert_agreement(name, R.judge(got, ref, stable), b)                                # (a), (b), (c)
    print("    " + ", ".join(f"{k} {v if isinstance(v, int) else round(v, 3)}" for k, v in bump_tally.items() if v))


@pytest.mark.parametrize("name,mistake", BS.MISTAKES)
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
    import bump_scenes as BS, nee_scenes as NS
    for name in ("bump_sky", "bump_lights"):
        st = rtmi.Stats()
        img = BS.scene(rtmi, name).render(rtmi.Opts(seed=BS.seed_of(name), sample_count=NS.REF_K), st)
        assert st.kernel_variant & BS.FAMILIES == BS.family(name), st.kernel_variant
        np.save(os.path.join(sys.argv[1], name + ".npy"), img)
""") % (ROOT, ROOT)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    env = dict(os.environ, RTMI_LIB=os.path.join(PKG, "librtmi_product.so"))
    p = subprocess.run([sys.executable, "-c", _PRODUCT, str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    for name in ("bump_sky", "bump_lights"):
        sc, fam, seed, st = BS.scene(rtmi, name), BS.family(name), BS.seed_of(name), rtmi.Stats()
        ref = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K), st)
        assert st.kernel_variant & BS.FAMILIES == fam and st.kernel_variant & ~BS.FAMILIES in GENERAL_LAYOUTS
        twin = BS.scene(rtmi, name, bump=False).render(rtmi.Opts(seed=seed, sample_count=NS.REF_K), st)
        assert not np.array_equal(ref, twin)  # (the bumps show)
        for variant in GENERAL_LAYOUTS:
            got = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K, variant=variant), st)
            assert st.kernel_variant == variant | fam, (variant, st.kernel_variant)
            assert np.array_equal(got, ref), (name, variant, float(np.abs(got - ref).max()))
        acc, _ = sc.accumulate(None, rtmi.Opts(seed=seed, sample_first=0, sample_count=5), st)
        assert st.kernel_variant & BS.FAMILIES == fam
        acc, img = sc.accumulate(acc, rtmi.Opts(seed=seed, sample_first=5, sample_count=NS.REF_K - 5), st)
        assert np.array_equal(img, ref), (name, float(np.abs(img - ref).max()))
        assert np.array_equal(np.load(str(tmp_path / (name + ".npy"))), ref), name


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
    assert np.array_equal(sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st), flat) and st.kernel_variant in GENERAL_LAYOUTS
    sc = BS.nested(rtmi)
    assert sc.nested_info().cells > 0
    nested = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant == NESTED_LAYOUT
    twin = BS.nested(rtmi, bump=False).render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert not np.array_equal(nested, twin)  # (the bumps show)
    sc.set_nested_grid(False)
    flat = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant in GENERAL_LAYOUTS and np.array_equal(nested, flat)


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
    import trace_cases as TC
    sc, twin = BS.scene(rtmi, "bump_prims"), BS.scene(rtmi, "bump_prims", bump=False)
    boxes = [TC.prim_box(p) for p in sc.prims()[1:]]  # (every primitive but the far floor)
    lo, hi = np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)
    o, d = TC.make_rays(lo, hi)
    a, b = sc.trace(o, d), twin.trace(o, d)
    hit = a["prim"] >= 0
    assert hit.sum() >= 500
    assert a.tobytes() == b.tobytes()
    assert sum(sc.bump(int(m)) is not None for m in a["material"][hit]) >= 300


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_the_cli_renders_the_shipped_scene(rtmi, tmp_path, nee):
    out = str(tmp_path / "pond.ppm")
    p = subprocess.run([os.path.join(PKG, "rtmi"), "-f", os.path.join(PKG, "scenes", "bumpy_pond.json"), "-w", "64", "-h", "36", "-spp", "4",
                        "-o", out, "--no-png"] + (["--nee"] if nee else []), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    sc = rtmi.Scene.load(os.path.join(PKG, "scenes", "bumpy_pond.json"))
    sc.override(64, 36, 4)
    sc.set_light_sampling(nee)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(), st)
    assert bool(st.kernel_variant & BS.NEE) == nee and np.isfinite(img).all() and img.mean() > 0
    tokens = open(out).read().split()  # the reference's text PPM: P3, width, height, 255, then the 8-bit values
    assert tokens[:4] == ["P3", "64", "36", "255"] and len(tokens) == 4 + 64 * 36 * 3
    values = np.array(tokens[4:], np.int64)
    assert values.min() >= 0 and values.max() <= 255 and values.max() > 0


def test_light_sampling_is_unbiased_against_the_plain_estimator(rtmi):
    """bump_lights at 64 x 36 x 256 spp with and without light sampling: equal frame and block means, by the test and the bounds
    test_gpu_light_sampling.py uses (8 seeds each; c_max: the brightest emission, the sphere light's 7.0, over the roulette's
    survival probability)"""
    from test_gpu_light_sampling import compare, seeds_of
    sc = BS.lights(rtmi, w=64, h=36, spp=256)
    compare(seeds_of(rtmi, sc), seeds_of(rtmi, sc, nee=True), "bump_lights", c_max=7.0 / 0.9)
