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
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import nee_scenes as NS
import normal_map_scenes as NMS
import per_sample as PS
import ref64 as R
import ref64_normal_map as NM

pytestmark = pytest.mark.gpu
ROOT = PS.ROOT
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
GENERAL_LAYOUTS = (16, 36, 44)  # a scene with a map runs the general (EXT) builds: never the compact layouts 2 / 6
NESTED_LAYOUT = 52


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    made = {}

    def of(name):
        key = (NMS.seed_of(name), NMS.family(name) == NMS.MOTION)
        if key not in made:
            made[key] = NMS.inputs(rtmi, name)
        return made[key]
    return of


@pytest.fixture(scope="module")
def cases(rtmi, inputs):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally), map tally): rendered and traced once, shared"""
    made = {}

    def of(name):
        if name not in made:
            words, shutter = inputs(name)
            sc = NMS.scene(rtmi, name)
            S = R.RefScene(sc)
            st = rtmi.Stats()
            sc.render(rtmi.Opts(seed=NMS.seed_of(name), sample_count=1), st)
            assert st.kernel_variant & ~NMS.FAMILIES in GENERAL_LAYOUTS and st.kernel_variant & NMS.FAMILIES == NMS.family(name), st.kernel_variant
            got = PS.kernel_samples(rtmi, sc, NMS.seed_of(name), NS.REF_K, NMS.FAMILIES, NMS.family(name))
            ref = R.reference(S, words, shutter)
            made[name] = (sc, S, got, ref, {k: v for k, v in ref[3].items() if k.startswith("nm_")})
        return made[name]
    return of


@pytest.mark.parametrize("name", list(NMS.CASES))
def test_kernel_against_fp64(rtmi, inputs, cases, name):
    words, shutter = inputs(name)
    assert len(words) >= 16000
    sc, S, got, (ref, stable, draws, tally), map_tally = cases(name)
    assert draws.max() <= NS.REF_DRAWS, draws.max()                                        # (d)
    print("\n    " + ", ".join(f"{k} {v if isinstance(v, int) else round(v, 3)}" for k, v in map_tally.items() if v))
    NMS.check_contents(name, map_tally)
    plain = NMS.plain_twin(rtmi, name)
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    b = R.judge(PS.kernel_samples(rtmi, plain, NMS.seed_of(name), NS.REF_K, NMS.FAMILIES, 0), bref, bstable)
    PS.assert_agreement(name, R.judge(got, ref, stable), b)                                # (a), (b), (c)


@pytest.mark.parametrize("name,mistake", NMS.MISTAKES)
def test_a_mistake_fails_the_agreement(inputs, cases, name, mistake):
    """(d): against the kernel, a reference with one deliberate mistake of the model is far from 97 %"""
    words, shutter = inputs(name)
    sc, S, got, (ref, stable, _, _), _ = cases(name)
    wrong, _, _ = R.trace(S, words, shutter=shutter, perturb=(mistake,))
    good, bad = R.judge(got, ref, stable), R.judge(got, wrong, stable)
    print(f"\n{name}, {mistake}: within tolerance {100 * good['share']:.2f} % -> {100 * bad['share']:.2f} %")
    PS.assert_perturbation_noticed(good, bad)


@pytest.mark.parametrize("name", ["nm_sky", "nm_lights"])
def test_a_constant_map_renders_the_twins_bytes(rtmi, name):
    """every map replaced by a constant (128, 128, 255) image: such a texel leaves n untouched, so the frame is the twin's in
    every general layout -- and the maps were read: the material word is set, the scene packs to other bytes"""
    still, twin = NMS.scene(rtmi, name, maps="flat"), NMS.scene(rtmi, name, maps=False)
    assert sum(still.normal_map(m) is not None for m in range(len(still.materials()))) >= 4
    assert still.table_image().tobytes() != twin.table_image().tobytes()
    st = rtmi.Stats()
    for variant in GENERAL_LAYOUTS:
        o = rtmi.Opts(seed=NMS.seed_of(name), sample_count=NS.REF_K, variant=variant)
        a = still.render(o, st)
        assert st.kernel_variant == variant | NMS.family(name), (variant, st.kernel_variant)
        b = twin.render(o, st)
        assert st.kernel_variant == variant | NMS.family(name), (variant, st.kernel_variant)
        assert a.tobytes() == b.tobytes(), (name, variant, float(np.abs(a - b).max()))
    assert not np.array_equal(NMS.scene(rtmi, name).render(rtmi.Opts(seed=NMS.seed_of(name), sample_count=NS.REF_K), st), b)  # (a relief shows)


_PRODUCT = textwrap.dedent("""
    import os, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, os.path.join(%r, "tests"))
    from __graft_entry__ import load_package
    rtmi = load_package()
    assert not rtmi.has_ablations()
    import normal_map_scenes as NMS, nee_scenes as NS
    for name in ("nm_sky", "nm_lights"):
        st = rtmi.Stats()
        img = NMS.scene(rtmi, name).render(rtmi.Opts(seed=NMS.seed_of(name), sample_count=NS.REF_K), st)
        assert st.kernel_variant & NMS.FAMILIES == NMS.family(name), st.kernel_variant
        np.save(os.path.join(sys.argv[1], name + ".npy"), img)
""") % (ROOT, ROOT)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    env = dict(os.environ, RTMI_LIB=os.path.join(PKG, "librtmi_product.so"))
    p = subprocess.run([sys.executable, "-c", _PRODUCT, str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    for name in ("nm_sky", "nm_lights"):
        sc, fam, seed, st = NMS.scene(rtmi, name), NMS.family(name), NMS.seed_of(name), rtmi.Stats()
        ref = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K), st)
        assert st.kernel_variant & NMS.FAMILIES == fam and st.kernel_variant & ~NMS.FAMILIES in GENERAL_LAYOUTS
        for variant in GENERAL_LAYOUTS:
            got = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K, variant=variant), st)
            assert st.kernel_variant == variant | fam, (variant, st.kernel_variant)
            assert np.array_equal(got, ref), (name, variant, float(np.abs(got - ref).max()))
        acc, _ = sc.accumulate(None, rtmi.Opts(seed=seed, sample_first=0, sample_count=5), st)
        assert st.kernel_variant & NMS.FAMILIES == fam
        acc, img = sc.accumulate(acc, rtmi.Opts(seed=seed, sample_first=5, sample_count=NS.REF_K - 5), st)
        assert np.array_equal(img, ref), (name, float(np.abs(img - ref).max()))
        assert np.array_equal(np.load(str(tmp_path / (name + ".npy"))), ref), name


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
    assert st.kernel_variant == NESTED_LAYOUT
    twin = NMS.nested(rtmi, maps=False).render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert not np.array_equal(nested, twin)  # (the maps show)
    sc.set_nested_grid(False)
    flat = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant in GENERAL_LAYOUTS and np.array_equal(nested, flat)


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
    import trace_cases as TC
    sc, twin = NMS.scene(rtmi, "nm_prims"), NMS.scene(rtmi, "nm_prims", maps=False)
    boxes = [TC.prim_box(p) for p in sc.prims()[1:] if int(p["type"]) != 6]  # (every primitive but the far floor; the box's faces lie among them)
    lo, hi = np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)
    o, d = TC.make_rays(lo, hi)
    a, b = sc.trace(o, d), twin.trace(o, d)
    hit = a["prim"] >= 0
    assert hit.sum() >= 500
    assert a.tobytes() == b.tobytes()
    assert sum(sc.normal_map(int(m)) is not None for m in a["material"][hit]) >= 300


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_the_cli_renders_the_shipped_scene(rtmi, tmp_path, nee):
    out = str(tmp_path / "wall.ppm")
    p = subprocess.run([os.path.join(PKG, "rtmi"), "-f", os.path.join(PKG, "scenes", "normal_map_wall.json"), "-w", "64", "-h", "36", "-spp", "4",
                        "-o", out, "--no-png"] + (["--nee"] if nee else []), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    sc = rtmi.Scene.load(os.path.join(PKG, "scenes", "normal_map_wall.json"))
    assert sum(sc.normal_map(m) is not None for m in range(len(sc.materials()))) >= 5
    sc.override(64, 36, 4)
    sc.set_light_sampling(nee)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(), st)
    assert bool(st.kernel_variant & NMS.NEE) == nee and np.isfinite(img).all() and img.mean() > 0
    tokens = open(out).read().split()  # the reference's text PPM: P3, width, height, 255, then the 8-bit values
    assert tokens[:4] == ["P3", "64", "36", "255"] and len(tokens) == 4 + 64 * 36 * 3
    values = np.array(tokens[4:], np.int64)
    assert values.min() >= 0 and values.max() <= 255 and values.max() > 0


def test_light_sampling_is_unbiased_against_the_plain_estimator(rtmi):
    """nm_lights' area light at 64 x 36 x 256 spp with and without light sampling: equal frame and block means, by the test and
    the bounds test_gpu_light_sampling.py uses (8 seeds each; c_max: the brightest emission, 6.0, over the roulette's survival
    probability).  The point light is taken out: the plain estimator cannot see a light without area"""
    from test_gpu_light_sampling import compare, seeds_of
    sc = NMS.lights(rtmi, w=64, h=36, spp=256)
    sc.clear_analytic_lights()
    compare(seeds_of(rtmi, sc), seeds_of(rtmi, sc, nee=True), "nm_lights", c_max=6.0 / 0.9)
