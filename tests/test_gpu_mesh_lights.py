"""Mesh lights (emissive triangles among the sampled emitters) on the GPU, against the fp64 statement of ref64.py
with ref64's triangle sample, sample by sample on the same draws: criteria (a) - (c) of test_gpu_nee_reference.py
with per_sample's thresholds on the five cases of mesh_light_scenes.py.  The (b) baseline is the plain kernel on the case's
plain twin (light sampling off, environment cleared, glossy materials replaced by lambertian) against the twin's reference.
Each case asserts from the reference's signatures that it holds the pinned counts of what it is there for, and prints the share
of the same formulas at fp32 in NumPy beside the kernel's.

Then: a reference with a deliberate mistake is noticed; a known answer (the analytic floor under two triangles that tile the
rectangle); the estimator against the plain one; and what every feature keeps -- the same bytes in every layout, through a
sample split and from the product library, the compact layouts refuse, and with the switch off the bytes of a scene whose
switch was never touched.

Every case prints one row of figures (pytest -s); DESIGN 7n holds the rows measured on the MI355X."""
import os
import subprocess
import sys
import textwrap
import zlib

import numpy as np
import pytest

import ext_scenes as X
import mesh_light_scenes as ML
import nee_scenes as NS
import per_sample as PS
import ref64 as R

pytestmark = pytest.mark.gpu
ROOT = PS.ROOT
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
GENERAL_LAYOUTS = (16, 36, 44)


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def words(rtmi):
    return ML.inputs(rtmi)


@pytest.fixture(scope="module")
def cases(rtmi, words):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally of ref64)): rendered and traced once"""
    made = {}

    def of(name):
        if name not in made:
            sc = ML.scene(rtmi, name)
            S = R.RefScene(sc)
            st = rtmi.Stats()
            sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=1), st)
            assert st.kernel_variant & ~ML.FAMILIES in GENERAL_LAYOUTS and st.kernel_variant & ML.FAMILIES == ML.family(name), st.kernel_variant
            got = PS.kernel_samples(rtmi, sc, NS.REF_SEED, NS.REF_K, ML.FAMILIES, ML.family(name))
            made[name] = (sc, S, got, R.reference(S, words))
        return made[name]
    return of


@pytest.mark.parametrize("name", list(ML.CASES))
def test_kernel_against_fp64(rtmi, words, cases, name):
    assert len(words) >= 16000
    sc, S, got, (ref, stable, draws, tally) = cases(name)
    assert draws.max() <= NS.REF_DRAWS, draws.max()
    ML.check_contents(name, tally)
    plain = ML.plain_twin(rtmi, name)
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    b = R.judge(PS.kernel_samples(rtmi, plain, NS.REF_SEED, NS.REF_K, ML.FAMILIES, 0), bref, bstable)
    r32, _, _ = R.trace(S, words, dtype=np.float32)
    j32 = R.judge(r32, ref, stable)
    print(f"\n    fp32 NumPy within {100 * j32['share']:.3f} %; " + ", ".join(f"{k} {v}" for k, v in tally.items() if k in ML.TALLY_KEYS))
    PS.assert_agreement(name, R.judge(got, ref, stable), b)                                # (a), (b), (c)


@pytest.mark.parametrize("name,mistake", [("lone triangle", "tri_no_sqrt"), ("lone triangle", "tri_vertex_normal"),
                                          (ML.MIXED, "tri_vertex_normal")])
def test_a_wrong_reference_is_noticed(words, cases, name, mistake):
    """against the kernel, a reference with one deliberate mistake of the triangle sample is far from 97 % (on the smooth mesh
    the vertex normal is the triangle's own first vertex normal: the density must be stated with the geometric one)"""
    sc, S, got, (ref, stable, _, _) = cases(name)
    wrong, _, _ = R.trace(S, words, perturb=(mistake,))
    good, bad = R.judge(got, ref, stable), R.judge(got, wrong, stable)
    print(f"\n{name}, {mistake}: within tolerance {100 * good['share']:.2f} % -> {100 * bad['share']:.2f} %")
    PS.assert_perturbation_noticed(good, bad)


def _mean(sc, img):
    return img.astype(np.float64).mean(axis=2) / sc.spp


def test_analytic_known_answer(rtmi):
    """nee_scenes.analytic_scene with its rectangle as two emissive triangles, 64 x 36 x 256, mesh lights on: the frame mean
    within 3 standard errors (4 seeds) + 1e-4 of the closed form, and the per-pixel error below 5 % and a quarter of the plain
    estimator's -- test_gpu_light_sampling.test_analytic_known_answer's criteria for the rectangle; then the per-pixel variance
    over 8 seeds against the same scene with mesh lights off (printed: DESIGN 7n records the ratio)"""
    from test_gpu_light_sampling import seeds_of
    sc = ML.analytic_twin(rtmi)
    exp = NS.analytic_expected(sc)
    ok = np.isfinite(exp) & (exp > 1e-3)
    assert ok.mean() > 0.9
    sc.set_light_sampling(True)
    st = rtmi.Stats()
    off = _mean(sc, sc.render(rtmi.Opts(seed=0), st))
    assert not st.kernel_variant & ML.NEE and len(sc.lights()) == 0  # switch off: no light to sample, the plain kernel
    sc.set_mesh_lights(True)
    assert len(sc.lights()) == 2
    on = [_mean(sc, sc.render(rtmi.Opts(seed=s), st)) for s in range(4)]
    assert st.kernel_variant & ML.NEE
    pm = np.array([p[ok].mean() for p in on])
    se = pm.std(ddof=1) / np.sqrt(len(pm))
    print(f"\nanalytic, two triangles: frame mean {pm.mean():.6f} against {exp[ok].mean():.6f}, standard error {se:.2e}")
    assert abs(pm.mean() - exp[ok].mean()) < 3 * se + 1e-4, (pm.mean(), exp[ok].mean(), se)
    rel_on = np.sqrt(np.mean(((on[0] - exp) / exp)[ok] ** 2))
    rel_off = np.sqrt(np.mean(((off - exp) / exp)[ok] ** 2))
    print(f"analytic, two triangles: RMS relative error per pixel at 256 spp: mesh lights off {rel_off:.4f}, on {rel_on:.4f}")
    assert rel_on < 0.05 and rel_on <= 0.25 * rel_off, (rel_on, rel_off)
    b = seeds_of(rtmi, sc, nee=True)
    sc.set_mesh_lights(False)
    a = seeds_of(rtmi, sc, nee=True)
    va, vb = a.var(axis=0, ddof=1), b.var(axis=0, ddof=1)
    lit = va > 0
    ratio = float(np.median(va[lit] / np.maximum(vb[lit], 1e-12)))
    print(f"analytic, two triangles: median per-pixel variance mesh lights off / on = {ratio:.1f}")
    assert ratio > 1.0, ratio


def test_unbiased_against_the_plain_estimator(rtmi):
    """case (iii) at 64 x 36 x 256 with and without mesh lights (light sampling on in both: without, the rectangle and the sphere
    are sampled and the mesh is found by BSDF rays alone): equal block and frame means by test_gpu_light_sampling.compare (8
    seeds each; c_max: the brightest emission)"""
    from test_gpu_light_sampling import compare, seeds_of
    sc = ML.mixed(rtmi, w=64, h=36, spp=256)
    a = seeds_of(rtmi, sc, nee=True)
    assert len(sc.lights()) == 2
    sc.set_mesh_lights(True)
    assert len(sc.lights()) == 18
    b = seeds_of(rtmi, sc, nee=True)
    compare(a, b, "smooth mesh + rect + sphere, mesh lights off / on", c_max=7.0)
    # and against the estimator without any light sampling
    sc.set_mesh_lights(False)
    compare(seeds_of(rtmi, sc), b, "smooth mesh + rect + sphere, plain / mesh lights", c_max=7.0)


_PRODUCT = textwrap.dedent("""
    import os, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, os.path.join(%r, "tests"))
    from __graft_entry__ import load_package
    rtmi = load_package()
    assert not rtmi.has_ablations()
    import mesh_light_scenes as ML, nee_scenes as NS
    for name in ("checker quad", ML.MIXED + ", env"):
        st = rtmi.Stats()
        img = ML.scene(rtmi, name).render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
        assert st.kernel_variant & ML.FAMILIES == ML.family(name), st.kernel_variant
        np.save(os.path.join(sys.argv[1], name.replace(" ", "_") + ".npy"), img)
""") % (ROOT, ROOT)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    env = dict(os.environ, RTMI_LIB=os.path.join(PKG, "librtmi_product.so"))
    p = subprocess.run([sys.executable, "-c", _PRODUCT, str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    for name in ("checker quad", ML.MIXED + ", env"):
        sc, fam, seed, st = ML.scene(rtmi, name), ML.family(name), NS.REF_SEED, rtmi.Stats()
        ref = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K), st)
        assert st.kernel_variant & ML.FAMILIES == fam and st.kernel_variant & ~ML.FAMILIES in GENERAL_LAYOUTS
        for variant in GENERAL_LAYOUTS:
            got = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K, variant=variant), st)
            assert st.kernel_variant == variant | fam, (variant, st.kernel_variant)
            assert np.array_equal(got, ref), (name, variant, float(np.abs(got - ref).max()))
        acc, _ = sc.accumulate(None, rtmi.Opts(seed=seed, sample_first=0, sample_count=5), st)
        assert st.kernel_variant & ML.FAMILIES == fam
        acc, img = sc.accumulate(acc, rtmi.Opts(seed=seed, sample_first=5, sample_count=NS.REF_K - 5), st)
        assert np.array_equal(img, ref), (name, float(np.abs(img - ref).max()))
        assert np.array_equal(np.load(str(tmp_path / (name.replace(" ", "_") + ".npy"))), ref), name
    # the compact layouts list spheres for the sphere-only kernels: a scene with a light to sample is refused there
    for variant in (2, 6):
        with pytest.raises(rtmi.RtmiError):
            ML.scene(rtmi, "lone triangle").render(rtmi.Opts(variant=variant))


def test_switch_off_renders_the_bytes_of_a_scene_never_switched(rtmi):
    """ext_scenes' "unlisted emitters" (light sampling on, a triangle emitter that is no light): a scene whose switch was never
    touched, one switched on and off again, and one switched off explicitly give the same bytes; switched on, others"""
    opts = lambda: rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K)
    st = rtmi.Stats()
    untouched = X._unlisted(rtmi).render(opts(), st)
    assert st.kernel_variant & ML.NEE
    crc = zlib.crc32(untouched.tobytes())
    sc = X._unlisted(rtmi)
    sc.set_mesh_lights(False)
    assert zlib.crc32(sc.render(opts()).tobytes()) == crc
    sc.set_mesh_lights(True)
    on = sc.render(opts(), st)
    assert st.kernel_variant & ML.NEE and zlib.crc32(on.tobytes()) != crc
    sc.set_mesh_lights(False)
    assert zlib.crc32(sc.render(opts()).tobytes()) == crc
    # without light sampling the switch changes nothing that is rendered
    plain = X._unlisted(rtmi)
    plain.set_light_sampling(False)
    a = plain.render(opts(), st)
    assert not st.kernel_variant & ML.NEE
    plain.set_mesh_lights(True)
    assert np.array_equal(plain.render(opts(), st), a) and not st.kernel_variant & ML.NEE
