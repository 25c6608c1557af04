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
import zlib

import numpy as np
import pytest

import ext_scenes as X
import mesh_light_scenes as ML
import nee_scenes as NS
import per_sample as PS
import ref64 as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    return PS.input_cache(rtmi, ML)


@pytest.fixture(scope="module")
def cases(rtmi, inputs):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)): rendered and traced once, shared by the tests"""
    return PS.case_cache(rtmi, ML, inputs)


@pytest.mark.parametrize("name", list(ML.CASES))
def test_kernel_against_fp64(rtmi, inputs, cases, name):
    sc, S, got, (ref, stable, draws, tally) = cases(name)
    r32, _, _ = R.trace(S, inputs(name)[0], dtype=np.float32)
    print(f"\n    fp32 NumPy within {100 * R.judge(r32, ref, stable)['share']:.3f} %; " + ", ".join(f"{k} {v}" for k, v in tally.items() if k in ML.TALLY_KEYS))
    PS.check_kernel_against_fp64(rtmi, ML, inputs, cases, name)


@pytest.mark.parametrize("name,mistake", [("lone triangle", "tri_no_sqrt"), ("lone triangle", "tri_vertex_normal"),
                                          (ML.MIXED, "tri_vertex_normal")])
def test_a_wrong_reference_is_noticed(inputs, cases, name, mistake):
    PS.check_a_mistake_fails_the_agreement(inputs, cases, name, mistake)


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


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    PS.check_same_bytes(rtmi, ML, ("checker quad", ML.MIXED + ", env"), tmp_path)
    PS.check_compact_layouts_refuse(rtmi, lambda: ML.scene(rtmi, "lone triangle"))  # (a scene with a light to sample)


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
