"""What the GPU tests of the per-sample comparison share (test_gpu_nee_reference.py states the criteria (a)-(d)): the package
with a device behind it, the one-sample frames of a kernel family, the verdict on a comparison, and the refusal check.  Then
the bodies of the fixtures and tests that every feature suite (test_gpu_{quads,glossy,glass,noise,bump,normal_map,pbr,alpha,
mesh_lights,analytic_lights}.py) holds: the case cache, the fp64 check, the mistake check, the same-bytes check, the command-line
check and the ray-query check.  Each takes the feature's scenes module M (feature_scenes.py says what one provides).  Plain
functions: the fixtures stay in the test files, which skip each on its own.  Last, what test_phase.py and test_media_nee.py
share on the host: the check against golden/ref64_media_pin.npz."""
import hashlib
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import feature_scenes as FS
import nee_scenes as NS
import ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
GENERAL_LAYOUTS = (16, 36, 44)  # a scene with a feature runs the general (EXT) builds: never the compact layouts 2 / 6
NESTED_LAYOUT = 52


def gpu_package():
    """the package, or a skip where there is no device"""
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    mod = load_package()
    if mod.device_count() < 1:
        pytest.skip("no HIP device")
    return mod


def kernel_samples(rtmi, sc, seed, k, mask, family, variant=0):
    """[k x H x W][3]: the radiance of every sample, from one-sample frames; the kernel family is checked on each, and the
    layout where one is asked for (variant: 0 is the scene's own)"""
    out = []
    for i in range(k):
        st = rtmi.Stats()
        out.append(sc.render(rtmi.Opts(seed=seed, sample_first=i, sample_count=1, variant=variant), st))
        assert st.kernel_variant & mask == family, (st.kernel_variant, family)
        if variant:
            assert st.kernel_variant & ~mask == variant, (st.kernel_variant, variant)
    return np.stack(out).reshape(-1, 3).astype(np.float64)


def assert_agreement(name, j, b):
    """the verdict on R.judge's figures of a kernel (j) and of the plain kernel on the scene's plain twin (b); prints the row"""
    print("\n" + R.row(name, j, b["share_stable"]))
    assert j["flips"] <= 0.01, j["flips"]
    assert j["share"] >= 0.97, j                                                                   # (a)
    assert j["share_stable"] >= b["share_stable"] - 0.005, (j["share_stable"], b["share_stable"])  # (b)
    assert j["bias_ok"], (j["mean_diff"], j["z"])                                                  # (c)


def assert_perturbation_noticed(good, bad):
    """(d): the kernel agrees with the reference and is far from 97 % against a reference with a deliberate mistake"""
    assert good["share"] >= 0.97 and bad["share"] < 0.97, (good["share"], bad["share"])


def refused(rtmi, call):
    with pytest.raises(rtmi.RtmiError) as e:
        call()
    assert e.value.status == 1, str(e.value)  # RT_ERR_ARG
    return str(e.value)


# ---------------------------------------------------------------------------------------------- what the feature suites share
def input_cache(rtmi, M):
    """the body of an `inputs` fixture: of(name) -> (uniforms, shutter times or None), made once per seed and family"""
    made = {}

    def of(name):
        key = (M.seed_of(name), M.family(name) == FS.MOTION)
        if key not in made:
            made[key] = M.inputs(rtmi, name)
        return made[key]
    return of


def case_cache(rtmi, M, inputs, nested=()):
    """the body of a `cases` fixture: of(name) -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)), rendered and
    traced once.  The first frame's layout is a general one (the nested one for the cases named in `nested`) and its family bits
    are the case's"""
    made = {}

    def of(name):
        if name not in made:
            words, shutter = inputs(name)
            sc = M.scene(rtmi, name)
            S = R.RefScene(sc)
            st = rtmi.Stats()
            sc.render(rtmi.Opts(seed=M.seed_of(name), sample_count=1), st)
            layouts = (NESTED_LAYOUT,) if name in nested else GENERAL_LAYOUTS
            assert st.kernel_variant & ~M.FAMILIES in layouts and st.kernel_variant & M.FAMILIES == M.family(name), st.kernel_variant
            got = kernel_samples(rtmi, sc, M.seed_of(name), NS.REF_K, M.FAMILIES, M.family(name))
            made[name] = (sc, S, got, R.reference(S, words, shutter))
        return made[name]
    return of


def check_kernel_against_fp64(rtmi, M, inputs, cases, name):
    """the body of test_kernel_against_fp64: the draws bound (d), the case's contents, and criteria (a) - (c) with the plain
    kernel on the case's plain twin as the baseline of (b)"""
    words, shutter = inputs(name)
    assert len(words) >= 16000
    sc, S, got, (ref, stable, draws, tally) = cases(name)
    assert draws.max() <= NS.REF_DRAWS, draws.max()                                        # (d)
    M.check_contents(name, tally)
    plain = M.plain_twin(rtmi, name)
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    b = R.judge(kernel_samples(rtmi, plain, M.seed_of(name), NS.REF_K, M.FAMILIES, 0), bref, bstable)
    assert_agreement(name, R.judge(got, ref, stable), b)                                   # (a), (b), (c)


def check_a_mistake_fails_the_agreement(inputs, cases, name, mistake):
    """(d): against the kernel, a reference with one deliberate mistake of the model is far from 97 %"""
    words, shutter = inputs(name)
    sc, S, got, (ref, stable, _, _) = cases(name)
    wrong, _, _ = R.trace(S, words, shutter=shutter, perturb=(mistake,))
    good, bad = R.judge(got, ref, stable), R.judge(got, wrong, stable)
    print(f"\n{name}, {mistake}: within tolerance {100 * good['share']:.2f} % -> {100 * bad['share']:.2f} %")
    assert_perturbation_noticed(good, bad)


# the child of check_same_bytes: argv = [directory, scenes module, case names ...], RTMI_LIB names the product library
_PRODUCT = textwrap.dedent("""
    import importlib, os, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, os.path.join(%r, "tests"))
    from __graft_entry__ import load_package
    rtmi = load_package()
    assert not rtmi.has_ablations()
    import nee_scenes as NS
    M = importlib.import_module(sys.argv[2])
    for name in sys.argv[3:]:
        st = rtmi.Stats()
        img = M.scene(rtmi, name).render(rtmi.Opts(seed=M.seed_of(name), sample_count=NS.REF_K), st)
        assert st.kernel_variant & M.FAMILIES == M.family(name), st.kernel_variant
        np.save(os.path.join(sys.argv[1], name.replace(" ", "_") + ".npy"), img)
""") % (ROOT, ROOT)


def check_same_bytes(rtmi, M, names, tmp_path, twin=None):
    """the body of test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes: every general layout, a 5 + 8 sample
    split and the product library (a fresh process) give the frame of the scene's own layout; twin(name), where given, is a
    scene without the feature whose frame must differ"""
    env = dict(os.environ, RTMI_LIB=os.path.join(PKG, "librtmi_product.so"))
    p = subprocess.run([sys.executable, "-c", _PRODUCT, str(tmp_path), M.__name__] + list(names), capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    for name in names:
        sc, fam, seed, st = M.scene(rtmi, name), M.family(name), M.seed_of(name), rtmi.Stats()
        ref = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K), st)
        assert st.kernel_variant & M.FAMILIES == fam and st.kernel_variant & ~M.FAMILIES in GENERAL_LAYOUTS
        if twin is not None:
            assert not np.array_equal(ref, twin(name).render(rtmi.Opts(seed=seed, sample_count=NS.REF_K), st))  # (the feature shows)
        for variant in GENERAL_LAYOUTS:
            got = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K, variant=variant), st)
            assert st.kernel_variant == variant | fam, (variant, st.kernel_variant)
            assert np.array_equal(got, ref), (name, variant, float(np.abs(got - ref).max()))
        acc, _ = sc.accumulate(None, rtmi.Opts(seed=seed, sample_first=0, sample_count=5), st)
        assert st.kernel_variant & M.FAMILIES == fam
        acc, img = sc.accumulate(acc, rtmi.Opts(seed=seed, sample_first=5, sample_count=NS.REF_K - 5), st)
        assert np.array_equal(img, ref), (name, float(np.abs(img - ref).max()))
        assert np.array_equal(np.load(str(tmp_path / (name.replace(" ", "_") + ".npy"))), ref), name


def check_compact_layouts_refuse(rtmi, make):
    """the compact layouts list spheres for the sphere-only kernels, which know no feature: make()'s scene is refused there"""
    for variant in (2, 6):
        with pytest.raises(rtmi.RtmiError):
            make().render(rtmi.Opts(variant=variant))


def check_cli(rtmi, tmp_path, scene_file, nee, nee_bit, height=36, loaded=None):
    """the body of test_the_cli_renders_the_shipped_scene: rtmi renders scenes/<scene_file> at 64 x height x 4 to a text PPM, with
    or without --nee; the library renders it in the family that says; loaded(scene): what else must hold of the file's scene"""
    out, scene = str(tmp_path / "out.ppm"), os.path.join(PKG, "scenes", scene_file)
    p = subprocess.run([os.path.join(PKG, "rtmi"), "-f", scene, "-w", "64", "-h", str(height), "-spp", "4", "-o", out, "--no-png"]
                       + (["--nee"] if nee else []), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    sc = rtmi.Scene.load(scene)
    assert loaded is None or loaded(sc)
    sc.override(64, height, 4)
    sc.set_light_sampling(nee)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(), st)
    assert bool(st.kernel_variant & nee_bit) == nee and np.isfinite(img).all() and img.mean() > 0
    tokens = open(out).read().split()  # the reference's text PPM: P3, width, height, 255, then the 8-bit values
    assert tokens[:4] == ["P3", "64", str(height), "255"] and len(tokens) == 4 + 64 * height * 3
    values = np.array(tokens[4:], np.int64)
    assert values.min() >= 0 and values.max() <= 255 and values.max() > 0


def check_ray_queries_of_twins(sc, twin, bound):
    """the body of test_ray_queries_report_the_twins_records: Scene.trace returns the same records on a scene and its twin
    (queries are for geometry), on rays into the box of the primitives bound(sc.prims()) selects, at least 500 of which hit.
    Returns (the records, which of them hit) for what the feature asserts about them"""
    import trace_cases as TC
    boxes = [TC.prim_box(p) for p in bound(sc.prims())]
    lo, hi = np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)
    o, d = TC.make_rays(lo, hi)
    a, b = sc.trace(o, d), twin.trace(o, d)
    hit = a["prim"] >= 0
    assert hit.sum() >= 500
    assert a.tobytes() == b.tobytes()
    return a, hit


def check_media_pin(rtmi, golden_dir, key, sc):
    """golden/ref64_media_pin.npz holds what the reference returned on `key`'s case while anisotropic media and light sampling
    in media were path tracers of their own beside ref64.trace (golden/make_ref64_media_pin.py).  Exact: the draws of the fp64 and
    the fp32 run, which samples took the same branches at fp32, every count of that commit's tally; the fp64 radiance after
    rounding to float32, as it is stored; the fp32 run's by its bytes.  sc: the case's scene, brought to the pinned frame here.
    Returns (RefScene, the uniforms, the fp64 radiance, the tally)"""
    pin = np.load(os.path.join(golden_dir, "ref64_media_pin.npz"))
    cases = json.loads(str(pin["cases"]))
    size = lambda c: c["width"] * c["height"] * c["samples"]
    rec, at = cases[key], sum(size(c) for c in list(cases.values())[:list(cases).index(key)])
    n = size(rec)
    sc.override(width=rec["width"], height=rec["height"])
    words = R.uniforms(rtmi, rec["seed"], rec["width"], rec["height"], 0, rec["samples"], rec["draws"])
    S, log = R.RefScene(sc), R.new_log()
    rgb, sig, draws = R.trace(S, words, log=log)
    rgb32, sig32, draws32 = R.trace(S, words, dtype=np.float32)
    tally = R.tally(sig, S, log)
    assert np.array_equal(draws, pin["draws64"][at:at + n]) and np.array_equal(draws32 - draws, pin["draws32_minus_64"][at:at + n]), key
    assert np.array_equal(np.packbits(R.same_signature(sig, sig32)), pin["stable"][at // 8:(at + n) // 8]), key
    assert {k: tally[k] for k in rec["tally"]} == rec["tally"], (key, tally)
    assert np.allclose(rgb.astype(np.float32), pin["rgb64"][at:at + n], rtol=1e-9, atol=1e-12), key
    assert hashlib.sha256(np.ascontiguousarray(rgb32).tobytes()).hexdigest() == rec["rgb32"], key
    return S, words, rgb, tally
