"""Quads and boxes on the GPU, against the fp64 statement of ref64.py, sample by sample on
the same draws: criteria (a) - (c) of test_gpu_nee_reference.py with per_sample's thresholds on the six cases of
quad_scenes.py.  The (b) baseline is the plain kernel on the case's triangle twin (every quad as its two triangles; light
sampling off, environment, media and movers cleared) against that twin's reference.  Each case asserts from the reference's
signatures that it holds what it is there for.

Then: (d) a reference with one of the three deliberate mistakes is noticed; and what every feature keeps -- the same bytes in
every layout (the nested one on a scene that nests), through a sample split and from the product library; feature buffers on
quad pixels; ray queries on arbitrary rays against fp64; light sampling against the plain estimator; the command line on the
shipped scene.

Every case prints one row of figures (pytest -s); DESIGN 7q holds the rows measured on the MI355X."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import nee_scenes as NS
import per_sample as PS
import quad_scenes as Q
import ref64 as R

pytestmark = pytest.mark.gpu
ROOT = PS.ROOT
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
GENERAL_LAYOUTS = (16, 36, 44)


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    made = {}

    def of(name):
        key = Q.seed_of(name), Q.family(name) == Q.MOTION
        if key not in made:
            made[key] = Q.inputs(rtmi, name)
        return made[key]
    return of


@pytest.fixture(scope="module")
def cases(rtmi, inputs):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally of ref64)): rendered and traced once"""
    made = {}

    def of(name):
        if name not in made:
            sc = Q.scene(rtmi, name)
            S = R.RefScene(sc)
            words, shutter = inputs(name)
            got = PS.kernel_samples(rtmi, sc, Q.seed_of(name), NS.REF_K, Q.FAMILIES, Q.family(name))
            made[name] = (sc, S, got, R.reference(S, words, shutter))
        return made[name]
    return of


@pytest.mark.parametrize("name", list(Q.CASES))
def test_kernel_against_fp64(rtmi, inputs, cases, name):
    sc, S, got, (ref, stable, draws, tally) = cases(name)
    words, shutter = inputs(name)
    assert len(words) >= 16000 and draws.max() <= NS.REF_DRAWS, draws.max()
    Q.check_contents(name, tally)
    plain = Q.plain_twin(rtmi, name)
    assert not (plain.prims()["type"] == Q.QUAD).any()
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    b = R.judge(PS.kernel_samples(rtmi, plain, Q.seed_of(name), NS.REF_K, Q.FAMILIES, 0), bref, bstable)
    print("\n    " + ", ".join(f"{k} {tally[k]}" for k in Q.CASES[name][3]))
    PS.assert_agreement(name, R.judge(got, ref, stable), b)                                # (a), (b), (c)


@pytest.mark.parametrize("name,mistake", Q.MISTAKES)
def test_a_wrong_reference_is_noticed(inputs, cases, name, mistake):
    """(d): against the kernel, a reference with one deliberate mistake is far from 97 %"""
    sc, S, got, (ref, stable, _, _) = cases(name)
    words, shutter = inputs(name)
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
    import quad_scenes as Q, nee_scenes as NS
    for name in ("quad_sky", Q.CORNELL):
        st = rtmi.Stats()
        img = Q.scene(rtmi, name).render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
        assert st.kernel_variant & Q.FAMILIES == Q.family(name), st.kernel_variant
        np.save(os.path.join(sys.argv[1], name + ".npy"), img)
""") % (ROOT, ROOT)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    env = dict(os.environ, RTMI_LIB=os.path.join(PKG, "librtmi_product.so"))
    p = subprocess.run([sys.executable, "-c", _PRODUCT, str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    for name in ("quad_sky", Q.CORNELL):
        sc, fam, seed, st = Q.scene(rtmi, name), Q.family(name), NS.REF_SEED, rtmi.Stats()
        ref = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K), st)
        assert st.kernel_variant & Q.FAMILIES == fam and st.kernel_variant & ~Q.FAMILIES in GENERAL_LAYOUTS
        for variant in GENERAL_LAYOUTS:
            got = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K, variant=variant), st)
            assert st.kernel_variant == variant | fam, (variant, st.kernel_variant)
            assert np.array_equal(got, ref), (name, variant, float(np.abs(got - ref).max()))
        acc, _ = sc.accumulate(None, rtmi.Opts(seed=seed, sample_first=0, sample_count=5), st)
        assert st.kernel_variant & Q.FAMILIES == fam
        acc, img = sc.accumulate(acc, rtmi.Opts(seed=seed, sample_first=5, sample_count=NS.REF_K - 5), st)
        assert np.array_equal(img, ref), (name, float(np.abs(img - ref).max()))
        assert np.array_equal(np.load(str(tmp_path / (name + ".npy"))), ref), name
    # the nested clump of boxes: its own layout against the flat wide-table walk and the linear scan of the same scene
    sc, st = Q.nested(rtmi), rtmi.Stats()
    nested = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant == Q.NESTED_LAYOUT and nested.mean() > 0
    scan = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K, variant=16), st)
    assert st.kernel_variant == 16 and np.array_equal(nested, scan)
    sc.set_nested_grid(False)
    flat = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant in GENERAL_LAYOUTS and np.array_equal(nested, flat)
    # the compact layouts list spheres for the sphere-only kernels, which know no quad: refused
    for variant in (2, 6):
        with pytest.raises(rtmi.RtmiError):
            Q.scene(rtmi, "quad_sky").render(rtmi.Opts(variant=variant))


def test_feature_buffers_on_quad_pixels(rtmi):
    """four-sample feature passes of the Cornell case: a pixel whose summed normal has length 4 saw one flat face with all four
    samples -- its normal is then a stored quad normal, turned, and its albedo that quad's colour; such pixels are most of the
    frame; the depth pass covers every pixel (the room closes the view)"""
    sc = Q.scene(rtmi, Q.CORNELL)
    o = rtmi.Opts(seed=NS.REF_SEED, sample_first=0, sample_count=4)
    nrm = sc.render_feature(rtmi.FEATURE_NORMAL, o).reshape(-1, 3).astype(np.float64) / 4
    alb = sc.render_feature(rtmi.FEATURE_ALBEDO, o).reshape(-1, 3).astype(np.float64) / 4
    dep = sc.render_feature(rtmi.FEATURE_DEPTH, o).reshape(-1, 3).astype(np.float64) / 4
    flat = np.abs(np.linalg.norm(nrm, axis=1) - 1) < 1e-6
    assert flat.mean() > 0.8, flat.mean()
    P = sc.prims()
    quads = P[P["type"] == Q.QUAD]
    N = quads["m"][:, 9:12].astype(np.float64)
    cos = nrm[flat] @ N.T
    assert (np.abs(cos).max(axis=1) > 1 - 1e-6).all()
    mats, texs = sc.materials(), sc.textures()
    colours = {tuple(np.round(texs["c0"][mats["texture"][m]].astype(np.float64), 6)) for m in set(quads["material"].tolist()) if mats["texture"][m] >= 0}
    colours.add((0.8, 0.8, 0.85))  # the metal box's albedo
    seen = {tuple(np.round(c, 6)) for c in alb[flat]}
    assert len(seen & colours) >= 4 and (dep[:, 1] > 0.9).mean() > 0.95, (seen & colours, dep[:, 1].mean())


def test_ray_queries_against_fp64(rtmi):
    """Scene.trace on arbitrary rays into the sky case's boxes over a floor quad, test_gpu_trace.py's thresholds: the
    same primitive as the fp64 closest hit for at least 99 % of the rays, t within 2e-5 relative; point within 1e-5, normal
    within 2e-5 and `front` of ref64's hit record at the kernel's own t; and on quads (u, v) = (a, b) within 1e-5"""
    sc = Q.boxes_on_a_floor(rtmi)
    S = R.RefScene(sc)
    rng = np.random.default_rng(11)
    n = 6000
    o = rng.uniform(-4, 4, (n, 3)).astype(np.float32)
    o[:, 1] = np.abs(o[:, 1]) + 0.05
    target = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(0.0, 1.5, n), rng.uniform(-1.5, 2.0, n)], axis=1)
    d = ((target - o) * rng.uniform(0.2, 3.0, (n, 1))).astype(np.float32)
    h = sc.trace(o, d)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    t64, p64 = R.closest_hit(S, o64, d64, np.inf, np.float64)
    same = h["prim"] == p64
    both = same & (p64 >= 0)
    rel = np.abs(h["t"][both] - t64[both]) / np.maximum(1.0, np.abs(t64[both]))
    isq = both & (S.prims["type"][np.clip(p64, 0, None)] == Q.QUAD)
    print("same primitive", same.mean(), "hits", int(both.sum()), "on quads", int(isq.sum()), "max rel t", rel.max())
    assert same.mean() >= 0.99 and rel.max() <= 2e-5 and isq.sum() > 500
    hit = h["prim"] >= 0
    p, nn, front = R.hit_record(S, o64[hit], d64[hit], h["t"][hit].astype(np.float64), h["prim"][hit].astype(np.int64), np.float64)
    dp = np.sqrt(((h["point"][hit] - p) ** 2).sum(axis=1)) / np.maximum(1.0, np.sqrt((p * p).sum(axis=1)))
    dn = np.abs(h["normal"][hit] - nn).max(axis=1)
    assert dp.max() <= 1e-5 and dn.max() <= 2e-5, (dp.max(), dn.max())
    clear = np.abs((d64[hit] * nn).sum(axis=1)) / np.sqrt((d64[hit] * d64[hit]).sum(axis=1)) > 1e-4
    assert clear.mean() > 0.99 and np.array_equal(h["front"][hit][clear] != 0, front[clear])
    fq = h["front"][isq] != 0
    assert 0.05 < fq.mean() < 1.0  # (rays that start inside a box meet its faces from behind)
    u, v = R.hit_uv(S, o64[isq], d64[isq], h["t"][isq].astype(np.float64), p64[isq], np.float64)
    assert np.abs(h["u"][isq] - u).max() <= 1e-5 and np.abs(h["v"][isq] - v).max() <= 1e-5
    assert sc.trace(o, d, occluded=True).tolist() == (h["prim"] >= 0).tolist()


def test_light_sampling_is_unbiased_against_the_plain_estimator(rtmi):
    """the Cornell case at 64 x 36 x 256 with and without light sampling: equal block and frame means by
    test_gpu_light_sampling.compare (8 seeds each; c_max: the brightest emission over the roulette's survival probability)"""
    from test_gpu_light_sampling import compare, seeds_of
    sc = Q.cornell(rtmi, w=64, h=36, spp=256)
    assert len(sc.lights()) == 2 and sorted(sc.lights()["shape"].tolist()) == [2, 6]
    compare(seeds_of(rtmi, sc), seeds_of(rtmi, sc, nee=True), "quad_cornell", c_max=9.0 / 0.85)


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_the_cli_renders_the_shipped_scene(rtmi, tmp_path, nee):
    out = str(tmp_path / "cornell.ppm")
    scene = os.path.join(PKG, "scenes", "cornell_box.json")
    p = subprocess.run([os.path.join(PKG, "rtmi"), "-f", scene, "-w", "64", "-h", "64", "-spp", "4", "-o", out, "--no-png"] + (["--nee"] if nee else []),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    sc = rtmi.Scene.load(scene)
    sc.override(64, 64, 4)
    sc.set_light_sampling(nee)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(), st)
    assert bool(st.kernel_variant & Q.NEE) == nee and np.isfinite(img).all() and img.mean() > 0
    tokens = open(out).read().split()
    assert tokens[:4] == ["P3", "64", "64", "255"] and len(tokens) == 4 + 64 * 64 * 3
    values = np.array(tokens[4:], np.int64)
    assert values.min() >= 0 and values.max() <= 255 and values.max() > 0
