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
import numpy as np
import pytest

import nee_scenes as NS
import per_sample as PS
import quad_scenes as Q
import ref64 as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    return PS.input_cache(rtmi, Q)


@pytest.fixture(scope="module")
def cases(rtmi, inputs):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)): rendered and traced once, shared by the tests"""
    return PS.case_cache(rtmi, Q, inputs)


@pytest.mark.parametrize("name", list(Q.CASES))
def test_kernel_against_fp64(rtmi, inputs, cases, name):
    assert not (Q.plain_twin(rtmi, name).prims()["type"] == Q.QUAD).any()
    print("\n    " + ", ".join(f"{k} {cases(name)[3][3][k]}" for k in Q.CASES[name][3]))
    PS.check_kernel_against_fp64(rtmi, Q, inputs, cases, name)


@pytest.mark.parametrize("name,mistake", Q.MISTAKES)
def test_a_wrong_reference_is_noticed(inputs, cases, name, mistake):
    PS.check_a_mistake_fails_the_agreement(inputs, cases, name, mistake)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    PS.check_same_bytes(rtmi, Q, ("quad_sky", Q.CORNELL), tmp_path)
    # the nested clump of boxes: its own layout against the flat wide-table walk and the linear scan of the same scene
    sc, st = Q.nested(rtmi), rtmi.Stats()
    nested = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant == Q.NESTED_LAYOUT and nested.mean() > 0
    scan = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K, variant=16), st)
    assert st.kernel_variant == 16 and np.array_equal(nested, scan)
    sc.set_nested_grid(False)
    flat = sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_count=NS.REF_K), st)
    assert st.kernel_variant in PS.GENERAL_LAYOUTS and np.array_equal(nested, flat)
    PS.check_compact_layouts_refuse(rtmi, lambda: Q.scene(rtmi, "quad_sky"))


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
    PS.check_cli(rtmi, tmp_path, "cornell_box.json", nee, Q.NEE, height=64)