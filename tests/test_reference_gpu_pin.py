"""Pins the fp32 CPU restatement (oracle/rt_oracle.c) to the COMPILED gpu-version of the reference on what exists only there:
xy_rect / xz_rect / yz_rect, cylinder with its transforms, diffuse_light, the constant background, checker_texture, the hit
record's (u, v), front and normal, and the list's tie rule.  The fixtures (tests/golden/refgpu_*.npz, written by
tests/golden/make_ref_gpu_pin.py from oracle/_ref/libref_gpu.so: the reference's own object.cuh, material.cuh, texture.cuh,
camera.cuh and ray_color behind oracle/shim/) are checked everywhere; the live library where it has been built.

Records: the restatement's probe (rto_hit_record) against the reference's records on the decided rays -- refgpu_pin.py states the
rule, a rule on the inputs alone -- hit or miss, winner and front equal, t, p, normal and (u, v) within the bound the project holds
against fp64 plus the reference's own stored distance from fp64.  Paths (dielectric and diffuse_light only: gpu-version's
random_in_unit_sphere is not this project's): rto_sample against the reference's per-sample radiance with
test_oracle_pin.py's gates.  The same comparisons must FAIL on five doctored copies of the fixtures."""
import os

import numpy as np
import pytest

import ref64 as R
import refgpu_pin as P


@pytest.fixture(scope="module")
def records(rtmi, rtcheck, golden_dir):
    """name -> everything about a record scene, made once: the scene, its rays, the reference's records out of the fixture, the
    rule's verdicts, the restatement's records"""
    made = {}

    def of(name):
        if name not in made:
            made[name] = P.load_record_case(rtmi, golden_dir, name)
            made[name]["got"] = rtcheck.oracle_hit_records(made[name]["sc"], made[name]["o"], made[name]["d"])
        return made[name]
    return of


@pytest.fixture(scope="module")
def paths(rtmi, rtcheck, golden_dir):
    """name -> the scene of a path fixture, the reference's per-sample radiance and draws, and the restatement's"""
    z = np.load(os.path.join(golden_dir, "refgpu_paths.npz"))
    assert (int(z["seed"]), int(z["width"]), int(z["height"]), int(z["spp"])) == (P.SEED, P.W, P.H, P.SPP)
    ids = P.sample_ids()
    made = {}

    def of(name):
        if name not in made:
            k = P.key(name)
            sc = rtmi.Scene.parse(str(z[f"{k}/scene"]))
            assert (sc.width, sc.height, sc.spp) == (P.W, P.H, P.SPP)
            osc = rtcheck.OracleScene(sc)
            got = [rtcheck.oracle_sample_draws(osc, P.SEED, int(x), int(y), int(s)) for x, y, s in ids]
            made[name] = dict(z=z, k=k, sc=sc, ref=z[f"{k}/rgb"], ref_draws=z[f"{k}/draws"].astype(np.int64),
                              cut=np.unpackbits(z[f"{k}/cut"])[:len(ids)].astype(bool), ref_median=float(z[f"{k}/ref_fp64_median"]),
                              got=np.array([g[0] for g in got]), got_draws=np.array([g[1] for g in got], np.int64))
        return made[name]
    return of


# ------------------------------------------------------------------------------------------------------------------ records
@pytest.mark.parametrize("name", P.RECORD_SCENES)
def test_the_rule_and_the_reference_against_fp64(records, name):
    """what the builder chose and stored, checked again here without any code under test: the rule sets aside at most 5 % of the
    scene's rays (and exactly the stored ones); among the rest the reference and ref64 in fp64 agree on hit / miss, winner and
    front on every ray, and their distances are the stored ones"""
    c = records(name)
    z = c["z"]
    assert np.array_equal(c["judged"], np.unpackbits(z["decided"])[:len(c["o"])].astype(bool))
    assert 1 - c["judged"].mean() <= P.CAP and int(z["ref_fp64_disagreements"]) == 0
    f64 = P.fp64_records(R.RefScene(c["sc"]), c["o"], c["d"])
    fig, wrong = P.measure(c["prims"], c["ref"], f64, c["judged"])
    assert wrong == 0 and np.array_equal(c["ref"]["front"][c["judged"]], f64["front"][c["judged"]])
    for q, stored in c["dev"].items():
        assert abs(fig[q][0] - stored) <= 1e-9, (q, fig[q][0], stored)
        assert stored <= 5e-5, (q, stored)  # fp32 noise, not a second opinion
    print(f"\n{name}: set aside {100 * (1 - c['judged'].mean()):.2f} %, reference vs fp64 " + ", ".join(f"{q} {v[0]:.2e}" for q, v in fig.items()))


@pytest.mark.parametrize("name", P.RECORD_SCENES)
def test_restatement_records_against_the_reference(records, name):
    c = records(name)
    fig = P.compare_records(name, c["prims"], c["got"], c["ref"], c["judged"], c["dev"])
    print(f"\n{name}: restatement vs reference " + ", ".join(f"{q} max {v[0]:.2e} median {v[1]:.2e}" for q, v in fig.items()))


def test_every_kind_of_hit_is_among_the_decided_rays(records):
    """the scenes contain what they are there for, counted on the fixture's decided rays"""
    c = records("zoo")
    ty = c["prims"]["type"][np.maximum(c["ref"]["index"], 0)]
    hit = c["judged"] & (c["ref"]["index"] >= 0)
    for kind in (R.XY_RECT, R.XZ_RECT, R.YZ_RECT):  # each rect from both sides
        k = hit & (ty == kind)
        assert (c["ref"]["front"][k] == 1).sum() >= 20 and (c["ref"]["front"][k] == 0).sum() >= 20, kind
    for i in np.flatnonzero(c["prims"]["type"] == R.CYLINDER):  # every tube, its wall from outside and from inside
        k = hit & (c["ref"]["index"] == i)
        assert (c["ref"]["front"][k] == 1).sum() >= 20 and (c["ref"]["front"][k] == 0).sum() >= 10, i
    c = records("inside")
    hit = c["judged"] & (c["ref"]["index"] >= 0)
    assert (hit & (c["ref"]["front"] == 0)).sum() >= 800
    shell = hit & (c["prims"]["f"][np.maximum(c["ref"]["index"], 0), 3] < 0) & (c["prims"]["type"][np.maximum(c["ref"]["index"], 0)] == R.SPHERE)
    assert shell.sum() >= 100 and 0 < c["ref"]["front"][shell].mean() < 1  # the negative radius, from either side
    c = records("ties")
    k = c["judged"] & (c["tie"] >= 0)
    assert k.sum() >= 300 and (c["ref"]["index"][k] > c["tie"][k]).all()  # the later entry wins, on every one of them
    assert len(set(c["ref"]["index"][k].tolist())) >= 3                   # (rect pair, overlapping rects, sphere pair)
    # a point exactly on an edge (the ray runs along the rect's normal): inside, by the inclusive bounds
    exact = c["judged"] & ((c["d"] != 0).sum(axis=1) == 1)
    on_edge = np.zeros(len(exact), bool)
    for i in np.flatnonzero(exact & (c["ref"]["index"] >= 0)):
        pr = c["prims"][c["ref"]["index"][i]]
        if int(pr["type"]) in (R.XY_RECT, R.XZ_RECT, R.YZ_RECT):
            _, aa, ba = P._rect_axes(pr["type"])
            on_edge[i] = c["o"][i, aa] in (pr["f"][0], pr["f"][1]) or c["o"][i, ba] in (pr["f"][2], pr["f"][3])
    assert on_edge.sum() >= 20, int(on_edge.sum())


@pytest.mark.parametrize("mistake", P.RECORD_MISTAKES)
def test_a_doctored_record_fixture_is_rejected(records, mistake):
    """the comparison that passes above fails when the reference's records carry one deliberate mistake"""
    name = "ties" if mistake == "earlier entry wins a tie" else "zoo"
    c = records(name)
    P.compare_records(name, c["prims"], c["got"], c["ref"], c["judged"], c["dev"])
    wrong, changed = P.doctored(mistake, c["prims"], c["ref"], c["tie"])
    assert changed >= 50, (mistake, changed)
    with pytest.raises(AssertionError):
        P.compare_records(name, c["prims"], c["got"], wrong, c["judged"], c["dev"])


# -------------------------------------------------------------------------------------------------------------------- paths
@pytest.mark.parametrize("name", P.PATH_SCENES)
def test_restatement_paths_against_the_reference(paths, name):
    c = paths(name)
    z, k = c["z"], c["k"]
    assert float(z[f"{k}/two_event_share"]) >= 0.30 and z[f"{k}/light_shares"][:, 1].min() >= 0.01  # the builder's conditions
    assert float(z[f"{k}/ref_fp64_share"]) >= 0.97
    share, median = P.compare_paths(name, c["got"], c["ref"], c["ref_median"], got_draws=c["got_draws"], ref_draws=c["ref_draws"])
    print(f"\n{name}: within 1e-4 {100 * share:.3f} %, median {median:.2e}; reference vs fp64 {100 * float(z[f'{k}/ref_fp64_share']):.3f} %, "
          f"median {c['ref_median']:.2e}")


def test_a_fixture_whose_cut_samples_went_on_is_rejected(paths):
    """"depth 3" with the radiance of the samples that were cut at depth replaced by what the full-depth scene returns"""
    c, full = paths("depth 3"), paths("glass and lights")
    assert float(c["z"]["depth_3/cut_lit_share"]) >= 0.01 and c["cut"].mean() >= 0.03
    P.compare_paths("depth 3", c["got"], c["ref"], c["ref_median"])
    wrong = c["ref"].copy()
    wrong[c["cut"]] = full["ref"][c["cut"]]
    assert (np.abs(wrong - c["ref"]).max(axis=1) > 1e-3).mean() >= 0.03
    with pytest.raises(AssertionError):
        P.compare_paths("depth 3", c["got"], wrong, c["ref_median"])


# ------------------------------------------------------------------------------------------------------------------ checker
def test_checker_parity_against_the_reference(rtcheck, golden_dir):
    """checker_texture::value's choice at 10 000 points of [-5, 5]^3, outside |sin 10x sin 10y sin 10z| <= 1e-4: the
    restatement's floor-parity form and ref64's take the colour the reference's sign of the product takes"""
    z = np.load(os.path.join(golden_dir, "refgpu_paths.npz"))
    pts = P.checker_points()
    assert P.digest(pts, pts[:0]) == str(z["checker/points_sha256"])
    ref = np.unpackbits(z["checker/odd"])[:len(pts)].astype(bool)
    clear = P.checker_clear(pts)
    assert clear.mean() >= 0.99 and 0.45 < ref.mean() < 0.55
    assert np.array_equal(rtcheck.oracle_checker_odd(pts)[clear], ref[clear])
    assert np.array_equal(R.checker_odd(pts.astype(np.float64), np.float64)[clear], ref[clear])


# --------------------------------------------------------------------------------------------------------------------- live
def _need_live(rtcheck):
    if not (rtcheck.have_ref() and rtcheck.have_ref_gpu()):
        pytest.skip("oracle/_ref not built here")


@pytest.mark.parametrize("name", P.RECORD_SCENES)
def test_live_reference_reproduces_the_record_fixture(rtcheck, records, name):
    _need_live(rtcheck)
    c = records(name)
    live = P.reference_records(rtcheck.RefGpuScene(c["sc"]), c["prims"], c["o"][:800], c["d"][:800])
    for q in rtcheck.RECORD_FIELDS:
        assert np.array_equal(live[q], c["ref"][q][:800]), (name, q)


@pytest.mark.parametrize("name", P.PATH_SCENES)
def test_live_reference_reproduces_the_path_fixture(rtcheck, paths, name):
    _need_live(rtcheck)
    c = paths(name)
    rs = rtcheck.RefGpuScene(c["sc"])
    ids = P.sample_ids()
    for i in range(0, len(ids), 37):
        rgb, draws, (events, ended_by, cut) = rs.sample(P.SEED, int(ids[i, 0]), int(ids[i, 1]), int(ids[i, 2]))
        assert np.array_equal(rgb, c["ref"][i]) and draws == c["ref_draws"][i] and bool(cut) == c["cut"][i], (name, i)
    # the hook is really keyed
    assert any(not np.array_equal(rs.sample(P.SEED + 1, int(x), int(y), int(s))[0], c["ref"][i]) for i, (x, y, s) in enumerate(ids[:200]))


def test_live_checker(rtcheck, golden_dir):
    _need_live(rtcheck)
    z = np.load(os.path.join(golden_dir, "refgpu_paths.npz"))
    pts = P.checker_points()
    assert np.array_equal(rtcheck.ref_gpu_checker(pts), np.unpackbits(z["checker/odd"])[:len(pts)].astype(bool))


def test_reference_gpu_refuses_what_it_cannot_express(rtmi, rtcheck, records, scenes_dir):
    _need_live(rtcheck)
    import ext_scenes as X

    def frame():
        sc = rtmi.Scene.new(16, 9, 1, 5)
        sc.set_background((0.1, 0.2, 0.3), sky_gradient=False, defocus_blur=False)
        sc.camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0)
        return sc
    ok = frame()
    ok.sphere((0, 0, 0), 1.0, ok.dielectric(1.5))
    assert rtcheck.RefGpuScene(ok).hit([(0, 0, 5)], [(0, 0, -1)])["index"][0] == 0
    tri = frame()
    tri.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), tri.lambertian((0.5, 0.5, 0.5)))
    quad = frame()
    quad.quad((0, 0, 0), (1, 0, 0), (0, 1, 0), quad.lambertian((0.5, 0.5, 0.5)))
    img = frame()
    img.sphere((0, 0, 0), 1.0, img.lambertian(img.image_texture(X.image(4, 4, 1))))
    sky = frame()
    sky.set_background((0.1, 0.2, 0.3), sky_gradient=True, defocus_blur=False)
    blur = frame()
    blur.set_background((0.1, 0.2, 0.3), sky_gradient=False, defocus_blur=True)
    for what, sc in (("triangle", tri), ("quad", quad), ("image texture", img), ("sky gradient", sky), ("blur", blur)):
        with pytest.raises(ValueError):
            rtcheck.RefGpuScene(sc)
        print(what, "refused")
    # records of any material, whole paths of dielectric and diffuse_light only
    rs = rtcheck.RefGpuScene(records("zoo")["sc"])
    with pytest.raises(ValueError):
        rs.sample(P.SEED, 3, 4, 0)
