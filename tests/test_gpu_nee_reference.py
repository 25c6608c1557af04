"""render_nee_kernel and render_env_kernel (7e) against the fp64 statement of their estimators (ref64.py),
sample by sample on the same draws.  A one-sample frame is that sample's radiance in 2^-24 fixed point (each contribution
rounded separately: at most (max_depth + 1) 2^-25, negligible against the tolerance).  Per scene:

  (a) at least 97 % of the samples lie within 1e-4 max(1, |ref|) in every channel (gate G2's number);
  (b) among the samples whose branches do not depend on the precision (fp32 and fp64 reference signatures agree), the share
      within tolerance is at least that of the plain, bit-exactly pinned kernel on the same geometry, minus 0.5 points;
  (c) kernel and reference consume the same draws, so mean(kernel - reference) has expectation 0 and only the few
      branch-flipped samples give it a variance: |mean| < 5 std / sqrt(N) + 1e-6 per channel over ALL samples;
  (d) the reference never reads past the draws it requested, and a reference that skips one draw position at the light
      sample fails (a) -- the comparison is sensitive to the order of the draws.

A case named for a special vertex (inside the sphere light, a dielectric, an absorbed metal vertex, alias picks) asserts from
the reference's signatures that such vertices occurred (nee_scenes.SPECIAL_VERTICES).

Every scene prints one row of figures (pytest -s); DESIGN 2 holds the rows measured on the MI355X."""
import pytest

import ref64 as R
import nee_scenes as NS
import per_sample as PS

pytestmark = pytest.mark.gpu
NEE, ENV = 256, 1024


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def words(rtmi):
    return R.uniforms(rtmi, NS.REF_SEED, NS.REF_W, NS.REF_H, 0, NS.REF_K, NS.REF_DRAWS)


def kernel_samples(rtmi, sc, family):
    return PS.kernel_samples(rtmi, sc, NS.REF_SEED, NS.REF_K, NEE | ENV, family)


def check(rtmi, words, name, sc, plain, family):
    assert len(words) >= 16000
    ref, stable, draws, tally = R.reference(R.RefScene(sc), words)
    assert draws.max() <= NS.REF_DRAWS, draws.max()                                        # (d)
    NS.check_special_vertices(name, tally)
    j = R.judge(kernel_samples(rtmi, sc, family), ref, stable)
    plain.set_light_sampling(False)
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    b = R.judge(kernel_samples(rtmi, plain, 0), bref, bstable)
    PS.assert_agreement(name, j, b)                                                        # (a), (b), (c)
    if name in NS.SPECIAL_VERTICES:
        print("    " + ", ".join(f"{k} {tally[k]}" for k in NS.SPECIAL_VERTICES[name]))


@pytest.mark.parametrize("name", list(NS.nee_cases()))
def test_light_sampling_kernel(rtmi, words, name):
    build = NS.nee_cases()[name]
    sc, plain = build(rtmi), build(rtmi)
    sc.set_light_sampling(True)
    assert len(sc.lights()) >= 1
    check(rtmi, words, name, sc, plain, NEE)


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "light sampling"])
@pytest.mark.parametrize("name", list(NS.env_cases()))
def test_environment_kernel(rtmi, words, name, nee):
    case = NS.env_cases()[name]
    sc, plain = NS.env_scene_of(rtmi, case), NS.env_scene_of(rtmi, case, with_env=False)
    sc.set_light_sampling(nee)
    if nee:
        assert sc.lights()[-1]["shape"] == R.ENVIRONMENT and len(sc.lights()) == (2 if case[3] else 1)
    check(rtmi, words, f"{name}, {'light sampling' if nee else 'plain'}", sc, plain, ENV | (NEE if nee else 0))


def test_a_skipped_draw_fails_the_agreement(rtmi, words):
    """(d): against the kernel, a reference that leaves out one draw position before the light sample's three is far from 97 %"""
    sc = NS.nee_cases()["lambert x xz"](rtmi)
    sc.set_light_sampling(True)
    S = R.RefScene(sc)
    got = kernel_samples(rtmi, sc, NEE)
    ref, stable, _, _ = R.reference(S, words)
    wrong, _, _ = R.trace(S, words, perturb=("skip_draw",))
    good, bad = R.judge(got, ref, stable), R.judge(got, wrong, stable)
    print(f"\nskipped draw: within tolerance {100 * good['share']:.2f} % -> {100 * bad['share']:.2f} %")
    PS.assert_perturbation_noticed(good, bad)
