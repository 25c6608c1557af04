"""render_nee_kernel and render_env_kernel (7e) against the fp64 statement of their estimators (nee_ref64.py),
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
import os
import sys

import numpy as np
import pytest

import nee_ref64 as R
import nee_scenes as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
NEE, ENV = 256, 1024


@pytest.fixture(scope="module")
def rtmi():
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    mod = load_package()
    if mod.device_count() < 1:
        pytest.skip("no HIP device")
    return mod


@pytest.fixture(scope="module")
def words(rtmi):
    return R.uniforms(rtmi, NS.REF_SEED, NS.REF_W, NS.REF_H, 0, NS.REF_K, NS.REF_DRAWS)


def kernel_samples(rtmi, sc, family):
    """[K x H x W][3]: the radiance of every sample, from one-sample frames; the kernel family is checked on each"""
    out = []
    for k in range(NS.REF_K):
        st = rtmi.Stats()
        out.append(sc.render(rtmi.Opts(seed=NS.REF_SEED, sample_first=k, sample_count=1), st))
        assert st.kernel_variant & (NEE | ENV) == family, (st.kernel_variant, family)
    return np.stack(out).reshape(-1, 3).astype(np.float64)


def check(rtmi, words, name, sc, plain, family):
    assert len(words) >= 16000
    ref, stable, draws, tally = R.reference(R.RefScene(sc), words)
    assert draws.max() <= NS.REF_DRAWS, draws.max()                                        # (d)
    NS.check_special_vertices(name, tally)
    j = R.judge(kernel_samples(rtmi, sc, family), ref, stable)
    plain.set_light_sampling(False)
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    b = R.judge(kernel_samples(rtmi, plain, 0), bref, bstable)
    print("\n" + R.row(name, j, b["share_stable"]))
    if name in NS.SPECIAL_VERTICES:
        print("    " + ", ".join(f"{k} {tally[k]}" for k in NS.SPECIAL_VERTICES[name]))
    assert j["flips"] <= 0.01, j["flips"]
    assert j["share"] >= 0.97, j                                                           # (a)
    assert j["share_stable"] >= b["share_stable"] - 0.005, (j["share_stable"], b["share_stable"])  # (b)
    assert j["bias_ok"], (j["mean_diff"], j["z"])                                          # (c)
    return j


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
    assert good["share"] >= 0.97 and bad["share"] < 0.97, (good["share"], bad["share"])
