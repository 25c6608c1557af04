"""The four render families that exist only in the build with triangles and image textures -- light sampling,
environment (7e), media (7f), motion (7g) -- on scenes WITH triangles and image textures (ext_scenes.py), against the fp64
statement (ref64.py), sample by sample on the same draws: criteria (a) - (d) of test_gpu_nee_reference.py with per_sample's
thresholds.  The (b) baseline is the plain kernel on the case's plain twin (light sampling off, environment, media and movers
cleared) against the twin's reference.  Each case asserts from the reference's signatures that it contains the vertices it is
there for: a light sample at a vertex whose albedo is an image texel or that lies on a triangle, a shadow ray stopped by a
triangle or by an image-textured primitive, an emitter that is no listed light hit after a light sample, a medium event before
an image-textured surface, an image-textured mover.

(d) here: a reference whose image lookup is transposed is far from 97 % against the kernel.

The light-sampling cases are also rendered whole through every layout and through sample splits, byte for byte: a texel is
held in the lane's state while the lane walks the shadow ray, across the points where an item is put down and resumed.

Every scene prints one row of figures (pytest -s); DESIGN 2 holds the rows measured on the MI355X."""
import numpy as np
import pytest

import ext_scenes as XS
import nee_scenes as NS
import per_sample as PS
import ref64 as R

pytestmark = pytest.mark.gpu
FAMILIES = XS.NEE | XS.ENV | XS.MEDIA | XS.MOTION


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    """name -> (uniforms, shutter times or None), computed once per seed"""
    made = {}

    def of(name):
        key = (XS.seed_of(name), XS.family(name) == XS.MOTION)
        if key not in made:
            made[key] = XS.inputs(rtmi, name)
        return made[key]
    return of


@pytest.fixture(scope="module")
def baselines(rtmi, inputs):
    """name -> judge() of the plain kernel on the case's plain twin against the twin's reference; twins that are the same scene
    under the same seed (the two environment cases) are rendered and traced once"""
    made = {}

    def of(name):
        plain = XS.plain_twin(rtmi, name)
        key = (XS.seed_of(name), plain.prims().tobytes(), plain.materials().tobytes(), plain.info.max_depth, plain.info.russian_roulette)
        if key not in made:
            bref, bstable, _, _ = R.reference(R.RefScene(plain), inputs(name)[0])
            made[key] = R.judge(PS.kernel_samples(rtmi, plain, XS.seed_of(name), NS.REF_K, FAMILIES, 0), bref, bstable)
        return made[key]
    return of


def check(rtmi, inputs, baselines, name):
    words, shutter = inputs(name)
    assert len(words) >= 16000
    sc = XS.scene(rtmi, name)
    ref, stable, draws, tally = R.reference(R.RefScene(sc), words, shutter)
    assert draws.max() <= NS.REF_DRAWS, draws.max()                                        # (d)
    XS.check_contents(name, tally, len(words))
    j = R.judge(PS.kernel_samples(rtmi, sc, XS.seed_of(name), NS.REF_K, FAMILIES, XS.family(name)), ref, stable)
    PS.assert_agreement(name, j, baselines(name))                                          # (a), (b), (c)
    print("    " + ", ".join(f"{k} {tally[k]}" for k in R.EXT_KEYS + R.MEDIA_KEYS[:2] + R.MOTION_KEYS[2:] if tally[k]))


@pytest.mark.parametrize("name", XS.LIGHT_SAMPLING_CASES)
def test_light_sampling_kernel(rtmi, inputs, baselines, name):
    check(rtmi, inputs, baselines, name)


@pytest.mark.parametrize("name", [n for n in XS.CASES if XS.family(n) & XS.ENV])
def test_environment_kernel(rtmi, inputs, baselines, name):
    check(rtmi, inputs, baselines, name)


@pytest.mark.parametrize("name", [n for n in XS.CASES if XS.family(n) == XS.MEDIA])
def test_media_kernel(rtmi, inputs, baselines, name):
    check(rtmi, inputs, baselines, name)


@pytest.mark.parametrize("name", [n for n in XS.CASES if XS.family(n) == XS.MOTION])
def test_motion_kernel(rtmi, inputs, baselines, name):
    check(rtmi, inputs, baselines, name)


def test_a_transposed_lookup_fails_the_agreement(rtmi, inputs):
    """(d): against the kernel, a reference whose image lookup takes u for the column is far from 97 %"""
    sc = XS.scene(rtmi, XS.RECEIVERS)
    words, _ = inputs(XS.RECEIVERS)
    S = R.RefScene(sc)
    got = PS.kernel_samples(rtmi, sc, XS.seed_of(XS.RECEIVERS), NS.REF_K, FAMILIES, XS.NEE)
    ref, stable, _, _ = R.reference(S, words)
    wrong, _, _ = R.trace(S, words, perturb=("uv_transposed",))
    good, bad = R.judge(got, ref, stable), R.judge(got, wrong, stable)
    print(f"\ntransposed image lookup: within tolerance {100 * good['share']:.2f} % -> {100 * bad['share']:.2f} %")
    PS.assert_perturbation_noticed(good, bad)


@pytest.mark.parametrize("name", XS.LIGHT_SAMPLING_CASES)
def test_layouts_and_sample_splits_give_the_same_bytes(rtmi, name):
    """the whole frame at spp = REF_K through layouts 16, 36, 44 and through a sample split; and, since a 20 + rest split needs
    more than REF_K = 13 samples, the frame at 2 REF_K samples through 20 + 6"""
    sc = XS.scene(rtmi, name)
    seed, st = XS.seed_of(name), rtmi.Stats()
    ref = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K), st)
    assert st.kernel_variant & FAMILIES == XS.NEE
    for variant in (16, 36, 44):
        got = sc.render(rtmi.Opts(seed=seed, sample_count=NS.REF_K, variant=variant), st)
        assert st.kernel_variant == variant | XS.NEE, (variant, st.kernel_variant)
        assert np.array_equal(got, ref), (name, variant, float(np.abs(got - ref).max()))
    for total, cut in ((NS.REF_K, 5), (2 * NS.REF_K, 20)):
        whole = ref if total == NS.REF_K else sc.render(rtmi.Opts(seed=seed, sample_count=total))
        acc, _ = sc.accumulate(None, rtmi.Opts(seed=seed, sample_first=0, sample_count=cut), st)
        assert st.kernel_variant & FAMILIES == XS.NEE
        acc, img = sc.accumulate(acc, rtmi.Opts(seed=seed, sample_first=cut, sample_count=total - cut), st)
        assert np.array_equal(img, whole), (name, total, cut, float(np.abs(img - whole).max()))
