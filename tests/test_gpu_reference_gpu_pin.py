"""-m gpu: the kernels against the COMPILED gpu-version of the reference, from the fixtures alone (tests/golden/refgpu_*.npz, which
tests/golden/make_ref_gpu_pin.py wrote from oracle/_ref/libref_gpu.so; neither the reference nor oracle/_ref is read here).

Records: Scene.trace on each record scene, in the scene's own layout and in layout 16, against the reference's hit records with
the comparison, bounds and cap of test_reference_gpu_pin.py (refgpu_pin.py).  The rays of the quirk classes -- parallel to a
tube's axis: the reference divides 0 by 0 there -- are never judged and are not traced.  Paths: one-sample frames of the three
path scenes against the reference's per-sample radiance and image with the same gates, and each whole frame bit-equal to the
restatement (rtcheck.oracle_render).  Frames are 48 x 27, about 3400 rays per scene."""
import os

import numpy as np
import pytest

import feature_scenes as FS
import per_sample as PS
import refgpu_pin as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def record_cases(rtmi, golden_dir):
    made = {}

    def of(name):
        if name not in made:
            made[name] = P.load_record_case(rtmi, golden_dir, name)
        return made[name]
    return of


@pytest.mark.parametrize("variant", [0, 16])
@pytest.mark.parametrize("name", P.RECORD_SCENES)
def test_trace_records_against_the_reference(rtmi, record_cases, name, variant):
    c = record_cases(name)
    assert 1 - c["judged"].mean() <= P.CAP
    keep = ~c["quirk"]
    st = rtmi.Stats()
    h = c["sc"].trace(c["o"][keep], c["d"][keep], opts=rtmi.Opts(variant=variant), stats=st)
    assert st.launches == 1 and st.kernel_variant & rtmi.TRACE_LAYOUT
    layout = st.kernel_variant & ~rtmi.TRACE_LAYOUT
    assert layout == 16 if variant else layout in (16, 24, 36, 44), st.kernel_variant
    got = P.records_of_hits(h)
    ref = {q: v[keep] for q, v in c["ref"].items()}
    fig = P.compare_records(name, c["prims"], got, ref, c["judged"][keep], c["dev"])
    assert np.array_equal(h["material"][h["prim"] >= 0], c["prims"]["material"][h["prim"][h["prim"] >= 0]])
    print(f"\n{name}, layout {layout}: kernel vs reference " + ", ".join(f"{q} max {v[0]:.2e} median {v[1]:.2e}" for q, v in fig.items())
          + f"; set aside {100 * (1 - c['judged'].mean()):.2f} %")


def test_a_doctored_record_fixture_is_rejected_on_the_device(rtmi, record_cases):
    """the kernel's records, too, fail the comparison with each doctored copy of the reference's"""
    for mistake in P.RECORD_MISTAKES:
        name = "ties" if mistake == "earlier entry wins a tie" else "zoo"
        c = record_cases(name)
        keep = ~c["quirk"]
        got = P.records_of_hits(c["sc"].trace(c["o"][keep], c["d"][keep]))
        wrong, changed = P.doctored(mistake, c["prims"], {q: v[keep] for q, v in c["ref"].items()}, c["tie"][keep])
        assert changed >= 50
        with pytest.raises(AssertionError):
            P.compare_records(name, c["prims"], got, wrong, c["judged"][keep], c["dev"])


@pytest.mark.parametrize("name", P.PATH_SCENES)
def test_path_scenes_against_the_reference(rtmi, rtcheck, golden_dir, name):
    z = np.load(os.path.join(golden_dir, "refgpu_paths.npz"))
    k = P.key(name)
    sc = rtmi.Scene.parse(str(z[f"{k}/scene"]))
    assert (sc.width, sc.height, sc.spp, int(z["seed"])) == (P.W, P.H, P.SPP, P.SEED)
    got = PS.kernel_samples(rtmi, sc, P.SEED, P.SPP, FS.FAMILIES, 0)  # ordered (s, y, x), as refgpu_pin.sample_ids
    st = rtmi.Stats()
    frame = sc.render(rtmi.Opts(seed=P.SEED), st)
    assert st.kernel_variant & FS.FAMILIES == 0 and st.kernel_variant & ~FS.FAMILIES in PS.GENERAL_LAYOUTS, st.kernel_variant
    share, median = P.compare_paths(name, got, z[f"{k}/rgb"], float(z[f"{k}/ref_fp64_median"]), got_image=frame)
    print(f"\n{name}: kernel vs reference within 1e-4 {100 * share:.3f} %, median {median:.2e}")
    assert np.array_equal(frame, rtcheck.oracle_render(sc, seed=P.SEED)[0])
