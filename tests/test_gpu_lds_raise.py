"""Launches with more than 64 KB of dynamic LDS per workgroup: the host raises the limit on the ONE kernel instance it
resolved (csrc/kernels.h: set_max_dynamic_lds on the row), for a kernel of render_kernel.hip and for one of a side
translation unit (render_motion.hip).

The scene is a lattice of 3000 small spheres (radius 0.08 to 0.13) seen from 2.2 above.  Variant 16, the linear scan, stages
every scan table in LDS: (ns + 4) sphere slots + 6 camera records + 2 boxes per cluster (+ the ablation searches' windows and
groups), 16 bytes each (device_scene.h, pack.hip lay_out_image), + the 6144-byte tile accumulators -- with ns = 3404 and 375
clusters between 72 768 and 100 800 bytes, inside (64 KB, 160 KB); the default build's 200 window and group records make it 75 968.  The tests read the figure the host prints under
RTMI_DEBUG_LAYOUT and assert the range on it.

Why the camera is close: a sphere test's discriminant half_b^2 - a c cancels by (distance / radius)^2, so at fp32 the normal of
a sphere of radius 0.1 seen from 13 away (ratio 130) is off by ~5e-4 and a per-sample tolerance of 1e-4 measures the scene, not
the kernel: ref64's own float32 statement then agrees with its float64 one on 96.7 % of the samples.  From 2.2 away
(ratio ~20) the two statements agree on all 512 samples, with no branch flips, so the 97 % of test_gpu_motion.py's test 4 is a
bound the kernel can be held to here.  All 3000 spheres are in the scanned tables either way.
the range on it."""
import math
import re

import numpy as np
import pytest

import media_scenes as MS
import motion_scenes as MO
import ref64 as R
import per_sample as PS

pytestmark = pytest.mark.gpu
W, H, SEED, SPHERES = 32, 16, 31, 3000


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


def field(rtmi, mover=False):
    sc = rtmi.Scene.new(W, H, 1, 2)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((0.0, 2.2, 0.0), (0.0, 0.0, 0.0), (0, 0, -1), 40.0)
    mats = [sc.lambertian((0.7, 0.3, 0.3)), sc.metal((0.8, 0.8, 0.7), 0.2), sc.dielectric(1.5), sc.lambertian((0.2, 0.6, 0.3))]
    side = math.isqrt(SPHERES - 1) + 1
    rng = np.random.default_rng(5)
    for i in range(SPHERES):
        r = float(rng.uniform(0.08, 0.13))
        sc.sphere(((i % side - side / 2) * 0.3, r, (i // side - side / 2) * 0.3), r, mats[i % 4])
    if mover:
        sc.add_moving_sphere((-0.7, 0.9, 0.1), (0.7, 1.0, -0.1), 0.3, mats[0])
    return sc


def render_in_raised_lds(rtmi, sc, monkeypatch, capfd, **opts):
    """renders with variant 16 and returns the image, the stats and the LDS bytes per workgroup the host reports"""
    monkeypatch.setenv("RTMI_DEBUG_LAYOUT", "1")
    capfd.readouterr()
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED, variant=16, **opts), st)
    monkeypatch.delenv("RTMI_DEBUG_LAYOUT")
    lds = int(re.search(r"variant 16: LDS (\d+) bytes per workgroup", capfd.readouterr().err).group(1))
    print(f"\nvariant 16: {lds} bytes of LDS per workgroup")
    assert 64 * 1024 < lds < 160 * 1024, lds
    return img, st, lds


def test_linear_scan_above_64_kb_of_lds_gives_the_bytes_of_variant_0(rtmi, monkeypatch, capfd):
    sc = field(rtmi)
    st0 = rtmi.Stats()
    ref = sc.render(rtmi.Opts(seed=SEED), st0)
    assert st0.kernel_variant == 44  # (the grid walk over global memory: no LDS beyond the accumulators)
    img, st, _ = render_in_raised_lds(rtmi, sc, monkeypatch, capfd)
    assert st.kernel_variant == 16
    assert np.isfinite(ref).all() and ref.sum() > 0 and np.array_equal(img, ref)


def test_motion_kernel_above_64_kb_of_lds_against_fp64(rtmi, monkeypatch, capfd):
    """the motion kernel of layout 16 against ref64.py, criteria (a)-(d) of test_gpu_motion.py's test 4 on the frame's 512
    samples, and against the bytes of the scene's own layout"""
    sc = field(rtmi, mover=True)
    words = R.uniforms(rtmi, SEED, W, H, 0, 1, MS.REF_DRAWS)
    shutter = MO.shutter_times(rtmi, SEED, W, H, 0, 1)
    ref, stable, draws, tally = R.reference(R.RefScene(sc), words, shutter)
    assert draws.max() <= MS.REF_DRAWS, draws.max()                                         # (d)
    assert tally["movers_hit"] == [0] and tally["mover_then_static"] >= 1 and tally["static_then_mover"] >= 1, tally
    img, st, _ = render_in_raised_lds(rtmi, sc, monkeypatch, capfd)
    assert st.kernel_variant == 16 | MO.MOTION
    j = R.judge(img.reshape(-1, 3).astype(np.float64), ref, stable)
    plain = field(rtmi)
    bref, bstable, _, _ = R.reference(R.RefScene(plain), words)
    got_plain, pst, _ = render_in_raised_lds(rtmi, plain, monkeypatch, capfd)
    b = R.judge(got_plain.reshape(-1, 3).astype(np.float64), bref, bstable)
    PS.assert_agreement("3000 spheres and a mover, layout 16", j, b)                        # (a), (b), (c)
    st0 = rtmi.Stats()
    assert np.array_equal(sc.render(rtmi.Opts(seed=SEED), st0), img) and st0.kernel_variant == 44 | MO.MOTION
