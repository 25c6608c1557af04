"""-m gpu: the headline kernel's square roots.  rt_sqrtf (csrc/render_device.h) must return sqrtf's bits for every fp32 bit
pattern: its fast path is v_rsq_f32 and seven plain instructions, its guard a vote of the wave, and no CPU stands in for
v_rsq_f32 -- so the default library carries a sweep over all 2^32 patterns (csrc/sqrt_sweep.hip, not part of include/rtmi.h
nor of the product library).  Then three small frames through the kernels that take those roots, each equal to the
reference's linear scan (variant 16) byte for byte and two of its rows equal to the CPU checker."""
import ctypes

import numpy as np
import pytest

from test_tables import Tables

pytestmark = pytest.mark.gpu
SEED = 2023


# ---- every bit pattern

@pytest.mark.parametrize("layout", [0, 1], ids=["consecutive_lanes", "one_odd_lane_per_wave"])
def test_rt_sqrtf_equals_sqrtf_on_every_bit_pattern(rtmi, layout):
    """Layout 0: consecutive patterns in consecutive lanes, a wave starting at 64 w + 32, so that waves straddle 2^-96, 0, inf
    and the sign (the guard's whole-wave fallback runs for part of a wave's range).  Layout 1: 0, a denormal, inf, NaN or -1 in
    one of lanes 0 .. 4 of a wave whose other 63 lanes hold consecutive patterns: the fallback runs with ordinary lanes in it.
    Equal means the same bits, or both NaN; the required number of mismatches is 0."""
    lib = ctypes.CDLL(rtmi.LIB_PATH)
    fn = lib.rtmi_test_sqrt_sweep
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_uint32)]
    bad, first = ctypes.c_ulonglong(1 << 40), ctypes.c_uint32(0)
    assert fn(layout, ctypes.byref(bad), ctypes.byref(first)) == 0
    print(f"layout {layout}: {bad.value} mismatches" + (f", the first at bit pattern {first.value:#010x}" if bad.value else ""))
    assert bad.value == 0, f"{bad.value} of 2^32 patterns differ from sqrtf, the first at {first.value:#010x}"


# ---- frames

def _held(rtmi, rtcheck, sc, variants=(0,)):
    """The variants equal the linear scan byte for byte; the frame's last two rows equal the CPU checker.  Returns the
    kernel that variant 0 resolved to."""
    scan = sc.render(rtmi.Opts(seed=SEED, variant=16))
    assert scan.any()
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED), st)
    assert np.array_equal(img, scan), f"variant 0 (kernel {st.kernel_variant}): {(img != scan).any(axis=2).sum()} pixels differ from the linear scan"
    for v in variants:
        if v:
            other = sc.render(rtmi.Opts(seed=SEED, variant=v))
            assert np.array_equal(other, scan), f"variant {v}: {(other != scan).any(axis=2).sum()} pixels differ from the linear scan"
    y0, y1 = sc.height - 2, sc.height
    ref, _ = rtcheck.oracle_render(sc, seed=SEED, rows=(y0, y1))
    assert ref[y0:y1].any()
    assert np.array_equal(img[y0:y1], ref[y0:y1]), f"rows {y0} and {y1 - 1} differ from the CPU checker"
    return st.kernel_variant


def test_rtiow_through_the_sheet_walk(rtmi, rtcheck):
    """Scene.rtiow(7) at 96 x 54, 8 spp, depth 50: the headline instance (the x-z walk, kernel 2)."""
    assert _held(rtmi, rtcheck, rtmi.Scene.rtiow(7, 96, 54, 8, 50)) == 2


def test_rtiow_and_a_volume_through_the_3d_walk(rtmi, rtcheck):
    """The same scene at 64 x 32, 4 spp through the 3-D walk (variant 6 reads the sheet's tables), and a scene more than one
    cell high -- 200 spheres in a volume -- on which variant 0 is the 3-D walk."""
    _held(rtmi, rtcheck, rtmi.Scene.rtiow(7, 64, 32, 4, 50), variants=(6,))
    sc = rtmi.Scene.new(64, 32, 4, 12)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((0.0, 2.0, 14.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0)
    rng = np.random.default_rng(23)
    mats = [sc.lambertian(rng.uniform(0.2, 0.9, 3)) for _ in range(4)] + [sc.metal((0.8, 0.8, 0.8), 0.1), sc.dielectric(1.5)]
    for i in range(200):
        sc.sphere(rng.uniform(-3.0, 3.0, 3), float(rng.uniform(0.05, 0.25)), mats[i % len(mats)])
    assert sc.table_info().grid_n[1] > 1
    assert _held(rtmi, rtcheck, sc) == 6


def glass_and_metal_in_short_lists(rtmi, w=96, h=54, spp=4, depth=16):
    """A ground sphere and, on it, spheres of glass, fuzzy metal and matte paint: singles a few cells apart and triples that
    touch one another, so that cells list one sphere and cells list three -- lists of odd length, whose second half of the
    last pair pass reads past the list's end."""
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((0.0, 2.5, 9.0), (0.0, 0.3, 0.0), (0, 1, 0), 40.0)
    mats = [sc.dielectric(1.5), sc.metal((0.8, 0.7, 0.6), 0.1), sc.lambertian((0.6, 0.3, 0.2))]
    sc.sphere((0.0, -1000.0, 0.0), 1000.0, sc.lambertian((0.5, 0.5, 0.5)))
    r = 0.2
    n = 0
    for i in range(-3, 4):
        for j in range(-3, 4):
            x, z = 1.3 * i, 1.3 * j
            if (i + j) % 2 == 0:
                sc.sphere((x, r, z), r, mats[n % 3])
                n += 1
            else:  # three in a tight triangle: every cell one of them reaches, the others reach too
                for a in range(3):
                    sc.sphere((x + 0.05 * np.cos(2.1 * a), r, z + 0.05 * np.sin(2.1 * a)), r, mats[(n + a) % 3])
                n += 1
    return sc


def test_lists_of_one_and_three_with_glass_and_metal(rtmi, rtcheck):
    """Both roots of a sphere (glass: the ray leaves through the far one) and the dielectric's two square roots, in cells whose
    lists have length 1 and 3."""
    sc = glass_and_metal_in_short_lists(rtmi)
    t = Tables(sc)
    assert not t.t.grid_wide and t.t.grid_cells > 0
    # a sphere slot's material: the cold record's list index (.z) -> the primitive -> its material's type
    cold = t.img.view(np.int32)[t.t.off_sph_cold: t.t.off_sph_cold + t.t.ns]
    mat_type = sc.materials()["type"]
    kind = lambda slot: int(mat_type[t.prims["material"][cold[slot, 2]]])
    for length in (1, 3):
        kinds = set()
        for c in np.flatnonzero(t.n_near == length):
            kinds |= {kind(s) for s in t.near(c)}
        assert {1, 2} <= kinds, f"no cell's list of length {length} holds a metal and a glass sphere: {kinds}"
    assert _held(rtmi, rtcheck, sc, variants=(6,)) == 2
