"""Interface of the feature passes and the denoiser, as far as it goes without a GPU: exported symbols, the ctypes mirror of
rt_denoise, and the argument checks, which must return RT_ERR_ARG before any device is touched (this file runs on machines
that have none).  Then the numpy restatement that the kernel is held to (tests/test_gpu_denoise.py) against its float64
twin and against what the filter's definition implies."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_denoise import (ALBEDO_EPS, DEFAULTS, F, FEATURE_SPP, PASSES, SIZES, SPP, frame, frame_spp_map, restate, restate64,
                              tap_grid)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
RT_ERR_ARG = 1
NEW = ["rt_render_hip_feature", "rt_render_hip_feature_device", "rt_denoise_hip", "rt_denoise_hip_device"]


@pytest.mark.parametrize("lib", ["librtmi.so", "librtmi_product.so"])
def test_symbols_are_exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, lib)], capture_output=True, text=True, check=True).stdout
    have = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW) <= have


def test_struct_mirror(rtmi):
    assert set(NEW) <= set(rtmi.C_SYMBOLS)
    assert C.sizeof(rtmi.Denoise) == rtmi.struct_size(16) == 16
    assert rtmi.struct_size(11) == 0  # (left to the scene / render structs)
    assert (rtmi.FEATURE_ALBEDO, rtmi.FEATURE_NORMAL, rtmi.FEATURE_DEPTH) == (0, 1, 2)


def _status(rtmi, fn):
    with pytest.raises(rtmi.RtmiError) as e:
        fn()
    return e.value.status


def test_feature_arguments(rtmi):
    sc = rtmi.Scene.rtiow(7, 16, 9, 2, 4)
    for feature in (-1, 3, 99):
        assert _status(rtmi, lambda: sc.render_feature(feature)) == RT_ERR_ARG
    lib, o = rtmi._lib, rtmi.Opts()
    buf = np.zeros((9, 16, 3), np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert lib.rt_render_hip_feature(None, C.byref(o), 0, ptr, None) == RT_ERR_ARG
    assert lib.rt_render_hip_feature(sc._h, C.byref(o), 0, None, None) == RT_ERR_ARG
    assert lib.rt_render_hip_feature_device(sc._h, C.byref(o), 0, None, None, None) == RT_ERR_ARG
    assert lib.rt_render_hip_feature_device(None, C.byref(o), 0, ptr, None, None) == RT_ERR_ARG
    assert lib.rt_render_hip_feature_device(sc._h, C.byref(o), 3, ptr, None, None) == RT_ERR_ARG


def test_denoise_arguments(rtmi):
    h, w = 9, 16
    img = np.ones((h, w, 3), np.float32)
    good = dict(rgb_sum=img, spp=4, albedo_sum=img, normal_sum=img, depth_sum=img, feature_spp=4)

    def call(**kw):
        a = dict(good, **kw)
        return _status(rtmi, lambda: rtmi.denoise(a.pop("rgb_sum"), a.pop("spp"), a.pop("albedo_sum"), a.pop("normal_sum"),
                                                  a.pop("depth_sum"), a.pop("feature_spp"), **a))

    assert call(spp=0) == RT_ERR_ARG and call(spp=-3) == RT_ERR_ARG
    assert call(feature_spp=0) == RT_ERR_ARG and call(feature_spp=-1) == RT_ERR_ARG
    for name in ("sigma_color", "sigma_normal", "sigma_depth"):
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            assert call(**{name: bad}) == RT_ERR_ARG, (name, bad)
    assert call(iterations=-2) == RT_ERR_ARG and call(iterations=11) == RT_ERR_ARG
    # null pointers and sizes, straight through the C ABI (host and device entry points)
    lib = rtmi._lib
    p = img.ctypes.data_as(C.c_void_p)
    out = np.zeros_like(img)
    q = out.ctypes.data_as(C.c_void_p)
    par = rtmi.Denoise(iterations=1)
    for k in range(5):
        args = [p, p, p, p, q]
        args[k] = None
        assert lib.rt_denoise_hip(w, h, args[0], 4, None, args[1], args[2], args[3], 4, C.byref(par), 0, args[4], None) == RT_ERR_ARG
        assert lib.rt_denoise_hip_device(w, h, args[0], 4, None, args[1], args[2], args[3], 4, C.byref(par), 0, args[4], None, None) == RT_ERR_ARG
    for ww, hh in ((0, h), (w, 0), (-1, h), (w, -5)):
        assert lib.rt_denoise_hip(ww, hh, p, 4, None, p, p, p, 4, None, 0, q, None) == RT_ERR_ARG
        assert lib.rt_denoise_hip_device(ww, hh, p, 4, None, p, p, p, 4, None, 0, q, None, None) == RT_ERR_ARG
    assert "rt_denoise_hip" in lib.rt_last_error().decode()


@pytest.mark.parametrize("value", ["0", "-4", "x", "3.5", "", "99999999999"])
def test_cli_refuses_bad_feature_spp(value, tmp_path):
    p = subprocess.run([os.path.join(PKG, "rtmi"), "--rtiow", "-w", "16", "-h", "9", "-spp", "1", "--denoise", "--feature-spp", value,
                        "-o", str(tmp_path / "a.ppm"), "--no-png"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 2 and "--feature-spp" in p.stderr
    assert not (tmp_path / "a.ppm").exists()


def test_cli_feature_spp_needs_its_flag(tmp_path):
    p = subprocess.run([os.path.join(PKG, "rtmi"), "--rtiow", "--feature-spp", "4", "-o", str(tmp_path / "a.ppm")],
                       capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 2 and not (tmp_path / "a.ppm").exists()


def test_device_wrappers_refuse_null_pointers(rtmi):
    """Scene.render_feature_device and denoise_device: RT_ERR_ARG for a null pointer, before any device is touched (the other
    pointers dangle)."""
    sc = rtmi.Scene.rtiow(7, 16, 9, 2, 4)
    assert _status(rtmi, lambda: sc.render_feature_device(rtmi.FEATURE_ALBEDO, 0)) == RT_ERR_ARG
    assert _status(rtmi, lambda: sc.render_feature_device(rtmi.FEATURE_DEPTH, None, stream=0, stats=rtmi.Stats())) == RT_ERR_ARG
    assert _status(rtmi, lambda: sc.render_feature_device(3, 16)) == RT_ERR_ARG
    for k in range(5):
        ptr = [16, 16, 16, 16, 16]
        ptr[k] = 0 if k % 2 else None
        assert _status(rtmi, lambda: rtmi.denoise_device(16, 9, ptr[0], 4, ptr[1], ptr[2], ptr[3], 4, ptr[4])) == RT_ERR_ARG, k
        assert _status(rtmi, lambda: rtmi.denoise_device(16, 9, ptr[0], 4, ptr[1], ptr[2], ptr[3], 4, ptr[4], 0, d_spp_map=16,
                                                         params=rtmi.Denoise(iterations=0), timing=[])) == RT_ERR_ARG, k
    assert _status(rtmi, lambda: rtmi.denoise_device(16, 9, 16, 0, 16, 16, 16, 4, 16)) == RT_ERR_ARG  # spp 0 without a map
    assert _status(rtmi, lambda: rtmi.denoise_device(16, 9, 16, 4, 16, 16, 16, 4, 16, params=rtmi.Denoise(iterations=11))) == RT_ERR_ARG


# ---- the restatement itself (tests/test_gpu_denoise.py: restate, which the kernel is held to bit for bit) against higher
# precision and against what the filter's definition implies, on the synthetic frames of frame().  No GPU.

# Both bounds are 4 x the largest value measured with this generator (table in DESIGN.md section 7d, "The restatement against
# float64"): room for other seeds and another libm, none for a wrong formula -- a weight of 1/4 in place of 3/8, a tap across a
# coverage boundary or a fused multiply-add moves these figures by orders of magnitude.
FP64_MEASURED = 4.03e-6      # largest relative distance of restate from restate64 (130 x 70, 3 passes)
CONSTANT_MEASURED = 9.32e-7  # largest relative change of a constant demodulated frame (130 x 70, 5 and 10 passes)
FP64_BOUND = 4 * FP64_MEASURED
ROUNDING_BOUND = 4 * CONSTANT_MEASURED


def _cases(w, h):
    rgb, a, n, d = frame(w, h)
    for spp_map in (None, frame_spp_map(w, h)):
        for iterations in PASSES:
            yield rgb, a, n, d, spp_map, dict(DEFAULTS, iterations=iterations)


def _rel(got, want):
    """largest |got - want| / |want|; where want is exactly 0 (the zero-albedo block) got must be too"""
    got, want = got.astype(np.float64), want.astype(np.float64)
    zero = want == 0
    assert (got[zero] == 0).all()
    return float((np.abs(got - want)[~zero] / np.abs(want[~zero])).max()) if (~zero).any() else 0.0


@pytest.mark.parametrize("size", SIZES)
def test_restatement_against_its_float64_twin(size):
    worst = 0.0
    for rgb, a, n, d, spp_map, par in _cases(*size):
        out = restate(rgb, SPP, a, n, d, FEATURE_SPP, spp_map=spp_map, **par)
        assert out.dtype == F and np.isfinite(out).all()
        worst = max(worst, _rel(out, restate64(rgb, SPP, a, n, d, FEATURE_SPP, spp_map=spp_map, **par)))
    print(f"{size[0]} x {size[1]}: largest relative distance fp32 -> fp64 {worst:.3g}")
    assert worst < FP64_BOUND


@pytest.mark.parametrize("size", SIZES)
def test_covered_pixels_do_not_reach_uncovered_ones(size):
    """taps across a coverage boundary are skipped, so the colour of the covered pixels is no input of an uncovered one: exact"""
    w, h = size
    rgb, a, n, d = frame(w, h)
    covered = d[..., 1] != 0
    if covered.all():
        assert (w, h) == (1, 1)  # every larger frame has its block of misses
    brighter = np.where(covered[..., None], rgb * F(3), rgb)
    for spp_map in (None, frame_spp_map(w, h)):
        for iterations in PASSES:
            par = dict(DEFAULTS, iterations=iterations)
            one = restate(rgb, SPP, a, n, d, FEATURE_SPP, spp_map=spp_map, **par)
            two = restate(brighter, SPP, a, n, d, FEATURE_SPP, spp_map=spp_map, **par)
            assert np.array_equal(one[~covered].view(np.uint32), two[~covered].view(np.uint32))
            assert not covered.any() or not np.array_equal(one[covered], two[covered])


@pytest.mark.parametrize("size", SIZES)
def test_constant_demodulated_frame_is_a_fixed_point(size):
    """every weight multiplies the same colour, so (sum w e) / (sum w) is e up to the rounding of the sums"""
    w, h = size
    _, a, n, d = frame(w, h)
    worst = 0.0
    for spp_map in (None, frame_spp_map(w, h)):
        count = (np.maximum(spp_map, 1).astype(F) if spp_map is not None else np.full((h, w), F(SPP), F))[..., None]
        rgb = (np.array([0.7, 1.3, 0.2], F) * np.maximum(a / F(FEATURE_SPP), ALBEDO_EPS)) * count
        for iterations in PASSES:
            out = restate(rgb, SPP, a, n, d, FEATURE_SPP, spp_map=spp_map, **dict(DEFAULTS, iterations=iterations))
            worst = max(worst, _rel(out, rgb))
    print(f"{w} x {h}: largest relative change of a constant demodulated frame {worst:.3g}")
    assert worst < ROUNDING_BOUND


@pytest.mark.parametrize("size", SIZES)
def test_every_pass_is_a_convex_combination(size):
    """after a pass every channel of a pixel's demodulated colour lies between the smallest and the largest value of that
    channel over the taps the pixel took (in the image, of equal coverage), up to the rounding of the sums"""
    w, h = size
    for rgb, a, n, d, spp_map, par in _cases(w, h):
        passes = []
        restate(rgb, SPP, a, n, d, FEATURE_SPP, spp_map=spp_map, passes=passes, **par)
        (e, hit), after = passes[0], passes[1:]
        assert len(after) == par["iterations"]
        for it, e_next in enumerate(after):
            lo, hi = np.full_like(e, np.inf), np.full_like(e, -np.inf)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    yc, xc, ok = tap_grid(h, w, 1 << it, i, j, hit)
                    lo = np.where(ok[..., None], np.minimum(lo, e[yc, xc]), lo)
                    hi = np.where(ok[..., None], np.maximum(hi, e[yc, xc]), hi)
            assert (lo >= 0).all()  # (colours are not negative, so the relative widening below is outward)
            assert (e_next >= lo.astype(np.float64) * (1 - ROUNDING_BOUND)).all(), (it, spp_map is not None)
            assert (e_next <= hi.astype(np.float64) * (1 + ROUNDING_BOUND)).all(), (it, spp_map is not None)
            e = e_next
