"""Interface of the feature passes and the denoiser, as far as it goes without a GPU: exported symbols, the ctypes mirror of
rt_denoise, and the argument checks, which must return RT_ERR_ARG before any device is touched (this file runs on machines
that have none)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

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
