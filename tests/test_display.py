"""Interface of the display stage and the HDR writers, as far as it goes without a GPU: exported symbols, the ctypes mirrors,
the argument checks (RT_ERR_ARG before any device is touched: this file runs on machines that have none), the round trip of
both float image files through the environment reader, the numpy restatement of tests/test_gpu_display.py against closed
forms, and the command line's refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_display import ACES, B3, CLAMP, REINHARD, F, restate, tone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
RT_ERR_ARG, RT_ERR_IO = 1, 2
NEW = ["rt_display_hip", "rt_display_hip_device", "rt_display_timing", "rt_write_hdr", "rt_write_pfm", "rt_write_ppm_rgb8",
       "rt_write_png_rgb8"]


@pytest.mark.parametrize("lib", ["librtmi.so", "librtmi_product.so"])
def test_symbols_are_exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, lib)], capture_output=True, text=True, check=True).stdout
    have = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW) <= have


@pytest.mark.parametrize("lib", ["librtmi.so", "librtmi_product.so"])
def test_the_stage_has_kernels_of_its_own(lib):
    """by the kernels' names alone, in whatever host symbols the toolchain makes for them (stubs, handles)"""
    out = subprocess.run(["nm", "--defined-only", os.path.join(PKG, lib)], capture_output=True, text=True, check=True).stdout
    for k in ("display_reduce_kernel", "display_prepare_kernel", "display_blur_kernel", "display_finish_kernel"):
        assert any(k in line for line in out.splitlines()), k


def test_struct_mirrors(rtmi):
    assert set(NEW) <= set(rtmi.C_SYMBOLS)
    assert C.sizeof(rtmi.Display) == rtmi.struct_size(19) == 28
    assert C.sizeof(rtmi.DisplayStats) == rtmi.struct_size(20) == 24
    assert (rtmi.TONEMAP_CLAMP, rtmi.TONEMAP_REINHARD, rtmi.TONEMAP_ACES) == (0, 1, 2)
    assert rtmi.abi_version() == 3


def test_display_arguments(rtmi):
    h, w = 9, 16
    img = np.ones((h, w, 3), np.float32)
    lib = rtmi._lib
    p = img.ctypes.data_as(C.c_void_p)
    out, out8 = np.zeros_like(img), np.zeros((h, w, 3), np.uint8)
    q, q8 = out.ctypes.data_as(C.c_void_p), out8.ctypes.data_as(C.c_void_p)
    spp_map = np.ones((h, w), np.int32)
    m = spp_map.ctypes.data_as(C.c_void_p)

    def both(ww, hh, rgb, spp, mp, par, o, o8):
        par = C.byref(par) if par is not None else None
        a = lib.rt_display_hip(ww, hh, rgb, spp, mp, par, 0, o, o8, None)
        b = lib.rt_display_hip_device(ww, hh, rgb, spp, mp, par, 0, o, o8, None, None)
        assert a == b, (a, b)
        return a

    assert both(w, h, None, 4, None, None, q, q8) == RT_ERR_ARG      # a null input
    assert both(w, h, p, 4, None, None, None, None) == RT_ERR_ARG    # both outputs null
    assert "rt_display_hip" in lib.rt_last_error().decode()
    for ww, hh in ((0, h), (w, 0), (-1, h), (w, -5), (65537, h), (w, 65537)):
        assert both(ww, hh, p, 4, None, None, q, q8) == RT_ERR_ARG
    for spp in (0, -3):
        assert both(w, h, p, spp, None, None, q, q8) == RT_ERR_ARG   # spp <= 0 without a map
    for name in ("exposure", "auto_key", "white", "bloom_strength", "bloom_threshold"):
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            for mp in (None, m):
                assert both(w, h, p, 4, mp, rtmi.Display(**{name: bad}), q, q8) == RT_ERR_ARG, (name, bad)
    for t in (-1, 3, 99):
        assert both(w, h, p, 4, None, rtmi.Display(tonemap=t), q, q8) == RT_ERR_ARG
    for levels in (-1, 9):
        assert both(w, h, p, 4, None, rtmi.Display(bloom_levels=levels), q, None) == RT_ERR_ARG
        assert both(w, h, p, 4, None, rtmi.Display(bloom_levels=levels, bloom_strength=1.0), None, q8) == RT_ERR_ARG
    # and through the binding
    for kw in (dict(exposure=-1.0), dict(tonemap=5), dict(bloom_levels=9), dict(want_rgb=False, want_rgb8=False)):
        with pytest.raises(rtmi.RtmiError) as e:
            rtmi.display(img, 4, **kw)
        assert e.value.status == RT_ERR_ARG, kw
    with pytest.raises(rtmi.RtmiError) as e:
        rtmi.display(img, 0)
    assert e.value.status == RT_ERR_ARG
    assert lib.rt_display_timing(None, 0) == 0  # (no call with stats has run on this thread)


def _read_back(rtmi, path):
    sc = rtmi.Scene.new(8, 8, 1)
    assert rtmi._lib.rt_scene_set_environment_file(sc._h, os.fsencode(path), 1.0, 0.0) == 0, rtmi._lib.rt_last_error()
    rows, cols = C.c_int(), C.c_int()
    assert rtmi._lib.rt_scene_get_environment(sc._h, C.byref(rows), C.byref(cols), None, None, None, 0) == 0
    tex = np.zeros((rows.value, cols.value, 3), np.float32)
    assert rtmi._lib.rt_scene_get_environment(sc._h, None, None, None, None, tex.ctypes.data_as(C.c_void_p), tex.size) == 0
    return tex


def _frame_7x5():
    rng = np.random.default_rng(11)
    return np.exp(2.0 * rng.standard_normal((5, 7, 3))).astype(np.float32)


def test_pfm_round_trip(rtmi, tmp_path):
    img = _frame_7x5()
    path = str(tmp_path / "a.pfm")
    rtmi.write_pfm(img, 1, path)
    raw = open(path, "rb").read()
    assert raw.startswith(b"PF\n7 5\n-1.0\n") and len(raw) == 12 + 5 * 7 * 3 * 4
    tex = _read_back(rtmi, path)
    assert tex.shape == (5, 7, 3)
    for r in range(5):  # texel row r (0: the zenith) is frame row H - 1 - r (the frame's row 0 is its bottom)
        assert np.array_equal(tex[r].view(np.uint32), img[5 - 1 - r].view(np.uint32)), r
    # the mean: sums over 4 samples
    rtmi.write_pfm(img * np.float32(4), 4, path)
    assert np.array_equal(_read_back(rtmi, path)[::-1].view(np.uint32), img.view(np.uint32))


@pytest.mark.parametrize("which", ["random", "edge_values"])
def test_hdr_round_trip(rtmi, tmp_path, which):
    img = _frame_7x5()
    if which == "edge_values":  # zeros, one value at 2^15, one at 2^-20
        img[:] = 0
        img[1, 2, 0] = 2.0 ** 15
        img[3, 4, 1] = 2.0 ** -20
        img[4, 6] = (2.0 ** 15, 2.0 ** -20, 0.0)
    path = str(tmp_path / "a.hdr")
    rtmi.write_hdr(img * np.float32(2), 2, path)
    raw = open(path, "rb").read()
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 5 +X 7\n"
    assert raw.startswith(head) and len(raw) == len(head) + 5 * 7 * 4  # flat scanlines
    tex = _read_back(rtmi, path)
    assert tex.shape == (5, 7, 3)
    got = tex[::-1]  # texel row r is frame row H - 1 - r, as for the PFM file
    # RGBE: an 8-bit mantissa under the exponent of the largest channel, truncated
    bound = img.max(axis=2, keepdims=True) / np.float32(128)
    assert (np.abs(got.astype(np.float64) - img) <= bound).all()
    assert (got <= img).all()  # truncation never rounds up
    assert np.array_equal(got[img.max(axis=2) == 0], img[img.max(axis=2) == 0])
    if which == "edge_values":
        assert got[1, 2, 0] == 2.0 ** 15 and got[3, 4, 1] == 2.0 ** -20 and got[4, 6, 0] == 2.0 ** 15 and got[4, 6, 1] == 0
    else:
        assert not np.array_equal(tex[0], tex[4])  # (the orientation check above can tell rows apart)


def test_writer_arguments(rtmi, tmp_path):
    img = np.ones((4, 4, 3), np.float32)
    p = img.ctypes.data_as(C.c_void_p)
    for fn in (rtmi._lib.rt_write_hdr, rtmi._lib.rt_write_pfm):
        good = os.fsencode(str(tmp_path / "x.img"))
        assert fn(None, p, 4, 4, 1) == RT_ERR_ARG and fn(good, None, 4, 4, 1) == RT_ERR_ARG
        assert fn(good, p, 0, 4, 1) == RT_ERR_ARG and fn(good, p, 4, -1, 1) == RT_ERR_ARG and fn(good, p, 4, 4, 0) == RT_ERR_ARG
        assert fn(os.fsencode(str(tmp_path / "no_such_dir" / "x.img")), p, 4, 4, 1) == RT_ERR_IO


# ---- the restatement against closed forms ----
def test_restated_bloom_of_one_pixel_is_the_b3_kernel():
    img = np.zeros((9, 9, 3), np.float32)
    img[4, 4] = (8.0, 4.0, 2.0)
    out, _ = restate(img, 1, CLAMP, 1.0, bloom_strength=1.0, bloom_threshold=0.0, bloom_levels=1)
    h = np.array(B3, np.float32)
    glow = np.zeros((9, 9), np.float32)
    glow[2:7, 2:7] = np.outer(h, h)  # products of dyadic fractions: exact
    for c, v in enumerate((8.0, 4.0, 2.0)):
        assert np.array_equal(out[..., c], img[..., c] + np.float32(v) * glow)
    # a threshold takes its cut before the blur
    out, _ = restate(img, 1, CLAMP, 1.0, bloom_strength=1.0, bloom_threshold=2.0, bloom_levels=1)
    assert np.array_equal(out[..., 0], img[..., 0] + np.float32(6.0) * glow) and np.array_equal(out[..., 2], img[..., 2])


def test_restated_bloom_keeps_the_energy_of_a_constant_frame():
    img = np.full((12, 20, 3), 0.75, np.float32)
    for levels in (1, 4, 8):  # clamped coordinates: a constant plane stays constant at every level (the taps sum to 1 exactly)
        out, _ = restate(img, 1, CLAMP, 1.0, bloom_strength=0.5, bloom_threshold=0.25, bloom_levels=levels)
        assert np.allclose(out, 0.75 + 0.5 * 0.5, rtol=1e-6, atol=0)


def test_restated_curves():
    x = np.concatenate([np.zeros(1), np.exp(np.linspace(np.log(1e-6), np.log(1e6), 4001))]).astype(np.float32)
    assert np.array_equal(tone(x, CLAMP, 4.0), x)
    for white in (1.0, 4.0, 100.0):
        y = tone(x, REINHARD, white)
        assert (np.diff(y) >= 0).all() and y[0] == 0
        assert abs(float(tone(np.float32(white), REINHARD, white)) - 1.0) < 1e-6  # the white point maps to 1
    y = tone(x, ACES, 4.0)
    assert (np.diff(y) >= 0).all() and y[0] == 0 and y.max() == 1.0 and (y >= 0).all()
    img = np.abs(np.random.default_rng(3).standard_normal((6, 5, 3))).astype(np.float32)
    out, out8 = restate(img * np.float32(3), 3, CLAMP, 1.0)
    assert np.array_equal(out, img * np.float32(3) / np.float32(3)) and out8.shape == (6, 5, 3) and out8.dtype == np.uint8


def test_restated_defaults_quantise_as_the_writer(rtmi):
    """sums n k^2 / 65536 lie on the quantiser's steps, where sum / n and sum x (1 / n) part: the identity stage follows the writer"""
    k = np.arange(1, 256, dtype=np.float64)
    for n in (7, 41, 100):
        img = np.zeros((5, 17, 3), np.float32)
        img.reshape(-1)[:] = (n * k * k / 65536.0).astype(np.float32)
        _, out8 = restate(img, n)
        assert np.array_equal(out8, rtmi.quantize_rgb8(img, n, gamma=True))


# ---- command line ----
def _cli(tmp_path, *args):
    return subprocess.run([os.path.join(PKG, "rtmi"), "--rtiow", "-w", "16", "-h", "9", "-spp", "1", "-o", str(tmp_path / "a.ppm"), "--no-png",
                           *args], capture_output=True, text=True, timeout=120, cwd=tmp_path)


@pytest.mark.parametrize("args, word", [
    (["--tonemap", "filmic"], "--tonemap"), (["--tonemap", ""], "--tonemap"),
    (["--hdr-out", "frame.exr"], "--hdr-out"), (["--hdr-out", "frame"], "--hdr-out"), (["--hdr-out", "frame.hdr.png"], "--hdr-out"),
    (["--exposure", "bright"], "--exposure"), (["--exposure", "nan"], "--exposure"), (["--white", "-1"], "--white"),
    (["--white", "0"], "--white"), (["--bloom", "-0.5"], "--bloom"), (["--bloom-threshold", "x"], "--bloom-threshold"),
    (["--bloom-levels", "0"], "--bloom-levels"), (["--bloom-levels", "9"], "--bloom-levels"), (["--auto-exposure", "-1"], "--auto-exposure"),
])
def test_cli_refuses_bad_display_flags(args, word, tmp_path):
    p = _cli(tmp_path, *args)
    # the flag's own message, not the one an unknown argument gets
    assert p.returncode == 2 and f"rtmi: {word} needs" in p.stderr and "unknown argument" not in p.stderr, p.stderr
    assert not (tmp_path / "a.ppm").exists() and "HIP" not in p.stderr


def test_cli_help_lists_the_display_flags(tmp_path):
    p = subprocess.run([os.path.join(PKG, "rtmi"), "--help"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    for flag in ("--tonemap", "--exposure", "--auto-exposure", "--white", "--bloom", "--bloom-threshold", "--bloom-levels", "--hdr-out"):
        assert flag in p.stderr, flag
