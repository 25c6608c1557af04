"""Adaptive sampling (rt_render_hip_adaptive) without a GPU: the arguments are checked before any device access, the
ctypes mirrors match the C structs, and the CLI refuses what it cannot combine."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
SCENES = os.path.join(PKG, "scenes")
RTMI = os.path.join(PKG, "rtmi")

RT_ERR_ARG, RT_ERR_LIMIT = 1, 6


def _call(rtmi, sc, a, opts=None, out=True, spp_map=True, st=True):
    lib = rtmi._lib
    h, w = (sc.height, sc.width) if sc is not None else (8, 8)
    img = np.empty((h, w, 3), np.float32)
    spp = np.empty((h, w), np.int32)
    return lib.rt_render_hip_adaptive(sc._h if sc is not None else None, C.byref(opts or rtmi.Opts()),
                                      C.byref(a) if a is not None else None,
                                      img.ctypes.data_as(C.c_void_p) if out else None,
                                      spp.ctypes.data_as(C.c_void_p) if spp_map else None,
                                      C.byref(rtmi.AdaptiveStats()) if st else None)


def _device_call(rtmi, sc, a, opts=None):
    # the device entry point with dangling device pointers: an argument error must come back before they are touched
    return rtmi._lib.rt_render_hip_adaptive_device(sc._h, C.byref(opts or rtmi.Opts()), C.byref(a), C.c_void_p(16),
                                                   C.c_void_p(16), None, None)


@pytest.fixture()
def scene(rtmi):
    sc = rtmi.Scene.load(os.path.join(SCENES, "mixed_emissive.json"))
    sc.override(40, 24, 32)
    return sc


def test_struct_mirrors(rtmi):
    assert C.sizeof(rtmi.Adaptive) == rtmi.struct_size(8) == 12
    assert C.sizeof(rtmi.AdaptiveStats) == rtmi.struct_size(9) == 8 + 2 * 32 * 4 + 8 + 8
    assert rtmi.AdaptiveStats.samples.offset == 264 and rtmi.AdaptiveStats.kernel_ms.offset == 272


@pytest.mark.parametrize("fields, why", [
    ((1, 16, 0.1), "min_spp < 2"),
    ((0, 16, 0.1), "min_spp < 2"),
    ((-4, 16, 0.1), "min_spp < 2"),
    ((8, 4, 0.1), "max_spp < min_spp"),
    ((64, 0, 0.1), "max_spp 0 is the scene's 32 < min_spp"),
    ((4, 16, -0.5), "negative threshold"),
    ((4, 16, float("nan")), "NaN threshold"),
    ((4, 16, float("inf")), "infinite threshold"),
])
def test_bad_schedule(rtmi, scene, fields, why):
    a = rtmi.Adaptive(*fields)
    assert _call(rtmi, scene, a) == RT_ERR_ARG, why
    assert _device_call(rtmi, scene, a) == RT_ERR_ARG, why


def test_max_spp_beyond_the_exact_range(rtmi, scene):
    # the status of render_impl's per-pixel sample cap (2^23 samples keep the 64-bit sums exact)
    a = rtmi.Adaptive(16, (1 << 23) + 1, 0.1)
    assert _call(rtmi, scene, a) == RT_ERR_LIMIT
    assert _device_call(rtmi, scene, a) == RT_ERR_LIMIT


def test_null_arguments(rtmi, scene):
    a = rtmi.Adaptive(4, 16, 0.1)
    assert _call(rtmi, None, a) == RT_ERR_ARG
    assert _call(rtmi, scene, None) == RT_ERR_ARG
    assert _call(rtmi, scene, a, out=False) == RT_ERR_ARG
    assert _call(rtmi, scene, a, spp_map=False) == RT_ERR_ARG
    lib = rtmi._lib
    assert lib.rt_render_hip_adaptive_device(scene._h, None, C.byref(a), None, C.c_void_p(16), None, None) == RT_ERR_ARG
    assert lib.rt_render_hip_adaptive_device(scene._h, None, C.byref(a), C.c_void_p(16), None, None, None) == RT_ERR_ARG


@pytest.mark.parametrize("opts, why", [
    (dict(tile_stride=2), "shards"),
    (dict(tile_stride=4, tile_first=1), "shards"),
    (dict(sample_first=8), "the schedule owns the samples"),
    (dict(sample_count=8), "the schedule owns the samples"),
    (dict(variant=3), "unknown variant"),
    (dict(variant=12345), "unknown variant"),
])
def test_bad_options(rtmi, scene, opts, why):
    a = rtmi.Adaptive(4, 16, 0.1)
    assert _call(rtmi, scene, a, rtmi.Opts(**opts)) == RT_ERR_ARG, why
    assert _device_call(rtmi, scene, a, rtmi.Opts(**opts)) == RT_ERR_ARG, why


def test_python_wrapper_raises(rtmi, scene):
    with pytest.raises(rtmi.RtmiError) as e:
        scene.render_adaptive(-1.0)
    assert e.value.status == RT_ERR_ARG
    with pytest.raises(rtmi.RtmiError) as e:
        scene.render_adaptive(0.1, min_spp=1)
    assert e.value.status == RT_ERR_ARG
    with pytest.raises(rtmi.RtmiError) as e:
        scene.render_adaptive(0.1, opts=rtmi.Opts(tile_stride=2))
    assert e.value.status == RT_ERR_ARG


def test_device_wrapper_refuses_null_pointers(rtmi, scene):
    """Scene.render_adaptive_device: RT_ERR_ARG for a null pointer or a bad schedule, before any device is touched (the other
    pointer dangles)."""
    for rgb, spp in ((0, 16), (16, 0), (None, 16), (16, None), (0, 0)):
        with pytest.raises(rtmi.RtmiError) as e:
            scene.render_adaptive_device(0.1, rgb, spp, min_spp=4, max_spp=16)
        assert e.value.status == RT_ERR_ARG, (rgb, spp)
    with pytest.raises(rtmi.RtmiError) as e:
        scene.render_adaptive_device(-1.0, 16, 16, stream=0)
    assert e.value.status == RT_ERR_ARG
    with pytest.raises(rtmi.RtmiError) as e:
        scene.render_adaptive_device(0.1, 16, 16, min_spp=4, opts=rtmi.Opts(tile_stride=2))
    assert e.value.status == RT_ERR_ARG


@pytest.mark.parametrize("extra", [
    ["--gpus", "2"],
    ["--acc-out", "sums.bin"],
    ["--acc-in", "sums.bin"],
    ["--spp-begin", "0"],
    ["--count"],
    ["--min-spp", "1"],
    ["--max-spp", "4", "--min-spp", "8"],
])
def test_cli_refuses(tmp_path, extra):
    p = subprocess.run([RTMI, "-f", os.path.join(SCENES, "mixed_emissive.json"), "--adaptive", "0.05", "-o",
                        str(tmp_path / "x.ppm")] + extra, capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode != 0
    assert "rtmi:" in p.stderr
    assert not (tmp_path / "x.ppm").exists()


@pytest.mark.parametrize("args", [["--adaptive", "-0.1"], ["--adaptive", "nan"], ["--adaptive", "inf"], ["--adaptive", "x"],
                                  ["--min-spp", "4"], ["--max-spp", "64"]])
def test_cli_bad_values(tmp_path, args):
    p = subprocess.run([RTMI, "-f", os.path.join(SCENES, "mixed_emissive.json"), "-o", str(tmp_path / "x.ppm")] + args,
                       capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 2, p.stderr
    assert not (tmp_path / "x.ppm").exists()
