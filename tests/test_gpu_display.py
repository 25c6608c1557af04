"""The display stage on the GPU: rt_display_hip against a numpy float32 restatement of DESIGN.md section 7i, bit for bit on both
outputs.  The input frames are synthetic (nothing is rendered, except for the one frame that pins the defaults to the existing
writer).  The restatement is imported by tests/test_display.py, which checks it against closed forms without a GPU: only the
tests are marked `gpu`, not the module."""
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes")
F = np.float32
B3 = [F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625)]
CLAMP, REINHARD, ACES = 0, 1, 2
SPP = 7
SIZES = [(1, 1), (37, 23), (130, 70)]  # (width, height): one pixel; below the step-16 halo and no multiple of a tile; several workgroups per axis


def counts(h, w, spp, spp_map):
    return (np.maximum(spp_map, 1).astype(F) if spp_map is not None else np.full((h, w), F(spp), F))[..., None]


def quantize(y):
    """int(256 clamp(sqrt(y), 0, 0.999)) in fp32, NaN written black, rows flipped to top-first"""
    with np.errstate(invalid="ignore"):
        v = np.sqrt(y.astype(F))
    v = np.where(np.isnan(v), F(0), np.minimum(np.maximum(v, F(0)), F(0.999)))
    return (F(256) * v).astype(np.int32).astype(np.uint8)[::-1]


def blur(b, step, axis):
    """one direction of one level: five taps `step` apart, clamped coordinates, accumulated from 0 in tap order"""
    n = b.shape[axis]
    acc = np.zeros_like(b)
    for d in range(-2, 3):
        idx = np.clip(np.arange(n) + step * d, 0, n - 1)
        acc = acc + B3[d + 2] * np.take(b, idx, axis=axis)
    return acc


def tone(x, tonemap, white):
    if tonemap == REINHARD:
        iw2 = F(1) / (F(white) * F(white))
        return (x * (F(1) + x * iw2)) / (F(1) + x)
    if tonemap == ACES:
        num = x * (F(2.51) * x + F(0.03))
        den = x * (F(2.43) * x + F(0.59)) + F(0.14)
        return np.minimum(np.maximum(num / den, F(0)), F(1))
    return x


def restate(rgb, spp, tonemap=CLAMP, E=1.0, white=4.0, bloom_strength=0.0, bloom_threshold=0.0, bloom_levels=5, spp_map=None, auto=False):
    """DESIGN 7i in numpy float32, every operation a single correctly rounded fp32 one in the kernels' order, for a given
    multiplier E (auto: it was chosen from the frame, not given) -> (out_rgb, out_rgb8)"""
    h, w = rgb.shape[:2]
    n = counts(h, w, spp, spp_map)
    E = F(E)
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.fmax(rgb / n, F(0)) * E
        if bloom_strength > 0:
            b = np.maximum(x - F(bloom_threshold), F(0))
            s = None
            for k in range(bloom_levels):
                b = blur(blur(b, 1 << k, 1), 1 << k, 0)
                s = b if s is None else s + b
            x = x + F(bloom_strength) * ((F(1) / F(bloom_levels)) * s)
        y = tone(x, tonemap, white)
        assert y.dtype == F
        if tonemap == CLAMP and E == F(1) and not auto and not bloom_strength > 0:
            return y, quantize(rgb * (F(1) / n))  # the identity: the byte in the host writer's form (include/rtmi.h)
        return y, quantize(y)


def log_sum(rgb, spp, spp_map=None):
    """step 2: the exact integer sum of the clamped luminances' bit patterns"""
    h, w = rgb.shape[:2]
    c = np.fmax(rgb / counts(h, w, spp, spp_map), F(0))
    lum = (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]
    lum = np.minimum(np.maximum(lum, F(2.0 ** -20)), F(2.0 ** 20))
    return int((lum.view(np.int32).astype(np.int64) - 0x3F800000).sum())


def auto_exposure(total, pixels, key, exposure=1.0):
    m = total / (pixels * 2.0 ** 23)
    return float(F(key)) * float(F(exposure)) / 2.0 ** m


def frame(w, h, seed=0):
    """a heavy-tailed HDR frame of SUMS over SPP samples, with a block of exact zeros and one "sun" pixel"""
    rng = np.random.default_rng(1000 * w + h + seed)
    mean = np.exp(3.0 * rng.standard_normal((h, w, 3))).astype(F)
    mean[h // 4: h // 4 + max(h // 5, 1), w // 3: w // 3 + max(w // 4, 1)] = 0
    mean[(2 * h) // 3, w // 2] = F(3e4)
    return np.ascontiguousarray(mean * F(SPP))


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


BLOOMS = [None, 1, 5]


@gpu
@pytest.mark.parametrize("tonemap", [CLAMP, REINHARD, ACES])
@pytest.mark.parametrize("size", SIZES)
def test_kernel_equals_the_numpy_restatement(rtmi, size, tonemap):
    w, h = size
    img = frame(w, h)
    for levels in BLOOMS + ([8] if size == (37, 23) else []):
        par = dict(bloom_strength=0.6, bloom_threshold=1.5, bloom_levels=levels) if levels else {}
        rgb, rgb8 = rtmi.display(img, SPP, tonemap=tonemap, exposure=0.37, **par)
        want, want8 = restate(img, SPP, tonemap, 0.37, **par)
        bad = (rgb.view(np.uint32) != want.view(np.uint32)).any(axis=2).sum()
        assert bad == 0, f"{w}x{h} tonemap {tonemap} levels {levels}: {bad} pixels differ in their bits"
        assert np.array_equal(rgb8, want8), (size, tonemap, levels)
        # one output alone is the same output
        assert same_bits(rtmi.display(img, SPP, tonemap=tonemap, exposure=0.37, want_rgb8=False, **par)[0], rgb)
        assert np.array_equal(rtmi.display(img, SPP, tonemap=tonemap, exposure=0.37, want_rgb=False, **par)[1], rgb8)
    if size == (130, 70):  # a white point and a level count of its own, threshold 0
        par = dict(white=2.5, bloom_strength=0.25, bloom_threshold=0.0, bloom_levels=3)
        rgb, rgb8 = rtmi.display(img, SPP, tonemap=tonemap, exposure=0.37, **par)
        want, want8 = restate(img, SPP, tonemap, 0.37, **par)
        assert same_bits(rgb, want) and np.array_equal(rgb8, want8)


@gpu
@pytest.mark.parametrize("size", SIZES)
def test_auto_exposure(rtmi, size):
    w, h = size
    img = frame(w, h)
    want_sum = log_sum(img, SPP)
    for tonemap, exposure, par in ((REINHARD, 0.0, {}), (ACES, 1.7, dict(bloom_strength=0.4, bloom_threshold=1.0, bloom_levels=2))):
        st = rtmi.DisplayStats()
        rgb, rgb8 = rtmi.display(img, SPP, tonemap=tonemap, auto_key=0.18, exposure=exposure, stats=st, **par)
        assert st.log_sum == want_sum
        want_e = auto_exposure(want_sum, w * h, 0.18, exposure or 1.0)
        print(f"{w}x{h}: log_sum {st.log_sum}, exposure_used {st.exposure_used!r} (fp64 restatement {want_e!r})")
        # the one inexact step is a double-precision exp2, then one rounding to fp32 (2^-24 relative)
        assert abs(st.exposure_used - want_e) <= 1e-6 * want_e
        want, want8 = restate(img, SPP, tonemap, st.exposure_used, auto=True, **par)
        assert same_bits(rgb, want) and np.array_equal(rgb8, want8)
        # the atomic sum is order-free: a second call gives the same bytes
        st2 = rtmi.DisplayStats()
        rgb2, rgb8_2 = rtmi.display(img, SPP, tonemap=tonemap, auto_key=0.18, exposure=exposure, stats=st2, **par)
        assert st2.log_sum == st.log_sum and st2.exposure_used == st.exposure_used
        assert same_bits(rgb2, rgb) and np.array_equal(rgb8_2, rgb8)
    st = rtmi.DisplayStats()
    rtmi.display(img, SPP, tonemap=ACES, exposure=0.5, stats=st)
    assert st.log_sum == 0 and st.exposure_used == 0.5 and st.ms > 0


@gpu
@pytest.mark.parametrize("size", SIZES)
def test_defaults_are_todays_output(rtmi, size):
    w, h = size
    img = frame(w, h)
    rgb, rgb8 = rtmi.display(img, SPP)  # a NULL rt_display
    assert same_bits(rgb, img / F(SPP))
    assert np.array_equal(rgb8, rtmi.quantize_rgb8(img, SPP, gamma=True))
    # the same with the defaults spelled out
    rgb_b, rgb8_b = rtmi.display(img, SPP, tonemap=CLAMP, exposure=1.0)
    assert same_bits(rgb_b, rgb) and np.array_equal(rgb8_b, rgb8)


@gpu
def test_defaults_are_todays_output_on_a_render(rtmi):
    sc = rtmi.Scene.load(os.path.join(SCENES, "mixed_emissive.json"))
    sc.override(64, 36, 4)
    img = sc.render(rtmi.Opts(seed=2023))
    rgb, rgb8 = rtmi.display(img, 4)
    assert same_bits(rgb, img / F(4))
    assert np.array_equal(rgb8, rtmi.quantize_rgb8(img, 4, gamma=True))


@gpu
@pytest.mark.parametrize("size", SIZES)
def test_spp_map_path(rtmi, size):
    w, h = size
    img = frame(w, h)
    spp_map = np.array([1, 4, 0], np.int32)[np.random.default_rng(5).integers(0, 3, (h, w))]
    if w * h >= 3:
        spp_map.flat[:3] = (1, 4, 0)
    par = dict(bloom_strength=0.6, bloom_threshold=1.5, bloom_levels=5)
    for tonemap in (CLAMP, ACES):
        rgb, rgb8 = rtmi.display(img, 99, spp_map=spp_map, tonemap=tonemap, exposure=0.37, **par)
        want, want8 = restate(img, 99, tonemap, 0.37, spp_map=spp_map, **par)
        assert same_bits(rgb, want) and np.array_equal(rgb8, want8)
    st, want_sum = rtmi.DisplayStats(), log_sum(img, 99, spp_map)
    rtmi.display(img, 0, spp_map=spp_map, tonemap=REINHARD, auto_key=0.18, stats=st)
    assert st.log_sum == want_sum
    # the defaults through the map: the mean, and the writer's byte
    rgb, rgb8 = rtmi.display(img, 0, spp_map=spp_map)
    want, want8 = restate(img, 0, spp_map=spp_map)
    assert same_bits(rgb, img / counts(h, w, 0, spp_map)) and same_bits(rgb, want) and np.array_equal(rgb8, want8)
    # a constant map is the scalar spp
    const = np.full((h, w), SPP, np.int32)
    for kw in (dict(tonemap=ACES, exposure=0.37, **par), {}):
        a, a8 = rtmi.display(img, 1, spp_map=const, **kw)
        b, b8 = rtmi.display(img, SPP, **kw)
        assert same_bits(a, b) and np.array_equal(a8, b8)


@gpu
def test_device_entry_equals_host_entry(rtmi):
    import torch
    w, h = 130, 70
    img = frame(w, h)
    p = rtmi.Display(tonemap=ACES, exposure=0.37, bloom_strength=0.6, bloom_threshold=1.5, bloom_levels=5)
    want, want8 = rtmi.display(img, SPP, tonemap=ACES, exposure=0.37, bloom_strength=0.6, bloom_threshold=1.5, bloom_levels=5)
    d_in = torch.from_numpy(img).to("cuda:0")
    second = torch.cuda.Stream()
    for stream in (None, second):
        d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        d_out8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        if stream is None:
            rtmi.display_device(w, h, d_in.data_ptr(), SPP, d_out.data_ptr(), d_out8.data_ptr(), 0, params=p)
            torch.cuda.synchronize()
        else:
            with torch.cuda.stream(stream):
                rtmi.display_device(w, h, d_in.data_ptr(), SPP, d_out.data_ptr(), d_out8.data_ptr(), stream.cuda_stream, params=p)
            stream.synchronize()
        assert same_bits(d_out.cpu().numpy(), want) and np.array_equal(d_out8.cpu().numpy(), want8)
    # auto exposure and stats through the device entry, on the second stream
    st, st_host = rtmi.DisplayStats(), rtmi.DisplayStats()
    pa = rtmi.Display(tonemap=REINHARD, auto_key=0.18)
    want, want8 = rtmi.display(img, SPP, tonemap=REINHARD, auto_key=0.18, stats=st_host)
    d_out, d_out8 = torch.zeros_like(d_out), torch.zeros_like(d_out8)
    torch.cuda.synchronize()
    with torch.cuda.stream(second):
        rtmi.display_device(w, h, d_in.data_ptr(), SPP, d_out.data_ptr(), d_out8.data_ptr(), second.cuda_stream, params=pa, stats=st)
    second.synchronize()
    assert st.log_sum == st_host.log_sum == log_sum(img, SPP) and st.exposure_used == st_host.exposure_used
    assert same_bits(d_out.cpu().numpy(), want) and np.array_equal(d_out8.cpu().numpy(), want8)
    # prepare, five levels of two passes, finish -- and the reduction in front of them with auto exposure
    rtmi.display(img, SPP, tonemap=ACES, exposure=0.37, bloom_strength=0.6, bloom_levels=5, stats=st)
    assert len(rtmi.display_timing()) == 12 and abs(sum(rtmi.display_timing()) - st.ms) < 1e-9
    rtmi.display(img, SPP, tonemap=ACES, auto_key=0.18, stats=st)
    assert len(rtmi.display_timing()) == 3


@gpu
def test_kept_buffers_regrow(rtmi):
    """The planes and the staging a device keeps between calls: a small frame, a larger one, the small one again (bloom on at
    2 levels: the four-plane scratch).  A stale or mis-sized buffer would show in the third output or in the second."""
    par = dict(tonemap=ACES, exposure=0.37, bloom_strength=0.6, bloom_threshold=1.5, bloom_levels=2)
    small, large = frame(8, 8), frame(32, 16)
    first, first8 = rtmi.display(small, SPP, **par)
    rgb, rgb8 = rtmi.display(large, SPP, **par)
    third, third8 = rtmi.display(small, SPP, **par)
    assert same_bits(first, third) and np.array_equal(first8, third8)
    want, want8 = restate(large, SPP, ACES, 0.37, bloom_strength=0.6, bloom_threshold=1.5, bloom_levels=2)
    assert same_bits(rgb, want) and np.array_equal(rgb8, want8)


@gpu
@pytest.mark.parametrize("size", SIZES)
def test_bloom_leaves_dark_frames_alone(rtmi, size):
    w, h = size
    img = frame(w, h)
    top = float((img / F(SPP)).max()) * 0.37
    for tonemap in (CLAMP, REINHARD, ACES):
        plain, plain8 = rtmi.display(img, SPP, tonemap=tonemap, exposure=0.37)
        for levels in (1, 5):
            rgb, rgb8 = rtmi.display(img, SPP, tonemap=tonemap, exposure=0.37, bloom_strength=0.8, bloom_threshold=1.01 * top,
                                     bloom_levels=levels)
            assert same_bits(rgb, plain) and np.array_equal(rgb8, plain8)
