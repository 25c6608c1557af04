"""The denoiser on the GPU: rt_denoise_hip against a numpy float32 restatement of DESIGN.md section 7d, bit for bit -- on rendered
frames and, through both entry points, on synthetic ones -- and its effect on the error of a 16-spp frame against a 4096-spp
render of another seed.  The restatement and the synthetic frames are imported by tests/test_denoise.py, which checks the
restatement against its float64 twin without a GPU: only the tests are marked `gpu`, not the module."""
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes")
SEED = 2023
F = np.float32
ALBEDO_EPS, DEPTH_FLOOR, LUM_FLOOR2 = F(1.0 / 1024.0), F(1e-6), F(1.0 / 16.0)
DEFAULTS = dict(iterations=3, sigma_color=0.5, sigma_normal=0.125, sigma_depth=0.05)  # include/rtmi.h
B3 = [F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625)]


def tap_grid(h, w, step, i, j, hit):
    """tap (i, j) of a pass: its clamped row and column indices, and which pixels take it (inside the image, equal coverage)"""
    ys, xs = np.mgrid[0:h, 0:w]
    yy, xx = ys + j * step, xs + i * step
    ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
    yc, xc = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
    return yc, xc, ok & (hit[yc, xc] == hit)


def _restate(T, rgb, spp, albedo, normal, depth, nf, iterations, sigma_color, sigma_normal, sigma_depth, spp_map=None, passes=None):
    """DESIGN 7d in numpy arithmetic of type T, in the kernel's order.  The parameters and constants are the kernel's fp32
    values whatever T is.  passes: a list that receives (demodulated image, coverage mask) before the first pass and the
    demodulated image after every pass."""
    if iterations == 0:
        return rgb.copy()
    rgb, albedo, normal, depth = (a.astype(T) for a in (rgb, albedo, normal, depth))
    h, w = rgb.shape[:2]
    n = (np.maximum(spp_map, 1).astype(T) if spp_map is not None else np.full((h, w), T(spp), T))[..., None]
    nf = T(nf)
    alb = np.maximum(albedo / nf, T(ALBEDO_EPS))
    e = (rgb / n) / alb
    t = depth[..., 0] / nf
    nrm = normal / nf
    cov = depth[..., 1] / nf
    sn, sd, sc = T(F(sigma_normal)), T(F(sigma_depth)), T(F(sigma_color))
    inv_sn2, inv_sd2, inv_sc2 = T(1) / (sn * sn), T(1) / (sd * sd), T(1) / (sc * sc)
    t_ref = np.maximum(t, T(DEPTH_FLOOR))
    hit = cov != 0
    if passes is not None:
        passes.append((e, hit))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for it in range(iterations):
            step = 1 << it
            lum = (e[..., 0] + e[..., 1]) + e[..., 2]
            inv_c = inv_sc2 / (lum * lum + T(LUM_FLOOR2))
            sw = np.zeros((h, w), T)
            acc = np.zeros((h, w, 3), T)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    yc, xc, ok = tap_grid(h, w, step, i, j, hit)
                    dn = nrm[yc, xc] - nrm
                    kn = T(1) / (T(1) + ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]) * inv_sn2)
                    r = np.abs(t[yc, xc] - t) / t_ref
                    kd = T(1) / (T(1) + (r * r) * inv_sd2)
                    eq = e[yc, xc]
                    de = eq - e
                    kc = T(1) / (T(1) + ((de[..., 0] * de[..., 0] + de[..., 1] * de[..., 1]) + de[..., 2] * de[..., 2]) * inv_c)
                    wgt = (((T(B3[i + 2]) * T(B3[j + 2])) * (kn * kn)) * (kd * kd)) * (kc * kc)
                    sw = np.where(ok, sw + wgt, sw)
                    acc = np.where(ok[..., None], acc + wgt[..., None] * eq, acc)
            e = acc / sw[..., None]
            inv_sc2 = inv_sc2 * T(4)
            if passes is not None:
                passes.append(e)
    assert e.dtype == T
    return (e * alb) * n


def restate(rgb, spp, albedo, normal, depth, nf, iterations, sigma_color, sigma_normal, sigma_depth, spp_map=None, passes=None):
    """DESIGN 7d in numpy float32: every operation a single correctly rounded fp32 one, in the kernel's order"""
    return _restate(F, rgb, spp, albedo, normal, depth, nf, iterations, sigma_color, sigma_normal, sigma_depth, spp_map, passes)


def restate64(rgb, spp, albedo, normal, depth, nf, iterations, sigma_color, sigma_normal, sigma_depth, spp_map=None, passes=None):
    """the float64 twin: the same formulas, order, parameters and constants, every operation in float64"""
    return _restate(np.float64, rgb, spp, albedo, normal, depth, nf, iterations, sigma_color, sigma_normal, sigma_depth, spp_map,
                    passes)


SPP, FEATURE_SPP = 7, 5
# (width, height): one pixel; smaller than the tap spacing of every pass but the first two; no multiple of the 16 x 16 workgroup
# and inside the step-16 halo; several workgroups per axis
SIZES = [(1, 1), (5, 3), (37, 23), (130, 70)]
PASSES = [1, 3, 5, 10]


def frame(w, h):
    """A synthetic frame for the filter: (rgb_sum, albedo_sum, normal_sum, depth_sum), sums over SPP and FEATURE_SPP samples,
    seeded per size.  The left half has one normal and a gentle depth ramp, the right half random unit normals and depths; a
    block of exactly zero albedo (the demodulation floor); a block of misses (coverage, normal and depth 0) among hits;
    scattered pixels of partial coverage; colour = albedo x a log-normal factor."""
    rng = np.random.default_rng(7000 * w + h)
    ys, xs = np.mgrid[0:h, 0:w]
    left = xs < (w + 1) // 2
    nrm = rng.standard_normal((h, w, 3))
    nrm /= np.sqrt((nrm * nrm).sum(axis=2, keepdims=True))
    nrm[left] = (0.0, 0.6, 0.8)
    t = rng.uniform(1.0, 20.0, (h, w))
    t[left] = (5.0 + 0.01 * xs + 0.02 * ys)[left]
    hits = np.full((h, w), FEATURE_SPP, np.int64)  # feature samples that hit
    partial = rng.random((h, w)) < 0.06
    hits[partial] = rng.integers(1, FEATURE_SPP, (h, w))[partial]
    hits[h // 2: h // 2 + (h + 2) // 4, w // 4: w // 4 + (w + 1) // 3] = 0  # (1 x 1: no block, one covered pixel; 5 x 3: 1 x 2)
    albedo = rng.uniform(0.05, 1.0, (h, w, 3))
    albedo[h // 5: h // 5 + (h + 2) // 5, (3 * w) // 5: (3 * w) // 5 + (w + 2) // 4] = 0.0  # (5 x 3: one pixel)
    mean = albedo * np.exp(rng.standard_normal((h, w, 3)))
    depth = np.stack([t * hits, hits.astype(np.float64), np.zeros((h, w))], axis=2)
    return tuple(np.ascontiguousarray(a, dtype=F) for a in (mean * SPP, albedo * FEATURE_SPP, nrm * hits[..., None], depth))


def frame_spp_map(w, h):
    """per-pixel sample counts for frame(w, h), drawn from {0, 1, 4} (an entry < 1 counts as 1)"""
    return np.random.default_rng(7000 * w + h + 1).choice(np.array([0, 1, 4], np.int32), size=(h, w))


def mixed(rtmi, w, h, spp, nee=False):
    sc = rtmi.Scene.load(os.path.join(SCENES, "mixed_emissive.json"))
    sc.override(w, h, spp)
    sc.set_light_sampling(nee)
    return sc


def features(rtmi, sc, nf, seed=SEED):
    return [sc.render_feature(f, rtmi.Opts(seed=seed, sample_count=nf)) for f in range(3)]


@gpu
@pytest.mark.parametrize("which", ["mixed_emissive", "rtiow"])
def test_kernel_equals_the_numpy_restatement(rtmi, which):
    sc = mixed(rtmi, 64, 36, 16) if which == "mixed_emissive" else rtmi.Scene.rtiow(7, 64, 36, 16, 20)
    a, n, d = features(rtmi, sc, 8)
    img = sc.render(rtmi.Opts(seed=SEED))
    ad_img, ad_map, _ = sc.render_adaptive(0.05, min_spp=4, max_spp=32, opts=rtmi.Opts(seed=SEED))
    assert len(np.unique(ad_map)) > 1
    for iterations in (1, 3, 5):
        par = dict(DEFAULTS, iterations=iterations)
        for rgb, spp_map in ((img, None), (ad_img, ad_map)):
            got = rtmi.denoise(rgb, 16, a, n, d, 8, spp_map=spp_map, iterations=iterations)
            want = restate(rgb, 16, a, n, d, 8, spp_map=spp_map, **par)
            bad = (got.view(np.uint32) != want.view(np.uint32)).any(axis=2).sum()
            assert bad == 0, f"{iterations} passes, spp_map {spp_map is not None}: {bad} pixels differ in their bits"
            assert np.isfinite(got).all()
    # explicit sigmas, and the defaults spelled out
    got = rtmi.denoise(img, 16, a, n, d, 8, iterations=2, sigma_color=1.5, sigma_normal=0.25, sigma_depth=0.125)
    want = restate(img, 16, a, n, d, 8, 2, 1.5, 0.25, 0.125)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(rtmi.denoise(img, 16, a, n, d, 8), rtmi.denoise(img, 16, a, n, d, 8, **DEFAULTS))
    # no pass: the input bits
    assert np.array_equal(rtmi.denoise(img, 16, a, n, d, 8, iterations=0).view(np.uint32), img.view(np.uint32))
    assert np.array_equal(rtmi.denoise(ad_img, 16, a, n, d, 8, spp_map=ad_map, iterations=0).view(np.uint32), ad_img.view(np.uint32))


@gpu
def test_kept_buffers_regrow(rtmi):
    """The records a device keeps between calls: a small frame, a larger one, the small one again.  A stale or mis-sized
    buffer would show in the third output or in the second."""
    frames = {}
    for w, h in ((8, 8), (32, 16)):
        sc = mixed(rtmi, w, h, 4)
        frames[w, h] = (sc.render(rtmi.Opts(seed=SEED)), *features(rtmi, sc, 2))
    outs = [rtmi.denoise(frames[size][0], 4, *frames[size][1:], 2) for size in ((8, 8), (32, 16), (8, 8))]
    assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))
    img, a, n, d = frames[32, 16]
    want = restate(img, 4, a, n, d, 2, **DEFAULTS)
    bad = (outs[1].view(np.uint32) != want.view(np.uint32)).any(axis=2).sum()
    assert bad == 0, f"{bad} pixels differ in their bits"


def _rmse(mean, ref):
    return float(np.sqrt(np.mean((mean.astype(np.float64) - ref) ** 2)))


@gpu
@pytest.mark.parametrize("which", ["mixed_emissive_nee", "rtiow"])
def test_denoised_frame_is_closer_to_the_converged_one(rtmi, which):
    w, h, spp = 160, 90, 16
    make = (lambda n: mixed(rtmi, w, h, n, nee=True)) if which == "mixed_emissive_nee" else (lambda n: rtmi.Scene.rtiow(7, w, h, n, 50))
    ref = make(4096).render(rtmi.Opts(seed=SEED + 1)).astype(np.float64) / 4096.0  # the existing render path, another seed
    sc = make(spp)
    img = sc.render(rtmi.Opts(seed=SEED))
    a, n, d = features(rtmi, sc, spp)
    out = rtmi.denoise(img, spp, a, n, d, spp)
    before, after = _rmse(img / F(spp), ref), _rmse(out / F(spp), ref)
    print(f"{which}: RMSE {before:.5f} -> {after:.5f} (ratio {after / before:.3f})")
    assert after < before


def denoise_on_device(rtmi, rgb, spp, albedo, normal, depth, nf, spp_map=None, iterations=None, stream=None, timing=None):
    """rt_denoise_hip_device on torch tensors; the output tensor starts as NaN, so an unwritten element shows"""
    import torch
    h, w = rgb.shape[:2]
    d = [torch.from_numpy(a).to("cuda:0") for a in (rgb, albedo, normal, depth)]
    d_map = torch.from_numpy(spp_map).to("cuda:0") if spp_map is not None else None
    d_out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda:0")
    par = rtmi.Denoise(iterations=rtmi.DENOISE_DEFAULT_ITERATIONS if iterations is None else iterations)
    torch.cuda.synchronize()
    rtmi.denoise_device(w, h, d[0].data_ptr(), spp, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), nf, d_out.data_ptr(),
                        stream.cuda_stream if stream is not None else 0, d_spp_map=d_map.data_ptr() if d_map is not None else None,
                        params=par, timing=timing)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@gpu
@pytest.mark.parametrize("size", SIZES)
def test_synthetic_frames_through_both_entries(rtmi, size):
    """frame(): frames smaller than the tap spacing, no multiple of the 16 x 16 workgroup, the albedo floor, misses beside hits,
    up to 10 passes (step 512), with and without an spp_map -- host and device entry, each bit for bit the restatement."""
    w, h = size
    rgb, a, n, d = frame(w, h)
    for spp_map in (None, frame_spp_map(w, h)):
        for iterations in PASSES:
            want = restate(rgb, SPP, a, n, d, FEATURE_SPP, spp_map=spp_map, **dict(DEFAULTS, iterations=iterations))
            assert np.isfinite(want).all()
            for entry in ("host", "device"):
                if entry == "host":
                    got = rtmi.denoise(rgb, SPP, a, n, d, FEATURE_SPP, spp_map=spp_map, iterations=iterations)
                else:
                    got = denoise_on_device(rtmi, rgb, SPP, a, n, d, FEATURE_SPP, spp_map=spp_map, iterations=iterations)
                assert np.isfinite(got).all(), (entry, iterations)
                bad = (got.view(np.uint32) != want.view(np.uint32)).any(axis=2).sum()
                assert bad == 0, f"{entry} entry, {iterations} passes, spp_map {spp_map is not None}: {bad} pixels differ in their bits"
