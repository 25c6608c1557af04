"""Environment maps on the GPU: the bit-exact invariants, the device lookup against the host evaluation, unbiasedness
against today's estimator (the same map as an image texture on a giant emissive sphere), an analytic known answer and the
refusals."""
import json
import os
import sys

import numpy as np
import pytest

from nee_scenes import PATCH_ROWS, PATCH_COLS, patch_expected, patch_scene
from test_gpu_light_sampling import compare
from test_nested_grid import dense_room

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes")

pytestmark = pytest.mark.gpu
SEED = 31
ENV = 1024


@pytest.fixture(scope="module")
def rtmi():
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    mod = load_package()
    if mod.device_count() < 1:
        pytest.skip("no HIP device")
    return mod


def sky_map(rows=8, cols=16, seed=2, sun=40.0):
    """a sky over a dark ground with a sun; multiples of 2^-8, which the exact 2^-24 fixed-point pixel sums hold without rounding"""
    rng = np.random.default_rng(seed)
    k = rng.integers(13, 218, (rows, cols, 3))
    k[rows // 2:] //= 3
    env = (k / 256.0).astype(np.float32)
    env[1, 3] = (sun, sun * 0.875, sun * 0.75)
    return env


def objects(sc, rtmi):
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.4, 0.2))))
    sc.sphere((-1.2, 0.6, 0.5), 0.6, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((1.3, 0.5, 0.8), 0.5, sc.metal((0.8, 0.7, 0.6), 0.3))
    sc.sphere((0.1, 0.45, 1.6), 0.45, sc.dielectric(1.5))
    sc.cylinder(0.2, -0.6, 0.6, sc.metal((0.9, 0.9, 0.9), 0.0), rotate=((1.0, 0.0, 0.0), 90.0), translate=(2.4, 0.6, -0.5))
    sc.triangle((-3, 0, -2), (-2, 0, -2.5), (-2.5, 1.5, -2.2), sc.lambertian((0.7, 0.3, 0.3)))


def env_scene(rtmi, env=None, w=64, h=36, spp=16, depth=6, nee=False, scale=1.0, rotate=25.0, background=(0, 0, 0), emitter=True):
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background(background, sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    objects(sc, rtmi)
    if emitter:
        sc.xz_rect(-0.6, 0.6, -0.6, 0.6, 2.5, sc.diffuse_light((6.0, 5.0, 4.0)))
    if env is not None:
        sc.set_environment(env, scale, rotate)
    sc.set_light_sampling(nee)
    return sc


# ---- bit-exact --------------------------------------------------------------------------------------------------------------
def test_constant_map_is_the_constant_background(rtmi):
    c = (0.25, 0.5, 0.75)
    bg = env_scene(rtmi, None, background=c)
    en = env_scene(rtmi, np.tile(np.float32(c), (4, 8, 1)), rotate=77.0)
    sa, sb = rtmi.Stats(), rtmi.Stats()
    a = bg.render(rtmi.Opts(seed=SEED, variant=16), sa)
    b = en.render(rtmi.Opts(seed=SEED, variant=16), sb)
    assert sa.kernel_variant == 16 and sb.kernel_variant == 16 | ENV
    assert np.array_equal(a, b)
    # ... and it replaces the sky gradient as well
    en.set_background((9, 9, 9), sky_gradient=True, defocus_blur=False)
    assert np.array_equal(en.render(rtmi.Opts(seed=SEED)), a)


@pytest.mark.parametrize("nee", [False, True])
def test_layouts_give_the_same_bytes(rtmi, nee):
    sc = env_scene(rtmi, sky_map(), nee=nee)
    assert len(sc.lights()) == 2
    imgs = {}
    for v in (16, 36, 44):
        st = rtmi.Stats()
        imgs[v] = sc.render(rtmi.Opts(seed=SEED, variant=v), st)
        assert st.kernel_variant == v | ENV | (256 if nee else 0)
    assert np.array_equal(imgs[16], imgs[36]) and np.array_equal(imgs[16], imgs[44])
    st = rtmi.Stats()
    assert np.array_equal(sc.render(rtmi.Opts(seed=SEED), st), imgs[16]) and st.kernel_variant & ENV
    assert imgs[16].max() > 0 and np.isfinite(imgs[16]).all()
    # a sphere-only scene with a map is packed wide and takes the same kernels
    rt = rtmi.Scene.rtiow(7, 64, 36, 4, 10)
    rt.set_environment(sky_map())
    rt.set_light_sampling(nee)
    a = rt.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & ENV and bool(st.kernel_variant & 256) == nee
    assert np.array_equal(a, rt.render(rtmi.Opts(seed=SEED, variant=16))) and np.array_equal(a, rt.render(rtmi.Opts(seed=SEED, variant=44)))


@pytest.mark.parametrize("nee", [False, True])
def test_splits_chunks_shards_tiles_and_adaptive(rtmi, nee):
    sc = env_scene(rtmi, sky_map(), spp=48, nee=nee)
    ref = sc.render(rtmi.Opts(seed=SEED))
    assert np.array_equal(sc.render(rtmi.Opts(seed=SEED)), ref)
    assert not np.array_equal(sc.render(rtmi.Opts(seed=SEED + 1)), ref)
    acc, _ = sc.accumulate(None, rtmi.Opts(seed=SEED, sample_first=0, sample_count=20))
    acc, img = sc.accumulate(acc, rtmi.Opts(seed=SEED, sample_first=20, sample_count=28))
    assert np.array_equal(img, ref)
    assert np.array_equal(sc.render(rtmi.Opts(seed=SEED, spp_chunk=8)), ref) and np.array_equal(sc.render(rtmi.Opts(seed=SEED, spp_chunk=48)), ref)
    for stride in (2, 3):
        full = np.zeros_like(ref)
        for r in range(stride):
            o = rtmi.Opts(seed=SEED, tile_first=r, tile_stride=stride, tile_rows=4)
            full[sc.shard_global_rows(o)] = sc.render(o)
        assert np.array_equal(full, ref), stride
    st = rtmi.Stats()
    assert np.array_equal(sc.render_tiles(None, rtmi.Opts(seed=SEED), st, n=1), ref)
    # adaptive sampling: every tile holds the plain render at its own count
    img, spp, ast = sc.render_adaptive(0.05, min_spp=4, max_spp=48, opts=rtmi.Opts(seed=SEED))
    counts = np.unique(spp)
    for n in counts:
        plain = sc.render(rtmi.Opts(seed=SEED, sample_count=int(n)))
        assert np.array_equal(img[spp == n], plain[spp == n]), n
    img, spp, ast = sc.render_adaptive(0.0, min_spp=4, max_spp=16, opts=rtmi.Opts(seed=SEED))
    assert (spp == 16).all() and np.array_equal(img, sc.render(rtmi.Opts(seed=SEED, sample_count=16)))


def emissive_clone(rtmi, sc):
    """every material a diffuse_light on the same texture (a metal: its albedo, a dielectric: white); the environment stays"""
    j = json.loads(sc.to_json())
    texs, mats = j["texture"]["data"], []
    for m in j["material"]["data"]:
        if m["type"] in ("lambertian", "diffuse_light"):
            mats.append({"type": "diffuse_light", "texture": m["texture"]})
        else:
            texs.append({"type": "solid_color", "color": m["albedo"] if m["type"] == "metal" else [1, 1, 1]})
            mats.append({"type": "diffuse_light", "texture": len(texs) - 1})
    j["material"]["data"] = mats
    for key in ("russian_roulette", "light_sampling"):
        j.pop(key, None)
    assert "environment" in j
    return rtmi.Scene.parse(json.dumps(j))


def test_feature_passes(rtmi):
    sc = env_scene(rtmi, sky_map(), spp=3, nee=True, scale=1.5)
    sc.set_russian_roulette(0.8)
    clone = emissive_clone(rtmi, sc)
    st = rtmi.Stats()
    want = clone.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & ENV and not st.kernel_variant & 256
    for v in (0, 16, 36, 44):
        got = sc.render_feature(0, rtmi.Opts(seed=SEED, variant=v), st)
        assert np.array_equal(got, want), v
        assert st.kernel_variant & ENV and st.kernel_variant & 512
    # a miss: environment radiance in the albedo pass, zeros in normal and depth
    depth = sc.render_feature(2, rtmi.Opts(seed=SEED, sample_count=1))
    normal = sc.render_feature(1, rtmi.Opts(seed=SEED, sample_count=1))
    albedo = sc.render_feature(0, rtmi.Opts(seed=SEED, sample_count=1))
    miss = depth[..., 1] == 0
    assert miss.any() and not miss.all()
    assert not normal[miss].any() and not depth[miss].any()
    texels = {tuple(np.float32(1.5) * t) for t in sc.environment[0].reshape(-1, 3)}
    assert all(tuple(p) in texels for p in albedo[miss])
    with pytest.raises(rtmi.RtmiError) as e:
        sc.render_feature(0, rtmi.Opts(seed=SEED, variant=24))
    assert e.value.status == 1


# ---- device against host -----------------------------------------------------------------------------------------------------
def test_device_lookup_is_the_host_evaluation(rtmi):
    rows, cols, W, H = 8, 16, 64, 36
    rng = np.random.default_rng(8)
    env = (rng.integers(26, 800, (rows, cols, 3)) / 256.0).astype(np.float32)  # (multiples of 2^-8: exact in the 2^-24 fixed-point sums)
    assert len({tuple(t) for t in env.reshape(-1, 3)}) == rows * cols
    sc = rtmi.Scene.new(W, H, 1, 4)
    sc.set_background((0, 0, 0), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 1.0, 0.0), (0.3, 1.4, -1.0), (0, 1, 0), 100.0)
    sc.sphere((0.0, 1.0, 50.0), 0.5, sc.lambertian((0.5, 0.5, 0.5)))  # behind the camera: no camera ray hits it
    sc.set_environment(env, 1.0, 0.0)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & ENV
    cam = sc.get_camera()
    org, ll = np.array(cam.origin, np.float64), np.array(cam.lower_left, np.float64)
    hor, ver = np.array(cam.horizontal, np.float64), np.array(cam.vertical, np.float64)
    texels = {tuple(t) for t in env.reshape(-1, 3)}
    excepted = 0
    for y in range(H):
        for x in range(W):
            w = rtmi.sample_stream(SEED, y * W + x, 0, 2)
            u = (x + (w[0] >> 8) * 2.0 ** -24) / (W - 1)
            v = (y + (w[1] >> 8) * 2.0 ** -24) / (H - 1)
            d = ll + u * hor + v * ver - org
            d /= np.linalg.norm(d)
            assert tuple(img[y, x]) in texels, (x, y)
            theta, phi = np.arccos(d[1]), np.arctan2(-d[2], d[0]) + np.pi
            ft, fp = theta / np.pi * rows, phi / (2 * np.pi) * cols
            near = min(abs(ft - round(ft)) * np.pi / rows, abs(fp - round(fp)) * 2 * np.pi / cols * np.sin(theta))
            if near < 1e-4:
                excepted += 1
                continue
            rgb, _ = sc.environment_eval(d)
            assert np.array_equal(img[y, x], rgb), (x, y, d)
    assert excepted <= 0.01 * W * H, excepted
    assert len({tuple(p) for p in img.reshape(-1, 3)}) >= 6  # (the frame spans several texels)


# ---- unbiasedness against today's estimator ----------------------------------------------------------------------------------
def seeds_of(rtmi, sc, n=8):
    return np.stack([sc.render(rtmi.Opts(seed=1000 + s)).astype(np.float64).mean(axis=2) / sc.spp for s in range(n)])


def test_unbiased_against_the_textured_sphere(rtmi):
    rows, cols = 8, 16
    rng = np.random.default_rng(4)
    env8 = rng.integers(20, 256, (rows, cols, 3), dtype=np.uint8)
    env8[rows // 2:] //= 3
    env = env8.astype(np.float32) / np.float32(255.0)
    # today's substitute: the map on a giant emissive sphere.  Its image texture is read as texel[int(u x rows)][int(v x cols)] with
    # u the azimuth and v = acos(-y) / pi counted from the nadir: the map transposed, and flipped along its rows
    ref = env_scene(rtmi, None, spp=256, emitter=False)
    tex = np.ascontiguousarray(env8.transpose(1, 0, 2)[:, ::-1])
    ref.sphere((0.0, 0.0, 0.0), 1.0e4, ref.diffuse_light(ref.image_texture(tex)))
    assert len(ref.lights()) == 0
    a = seeds_of(rtmi, ref)
    for nee in (False, True):
        sc = env_scene(rtmi, env, spp=256, nee=nee, rotate=0.0, emitter=False)
        st = rtmi.Stats()
        sc.render(rtmi.Opts(seed=1, sample_count=1), st)
        assert st.kernel_variant & ENV and bool(st.kernel_variant & 256) == nee
        compare(a, seeds_of(rtmi, sc), "environment %s vs textured sphere" % ("light sampling" if nee else "plain"), c_max=1.0)


# ---- known answer ------------------------------------------------------------------------------------------------------------
def test_known_answer_under_a_small_bright_patch(rtmi):
    rows, cols = PATCH_ROWS, PATCH_COLS
    # the patch: < 1 % of the upper hemisphere
    band = (2 * np.pi / cols) * (np.cos(np.pi * np.arange(rows) / rows) - np.cos(np.pi * (np.arange(rows) + 1) / rows))
    assert 3 * band[4:6].sum() < 0.01 * 2 * np.pi
    expected = patch_expected()
    sc = patch_scene(rtmi)
    mean = lambda img: img.astype(np.float64).mean(axis=2) / sc.spp
    stats = {}
    for nee in (False, True):
        sc.set_light_sampling(nee)
        st = rtmi.Stats()
        frames = [mean(sc.render(rtmi.Opts(seed=s), st)) for s in range(8)]
        assert st.kernel_variant & ENV and bool(st.kernel_variant & 256) == nee
        fm = np.array([f.mean() for f in frames])
        se = fm.std(ddof=1) / np.sqrt(len(fm))
        rel = np.sqrt(np.mean(((frames[0] - expected) / expected) ** 2))
        print(f"patch: light sampling {nee}: frame mean {fm.mean():.5f} (expected {expected:.5f}, se {se:.2g}), RMS relative error per pixel {rel:.4f}")
        stats[nee] = (fm.mean(), se, rel)
    for nee in (False, True):
        m, se, rel = stats[nee]
        assert abs(m - expected) < 3 * se + 1e-4, (nee, m, expected, se)
    assert stats[True][2] <= 0.05 and stats[True][2] <= 0.25 * stats[False][2], (stats[True][2], stats[False][2])


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(rtmi):
    sc = env_scene(rtmi, sky_map(), spp=2)
    variants = [2, 6, 52] + ([1, 40, 17, 24, 32, 64, 128] if rtmi.has_ablations() else [])
    for nee in (False, True):
        sc.set_light_sampling(nee)
        for v in variants:
            with pytest.raises(rtmi.RtmiError) as e:
                sc.render(rtmi.Opts(variant=v))
            assert e.value.status == 1 and "environment" in str(e.value), v
        if rtmi.has_ablations():
            with pytest.raises(rtmi.RtmiError) as e:
                sc.count()
            assert e.value.status == 1 and "environment" in str(e.value)
    room = dense_room(rtmi, w=64, h=36, spp=1)
    room.set_nested_grid(True)
    assert room.nested_info().cells > 0
    room.set_environment(sky_map())
    with pytest.raises(rtmi.RtmiError) as e:
        room.render(rtmi.Opts(seed=1))
    assert e.value.status == 1 and "nested" in str(e.value)
    room.set_nested_grid(False)
    st = rtmi.Stats()
    room.render(rtmi.Opts(seed=1), st)
    assert st.kernel_variant & ENV
