"""Adaptive sampling (rt_render_hip_adaptive) on the GPU.  A tile that stops after n samples holds exactly the sums of
samples [0, n), so every check here is bit-exact: the limits are plain renders, every tile equals the plain render at its
own n, and the tile decisions are those of a numpy restatement of the metric (include/rtmi.h) replayed on
rt_render_hip_accumulate sums of the same sample ranges."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
SCENES = os.path.join(PKG, "scenes")
SEED = 21

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtmi():
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    mod = load_package()
    if mod.device_count() < 1:
        pytest.skip("no HIP device")
    return mod


def tri_texture(rtmi, w=64, h=36, spp=8):
    sc = rtmi.Scene.new(w, h, spp, 6)
    sc.set_background((0.3, 0.4, 0.6), sky_gradient=True, defocus_blur=False)
    sc.camera((0, 1, 4), (0, 0.5, 0), (0, 1, 0), 50.0)
    sc.xz_rect(-5, 5, -5, 5, 0.0, sc.lambertian((0.5, 0.5, 0.5)))
    sc.triangle((-1, 1.5, -1), (1, 1.5, -1), (0, 1.5, 1), sc.diffuse_light((4.0, 4.0, 4.0)))
    tex = np.arange(4 * 4 * 3, dtype=np.uint8).reshape(4, 4, 3) * 5
    sc.xy_rect(-1, 1, 0, 1, -2, sc.lambertian(sc.image_texture(tex)))
    return sc


def mixed(rtmi, nee=False, w=64, h=36):
    sc = rtmi.Scene.load(os.path.join(SCENES, "mixed_emissive.json"))
    sc.override(w, h, 16)
    if nee:
        sc.set_light_sampling(True)
    return sc


def dna(rtmi):
    sc = rtmi.Scene.dna(0.0)
    sc.override(width=96, height=54, spp=16, max_depth=50)
    return sc


# (name, scene factory, variant, kernel_variant that a plain render reports)
CASES = [
    ("rtiow-sheet", lambda r: r.Scene.rtiow(7, 64, 36, 16, 20), 2),
    ("rtiow-3d-grid", lambda r: r.Scene.rtiow(7, 64, 36, 16, 20), 6),
    ("mixed-scan", lambda r: mixed(r), 16),
    ("dna-wide-lds", dna, 36),
    ("mixed-wide-global", lambda r: mixed(r), 44),
    ("triangle-texture", tri_texture, 0),
    ("mixed-light-sampling", lambda r: mixed(r, nee=True), 0),
    ("partial-tiles-100x60", lambda r: r.Scene.rtiow(7, 100, 60, 16, 20), 0),
]


def plain(rtmi, sc, n, variant=0, seed=SEED):
    return sc.render(rtmi.Opts(seed=seed, variant=variant, sample_count=n))


@pytest.mark.parametrize("name, make, variant", CASES, ids=[c[0] for c in CASES])
def test_limits_are_plain_renders(rtmi, name, make, variant):
    sc = make(rtmi)
    opts = rtmi.Opts(seed=SEED, variant=variant)
    img, spp, st = sc.render_adaptive(0.0, min_spp=4, max_spp=16, opts=opts)
    assert (spp == 16).all()
    assert np.array_equal(img, plain(rtmi, sc, 16, variant)), name
    assert list(st.spp_after[:st.passes]) == [4, 8, 16]
    img, spp, st = sc.render_adaptive(1e30, min_spp=4, max_spp=16, opts=opts)
    assert (spp == 4).all() and st.passes == 1
    assert np.array_equal(img, plain(rtmi, sc, 4, variant)), name


def _tiles_below(spp, max_spp):
    t = spp[::8, ::8]
    return float((t < max_spp).mean()), len(np.unique(t))


def _pick_threshold(rtmi, sc, min_spp, max_spp, opts):
    """The first threshold of a falling ladder that retires >= 20 % of the tiles early with >= 2 distinct counts."""
    for thr in (0.5, 0.3, 0.2, 0.12, 0.08, 0.05, 0.03, 0.02, 0.01, 0.005):
        img, spp, st = sc.render_adaptive(thr, min_spp=min_spp, max_spp=max_spp, opts=opts)
        below, distinct = _tiles_below(spp, max_spp)
        if below >= 0.2 and distinct >= 2 and (spp == max_spp).any():
            return thr, img, spp, st
    pytest.fail("no threshold of the ladder retires some tiles early and keeps others to max_spp")


@pytest.mark.parametrize("which", ["rtiow", "mixed-nee", "partial"])
def test_every_tile_is_the_plain_render_at_its_count(rtmi, which):
    sc = {"rtiow": lambda: rtmi.Scene.rtiow(7, 96, 54, 64, 20), "mixed-nee": lambda: mixed(rtmi, nee=True, w=96, h=54),
          "partial": lambda: rtmi.Scene.rtiow(7, 100, 60, 64, 20)}[which]()
    opts = rtmi.Opts(seed=SEED)
    thr, img, spp, st = _pick_threshold(rtmi, sc, 4, 64, opts)
    counts = np.unique(spp)
    assert len(counts) >= 2
    for n in counts:
        ref = plain(rtmi, sc, int(n))
        mask = spp == n
        assert np.array_equal(img[mask], ref[mask]), (which, thr, n)
    # the map is constant over each 8x8 tile
    for ty in range(0, sc.height, 8):
        for tx in range(0, sc.width, 8):
            t = spp[ty:ty + 8, tx:tx + 8]
            assert (t == t.flat[0]).all()


def replay(rtmi, sc, threshold, min_spp, max_spp, seed=SEED):
    """include/rtmi.h's schedule and metric, restated in numpy over rt_render_hip_accumulate sums."""
    W, H = sc.width, sc.height
    tx, ty = (W + 7) // 8, (H + 7) // 8
    T = float(np.float32(threshold))
    s = 1.0 / 16777216.0
    A = B = None
    nA = nB = prev = k = 0
    active = np.ones((ty, tx), bool)
    n_tile = np.zeros((ty, tx), np.int32)
    spp_after, n_active = [], []
    while active.any():
        n = min_spp if k == 0 else min(2 * prev, max_spp)
        d = n - prev
        h = d // 2
        if h:
            A, _ = sc.accumulate(A, rtmi.Opts(seed=seed, sample_first=prev, sample_count=h), want_image=False)
        B, _ = sc.accumulate(B, rtmi.Opts(seed=seed, sample_first=prev + h, sample_count=d - h), want_image=False)
        nA, nB = nA + h, nB + d - h
        a = (A.astype(np.float64) * s) / float(nA)
        b = (B.astype(np.float64) * s) / float(nB)
        m = ((A + B).astype(np.float64) * s) / float(n)
        dd = (np.abs(a[..., 0] - b[..., 0]) + np.abs(a[..., 1] - b[..., 1])) + np.abs(a[..., 2] - b[..., 2])
        M = np.maximum((m[..., 0] + m[..., 1]) + m[..., 2], 1e-4)
        conv = (dd * dd <= ((4.0 * T) * T) * M) if T > 0 else np.zeros((H, W), bool)
        pad = np.ones((ty * 8, tx * 8), bool)
        pad[:H, :W] = conv
        tile_conv = pad.reshape(ty, 8, tx, 8).all(axis=(1, 3))
        retire = active & (tile_conv | (n == max_spp))
        spp_after.append(n)
        n_active.append(int(active.sum()))
        n_tile[retire] = n
        active &= ~retire
        prev, k = n, k + 1
    return np.repeat(np.repeat(n_tile, 8, 0), 8, 1)[:H, :W], spp_after, n_active


@pytest.mark.parametrize("which", ["rtiow", "mixed-nee", "partial"])
def test_decisions_are_the_metric(rtmi, which):
    sc = {"rtiow": lambda: rtmi.Scene.rtiow(7, 96, 54, 64, 20), "mixed-nee": lambda: mixed(rtmi, nee=True, w=96, h=54),
          "partial": lambda: rtmi.Scene.rtiow(7, 100, 60, 64, 20)}[which]()
    thr, img, spp, st = _pick_threshold(rtmi, sc, 4, 64, rtmi.Opts(seed=SEED))
    for t in (thr, thr * 0.5, thr * 2.0):
        img, spp, st = sc.render_adaptive(t, min_spp=4, max_spp=64, opts=rtmi.Opts(seed=SEED))
        ref, spp_after, n_active = replay(rtmi, sc, t, 4, 64)
        assert np.array_equal(spp, ref), (which, t)
        assert list(st.spp_after[:st.passes]) == spp_after and list(st.active[:st.passes]) == n_active


def test_order_free(rtmi):
    sc = mixed(rtmi, nee=True, w=96, h=54)
    runs = [sc.render_adaptive(0.05, min_spp=4, max_spp=64, opts=rtmi.Opts(seed=SEED, spp_chunk=c)) for c in (0, 0, 4, 16, 64)]
    for img, spp, st in runs[1:]:
        assert np.array_equal(img, runs[0][0]) and np.array_equal(spp, runs[0][1])
    sc2 = rtmi.Scene.rtiow(7, 96, 54, 64, 20)
    a = sc2.render_adaptive(0.05, min_spp=2, max_spp=48, opts=rtmi.Opts(seed=SEED))
    b = sc2.render_adaptive(0.05, min_spp=2, max_spp=48, opts=rtmi.Opts(seed=SEED, spp_chunk=8))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_stats(rtmi):
    sc = rtmi.Scene.rtiow(7, 100, 60, 64, 20)
    for thr, lo, hi in ((0.05, 4, 64), (0.02, 2, 48), (0.0, 3, 20)):
        img, spp, st = sc.render_adaptive(thr, min_spp=lo, max_spp=hi, opts=rtmi.Opts(seed=SEED))
        assert st.samples == int(spp.astype(np.int64).sum())
        assert st.tiles == 13 * 8
        act = list(st.active[:st.passes])
        assert act[0] == st.tiles and all(x >= y for x, y in zip(act, act[1:]))
        n = list(st.spp_after[:st.passes])
        assert n[0] == lo and all(b == min(2 * a, hi) for a, b in zip(n, n[1:]))
        assert n[-1] == spp.max() and st.kernel_ms > 0
    # max_spp 0: the scene's spp
    img, spp, st = sc.render_adaptive(0.0, min_spp=16, max_spp=0, opts=rtmi.Opts(seed=SEED))
    assert (spp == 64).all() and np.array_equal(img, plain(rtmi, sc, 64))


_PRODUCT = textwrap.dedent("""
    import os, sys
    import numpy as np
    sys.path.insert(0, %r)
    from __graft_entry__ import load_package
    rtmi = load_package()
    assert not rtmi.has_ablations()
    out = {}
    sc = rtmi.Scene.load(os.path.join(%r, "mixed_emissive.json")); sc.override(96, 54, 16); sc.set_light_sampling(True)
    out["nee_img"], out["nee_spp"], _ = sc.render_adaptive(0.05, min_spp=4, max_spp=32, opts=rtmi.Opts(seed=%d))
    sc = rtmi.Scene.rtiow(7, 100, 60, 16, 20)
    out["rt_img"], out["rt_spp"], _ = sc.render_adaptive(0.05, min_spp=4, max_spp=32, opts=rtmi.Opts(seed=%d))
    np.savez(sys.argv[1], **out)
""") % (ROOT, SCENES, SEED, SEED)


def test_product_build_gives_the_same_bytes(rtmi, tmp_path):
    out = str(tmp_path / "prod.npz")
    env = dict(os.environ, RTMI_LIB=os.path.join(PKG, "librtmi_product.so"))
    p = subprocess.run([sys.executable, "-c", _PRODUCT, out], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    got = np.load(out)
    sc = mixed(rtmi, nee=True, w=96, h=54)
    img, spp, _ = sc.render_adaptive(0.05, min_spp=4, max_spp=32, opts=rtmi.Opts(seed=SEED))
    assert np.array_equal(got["nee_img"], img) and np.array_equal(got["nee_spp"], spp)
    sc = rtmi.Scene.rtiow(7, 100, 60, 16, 20)
    img, spp, _ = sc.render_adaptive(0.05, min_spp=4, max_spp=32, opts=rtmi.Opts(seed=SEED))
    assert np.array_equal(got["rt_img"], img) and np.array_equal(got["rt_spp"], spp)


def test_cli(tmp_path):
    rtmi_bin = os.path.join(PKG, "rtmi")
    scene = os.path.join(SCENES, "mixed_emissive.json")
    p = subprocess.run([rtmi_bin, "-f", scene, "-w", "96", "-h", "54", "--adaptive", "0.05", "--min-spp", "4", "--max-spp", "64",
                        "-o", str(tmp_path / "a.ppm"), "--no-png"], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "adaptive:" in p.stderr and "passes" in p.stderr and "saved" in p.stderr
    head = open(tmp_path / "a.ppm", "rb").read(16).split()
    assert head[0] == b"P3" and head[1:3] == [b"96", b"54"]
    p = subprocess.run([rtmi_bin, "-f", scene, "--adaptive", "0.05", "--gpus", "2", "-o", str(tmp_path / "b.ppm")],
                       capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert p.returncode != 0 and not (tmp_path / "b.ppm").exists()
