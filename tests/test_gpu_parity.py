"""-m gpu: the HIP render path, called through the C ABI, against the CPU checker
(oracle/rt_oracle.c) on the same seeded inputs.  The bar is BIT-EXACT fp32 framebuffers
(stricter than north_star's 1e-3 per-pixel tolerance, which is also asserted explicitly),
including the exact fixed-point pixel accumulation both sides define,
plus the reference-produced golden vectors and size-independent properties at the
BASELINE.json frame size."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 2023
TOL = 1e-3  # north_star: per-pixel max-abs error of the mean radiance


def _scene(rtmi, scenes_dir, golden_dir, name):
    if name == "rtiow":
        return rtmi.Scene.load(os.path.join(golden_dir, "rtiow_seed7.json"))
    if name == "dna":  # dna.py frame 30: 60 emissive spheres + 30 emissive rotated cylinders
        return rtmi.Scene.dna(30.0)
    if name in ("three_sphere", "mixed_emissive"):
        return rtmi.Scene.load(os.path.join(scenes_dir, name + ".json"))
    return rtmi.Scene.load(os.path.join(golden_dir, "scenes", name + ".json"))


def _assert_same(rtmi, rtcheck, sc, seed=SEED, **kw):
    img = sc.render(rtmi.Opts(seed=seed, **kw))
    ref, _ = rtcheck.oracle_render(sc, seed=seed, spp_chunk=kw.get("spp_chunk", 0),
                                   sample_first=kw.get("sample_first", 0),
                                   sample_count=kw.get("sample_count", None) or None)
    n = kw.get("sample_count", 0) or sc.spp
    assert np.abs(img - ref).max() / n < TOL
    assert np.array_equal(img, ref), f"{(img != ref).any(axis=2).sum()} pixels differ from the CPU checker"
    return img


def test_device_present(rtmi):
    assert rtmi.device_count() >= 1


@pytest.mark.parametrize("name,w,h,spp", [
    ("three_sphere", 96, 54, 8),      # config 1 scene
    ("three_sphere", 33, 17, 5),      # ragged: not a multiple of the 8x8 wave tile / 32-wide strip
    ("three_sphere", 2, 2, 3),        # smallest legal image
    ("three_sphere", 130, 9, 1),
    ("rtiow", 80, 45, 4),             # config 3/5 scene (485 spheres, checker ground, blur)
    ("mixed_emissive", 96, 54, 8),    # rects + cylinders + emitters + checker + constant background
    ("sample_scene", 64, 36, 8),      # the reference's gpu-version/sample_scene.json
    ("blue", 64, 36, 6),              # gpu-version/blue.json: rects, emissive cylinders, metal, glass
    ("blue2", 48, 27, 4),
    ("basic_scene", 40, 24, 2),       # ships with an EMPTY object list: pure background
    ("dna", 80, 45, 4),               # config 2b: the DNA animation frame (cylinder boxes are culled)
])
def test_bit_exact_vs_checker(rtmi, rtcheck, scenes_dir, golden_dir, name, w, h, spp):
    sc = _scene(rtmi, scenes_dir, golden_dir, name)
    sc.override(width=w, height=h, spp=spp)
    _assert_same(rtmi, rtcheck, sc)


@pytest.mark.parametrize("depth", [1, 2, 7])
def test_depth_limits(rtmi, rtcheck, scenes_dir, golden_dir, depth):
    sc = _scene(rtmi, scenes_dir, golden_dir, "mixed_emissive")
    sc.override(width=48, height=27, spp=4, max_depth=depth)
    _assert_same(rtmi, rtcheck, sc)


def test_depth_zero_is_black(rtmi):
    sc = rtmi.Scene.new(16, 16, 4, 0)
    sc.camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0)
    sc.sphere((0, 0, 0), 1, sc.lambertian((1, 1, 1)))
    assert not sc.render().any()


def test_blur_and_background_switches(rtmi, rtcheck, scenes_dir, golden_dir):
    d = json.loads(_scene(rtmi, scenes_dir, golden_dir, "three_sphere").to_json())
    d["width"], d["height"], d["samples_per_pixel"] = 40, 24, 4
    d["camera"]["aperture"] = 0.3
    imgs = []
    for sky in (True, False):
        for blur in (True, False):
            d["sky_gradient"], d["defocus_blur"] = sky, blur
            sc = rtmi.Scene.parse(json.dumps(d))
            imgs.append(_assert_same(rtmi, rtcheck, sc))
    assert not np.array_equal(imgs[0], imgs[1]) and not np.array_equal(imgs[0], imgs[2])


def test_seed_changes_image_and_is_deterministic(rtmi, scenes_dir, golden_dir):
    sc = _scene(rtmi, scenes_dir, golden_dir, "three_sphere")
    sc.override(width=48, height=27, spp=4)
    a, b, c = sc.render(rtmi.Opts(seed=1)), sc.render(rtmi.Opts(seed=1)), sc.render(rtmi.Opts(seed=2))
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    hi = sc.render(rtmi.Opts(seed=1 + (1 << 32)))  # the high key word matters too
    assert not np.array_equal(a, hi)


@pytest.mark.parametrize("entry", ["render", "accumulate", "render_adaptive"])
def test_kept_buffers_regrow(rtmi, scenes_dir, golden_dir, entry):
    """The device buffers a scene object keeps between calls (framebuffer, accumulators, adaptive planes, sample-count map):
    4 tiles, then 24, then 4 again on ONE object, each result bit-identical to the same call on a fresh clone, whose device
    residency is its own.  A stale or mis-sized kept buffer would show."""
    def call(sc):
        if entry == "render":
            return (sc.render(rtmi.Opts(seed=SEED)),)
        if entry == "accumulate":  # two calls of one sample each, continuing one accumulator
            acc, _ = sc.accumulate(None, rtmi.Opts(seed=SEED, sample_first=0, sample_count=1))
            acc, img = sc.accumulate(acc, rtmi.Opts(seed=SEED, sample_first=1, sample_count=1))
            return acc, img
        img, spp_map, _ = sc.render_adaptive(0.0, min_spp=2, max_spp=4, opts=rtmi.Opts(seed=SEED))
        return img, spp_map

    kept = _scene(rtmi, scenes_dir, golden_dir, "three_sphere")
    for w, h in ((16, 16), (48, 32), (16, 16)):
        kept.override(width=w, height=h, spp=2, max_depth=4)
        got, want = call(kept), call(kept.clone())
        for a, b in zip(got, want):
            assert a.shape == b.shape and a.any() and np.array_equal(a, b), (entry, w, h)


@pytest.mark.parametrize("world,tile_rows", [(2, 8), (3, 8), (8, 8), (2, 4), (5, 16)])
def test_partition_invariance(rtmi, scenes_dir, golden_dir, world, tile_rows):
    """G4: the assembled row-tile shards are bit-identical to the unsharded frame."""
    sc = _scene(rtmi, scenes_dir, golden_dir, "mixed_emissive")
    sc.override(width=72, height=45, spp=4)
    full = sc.render(rtmi.Opts(seed=SEED))
    out = np.zeros_like(full)
    for rotate in (0, 1, 2):  # plain interleave, rotated, there and back (rt_opts.tile_rotate)
        out[:] = 0
        for r in range(world):
            o = rtmi.Opts(seed=SEED, tile_rows=tile_rows, tile_first=r, tile_stride=world, tile_rotate=rotate)
            local = sc.render(o)
            assert local.shape[0] == sc.shard_rows(o)
            sc.scatter_rows(o, local, out)
        assert np.array_equal(out, full)


def test_sample_chunks_and_ranges(rtmi, rtcheck, scenes_dir, golden_dir):
    """The pixel sum is exact (64-bit fixed point), so how the samples are cut into
    work-items (spp_chunk) cannot change a bit; sample ranges select Philox streams."""
    sc = _scene(rtmi, scenes_dir, golden_dir, "three_sphere")
    sc.override(width=40, height=24, spp=13)
    whole = _assert_same(rtmi, rtcheck, sc)
    for chunk in (1, 4, 13, 64):
        assert np.array_equal(whole, sc.render(rtmi.Opts(seed=SEED, spp_chunk=chunk)))
    # progressive accumulation: samples [5, 13) alone
    _assert_same(rtmi, rtcheck, sc, sample_first=5, sample_count=8)
    # the frame is the sum of its one-sample frames (up to the single final rounding to fp32)
    per = [sc.render(rtmi.Opts(seed=SEED, sample_first=k, sample_count=1)).astype(np.float64) for k in range(13)]
    acc = np.sum(per, axis=0)
    assert np.abs(acc - whole).max() <= 13 * 2.0 ** -24 * max(1.0, acc.max())


COMPACT_VARIANTS = (1, 2, 6, 40)   # the compact grid tables: sphere-only scenes that fit LDS
WIDE_VARIANTS = (36, 44)           # the wide grid tables: every other scene


@pytest.mark.parametrize("variant", [0, 2, 6, 36, 44, 1, 40, 16, 17, 24, 32, 64, 128])
def test_kernel_variants_are_bit_identical(rtmi, rtcheck, scenes_dir, golden_dir, variant):
    """The product kernels (0 -> 2 / 6 / 36 / 44: uniform-grid walk over compact or wide tables, in LDS or global memory) and
    the measurement variants of the default build (1 strict one-lane-per-pixel ownership, 40 compact tables in global
    memory, 16 / 17 / 24 the reference's linear scan, 32 wave votes, 64 box hierarchy, 128 range tables): same bits as the
    checker in every combination; a variant whose table format the scene does not have is refused."""
    for name, w, h, spp, sphere_only in (("rtiow", 72, 40, 6, True), ("mixed_emissive", 50, 30, 5, False)):
        sc = _scene(rtmi, scenes_dir, golden_dir, name)
        sc.override(width=w, height=h, spp=spp)
        if variant in (WIDE_VARIANTS if sphere_only else COMPACT_VARIANTS):
            with pytest.raises(rtmi.RtmiError) as e:
                sc.render(rtmi.Opts(variant=variant))
            assert e.value.status == 6
            continue
        _assert_same(rtmi, rtcheck, sc, variant=variant)
        _assert_same(rtmi, rtcheck, sc, variant=variant, spp_chunk=2)
        st = rtmi.Stats()
        sc.render(rtmi.Opts(seed=SEED, variant=variant), st)
        assert st.kernel_variant == (variant if variant else (2 if sphere_only else 16))  # (12 primitives: nothing to list in a grid)
    with pytest.raises(rtmi.RtmiError, match="variant"):
        sc.render(rtmi.Opts(variant=9))
    for gone in (4, 8, 19, 104, 136):  # measurement variants of earlier rounds (DESIGN.md keeps their numbers)
        with pytest.raises(rtmi.RtmiError, match="variant"):
            sc.render(rtmi.Opts(variant=gone))


def test_exact_event_counters(rtmi, rtcheck, scenes_dir, golden_dir):
    """The diagnostic kernel's counters (roofline flop accounting) equal the checker's."""
    for name, w, h, spp in (("rtiow", 64, 36, 4), ("mixed_emissive", 64, 36, 4)):
        sc = _scene(rtmi, scenes_dir, golden_dir, name)
        sc.override(width=w, height=h, spp=spp)
        st, img = sc.count(rtmi.Opts(seed=SEED), want_image=True)
        _, want = rtcheck.oracle_render(sc, seed=SEED, want_counts=True)
        got = st.as_dict()
        for k, v in want.items():
            assert got[k] == v, (name, k)
        assert np.array_equal(img, sc.render(rtmi.Opts(seed=SEED)))
        assert got["samples"] == w * h * spp and got["hits"] + got["misses"] == got["queries"]


def test_golden_reference_vectors(rtmi, scenes_dir, golden_dir):
    """HIP path vs vectors produced by the compiled reference (cmake-cpu-version sources):
    G2 per-sample >= 97 % within 1e-4, G3 image mean |delta| and unbiasedness."""
    for which, name in (("three_sphere", "three_sphere"), ("rtiow", "rtiow")):
        z = np.load(os.path.join(golden_dir, f"ref_{which}.npz"))
        sc = _scene(rtmi, scenes_dir, golden_dir, name)
        w, h, spp = int(z["width"]), int(z["height"]), int(z["spp"])
        sc.override(width=w, height=h, spp=spp)
        seed = int(z["seed"])
        img = sc.render(rtmi.Opts(seed=seed)).astype(np.float64) / spp
        ref = z["image_sum"] / spp
        d = np.abs(img - ref)
        assert d.mean() <= 2e-3 * np.sqrt(100.0 / spp) and np.median(d) < 1e-6
        assert abs(img.mean() - ref.mean()) <= max(3 * ref.std() / np.sqrt(ref.size * spp), 2e-4)
        frames = [sc.render(rtmi.Opts(seed=seed, sample_first=k, sample_count=1)) for k in range(spp)]
        ids = z["sample_ids"]
        got = np.array([frames[s][y, x] for x, y, s in ids], dtype=np.float64)
        err = np.abs(got - z["sample_rgb"]).max(axis=1)
        assert (err <= 1e-4).mean() >= 0.97, which
        assert np.median(err) < 2e-6


def test_kat_scenes_on_device(rtmi, rtcheck):
    """The analytic scenes of test_primitives.py rendered by the kernel (exact expectations)."""
    import test_primitives as tp
    sc = tp._probe_scene(rtmi, bg=(0.25, 0.5, 0.75))
    sc.xy_rect(-1, 1, -1, 1, 0.0, sc.diffuse_light((2.0, 3.0, 4.0)))
    img = _assert_same(rtmi, rtcheck, sc)
    assert np.all(img[4, 4] == np.float32([8, 12, 16]))  # 4 spp x emission, furnace-exact
    for order in (0, 1):  # tie rule across primitive TYPES (grouped on the device, list order on the CPU)
        sc = tp._probe_scene(rtmi, bg=(0, 0, 0), vfov=30.0)
        a, b = sc.diffuse_light((1, 0, 0)), sc.diffuse_light((0, 1, 0))
        # a sphere of radius 1 at z=-1 touches the plane z=0 at the origin only; use a
        # cylinder cap-less tube and a rect that coincide on a line instead: rect vs rect
        # of different types cannot coincide, so test rect/sphere tangency + rect/rect
        if order == 0:
            sc.xy_rect(-1, 1, -1, 1, 0.0, a)
            sc.sphere((0, 0, -1), 1.0, b)
            sc.xy_rect(-2, 2, -2, 2, 0.0, b)
        else:
            sc.xy_rect(-2, 2, -2, 2, 0.0, b)
            sc.sphere((0, 0, -1), 1.0, b)
            sc.xy_rect(-1, 1, -1, 1, 0.0, a)
        img = _assert_same(rtmi, rtcheck, sc)
        assert np.all(img[4, 4] == np.float32([0, 4, 0] if order == 0 else [4, 0, 0]))
    # mirror corridor: exactly max_depth queries, black
    sc = tp._probe_scene(rtmi, bg=(1, 1, 1), depth=5)
    m = sc.metal((1, 1, 1), 0.0)
    sc.xy_rect(-50, 50, -50, 50, -1.0, m)
    sc.xy_rect(-50, 50, -50, 50, 6.0, m)
    assert not _assert_same(rtmi, rtcheck, sc).any()


def test_device_pointer_and_stream_api(rtmi, scenes_dir, golden_dir):
    """rt_render_hip_device into a torch tensor on a non-default HIP stream."""
    import torch
    sc = _scene(rtmi, scenes_dir, golden_dir, "three_sphere")
    sc.override(width=64, height=40, spp=4)
    want = sc.render(rtmi.Opts(seed=SEED))
    buf = torch.zeros((40, 64, 3), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        sc.render_device(rtmi.Opts(seed=SEED), buf.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(buf.cpu().numpy(), want)
    st = rtmi.Stats()
    sc.render_device(rtmi.Opts(seed=SEED), buf.data_ptr(), 0, st)
    assert st.kernel_ms > 0 and st.launches == 2 and st.local_rows == 40


def test_error_behaviour(rtmi, scenes_dir, golden_dir):
    sc = _scene(rtmi, scenes_dir, golden_dir, "three_sphere")
    sc.override(width=16, height=16, spp=1)
    with pytest.raises(rtmi.RtmiError, match="out of range"):
        sc.render(rtmi.Opts(device=63))
    big = rtmi.Scene.new(16, 16, 1)
    big.camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0)
    m = big.lambertian((0.5, 0.5, 0.5))
    for i in range(11000):  # 11000 x 16 B > 160 KiB of LDS
        big.sphere((i * 0.001, 0, -i), 0.5, m)
    # the default kernel switches to global-memory tables; variants that keep the tables in LDS cannot
    assert big.render().shape == (16, 16, 3)
    with pytest.raises(rtmi.RtmiError) as e:
        big.render(rtmi.Opts(variant=32))
    assert e.value.status == 6 and "LDS" in str(e.value)


def test_scene_too_large_for_lds_uses_global_tables(rtmi, rtcheck):
    """20000 spheres (320 KB of sphere records alone): the default kernel reads its tables from global
    memory (three box levels, per-lane cluster lists) and still equals the CPU checker bit for bit; the
    same kernel forced on a small scene equals the LDS-resident one."""
    sc = rtmi.Scene.new(40, 24, 2, 12)
    sc.camera((0, 6, 30), (0, 0, 0), (0, 1, 0), 40.0)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    rng = np.random.default_rng(9)
    mats = [sc.lambertian(rng.uniform(0.2, 0.9, 3)) for _ in range(6)] + [sc.metal((0.8, 0.8, 0.8), 0.0), sc.dielectric(1.5)]
    sc.sphere((0, -1010, 0), 1000.0, mats[0])
    for i in range(20000):
        sc.sphere(rng.uniform(-10, 10, 3), float(rng.uniform(0.05, 0.2)), mats[i % len(mats)])
    st = sc.count(rtmi.Opts(seed=SEED))
    assert st.cull_clusters > 64 * 10 and st.cull_clusters * st.cull_cluster_size >= 20000  # many 64-cluster windows
    _assert_same(rtmi, rtcheck, sc)
    small = rtmi.Scene.rtiow(7, 96, 54, 4, 50)
    assert np.array_equal(small.render(rtmi.Opts(seed=SEED, variant=40)), small.render(rtmi.Opts(seed=SEED)))


def test_many_spheres_above_64k_lds(rtmi, rtcheck):
    """Scenes between 64 KiB and 160 KiB of LDS need the raised dynamic-LDS limit."""
    sc = rtmi.Scene.new(24, 16, 2)
    sc.camera((0, 2, 12), (0, 0, 0), (0, 1, 0), 40.0)
    rng = np.random.default_rng(5)
    mats = [sc.lambertian(rng.uniform(0.2, 0.9, 3)) for _ in range(8)] + [sc.metal((0.8, 0.8, 0.8), 0.1), sc.dielectric(1.5)]
    for i in range(5000):
        sc.sphere(rng.uniform(-6, 6, 3), float(rng.uniform(0.05, 0.2)), mats[i % len(mats)])
    st = rtmi.Stats()
    sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant == 44               # default: wide tables in global memory at this size
    _assert_same(rtmi, rtcheck, sc)
    _assert_same(rtmi, rtcheck, sc, variant=32)  # tables in LDS (105 KB: the raised dynamic-LDS limit)
    _assert_same(rtmi, rtcheck, sc, variant=64)  # per-lane lists through the box hierarchy, LDS as well


def test_full_frame_properties(rtmi, rtcheck):
    """BASELINE.json frame size (RTIOW 1920x1080), few samples: determinism, partition
    invariance over 8 shards, and bit-exactness against the checker on sampled rows."""
    sc = rtmi.Scene.rtiow(7, 1920, 1080, 2, 50)
    full = sc.render(rtmi.Opts(seed=SEED))
    assert np.array_equal(full, sc.render(rtmi.Opts(seed=SEED)))
    out = np.zeros_like(full)
    for r in range(8):
        o = rtmi.Opts(seed=SEED, tile_first=r, tile_stride=8, tile_rotate=1)
        sc.scatter_rows(o, sc.render(o), out)
    assert np.array_equal(out, full)
    osc = rtcheck.OracleScene(sc)
    for y0 in (0, 333, 700, 1078):
        ref, _ = rtcheck.oracle_render(osc, seed=SEED, rows=(y0, y0 + 2))
        assert np.array_equal(full[y0:y0 + 2], ref[y0:y0 + 2])
    mean = full.astype(np.float64).mean() / 2
    assert 0.3 < mean < 0.7 and np.isfinite(full).all() and full.min() >= 0


def _axis_parallel_scene(rtmi):
    """Rays with a direction component of EXACTLY 0, by construction: the camera sits at x = 1000 and looks down -z with
    a field of view so narrow that `horizontal.x` is far below ulp(1000) -- lower_left.x + u * horizontal.x rounds to the
    origin's x for every pixel, so d.x = 0 exactly, while the clustered spheres around x = 1000 have boxes with positive
    faces: the case in which an unclamped 1 / d.x = inf turns the fma-form slab test into inf - inf = NaN."""
    sc = rtmi.Scene.new(9, 9, 4, 5)
    sc.set_background((0.25, 0.5, 0.75), sky_gradient=False, defocus_blur=False)
    sc.camera((1000.0, 0.0, 5.0), (1000.0, 0.0, 0.0), (0, 1, 0), 1e-6, 1.0, 0.0, 5.0)
    lights = [sc.diffuse_light((1.0 + k, 2.0, 3.0)) for k in range(3)]
    k = 0
    for ix in range(-3, 4):          # 7 x 7 small spheres on a lattice in the plane z = 0: 49 spheres -> 7 clusters
        for iy in range(-3, 4):
            sc.sphere((1000.0 + 1.5 * ix, 1.5 * iy, 0.0), 0.5, lights[k % 3])
            k += 1
    return sc


def test_axis_parallel_bounce_is_not_culled(rtmi, rtcheck):
    """A direction component of exactly 0 (a fuzz-free mirror produces them in the wild: round 1 found RTIOW 1920x1080,
    pixel (1745, 128), sample 8 with dy == 0): 1/0 = inf turned the fma-form slab test (b/d - o/d) into inf - inf = NaN
    on one face, min/max dropped the NaN together with the whole slab, and the ray skipped the cluster of the sphere it
    hits.  The reciprocals are clamped to +-1e18 since.  The case is constructed here instead of searched for."""
    sc = _axis_parallel_scene(rtmi)
    osc = rtcheck.OracleScene(sc)
    ref, queries = rtcheck.oracle_trace_sample(osc, SEED, 4, 4, 0)
    assert len(queries) == 1 and queries[0][3] == 0.0 and queries[0][7] == 1.0  # d.x == 0 exactly, and the ray hits
    assert abs(queries[0][6] - 0.9) < 1e-3                                      # the sphere at (1000, 0, 0), t = 4.5 / 5
    imgs = {}
    # (1000 units from the coordinate origin the lists' growth spans several cells: more than 63 entries per cell, so this
    #  scene gets the wide tables)
    for variant in (0, 36, 44, 32, 64, 128, 16):
        imgs[variant] = _assert_same(rtmi, rtcheck, sc, variant=variant)
        assert np.all(imgs[variant][4, 4] == np.float32([4.0, 8.0, 12.0]))  # 4 spp x the lattice centre's light (1, 2, 3)
    for variant in (0, 36, 44, 32, 64, 128):
        assert np.array_equal(imgs[variant], imgs[16])


def test_cluster_searches_on_a_sheet_and_a_volume(rtmi, rtcheck):
    """The measurement variants that search the sphere clusters (8 per cluster; round 1 also built 16) on both kinds of
    scene: wave votes, box hierarchy, range tables; the compact grid through global memory."""
    sc = rtmi.Scene.rtiow(5, 120, 68, 5, 50)   # a sheet
    st = sc.count(rtmi.Opts(seed=SEED))
    assert st.cull_cluster_size == 8 and st.kernel_variant == 6 and st.grid_sheet == 1
    _assert_same(rtmi, rtcheck, sc)
    for v in (32, 64, 128, 40):
        _assert_same(rtmi, rtcheck, sc, variant=v)
    vol = rtmi.Scene.new(64, 40, 3, 10)        # a volume
    vol.camera((0, 2, 14), (0, 0, 0), (0, 1, 0), 40.0)
    vol.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    rng = np.random.default_rng(21)
    mats = [vol.lambertian(rng.uniform(0.2, 0.9, 3)) for _ in range(4)] + [vol.metal((0.8, 0.8, 0.8), 0.1), vol.dielectric(1.5)]
    for i in range(300):
        vol.sphere(rng.uniform(-4, 4, 3), float(rng.uniform(0.05, 0.3)), mats[i % len(mats)])
    st = vol.count(rtmi.Opts(seed=SEED))
    assert st.cull_cluster_size == 8 and st.kernel_variant == 6 and st.grid_sheet == 0
    _assert_same(rtmi, rtcheck, vol)
    for v in (32, 64, 128, 40, 1):
        _assert_same(rtmi, rtcheck, vol, variant=v)


def test_culling_is_conservative_for_fp32_noise(rtmi, rtcheck):
    """AABB cluster culling vs the linear scan on the full frame, bit for bit.  Some paths leak
    ~2000 units inside the radius-1000 ground sphere, where the fp32 sphere test (|oc|^2 ~ 4e6,
    ulp 0.25 >> r^2 = 0.04) reports noise hits on small spheres; a fixed-margin box test skipped
    such a hit once in 33 M samples (found with an earlier random stream: pixel (90, 828)).  The
    per-lane margin 4e-3 (max|o_i| + extent + 1) keeps the culled kernel identical to the linear
    one and to the CPU checker."""
    sc = rtmi.Scene.rtiow(7, 1920, 1080, 24, 50)
    culled = sc.render(rtmi.Opts(seed=SEED))
    linear = sc.render(rtmi.Opts(seed=SEED, variant=16))
    assert np.array_equal(culled, linear)
    osc = rtcheck.OracleScene(sc)
    for y in (5, 828):
        ref, _ = rtcheck.oracle_render(osc, seed=SEED, rows=(y, y + 1))
        assert np.array_equal(culled[y], ref[y])
    st = sc.count(rtmi.Opts(seed=SEED))
    # the culled kernel really skips work: far fewer clusters visited than waves x clusters
    assert 0 < st.clusters_visited < 0.35 * st.wave_queries * st.cull_clusters
    # 4 big spheres are always tested; the 480 small ones make 60 clusters of 8 = one 64-cluster window
    assert st.cull_prefix == 4 and st.cull_cluster_size == 8 and st.cull_clusters == 60
    # the default walks the uniform grid: fewer sphere tests per query than one 8-sphere cluster
    assert st.cull_mode == 5 and 0 < st.lane_clusters < 8 * st.queries and 0 < st.lane_groups <= st.queries
    st = sc.count(rtmi.Opts(seed=SEED, variant=128))
    assert st.cull_mode == 3 and st.cull_windows == 1 and 0 < st.lane_clusters <= st.lane_cands
    # a second scene seed, and the DNA frame (30 cylinders culled by their world-space boxes)
    sc2 = rtmi.Scene.rtiow(11, 960, 540, 16, 50)
    assert np.array_equal(sc2.render(rtmi.Opts(seed=3)), sc2.render(rtmi.Opts(seed=3, variant=16)))
    sc3 = rtmi.Scene.dna(77.0)
    sc3.override(width=1280, height=720, spp=32)
    a = sc3.render(rtmi.Opts(seed=5))
    assert np.array_equal(a, sc3.render(rtmi.Opts(seed=5, variant=16))) and a.max() > 0
    ref, _ = rtcheck.oracle_render(rtcheck.OracleScene(sc3), seed=5, rows=(360, 362))
    assert np.array_equal(a[360:362], ref[360:362])


def test_bright_emitter_saturates_instead_of_wrapping(rtmi, rtcheck):
    """A 1e7-radiance light seen directly at 1024 spp: the reference's float sum reaches 1e10 and the written pixel is
    white.  The exact integer pixel sums must not wrap (a 2^-32 format did, at 2^31: negative sum, black pixel):
    samples are clamped to 2^16 in a 2^-24 format and at most 2^23 samples per pixel are accepted."""
    import test_primitives as tp
    sc = tp._probe_scene(rtmi, bg=(0, 0, 0))
    sc.xy_rect(-1, 1, -1, 1, 0.0, sc.diffuse_light((1e7, 3e4, 70000.0)))
    sc.override(spp=1024)
    img = _assert_same(rtmi, rtcheck, sc)
    centre = img[4, 4]
    assert np.all(centre == np.float32([65536.0 * 1024, 3e4 * 1024, 65536.0 * 1024]))  # clamp, exact, clamp
    assert np.all(rtmi.quantize_rgb8(img, 1024)[4, 4] == 255)
    with pytest.raises(rtmi.RtmiError) as e:
        sc.render(rtmi.Opts(sample_first=(1 << 23) - 5, sample_count=6))
    assert e.value.status == 6 and "samples per pixel" in str(e.value)
    assert sc.render(rtmi.Opts(sample_first=(1 << 23) - 6, sample_count=6)).shape == img.shape


def test_unpinned_edge_cases_on_device(rtmi, rtcheck):
    """The closed-form edge cases of the CUDA-only primitives (tests/test_primitives.py: cylinder far-root / end-cap
    clipping / inside-wall normal flip, inclusive rect bounds, edge-on rects) rendered by the kernel: equal to the
    checker bit for bit, and the expected values hold on the device too.  (The name is from when no reference run pinned
    these primitives; tests/test_gpu_reference_gpu_pin.py now holds the kernel to the compiled gpu-version's records.)"""
    import test_primitives as tp
    for name, sc, want in tp.edge_case_scenes(rtmi):
        img = _assert_same(rtmi, rtcheck, sc)
        if want is not None:
            assert np.all(img[4, 4] == np.float32(want) * sc.spp), name


def test_big_sheet_uses_range_tables_over_many_windows(rtmi, rtcheck):
    """3000 small spheres spread over a ground sheet: 375 clusters = 6 windows of 64 clusters, each with its own range
    tables (variant 136: 48 KB of sphere records + 36 KB of tables through global memory; 128: the same forced into
    LDS, one workgroup per CU at that size).  The default walks the grid instead (through global memory at this size).
    Same bits as the flat scan and the checker, all of them."""
    sc = rtmi.Scene.new(96, 54, 2, 10)
    sc.camera((0, 9, 26), (0, 0, 0), (0, 1, 0), 40.0)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    rng = np.random.default_rng(17)
    mats = [sc.lambertian(rng.uniform(0.2, 0.9, 3)) for _ in range(5)] + [sc.metal((0.8, 0.8, 0.8), 0.05), sc.dielectric(1.5)]
    sc.sphere((0, -1000, 0), 1000.0, mats[0])
    for i in range(3000):
        r = float(rng.uniform(0.05, 0.15))
        sc.sphere((float(rng.uniform(-20, 20)), r, float(rng.uniform(-20, 20))), r, mats[i % len(mats)])
    st = sc.count(rtmi.Opts(seed=SEED))
    assert st.cull_mode == 7 and st.kernel_variant == 44 and st.lane_clusters > 0 and st.lane_groups > 0
    st = sc.count(rtmi.Opts(seed=SEED, variant=128))
    assert st.cull_mode == 3 and st.cull_windows == 6 and st.cull_clusters == 375 and st.lane_cands >= st.lane_clusters > 0
    img = _assert_same(rtmi, rtcheck, sc)
    assert np.array_equal(img, sc.render(rtmi.Opts(seed=SEED, variant=16)))
    assert np.array_equal(img, sc.render(rtmi.Opts(seed=SEED, variant=36)))   # the wide grid tables in LDS
    assert np.array_equal(img, sc.render(rtmi.Opts(seed=SEED, variant=128)))  # range tables in LDS (90 KB per workgroup)
    assert np.array_equal(img, sc.render(rtmi.Opts(seed=SEED, variant=64)))   # the box hierarchy on the same clusters
    with pytest.raises(rtmi.RtmiError, match="compact"):
        sc.render(rtmi.Opts(seed=SEED, variant=1))  # no compact tables at this size


def _cloud(rtmi, n, half, seed, w=64, h=40, spp=3, depth=12, r=(0.05, 0.25)):
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    rng = np.random.default_rng(seed)
    mats = [sc.lambertian(rng.uniform(0.2, 0.9, 3)) for _ in range(4)] + [sc.metal((0.8, 0.8, 0.8), 0.1), sc.dielectric(1.5)]
    for i in range(n):
        sc.sphere(rng.uniform(-half, half, 3), float(rng.uniform(*r)), mats[i % len(mats)])
    return sc, mats


def test_grid_list_tiers_and_the_scan_beyond_them(rtmi, rtcheck):
    """The grid's cell lists are grown for ray origins near the cloud (near tier: within 1.5 cloud radii or the camera's
    distance) and for origins up to 64 units / 8 cloud radii out (far tier); further out a lane scans every clustered
    sphere.  A plane mirror sends the camera's rays back into a cloud of 300 spheres from 40 units away (far tier) or from
    90 (beyond the lists' reach): every pixel equals the flat scan and the checker."""
    for mirror_z, far_tier, beyond in ((-40.0, True, False), (-90.0, False, True)):
        sc, mats = _cloud(rtmi, 300, 3.0, 31, w=80, h=50, spp=4)
        sc.xy_rect(-300.0, 300.0, -300.0, 300.0, mirror_z, sc.metal((0.95, 0.95, 0.95), 0.0))
        sc.camera((0.0, 2.0, 14.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0)
        st = sc.count(rtmi.Opts(seed=SEED))
        assert st.cull_mode == 7 and st.kernel_variant == 36 and st.lane_groups > 0  # (the mirror makes it a wide-table scene)
        if far_tier:
            assert st.group_maxpop > 0, "no lane walked the far tier"
        if beyond:
            assert st.query_maxpop > 0, "no lane scanned from beyond the lists' reach"
        img = _assert_same(rtmi, rtcheck, sc)
        assert np.array_equal(img, sc.render(rtmi.Opts(seed=SEED, variant=16)))
        assert np.array_equal(img, sc.render(rtmi.Opts(seed=SEED, variant=44)))
        # the same with a mirror SPHERE of radius 1000 (always tested: no entry of the lists): a compact-table scene
        sph, _ = _cloud(rtmi, 300, 3.0, 31, w=80, h=50, spp=4)
        sph.sphere((0.0, 0.0, mirror_z - 1000.0), 1000.0, sph.metal((0.95, 0.95, 0.95), 0.0))
        sph.camera((0.0, 2.0, 14.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0)
        st = sph.count(rtmi.Opts(seed=SEED))
        assert st.cull_mode == 5 and st.kernel_variant == 6 and st.lane_groups > 0
        assert (st.group_maxpop > 0) if far_tier else (st.query_maxpop > 0)
        img = _assert_same(rtmi, rtcheck, sph)
        for v in (16, 40, 1):
            assert np.array_equal(img, sph.render(rtmi.Opts(seed=SEED, variant=v)))


def test_clumps_keep_their_grid(rtmi, rtcheck):
    """More than 63 spheres listed in one cell (a clump) is more than the compact tables hold: the scene gets the wide
    tables (1023 per cell).  A clump beyond those too is taken out of the lists and tested for every query -- in the limit
    the reference's scan.  (Until round 3 such scenes fell back to the cluster searches.)"""
    sc, mats = _cloud(rtmi, 200, 4.0, 41)
    rng = np.random.default_rng(42)
    for i in range(90):  # the clump
        sc.sphere(tuple(np.array([1.0, 1.0, 1.0]) + rng.uniform(-0.02, 0.02, 3)), 0.1, mats[i % len(mats)])
    sc.camera((0, 2, 14), (0, 0, 0), (0, 1, 0), 40.0)
    st = sc.count(rtmi.Opts(seed=SEED))
    assert st.cull_mode == 7 and st.kernel_variant == 36
    img = _assert_same(rtmi, rtcheck, sc)
    assert np.array_equal(img, sc.render(rtmi.Opts(seed=SEED, variant=16)))
    with pytest.raises(rtmi.RtmiError, match="compact"):
        sc.render(rtmi.Opts(seed=SEED, variant=1))
    big, mats = _cloud(rtmi, 100, 4.0, 43, w=32, h=20, spp=2, depth=4)
    for i in range(1100):  # beyond the wide tables' 1023 per cell
        big.sphere(tuple(np.array([-1.0, 0.5, 1.0]) + rng.uniform(-0.01, 0.01, 3)), 0.05, mats[i % len(mats)])
    big.camera((0, 2, 14), (0, 0, 0), (0, 1, 0), 40.0)
    st = big.count(rtmi.Opts(seed=SEED))
    assert st.cull_mode == 7 and st.cull_prefix >= 1100  # the clump's members are tested for every query
    img = _assert_same(rtmi, rtcheck, big)
    assert np.array_equal(img, big.render(rtmi.Opts(seed=SEED, variant=16)))


def test_headline_kernel_is_counted_by_the_3d_walk_over_the_same_cells(rtmi, rtcheck):
    """bench.py's roofline counts come from the counting build of the 3-D grid walk (variant 6), while the headline frame
    is rendered by the x-z walk (variant 2) that variant 0 picks for RTIOW's one-cell-high grid.  Same scene as the bench
    (rt_scene_rtiow(7)), smaller frame: the two kernels' images are equal, the counting launch reports which kernel ran, its
    event counts equal the CPU checker's, and asking it for variant 0, 2 or 6 gives the same counters."""
    sc = rtmi.Scene.rtiow(7, 192, 108, 8, 50)
    st = rtmi.Stats()
    sheet = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant == 2
    walk3d = sc.render(rtmi.Opts(seed=SEED, variant=6))
    assert np.array_equal(sheet, walk3d)
    counts = {}
    for asked in (0, 2, 6):
        c, img = sc.count(rtmi.Opts(seed=SEED, variant=asked), want_image=True)
        assert c.kernel_variant == 6 and c.cull_mode == 5 and c.grid_sheet == 1
        assert np.array_equal(img, sheet)
        d = c.as_dict()
        counts[asked] = {k: d[k] for k in ("samples", "queries", "hits", "misses", "scatter", "rng_draws", "lane_clusters",
                                           "lane_groups", "lane_cands", "cand_lanes")}
    assert counts[0] == counts[2] == counts[6]
    _, want = rtcheck.oracle_render(sc, seed=SEED, want_counts=True)
    for k, v in want.items():
        assert c.as_dict()[k] == v, k


def test_sheet_walk_equals_the_3d_walk_and_the_flat_scan(rtmi, rtcheck):
    """A grid that is one cell high (RTIOW's spheres on the ground) is walked along x and z only (variant 2, what
    variant 0 picks by itself there).  Same cells, same tests, same bytes as the 3-D walk (variant 6) and as the
    linear scan; a volume has no such grid and refuses variant 2."""
    sc = rtmi.Scene.rtiow(11, 160, 90, 6, 50)
    flat = sc.render(rtmi.Opts(seed=SEED, variant=16))
    auto = _assert_same(rtmi, rtcheck, sc, variant=0)
    sheet = sc.render(rtmi.Opts(seed=SEED, variant=2))
    assert np.array_equal(auto, flat) and np.array_equal(sheet, flat)
    assert np.array_equal(sc.render(rtmi.Opts(seed=SEED, variant=6)), flat)
    # a camera inside the sheet, looking along it: long walks through many cells, rays that leave through the top
    low = rtmi.Scene.rtiow(11, 160, 90, 4, 50)
    low.camera((0.3, 0.25, 0.2), (8.0, 0.3, 6.0), (0, 1, 0), 70.0, 160 / 90, 0.05, 4.0)
    assert np.array_equal(low.render(rtmi.Opts(seed=3, variant=2)), low.render(rtmi.Opts(seed=3, variant=16)))
    assert np.array_equal(low.render(rtmi.Opts(seed=3, variant=2)), low.render(rtmi.Opts(seed=3, variant=6)))  # (the 3-D walk)
    vol = rtmi.Scene.new(64, 40, 3, 10)
    vol.set_background((0.5, 0.7, 1.0), sky_gradient=True, defocus_blur=False)
    vol.camera((0, 0, 12), (0, 0, 0), (0, 1, 0), 40.0, 1.6, 0.0, 12.0)
    m = vol.lambertian((0.5, 0.5, 0.5))
    rng = np.random.default_rng(5)
    for _ in range(200):
        c = rng.uniform(-3, 3, 3)
        vol.sphere((float(c[0]), float(c[1]), float(c[2])), 0.15, m)
    with pytest.raises(rtmi.RtmiError):
        vol.render(rtmi.Opts(seed=1, variant=2))
    assert np.array_equal(vol.render(rtmi.Opts(seed=1)), vol.render(rtmi.Opts(seed=1, variant=16)))


def test_wide_grid_tables_for_65536_spheres_and_more(rtmi, rtcheck):
    """Scenes with 65536 sphere slots or more get the WIDE grid tables (32-bit list entries, two words per cell, up to 1023
    cells per axis).  A volume and a sheet (more than 255 cells along two axes) against the linear scan, and two row bands
    of each against the CPU checker."""
    rng = np.random.default_rng(17)
    vol = rtmi.Scene.new(48, 32, 2, 6)
    vol.set_background((0.5, 0.7, 1.0), sky_gradient=True, defocus_blur=False)
    vol.camera((0, 0, 30), (0, 0, 0), (0, 1, 0), 35.0, 1.5, 0.0, 30.0)
    mats = [vol.lambertian((0.6, 0.5, 0.4)), vol.metal((0.8, 0.8, 0.9), 0.1), vol.dielectric(1.5)]
    c = rng.uniform(-8, 8, (70000, 3)).astype(np.float32)
    for i in range(len(c)):
        vol.sphere((float(c[i, 0]), float(c[i, 1]), float(c[i, 2])), 0.06, mats[i % 3])
    st = rtmi.Stats()
    auto = vol.render(rtmi.Opts(seed=5), st)
    assert st.kernel_variant == 44
    assert np.array_equal(auto, vol.render(rtmi.Opts(seed=5, variant=24)))   # the linear scan (tables in global memory)
    osc = rtcheck.OracleScene(vol)
    for y in (3, 17):
        ref, _ = rtcheck.oracle_render(osc, seed=5, rows=(y, y + 2))
        assert np.array_equal(auto[y:y + 2], ref[y:y + 2])
    for bad in (1, 2, 6, 40):
        with pytest.raises(rtmi.RtmiError):
            vol.render(rtmi.Opts(seed=5, variant=bad))
    sheet = rtmi.Scene.new(48, 32, 2, 6)
    sheet.set_background((0.5, 0.7, 1.0), sky_gradient=True, defocus_blur=False)
    sheet.camera((3, 2.5, 9), (0, 0, 0), (0, 1, 0), 40.0, 1.5, 0.0, 9.0)
    m = [sheet.lambertian((0.3, 0.6, 0.3)), sheet.metal((0.9, 0.9, 0.9), 0.0)]
    sheet.sphere((0, -1000, 0), 1000.0, sheet.lambertian((0.5, 0.5, 0.5)))
    n = 260  # 260 x 260 = 67600 spheres on a lattice, jittered
    j = rng.uniform(-0.01, 0.01, (n, n, 2))
    for a in range(n):
        for b in range(n):
            sheet.sphere((float(0.1 * (a - n / 2) + j[a, b, 0]), 0.03, float(0.1 * (b - n / 2) + j[a, b, 1])), 0.03, m[(a + b) % 2])
    img = sheet.render(rtmi.Opts(seed=9), st)
    assert st.kernel_variant == 44
    assert np.array_equal(img, sheet.render(rtmi.Opts(seed=9, variant=24)))
    osc = rtcheck.OracleScene(sheet)
    for y in (2, 20):
        ref, _ = rtcheck.oracle_render(osc, seed=9, rows=(y, y + 2))
        assert np.array_equal(img[y:y + 2], ref[y:y + 2])
    with pytest.raises(rtmi.RtmiError):  # and a small sphere-only scene has no wide tables
        rtmi.Scene.rtiow(3, 32, 18, 1, 5).render(rtmi.Opts(seed=1, variant=44))
