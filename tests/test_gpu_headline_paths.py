"""-m gpu: the paths of the grid walk that the headline kernel's instruction diet touches -- 24-bit multiplies for pixel ids and
cell indices, 32-bit record offsets, the walk's live lanes as a scalar mask, bare minima in the step pass -- each held to the
reference's linear scan (variant 16) bit for bit, on scenes small enough for a few seconds per test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 2023


def _sheet(rtmi, w, h, spp, depth):
    """A ground sphere, a 6 x 6 sheet of small spheres on it, one sphere taller than the layer, and two fuzz-free mirror
    spheres of radius 1000 (the construction of test_grid_list_tiers_and_the_scan_beyond_them, both mirrors in one frame).
    Each mirror touches a point about 40 / about 90 units from the sheet and faces so that the camera's ray to that point
    goes on to the sheet's centre: the rays come back from the far tier of the cells' lists and from beyond the lists'
    reach.  The two points lie more than 64 degrees apart as seen from the sheet, or the nearer mirror would hide the
    other.  (The checker's trace of this frame at 96 x 54 x 4: 3403 queries reach the grid's bounds from the near tier, 61
    from the far tier, 12 from beyond.)  Spheres only: compact tables, a grid one cell high, so variant 0 is the x-z walk (2)
    and the 3-D walk (6) reads the same tables."""
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    cam = np.array([0.0, 2.0, 14.0])
    sc.camera(tuple(cam), (-3.1, 1.0, 0.0), (0, 1, 0), 40.0)
    rng = np.random.default_rng(5)
    mats = [sc.lambertian(rng.uniform(0.2, 0.9, 3)) for _ in range(4)] + [sc.metal((0.8, 0.8, 0.8), 0.1), sc.dielectric(1.5)]
    sc.sphere((0.0, -1000.0, 0.0), 1000.0, mats[0])
    for i in range(6):
        for j in range(6):
            r = float(rng.uniform(0.15, 0.25))
            sc.sphere((1.1 * (i - 2.5) + float(rng.uniform(-0.2, 0.2)), r, 1.1 * (j - 2.5) + float(rng.uniform(-0.2, 0.2))), r,
                      mats[(6 * i + j) % len(mats)])
    sc.sphere((0.4, 1.0, -0.3), 1.0, mats[5])  # taller than the layer of cells
    mirror = sc.metal((0.95, 0.95, 0.95), 0.0)
    for reach, towards in ((40.0, (-0.9, 0.25, -0.6)), (90.0, (0.35, 0.25, -1.0))):
        p = reach * np.array(towards) / np.linalg.norm(towards)
        n = (cam - p) / np.linalg.norm(cam - p) - p / np.linalg.norm(p)  # bisects the directions to the camera and to the sheet
        c = p - 1000.0 * n / np.linalg.norm(n)
        sc.sphere(tuple(float(x) for x in c), 1000.0, mirror)
    return sc


def _same_as_scan(rtmi, sc, variants, **kw):
    scan = sc.render(rtmi.Opts(seed=SEED, variant=16, **kw))
    assert scan.any()
    for v in variants:
        img = sc.render(rtmi.Opts(seed=SEED, variant=v, **kw))
        assert np.array_equal(img, scan), f"variant {v}: {(img != scan).any(axis=2).sum()} pixels differ from the linear scan"
    return scan


def test_pixel_ids_at_and_above_2_to_the_24(rtmi, rtcheck):
    """A sample's stream is keyed by its pixel id, row x width + column, which the refill forms with one 24-bit
    multiply-add.  RTIOW seed 7 on a frame 16384 wide and 1032 high: the last row tile (rows 1024 .. 1031) holds the ids
    2^24 .. 2^24 + 131071, past what a 24-bit RESULT would hold.  Only that tile is rendered (a shard of one tile); the default
    kernel equals the linear scan bit for bit, and two of its rows equal the CPU restatement."""
    w, h = 16384, 1032
    sc = rtmi.Scene.rtiow(7, w, h, 2, 8)
    tiles = h // 8
    shard = dict(tile_rows=8, tile_first=tiles - 1, tile_stride=tiles, tile_rotate=0)
    o = rtmi.Opts(seed=SEED, **shard)
    assert sc.shard_rows(o) == 8
    rows = sc.shard_global_rows(o)
    assert list(rows) == list(range(h - 8, h)) and int(rows[0]) * w == 1 << 24
    st = rtmi.Stats()
    img = sc.render(o, st)
    assert st.kernel_variant == 2 and img.shape == (8, w, 3)
    assert np.array_equal(img, sc.render(rtmi.Opts(seed=SEED, variant=16, **shard)))
    ref, _ = rtcheck.oracle_render(sc, seed=SEED, rows=(h - 2, h))
    assert ref[h - 2:].any()
    assert np.array_equal(img[6:], ref[h - 2:]), "rows 1030 and 1031 differ from the CPU checker"


def test_all_three_origin_tiers_on_a_sheet(rtmi):
    """Near tier, far tier and the scan from beyond the lists' reach in one frame of the sheet scene, through the x-z walk
    (2) and the 3-D walk (6): both equal the linear scan, and the counting build saw far-tier walks and beyond-range scans."""
    sc = _sheet(rtmi, 96, 54, 4, 12)
    st = sc.count(rtmi.Opts(seed=SEED))
    assert st.cull_mode == 5 and st.grid_sheet == 1 and st.lane_groups > 0
    assert st.group_maxpop > 0, "no lane walked the far tier"
    assert st.query_maxpop > 0, "no lane scanned from beyond the lists' reach"
    assert st.lane_groups > st.group_maxpop, "no lane walked the near tier"
    _same_as_scan(rtmi, sc, (2, 6))


def test_the_3d_walk_and_the_wide_tables(rtmi):
    """The same code walks a volume in 3-D (compact tables in LDS: 6, the default here; in global memory: 40) and the wide
    tables of a scene with other primitives (36, the default there): 200 random spheres in a volume, then the same with a
    rectangle and a cylinder among them, each against the linear scan."""
    def cloud():
        sc = rtmi.Scene.new(64, 36, 4, 12)
        sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
        sc.camera((0.0, 2.0, 14.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0)
        rng = np.random.default_rng(23)
        mats = [sc.lambertian(rng.uniform(0.2, 0.9, 3)) for _ in range(4)] + [sc.metal((0.8, 0.8, 0.8), 0.1), sc.dielectric(1.5)]
        for i in range(200):
            sc.sphere(rng.uniform(-3.0, 3.0, 3), float(rng.uniform(0.05, 0.25)), mats[i % len(mats)])
        return sc, mats

    sc, _ = cloud()
    st = rtmi.Stats()
    sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant == 6
    _same_as_scan(rtmi, sc, (0, 6, 40))
    wide, mats = cloud()
    wide.xy_rect(-1.0, 1.5, -0.5, 1.0, -1.0, mats[4])
    wide.cylinder(0.4, -1.0, 1.0, mats[1], rotate=((1.0, 0.0, 0.0), 35.0), translate=(1.0, 0.5, 1.0))
    st = rtmi.Stats()
    wide.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant == 36
    _same_as_scan(rtmi, wide, (0,))


def test_a_walk_cut_short_and_resumed(rtmi):
    """When few lanes of a wave still walk while most wait, the stragglers stop at their next cell boundary and take the walk
    up in the next iteration.  The sheet scene on one 8 x 8-aligned frame of 64 x 64 at depth 50: the counting build reports
    resumed walks, and the x-z walk equals the linear scan.  (The counting build walks in 3-D, variant 6, also on a sheet:
    the counter shows cuts in that kernel.  The x-z walk of variant 2 shares the tail's criterion and visits the same cells
    with the same lanes, so the 3-D walk's image is compared as well.)"""
    sc = _sheet(rtmi, 64, 64, 8, 50)
    st = sc.count(rtmi.Opts(seed=SEED))
    assert st.cull_mode == 5 and st.grid_sheet == 1
    assert st.walk_resumed > 0, "no walk was cut short and resumed"
    _same_as_scan(rtmi, sc, (2, 6))
