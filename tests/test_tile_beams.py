"""The beam table (csrc/rt_beam.h), on the CPU: every sphere that the fp32 sphere test flags for a camera ray of a
tile is in that tile's list, or the tile carries the overflow mark.  The camera ray and the predicate are restated in numpy
float32 (tile_beam_cases.py) and asked of random samples of the tile -- pixel, jitter, lens point -- and of its extremes:
the corner pixels with the jitter's end values and the rim of the lens.  No tile of a case overflows, except in the case
built to."""
import numpy as np
import pytest

import tile_beam_cases as tb

N = 192  # random samples per tile, beside the 64 extreme ones


def _check_tiles(sc, tiles, seed=1):
    """-> share of overflowing tiles among `tiles`; asserts the property for the others"""
    table = sc.tile_beams()
    _, slots, _ = tb.camera_records(sc)
    rng = np.random.default_rng(seed)
    over = 0
    for tx, ty in tiles:
        rec = table[ty, tx]
        if rec[0] == 0xFFFF:
            over += 1
            continue
        ids = set(int(i) for i in rec[1:1 + int(rec[0])])
        assert len(ids) == int(rec[0]) <= 15 and all(slots[i, 3] >= 0 for i in ids)
        o, d = tb.burst_rays(sc, *tb.tile_samples(sc, tx, ty, N, rng))
        hit = np.nonzero(tb.flagged(o, d, slots).any(axis=0))[0]
        missing = [int(i) for i in hit if int(i) not in ids]
        assert not missing, f"tile ({tx}, {ty}): the fp32 test flags slots {missing}, the list is {sorted(ids)}"
    return over / len(tiles)


def _all_tiles(sc):
    return [(tx, ty) for ty in range((sc.height + 7) // 8) for tx in range((sc.width + 7) // 8)]


def test_rtiow_bench_frame(rtmi):
    sc = rtmi.Scene.rtiow(7, 1920, 1080, 1024, 50)
    table = sc.tile_beams()
    assert table.shape == (135, 240, 16)
    counts = table[..., 0].astype(int)
    # gate 0: no tile of the bench frame overflows, and the bound is tight enough to pay (a mean under 4 entries)
    assert (counts != 0xFFFF).all() and counts.mean() < 4.0
    tiles = {(0, 0), (239, 0), (0, 134), (239, 134), (120, 134)}  # the corners, and a tile of sky
    assert table[134, 120, 0] == 0
    for c in ((0.0, 1.0, 0.0), (-4.0, 1.0, 0.0), (4.0, 1.0, 0.0)):  # the big spheres: the middle and the silhouette
        for dx, dy in ((0, 0), (0, 0.98), (0, -0.98), (0.98, 0), (-0.98, 0)):
            right = np.cross(np.array(c) - np.array((13.0, 2.0, 3.0)), (0, 1, 0))
            right /= np.linalg.norm(right)
            t = tb.film_tile(sc, np.array(c) + dx * right + np.array((0, dy, 0)))
            assert t is not None
            tiles.add(t)
    rng = np.random.default_rng(5)
    tiles |= {(int(rng.integers(0, 240)), int(rng.integers(0, 135))) for _ in range(24)}
    assert _check_tiles(sc, sorted(tiles)) == 0.0


def test_partial_tiles(rtmi):
    sc = tb.layer_scene(rtmi, 100, 52, 4, (9, 2, 7), (0, 0.5, 0), 0.1, 10.0, n=40)
    assert sc.tile_beams().shape == (7, 13, 16)
    assert _check_tiles(sc, _all_tiles(sc)) == 0.0


@pytest.mark.parametrize("name,kw", [
    ("no defocus", dict(eye=(9, 2, 7), lookat=(0, 0.5, 0), aperture=0.0, focus=10.0, defocus=False)),
    ("lens radius 1", dict(eye=(9, 2.5, 7), lookat=(0, 0.5, 0), aperture=2.0, focus=11.0, n=40)),
    ("focus plane in front of the spheres", dict(eye=(12, 3, 9), lookat=(0, 0.5, 0), aperture=0.04, focus=2.0, n=60)),
    ("focus plane behind the spheres", dict(eye=(9, 2, 7), lookat=(0, 0.5, 0), aperture=0.1, focus=60.0, n=60)),
    ("camera inside the layer", dict(eye=(2.0, 0.2, 3.0), lookat=(0, 0.4, 0), aperture=0.02, focus=3.0, n=60)),
])
def test_cameras(rtmi, name, kw):
    sc = tb.layer_scene(rtmi, 200, 120, 4, **kw)
    assert _check_tiles(sc, _all_tiles(sc)[::3]) == 0.0, name


def test_camera_inside_a_sphere_and_a_sphere_behind_it(rtmi):
    sc = rtmi.Scene.new(64, 40, 4, 6)
    sc.camera((0.0, 0.5, 4.0), (0.0, 0.5, 0.0), (0, 1, 0), 40.0, 0.0, 0.1, 4.0)
    sc.set_background((0.6, 0.7, 0.9), sky_gradient=True, defocus_blur=True)
    m = sc.dielectric(1.5)
    around = sc.sphere((0.0, 0.5, 4.2), 1.5, m)   # the camera sits inside this one
    behind = sc.sphere((0.0, 0.5, 9.0), 1.0, m)   # and this one lies behind it
    for i in range(12):
        sc.sphere((-3.0 + 0.5 * i, 0.3, 0.0), 0.2, m)
    table, (_, slots, _) = sc.tile_beams(), tb.camera_records(sc)
    slot_of = lambda c: int(np.nonzero((np.abs(slots[:, :3] - np.array(c, np.float32)).max(axis=1) == 0) & (slots[:, 3] >= 0))[0][0])
    s_around, s_behind = slot_of((0.0, 0.5, 4.2)), slot_of((0.0, 0.5, 9.0))
    assert around != behind
    for ty in range(table.shape[0]):
        for tx in range(table.shape[1]):
            rec = table[ty, tx]
            ids = [int(i) for i in rec[1:1 + int(rec[0])]]
            assert rec[0] != 0xFFFF and s_around in ids and s_behind not in ids
    assert _check_tiles(sc, _all_tiles(sc)) == 0.0


@pytest.mark.parametrize("sheet", [True, False])
@pytest.mark.parametrize("seed", [31, 32, 33])
def test_fuzz_generators(rtmi, seed, sheet):
    sc = tb.fuzz_scene(rtmi, seed, sheet)
    # (the generator draws frames of 40 .. 110 pixels, whose tiles each see a good part of the scene: the same scenes at
    #  twelve times the frame, so that no list overflows, on a sample of the tiles)
    sc.override(width=12 * sc.width, height=12 * sc.height)
    tiles = _all_tiles(sc)
    assert (sc.tile_beams()[..., 0] != 0xFFFF).all()
    assert _check_tiles(sc, tiles[::max(1, len(tiles) // 80)]) == 0.0


def test_row_of_spheres_overflows(rtmi):
    sc = tb.row_scene(rtmi)
    table = sc.tile_beams()
    assert rtmi._lib.rt_scene_tile_beams_capacity() == 15
    mid = table[2, 3:5]  # the line of sight leaves through the corner that tiles (3, 2) and (4, 2) share
    assert (mid[..., 0] == 0xFFFF).all() and (mid[..., 1:] == 0).all()
    share = _check_tiles(sc, _all_tiles(sc))
    assert 0.0 < share < 0.5


def test_lists_do_not_depend_on_shard_options(rtmi):
    """a record is indexed by whole-frame tile coordinates: the table is the frame's, whatever shard is asked for"""
    sc = rtmi.Scene.rtiow(7, 100, 52, 8, 50)
    whole = sc.tile_beams()
    for o in (rtmi.Opts(tile_first=1, tile_stride=3, tile_rotate=1), rtmi.Opts(tile_rows=16, tile_first=0, tile_stride=2)):
        assert sc.shard_rows(o) < 52
        assert np.array_equal(sc.tile_beams(o), whole)


def test_lists_follow_the_camera_and_the_frame(rtmi):
    make = lambda: tb.layer_scene(rtmi, 96, 56, 4, (9, 2, 7), (0, 0.5, 0), 0.1, 10.0, n=40)
    sc = make()
    first = sc.tile_beams()
    sc.camera((-9.0, 2.0, 7.0), (0.0, 0.5, 0.0), (0, 1, 0), 30.0, 0.0, 0.1, 10.0)
    moved = sc.tile_beams()
    assert moved.shape == first.shape and not np.array_equal(moved, first)
    fresh = make()
    fresh.camera((-9.0, 2.0, 7.0), (0.0, 0.5, 0.0), (0, 1, 0), 30.0, 0.0, 0.1, 10.0)
    assert np.array_equal(fresh.tile_beams(), moved)
    sc.override(width=200, height=120)
    wide = sc.tile_beams()
    assert wide.shape == (15, 25, 16)
    fresh.override(width=200, height=120)
    assert np.array_equal(fresh.tile_beams(), wide)
    assert _check_tiles(sc, _all_tiles(sc)[::7]) == 0.0
