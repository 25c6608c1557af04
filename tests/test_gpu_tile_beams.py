"""-m gpu: the bursts of variants 2 and 6 test their tile's list of the beam table (csrc/rt_beam.h, render_burst.h) instead of
running the prefix and the grid walk.  Whole-frame byte equality against the reference's linear scan (variant 16) is the
test: a sphere that is missing from a list, a stale table, a record of the wrong tile or a list path that resolves
differently changes pixels.  The frames are the smallest at which the path can go wrong -- several tiles, partial tiles,
more than one workgroup's worth of items -- so a case is a few launches of milliseconds; the scan of a configuration is
rendered once and shared by the two variants."""
import os

import numpy as np
import pytest

import tile_beam_cases as tb

pytestmark = pytest.mark.gpu
SEED = 2023
_scans = {}


def _scan(rtmi, key, sc, **opts):
    if key not in _scans:
        _scans[key] = sc.render(rtmi.Opts(seed=SEED, variant=16, **opts))
        assert _scans[key].any()
    return _scans[key]


def _variants(sc):
    """2 walks a grid that is one cell high; 6 reads the same compact tables in every scene that has them"""
    info = sc.table_info()
    assert not info.grid_wide
    return [2, 6] if info.grid_sheet else [6]


def _held(rtmi, key, sc, **opts):
    scan = _scan(rtmi, key, sc, **opts)
    for v in _variants(sc):
        st = rtmi.Stats()
        img = sc.render(rtmi.Opts(seed=SEED, variant=v, **opts), st)
        assert st.kernel_variant == v
        assert np.array_equal(img, scan), f"variant {v}: {(img != scan).any(axis=2).sum()} pixels differ from the linear scan"
    return scan


def _layer(rtmi, w, h, spp, **kw):
    args = dict(eye=(9, 2, 7), lookat=(0, 0.5, 0), aperture=0.1, focus=10.0)
    args.update(kw)
    return tb.layer_scene(rtmi, w, h, spp, **args)


CASES = {
    "rtiow_256x144": lambda rtmi: rtmi.Scene.rtiow(7, 256, 144, 8, 50),
    "rtiow_100x52_partial_tiles": lambda rtmi: rtmi.Scene.rtiow(7, 100, 52, 8, 50),
    "no_defocus_64x40": lambda rtmi: _layer(rtmi, 64, 40, 16, aperture=0.0, defocus=False),
    "camera_inside_the_layer": lambda rtmi: _layer(rtmi, 64, 40, 8, eye=(2.0, 0.2, 3.0), lookat=(0, 0.4, 0), aperture=0.02, focus=3.0, n=60),
    "row_of_spheres_overflow": lambda rtmi: tb.row_scene(rtmi),
    "all_sky": lambda rtmi: tb.sky_scene(rtmi),
}


@pytest.mark.parametrize("name", list(CASES))
def test_frames_equal_the_linear_scan(rtmi, name):
    sc = CASES[name](rtmi)
    table = sc.tile_beams()
    if name == "row_of_spheres_overflow":  # the fall-back walk runs in the marked tiles, the lists in the others
        assert (table[..., 0] == 0xFFFF).any() and (table[..., 0] != 0xFFFF).any()
    if name == "all_sky":
        assert (table[..., 0] == 0).all()
    _held(rtmi, name, sc)
    assert np.array_equal(sc.tile_beams(device=True), table)


@pytest.mark.parametrize("rr", [0.0, 0.8], ids=["roulette_off", "roulette_on"])
def test_roulette(rtmi, rr):
    sc = rtmi.Scene.rtiow(7, 100, 52, 8, 50)
    if rr > 0.0:
        sc.set_russian_roulette(rr)
    _held(rtmi, ("roulette", rr), sc)


def test_three_sphere_scene_through_variant_6(rtmi, scenes_dir):
    sc = rtmi.Scene.load(os.path.join(scenes_dir, "three_sphere.json"))
    sc.override(width=96, height=56, spp=8)
    info = sc.table_info()
    if info.grid_wide:
        pytest.fail("three_sphere.json no longer packs to compact tables: variant 6 cannot render it")
    scan = _scan(rtmi, "three", sc)
    assert np.array_equal(sc.render(rtmi.Opts(seed=SEED, variant=6)), scan)


@pytest.mark.parametrize("ranks,rotate", [(2, 0), (3, 1), (3, 2)])
def test_shards_assemble_to_the_unsharded_frame(rtmi, ranks, rotate):
    """tile_first / tile_stride shards over row tiles of 8 rows: every rank reads the frame's own table at whole-frame tile
    coordinates, through its deal of the row tiles"""
    sc = rtmi.Scene.rtiow(7, 100, 52, 8, 50)
    scan = _scan(rtmi, ("roulette", 0.0), sc)
    for v in _variants(sc):
        frame = np.full_like(scan, np.nan)
        for r in range(ranks):
            o = rtmi.Opts(seed=SEED, variant=v, tile_rows=8, tile_first=r, tile_stride=ranks, tile_rotate=rotate)
            rows = sc.shard_global_rows(o)
            frame[rows] = sc.render(o)
        assert np.array_equal(frame, scan), f"variant {v}, {ranks} ranks, deal {rotate}"


def test_device_table_equals_the_host_lists(rtmi):
    for sc in (rtmi.Scene.rtiow(7, 256, 144, 8, 50), tb.fuzz_scene(rtmi, 31, True), tb.fuzz_scene(rtmi, 32, False)):
        host = sc.tile_beams()
        assert np.array_equal(sc.tile_beams(device=True), host)
        _held(rtmi, ("table", id(sc)), sc)
        assert np.array_equal(sc.tile_beams(device=True), host)


MOVED = ((-9.0, 2.0, 7.0), (0.0, 0.5, 0.0), (0, 1, 0), 30.0, 0.0, 0.1, 10.0)


def test_a_moved_camera_and_a_resized_frame_rebuild_the_table(rtmi):
    """Render, move the camera, render again: the frame is a fresh scene's with that camera -- a stale table would test the old
    camera's lists.  The same after override(width, height), and over two frames of a driver whose camera moves between them."""
    for v in (2, 6):
        sc = _layer(rtmi, 64, 40, 8)
        _held(rtmi, "stale_first", sc)
        sc.camera(*MOVED)
        fresh = _layer(rtmi, 64, 40, 8)
        fresh.camera(*MOVED)
        want = _scan(rtmi, "stale_moved", fresh)
        assert not np.array_equal(want, _scans["stale_first"])
        assert np.array_equal(sc.render(rtmi.Opts(seed=SEED, variant=v)), want), f"variant {v}: a stale table after camera()"
        sc.override(width=100, height=52)
        fresh.override(width=100, height=52)
        want = _scan(rtmi, "stale_resized", fresh)
        assert np.array_equal(sc.render(rtmi.Opts(seed=SEED, variant=v)), want), f"variant {v}: a stale table after override()"
        # two frames of a camera that moves, on one scene object, against fresh scenes
        for k, eye in enumerate(((9.0, 2.0, 7.0), (8.5, 2.2, 7.5))):
            sc.camera(eye, (0, 0.5, 0), (0, 1, 0), 30.0, 0.0, 0.1, 10.0)
            fresh = _layer(rtmi, 100, 52, 8, eye=eye)
            assert np.array_equal(sc.render(rtmi.Opts(seed=SEED, variant=v)), _scan(rtmi, ("frames", k), fresh)), f"variant {v}: frame {k}"


def test_device_buffer_entry_point_on_a_callers_stream(rtmi):
    import torch
    stream = torch.cuda.Stream()
    for v in (2, 6):
        sc = rtmi.Scene.rtiow(7, 100, 52, 8, 50)
        scan = _scan(rtmi, ("roulette", 0.0), sc)
        with torch.cuda.stream(stream):
            out = torch.full((52, 100, 3), float("nan"), dtype=torch.float32, device="cuda")
            sc.render_device(rtmi.Opts(seed=SEED, variant=v), out.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(out.cpu().numpy(), scan), f"variant {v}"
        # ... and after the camera moved, on the same stream: the table is rebuilt in stream order
        moved = sc.clone()
        moved.camera((-13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0, 1, 0), 20.0, 0.0, 0.1, 10.0)
        want = _scan(rtmi, "stream_moved", moved)
        sc.camera((-13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0, 1, 0), 20.0, 0.0, 0.1, 10.0)
        with torch.cuda.stream(stream):
            sc.render_device(rtmi.Opts(seed=SEED, variant=v), out.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), f"variant {v}: after camera()"
