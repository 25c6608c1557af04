"""Row-tile shards (rt_opts tile_*), host-side scatter, and the world_size-2 gather (gloo)."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from rtcheck import tile_owner


def test_shard_geometry(rtmi, scenes_dir):
    sc = rtmi.Scene.load(os.path.join(scenes_dir, "three_sphere.json"))
    sc.override(width=32, height=45, spp=1)  # 45 rows: 5 full tiles of 8 + one of 5
    assert sc.shard_rows() == 45
    np.testing.assert_array_equal(sc.shard_global_rows(), np.arange(45))
    seen = []
    for world in (2, 3, 8):
        allrows = []
        for r in range(world):
            rows = sc.shard_global_rows(rtmi.Opts(tile_first=r, tile_stride=world))
            # tile t -> rank t mod world, rows of a tile stay together and ascending
            assert (tile_owner(np.asarray(rows) // 8, world, 0) == r).all()
            assert list(rows) == sorted(rows)
            allrows += list(rows)
        assert sorted(allrows) == list(range(45))
        seen.append(world)
    # the rotated interleave (rt_opts.tile_rotate = 1; what rt_render_hip_tiles and bench.py use for frames of >= 4 N^2
    # tiles): tile t -> rank (t + t // world) mod world -- one tile of every group of `world` tiles per rank, a different one
    # from group to group
    for world in (2, 3, 4, 8):
        allrows, counts = [], []
        for r in range(world):
            o = rtmi.Opts(tile_first=r, tile_stride=world, tile_rotate=1)
            rows = sc.shard_global_rows(o)
            t = np.asarray(rows) // 8
            assert np.array_equal(tile_owner(t, world, 1), np.full(len(rows), r))
            assert list(rows) == sorted(rows) and sc.shard_rows(o) == len(rows)
            if len(set(t)) > 1:
                assert len(set(t % world)) > 1                      # not one row phase for itself
            allrows += list(rows)
            counts.append(len(set(t)))
        assert sorted(allrows) == list(range(45)) and max(counts) - min(counts) <= 1
    # there and back (tile_rotate = 2): groups of 2 * world tiles go to ranks 0 .. world-1, then world-1 .. 0
    for world in (2, 3, 4, 8):
        allrows, counts = [], []
        for r in range(world):
            o = rtmi.Opts(tile_first=r, tile_stride=world, tile_rotate=2)
            rows = sc.shard_global_rows(o)
            t = np.asarray(rows) // 8
            assert np.array_equal(tile_owner(t, world, 2), np.full(len(rows), r))
            assert list(rows) == sorted(rows) and sc.shard_rows(o) == len(rows)
            allrows += list(rows)
            counts.append(len(set(t)))
        assert sorted(allrows) == list(range(45)) and max(counts) - min(counts) <= 1
    with pytest.raises(rtmi.RtmiError):
        sc.shard_rows(rtmi.Opts(tile_first=0, tile_stride=2, tile_rotate=3))
    # which deal rt_render_hip_tiles and bench.py use: rotated once the frame has 4 N^2 tiles, else there and back
    big = rtmi.Scene.rtiow(7, 64, 1080, 1, 5)
    assert [big.shard_deal(None, n) for n in (1, 2, 4, 8)] == [0, 1, 1, 2]
    assert sc.shard_deal(rtmi.Opts(tile_rows=1), 3) == 1 and sc.shard_deal(None, 3) == 2   # 45 rows: 45 tiles of 1 row, 6 of 8
    # tile_rows other than 8, partial last tile
    rows = sc.shard_global_rows(rtmi.Opts(tile_rows=16, tile_first=1, tile_stride=2))
    assert list(rows) == list(range(16, 32))
    rows = sc.shard_global_rows(rtmi.Opts(tile_rows=16, tile_first=0, tile_stride=2))
    assert list(rows) == list(range(0, 16)) + list(range(32, 45))
    # a rank beyond the last tile owns nothing
    assert sc.shard_rows(rtmi.Opts(tile_rows=32, tile_first=5, tile_stride=8)) == 0
    with pytest.raises(rtmi.RtmiError):
        sc.shard_rows(rtmi.Opts(tile_first=3, tile_stride=2))


@pytest.mark.parametrize("world", range(2, 9))
def test_shard_deal_partitions_the_frame(rtmi, scenes_dir, world):
    """rt_shard_deal on either side of its threshold (4 N^2 tiles of 8 rows; each side once with a ragged last tile): the deal
    it picks, and for that deal the ranks' rows partition the frame, ascend within a rank, and lie on the tiles tile_owner
    gives the rank."""
    edge = 4 * world * world
    for tiles, short in ((edge - 1, 0), (edge - 1, 3), (edge, 0), (edge, 5)):
        h = tiles * 8 - short
        sc = rtmi.Scene.load(os.path.join(scenes_dir, "three_sphere.json"))
        sc.override(width=8, height=h, spp=1)
        deal = sc.shard_deal(rtmi.Opts(tile_rows=8), world)
        assert deal == (1 if tiles >= edge else 2)
        allrows = []
        for r in range(world):
            rows = sc.shard_global_rows(rtmi.Opts(tile_rows=8, tile_first=r, tile_stride=world, tile_rotate=deal))
            assert (np.diff(rows) > 0).all()
            assert (tile_owner(rows // 8, world, deal) == r).all()
            allrows.append(rows)
        assert np.array_equal(np.sort(np.concatenate(allrows)), np.arange(h))


def test_host_scatter_rows(rtmi, scenes_dir):
    sc = rtmi.Scene.load(os.path.join(scenes_dir, "three_sphere.json"))
    sc.override(width=16, height=21, spp=1)
    full = np.arange(21 * 16 * 3, dtype=np.float32).reshape(21, 16, 3)
    out = np.zeros_like(full)
    for r in range(3):
        o = rtmi.Opts(tile_rows=4, tile_first=r, tile_stride=3)
        rows = sc.shard_global_rows(o)
        sc.scatter_rows(o, full[rows], out)
    np.testing.assert_array_equal(out, full)


def _worker(rank, world, port, height, tile_rows, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    from __graft_entry__ import load_package
    rtmi = load_package()
    import importlib
    rdist = importlib.import_module("rtmi.dist")
    import rtcheck
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sc = rtmi.Scene.load(os.path.join(root, "ray-tracing-in-cuda_amd", "scenes", "three_sphere.json"))
        sc.override(width=24, height=height, spp=2)
        # stand-in for the GPU render of this rank's rows (CPU test): the checker's image rows
        full_ref, _ = rtcheck.oracle_render(sc, seed=11, threads=1)
        frames = [full_ref, full_ref * 2.0 + 1.0]
        ok = True
        # every deal of the tiles (rt_opts.tile_rotate), one after the other on the same scene
        for deal in (0, 1, 2):
            base = rtmi.Opts(seed=11, tile_rows=tile_rows, tile_rotate=deal)
            rows = sc.shard_global_rows(rdist.shard_opts(base, rank, world))
            local = rdist.alloc_local(sc, base, world, "cpu")
            local[: len(rows)] = torch.from_numpy(full_ref[rows])
            full = rdist.gather_framebuffer(local, sc, base, rank, world)
            if rank == 0:
                ok = ok and bool(np.array_equal(full.numpy(), full_ref))
            else:
                assert full is None
            # the two-phase form bench.py pipelines (a frame's gather travels while the next frame renders): two frames in
            # flight in two local buffers and two receive slots, placed in order
            bufs = [rdist.alloc_local(sc, base, world, "cpu") for _ in range(2)]
            pend = []
            for i in range(2):
                bufs[i][: len(rows)] = torch.from_numpy(frames[i][rows])
                pend.append(rdist.gather_begin(bufs[i], rank, world, slot=i))
            for i in range(2):
                got = rdist.gather_end(pend[i], sc, base, rank, world, bufs[i].shape[0], "cpu")
                if rank == 0:
                    ok = ok and bool(np.array_equal(got.numpy(), frames[i]))
                else:
                    assert got is None
        if rank == 0:
            q.put(ok)
    finally:
        dist.destroy_process_group()


def _gather_gloo(world, height, tile_rows):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + height + tile_rows) % 2000
    procs = [ctx.Process(target=_worker, args=(r, world, port, height, tile_rows, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert q.get(timeout=5) is True


@pytest.mark.parametrize("height,tile_rows", [(32, 8), (29, 8), (20, 4)])
def test_gather_world2_gloo(height, tile_rows):
    _gather_gloo(2, height, tile_rows)


def test_gather_world3_gloo():
    """6 tiles of 8 rows (the last one 5), which deals 0, 1 and 2 give to the 3 ranks in three different ways (at world 2
    deals 1 and 2 coincide)."""
    _gather_gloo(3, 45, 8)


def test_gather_world1_no_comm(rtmi, scenes_dir):
    import importlib
    rdist = importlib.import_module("rtmi.dist")
    sc = rtmi.Scene.load(os.path.join(scenes_dir, "three_sphere.json"))
    sc.override(width=8, height=10, spp=1)
    base = rtmi.Opts()
    local = torch.arange(10 * 8 * 3, dtype=torch.float32).reshape(10, 8, 3)
    full = rdist.gather_framebuffer(local, sc, base, 0, 1)
    assert torch.equal(full, local)
