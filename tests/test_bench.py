"""Checks of bench.py.  CPU side: the rank launcher's refusal path, the flop accounting constants, the CPU-baseline leg
(the only part of bench.py that may use oracle/) and --dump-outputs' cap.  GPU: a plain run and a --full run."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_gpus_n_without_launcher_refuses_fewer_devices():
    """`python bench.py --gpus N` starts N ranks itself; with fewer than N GPUs it must fail, not fall back to one."""
    import torch
    n = torch.cuda.device_count() + 1
    if n < 2:
        n = 2
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n)], capture_output=True, text=True,
                       env=env, timeout=300)
    assert p.returncode != 0
    assert "GPU(s) visible" in p.stderr and "refusing" in p.stderr
    assert p.stdout.strip() == ""  # no JSON line that could be mistaken for a measurement


def test_tiles_abi_mode_refuses_fewer_devices():
    """`bench.py --tiles-abi --gpus N` (one process, rt_render_hip_tiles) on fewer than N devices: an error, no JSON line."""
    import torch
    n = max(2, torch.cuda.device_count() + 1)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--tiles-abi", "--gpus", str(n)], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode != 0 and "refusing" in p.stderr and p.stdout.strip() == ""


def test_world_size_mismatch_is_an_error():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert p.returncode != 0 and "WORLD_SIZE=1" in (p.stderr + p.stdout)


def test_flop_accounting_follows_survey_8d():
    b = _bench()
    # compares / selects / min / max count 0: the slab test is its 6 fma
    assert b.F_BOX == 12 and b.F_TEST[0] == 17 and b.F_SAMPLE == 46 and b.F_HIT == 30 and b.F_MISS == 25
    counts = {"samples": 10, "queries": 27, "hits": 17, "misses": 10, "scatter": [9, 4, 3, 1]}
    prim_types = [0] * 5 + [1, 4]
    want = 46 * 10 + (5 * 17 + 9 + 60) * 27 + 30 * 17 + 40 * 9 + 55 * 4 + 65 * 3 + 25 * 10
    assert b.algorithmic_flops(counts, prim_types) == want
    # cluster-box kernel: prefix + own clusters' spheres; every outer box + the cluster boxes of visited groups
    c = {"queries": 640, "cull_prefix": 4, "lane_clusters": 1000, "cull_cluster_size": 16, "cull_groups": 8,
         "groups_visited": 30}
    s, bx, setup = b.executed_tests(c, lanes=64.0)
    assert s == 640 * 4 + 1000 * 16 and bx == 640 * 8 + 64 * 30 * 4 and setup == b.F_CULL_SETUP * 640
    # uniform grid (the default): one bounds clip per query, one sphere test per list entry of the cells a lane visits
    c = {"queries": 640, "cull_prefix": 4, "lane_clusters": 1800, "cull_cluster_size": 8, "cull_mode": 5, "cull_windows": 1,
         "lane_cands": 450, "lane_groups": 470}
    s, bx, setup = b.executed_tests(c, lanes=64.0)
    assert s == 640 * 4 + 1800 and bx == 640 and setup == b.F_GRID_SETUP * 640 + b.F_GRID_ENTER * 470 + b.F_GRID_STEP * 450
    # range tables: one window-box clip per query and window, one box test per candidate cluster
    c = {"queries": 640, "cull_prefix": 4, "lane_clusters": 1200, "cull_cluster_size": 8, "cull_mode": 3, "cull_windows": 1,
         "lane_cands": 2000, "lane_groups": 470}
    s, bx, setup = b.executed_tests(c, lanes=64.0)
    assert s == 640 * 4 + 1200 * 8 and bx == 640 + 2000 and setup == b.F_CULL_SETUP * 640 + b.F_RANGE_LOOKUP * 470


def test_cpu_baseline_leg_runs_on_all_cores(rtmi):
    b = _bench()
    args = b.parse_args(["--width", "96", "--height", "64", "--cpu-spp", "2", "--depth", "50"])
    r = b.cpu_baseline(rtmi, args)
    assert r["affinity_cores"] == len(os.sched_getaffinity(0)) and r["nproc"] == os.cpu_count()
    q = b.cgroup_cpu_quota()
    assert r["cores"] == (r["affinity_cores"] if q is None else max(1, min(r["affinity_cores"], int(q + 0.999))))
    assert r["value"] > 0 and r["unit"] == "Msamples/s" and r["kind"] in ("reference", "port")
    legs = r["legs"]
    assert legs["iii_restatement_all_cores"]["Msamples_per_s"] > 0
    if r["kind"] == "reference":
        assert legs["ii_reference_all_cores"]["samples"] == 96 * 16 * 2  # rows 0-7 and 32-39 of 64
        assert "sampling_spread" in legs["ii_reference_all_cores"]
        if "error" not in legs.get("i_stock_single_thread", {"error": 1}):
            assert legs["i_stock_single_thread"]["Msamples_per_s_per_core"] > 0


def test_plain_run_is_lean_by_default():
    """The extra legs are behind --full; --dump-outputs is off unless given."""
    b = _bench()
    a = b.parse_args([])
    assert not a.full and a.dump_outputs is None
    a = b.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_caps_with_a_fixed_row_sample(tmp_path, monkeypatch):
    import numpy as np
    b = _bench()
    img = np.arange(40 * 7 * 3, dtype=np.float32).reshape(40, 7, 3)
    b.dump_outputs(str(tmp_path / "whole"), np, rgb_sum=img)
    np.testing.assert_array_equal(np.load(tmp_path / "whole" / "rgb_sum.npy"), img)
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 10 * 7 * 3 * 4)
    b.dump_outputs(str(tmp_path / "a"), np, rgb_sum=img)
    b.dump_outputs(str(tmp_path / "b"), np, rgb_sum=img)
    got = np.load(tmp_path / "a" / "rgb_sum.npy")
    assert got.shape == (10, 7, 3) and got.dtype == np.float32
    np.testing.assert_array_equal(got, np.load(tmp_path / "b" / "rgb_sum.npy"))
    rows = got[:, 0, 0].astype(np.int64) // 21
    assert list(rows) == sorted(set(rows)) and all(np.array_equal(img[r], g) for r, g in zip(rows, got))


def _bench_line(args, timeout=600):
    import json
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_frame(rtmi, tmp_path):
    """A plain run: the headline fields only, --steps timed steps, and DIR/rgb_sum.npy equal to the unsharded frame."""
    import numpy as np
    small = ["--width", "96", "--height", "54", "--spp", "8"]
    r = _bench_line(["--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)] + small)
    assert r["steps"] == 2 and r["ms_per_step"] > 0 and r["unit"] == "Msamples/s" and r["higher_is_better"] is True
    assert r["dtype"] == "f32" and r["value"] > 0
    assert not {"roofline", "roofline_linear_scan", "extra", "cpu_baseline"} & set(r)
    got = np.load(tmp_path / "rgb_sum.npy")
    want = rtmi.Scene.rtiow(7, 96, 54, 8, 50).render(rtmi.Opts(seed=2023))
    assert got.dtype == np.float32 and got.shape == (54, 96, 3)
    np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
def test_full_run_keeps_the_roofline_legs():
    r = _bench_line(["--gpus", "1", "--steps", "1", "--warmup", "0", "--full", "--no-extra", "--no-cpu-baseline",
                     "--width", "96", "--height", "54", "--spp", "8"])
    assert r["roofline"]["flops_per_launch"] > 0 and r["roofline_linear_scan"]["kernel_variant"] == 16
