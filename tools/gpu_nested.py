#!/usr/bin/env python3
"""Nested-grid probe (MI355X): ms per frame of the room scenes (a 160 x 160 height field of side S in a 20-unit room, the
fixture of tests/test_nested_grid.py) with the nested grid off and on, the counters that explain the difference, and a sweep
of the packer's two numbers (RTMI_NEST_OVER: a cell with more entries is nested; RTMI_NEST_CAP: cells per axis of a sub-grid).
usage: tools/gpu_nested.py [--width 1280] [--height 720] [--spp 16] [--reps 3] [--sides 1,2,20] [--budget-s 120] [--sweep]
Timing: kernel_ms of one frame (device events), best of --reps after one warm-up frame.  A configuration whose frame is
estimated from a 1/16-size frame to take more than --budget-s is reported by that estimate ("ms_estimated")."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402


def measure(rtmi, a, side, on):
    from test_nested_grid import room
    sc = room(rtmi, 160, side, w=a.width // 4, h=a.height // 4, spp=a.spp)
    sc.set_nested_grid(on)
    t, ni = sc.table_info(), sc.nested_info()
    row = {"side": side, "nested_grid": on, "kernel_variant": t.kernel_variant, "nt_a": t.nt_a, "nested_cells": ni.cells,
           "sub_cells": ni.sub_cells, "longest_list": ni.longest, "threshold": ni.threshold, "axis_cap": ni.axis_cap,
           "image_mib": round(t.image_floats * 4 / 2 ** 20, 1)}
    st = rtmi.Stats()
    sc.render(rtmi.Opts(seed=1), st)  # (warm-up: upload, first launch)
    sc.render(rtmi.Opts(seed=1), st)
    small_ms = st.kernel_ms
    c = sc.count(rtmi.Opts(seed=1, tile_rows=8, tile_first=a.height // 64, tile_stride=100000))
    always = t.np + t.nr_a + t.nc_a + t.nt_a
    row["examined_per_query"] = round(c.lane_clusters / max(1, c.queries) + always, 1)
    row["cell_steps_per_query"] = round(c.lane_cands / max(1, c.queries), 1)
    if small_ms * 16 > a.budget_s * 1e3:
        row["ms_estimated"] = round(small_ms * 16, 1)
        return row
    sc.override(a.width, a.height, a.spp)
    ms = []
    for r in range(a.reps + 1):
        sc.render(rtmi.Opts(seed=r), st)
        ms.append(st.kernel_ms)
    row["ms"] = round(min(ms[1:]), 2)
    row["ms_all"] = [round(x, 2) for x in ms[1:]]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sides", default="1,2,20")
    ap.add_argument("--budget-s", type=float, default=120.0)
    ap.add_argument("--sweep", action="store_true", help="RTMI_NEST_OVER x RTMI_NEST_CAP on the nested rooms (one child process each)")
    ap.add_argument("--only-on", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    sides = [float(x) for x in a.sides.split(",")]
    if a.sweep:
        for over in (32, 64, 128, 256):
            for cap in (16, 32, 64):
                env = dict(os.environ, RTMI_NEST_OVER=str(over), RTMI_NEST_CAP=str(cap))
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-on", "--width", str(a.width), "--height", str(a.height),
                                    "--spp", str(a.spp), "--reps", str(a.reps), "--sides", ",".join(str(s) for s in sides if s < 20)],
                                   env=env, timeout=600)
                if p.returncode != 0:  # (a failed child ends the sweep: nothing more is started on the device)
                    raise SystemExit(p.returncode)
        return
    rtmi = load_package()
    for side in sides:
        for on in ((True,) if a.only_on else ((False,) if side >= 20 else (False, True))):
            print(json.dumps(measure(rtmi, a, side, on)), flush=True)


if __name__ == "__main__":
    main()
