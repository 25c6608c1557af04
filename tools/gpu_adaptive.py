#!/usr/bin/env python3
"""Adaptive sampling probe (MI355X): what rt_render_hip_adaptive buys at equal error, scene by scene.
usage: tools/gpu_adaptive.py [--thresholds 0.03,0.1] [--min-spp 16] [--reps 2] [--only NAME]
For each scene: the plain frame time at max_spp and the adaptive frame time at each threshold (full size, best of --reps,
hipEvent kernel time of the call: render + estimate kernels and the per-pass read-back), the pixel samples rendered; then,
on a 1/4-size frame (same scene and thresholds), the RMSE of the mean image against a plain render at 4 x max_spp (another
seed), for adaptive and for plain at max_spp / 4, / 2, / 1.  The equal-error speed-up: plain's RMSE is interpolated in
log-log over those three spp to the spp where it matches adaptive's, plain's time is scaled to that spp (time ~ spp), and
divided by adaptive's time.  Below 1: adaptive loses."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "scenes_as_shipped")
MIXED = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "mixed_emissive.json")

# name, how to load, full-size frame, max_spp, light sampling
CASES = [
    ("sample_scene", lambda r: r.Scene.load(os.path.join(GOLDEN, "sample_scene.json")), (1920, 1080), 512, False),
    ("blue", lambda r: r.Scene.load(os.path.join(GOLDEN, "blue.json")), (1280, 720), 2000, False),
    ("mixed_emissive", lambda r: r.Scene.load(MIXED), (1280, 720), 512, False),
    ("mixed_emissive_nee", lambda r: r.Scene.load(MIXED), (1280, 720), 512, True),
    ("rtiow", lambda r: r.Scene.rtiow(7, 1920, 1080, 1024, 50), (1920, 1080), 1024, False),
]


def mean_image(img, spp):
    return img.astype(np.float64) / (spp[..., None] if isinstance(spp, np.ndarray) else float(spp))


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--thresholds", default="0.03,0.1")
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    rtmi = load_package()
    thresholds = [float(t) for t in a.thresholds.split(",")]
    for name, load, (W, H), max_spp, nee in CASES:
        if a.only and name != a.only:
            continue
        sc = load(rtmi)
        sc.set_light_sampling(nee)
        row = {"scene": name, "size": f"{W}x{H}", "max_spp": max_spp, "nee": nee}
        # ---- time, full size
        sc.override(W, H, max_spp)
        ms = []
        for r in range(a.reps):
            st = rtmi.Stats()
            sc.render(rtmi.Opts(seed=1 + r), st)
            ms.append(st.kernel_ms)
        row["plain_ms"] = round(min(ms), 2)
        full = W * H * max_spp
        for t in thresholds:
            ms = []
            for r in range(a.reps):
                _, spp, ast = sc.render_adaptive(t, min_spp=a.min_spp, max_spp=max_spp, opts=rtmi.Opts(seed=1 + r))
                ms.append(ast.kernel_ms)
            row[f"T{t}"] = {"ms": round(min(ms), 2), "samples_frac": round(ast.samples / full, 4), "passes": ast.passes,
                            "active": list(ast.active[:ast.passes])}
        # ---- error, 1/4 size
        w, h = W // 4, H // 4
        sc.override(w, h, 4 * max_spp)
        ref = mean_image(sc.render(rtmi.Opts(seed=999)), 4 * max_spp)
        errs = {}
        for f in (4, 2, 1):
            n = max_spp // f
            errs[n] = rmse(mean_image(sc.render(rtmi.Opts(seed=1, sample_count=n)), n), ref)
        row["plain_rmse"] = {str(n): round(e, 6) for n, e in errs.items()}
        ns = np.array(sorted(errs)), np.array([errs[n] for n in sorted(errs)])
        slope = np.polyfit(np.log(ns[0]), np.log(ns[1]), 1)  # log rmse = slope[0] log spp + slope[1]
        row["plain_rmse_slope"] = round(float(slope[0]), 3)
        for t in thresholds:
            img, spp, ast = sc.render_adaptive(t, min_spp=a.min_spp, max_spp=max_spp, opts=rtmi.Opts(seed=1))
            e = rmse(mean_image(img, spp), ref)
            spp_eq = float(np.exp((np.log(e) - slope[1]) / slope[0])) if slope[0] < 0 else float("nan")
            d = row[f"T{t}"]
            d["rmse"] = round(e, 6)
            d["small_samples_frac"] = round(ast.samples / (w * h * max_spp), 4)
            d["plain_spp_at_equal_rmse"] = round(spp_eq, 1)
            d["equal_error_speedup"] = round(row["plain_ms"] * spp_eq / max_spp / d["ms"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
