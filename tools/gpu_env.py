#!/usr/bin/env python3
"""Environment-map probe (MI355X): ms per frame and per-pixel noise, plain against light sampling, for the example scene under
its sun map and for a shipped scene under a uniform map.
usage: tools/gpu_env.py [--width 1280] [--height 720] [--spp N (default: the scene's)] [--seeds 4] [--noise-size 160x90]
Timing: one frame at --width x --height per mode (best of --reps).  Noise: --seeds renders per mode at the small size; the
per-pixel standard deviation of the pixel means across seeds, as the median over lit pixels relative to the pixel mean."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

SCENES = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes")


def cases(rtmi):
    yield "env_sun (sun map)", rtmi.Scene.load(os.path.join(SCENES, "env_sun.json"))
    sc = rtmi.Scene.load(os.path.join(SCENES, "mixed_emissive.json"))
    sc.set_environment(np.full((8, 16, 3), 0.5, np.float32))
    yield "mixed_emissive (uniform map 0.5)", sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--noise-size", default="160x90")
    a = ap.parse_args()
    rtmi = load_package()
    nw, nh = (int(x) for x in a.noise_size.split("x"))
    for name, sc in cases(rtmi):
        row = {"scene": name}
        spp = a.spp or sc.spp
        for nee in (False, True):
            tag = "nee" if nee else "plain"
            sc.override(a.width, a.height, spp)
            sc.set_light_sampling(nee)
            ms = []
            for r in range(a.reps):
                st = rtmi.Stats()
                sc.render(rtmi.Opts(seed=r), st)
                ms.append(st.kernel_ms)
            row[f"ms_{tag}"] = round(min(ms), 2)
            row[f"kernel_variant_{tag}"] = st.kernel_variant
            sc.override(nw, nh, spp)
            m = np.stack([sc.render(rtmi.Opts(seed=100 + s)).astype(np.float64).mean(axis=2) / spp for s in range(a.seeds)])
            mean, sd = m.mean(axis=0), m.std(axis=0, ddof=1)
            lit = mean > 1e-4
            row[f"rel_noise_{tag}"] = round(float(np.median(sd[lit] / mean[lit])), 4)
            row[f"frame_mean_{tag}"] = round(float(m.mean()), 5)
        row["spp"] = spp
        ratio = (row["rel_noise_plain"] / max(row["rel_noise_nee"], 1e-12)) ** 2
        row["variance_ratio"] = round(ratio, 2)
        row["equal_noise_speedup"] = round(row["ms_plain"] / (row["ms_nee"] / ratio), 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
