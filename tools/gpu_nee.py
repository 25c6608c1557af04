#!/usr/bin/env python3
"""Light sampling probe (MI355X): ms per frame and per-pixel noise of the emissive scenes with and without NEE.
usage: tools/gpu_nee.py [--width 1280] [--height 720] [--spp N (default: the scene's)] [--seeds 4] [--noise-size 160x90]
Timing: one frame at --width x --height per mode (best of --reps).  Noise: --seeds renders per mode at the small size; the
per-pixel standard deviation of the pixel means across seeds, as the median over lit pixels relative to the pixel mean,
and the spp at which NEE matches plain's noise at the scene's spp (noise ~ 1 / sqrt(spp))."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

SCENES = {
    "mixed_emissive": os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "mixed_emissive.json"),
    "blue": os.path.join(ROOT, "tests", "golden", "scenes_as_shipped", "blue.json"),
}


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
    for name, path in SCENES.items():
        row = {"scene": name}
        for nee in (False, True):
            tag = "nee" if nee else "plain"
            sc = rtmi.Scene.load(path)
            spp = a.spp or sc.spp
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
            row[f"rel_noise_{tag}"] = float(np.median(sd[lit] / mean[lit]))
            row["spp"] = spp
        ratio = (row["rel_noise_plain"] / max(row["rel_noise_nee"], 1e-12)) ** 2
        row["variance_ratio"] = round(ratio, 2)
        row["nee_spp_for_plain_noise"] = int(np.ceil(row["spp"] / ratio))
        row["equal_noise_speedup"] = round(row["ms_plain"] / (row["ms_nee"] / ratio), 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
