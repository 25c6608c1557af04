#!/usr/bin/env python3
"""The table of DESIGN.md section 7d (needs a GPU): per scene, the ms of the three feature passes and of the filter, and the RMSE
of the mean image before and after denoising against a render at 4 x spp (or --ref-spp) with another seed.
usage: tools/gpu_denoise.py [--width 160 --height 90 --spp 16 --ref-spp 4096] [--sweep]
--sweep tries a grid of (iterations, sigma_color, sigma_normal, sigma_depth) and prints the best rows by mean RMSE ratio."""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

rtmi = load_package()
SCENES = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes")
GOLDEN = os.path.join(ROOT, "tests", "golden", "scenes")


def scenes(w, h, spp):
    def mixed(n):
        sc = rtmi.Scene.load(os.path.join(SCENES, "mixed_emissive.json"))
        sc.override(w, h, n)
        sc.set_light_sampling(True)
        return sc

    def sample(n):
        sc = rtmi.Scene.load(os.path.join(GOLDEN, "sample_scene.json"))
        sc.override(w, h, n)
        return sc

    return [("mixed_emissive+nee", mixed), ("rtiow", lambda n: rtmi.Scene.rtiow(7, w, h, n, 50)), ("sample_scene", sample)]


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--height", type=int, default=90)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=0)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    ref_spp = a.ref_spp or 4 * a.spp
    frames = []
    for name, make in scenes(a.width, a.height, a.spp):
        ref = make(ref_spp).render(rtmi.Opts(seed=99)).astype(np.float64) / ref_spp
        sc = make(a.spp)
        st = rtmi.Stats()
        img = sc.render(rtmi.Opts(seed=2023), st)
        render_ms = st.kernel_ms
        feats, feat_ms = [], 0.0
        for f in range(3):
            feats.append(sc.render_feature(f, rtmi.Opts(seed=2023), st))
            feat_ms += st.kernel_ms
        t = []
        out = rtmi.denoise(img, a.spp, *feats, a.spp, timing=t)
        out = rtmi.denoise(img, a.spp, *feats, a.spp, timing=t)  # (second call: buffers and code objects are there)
        before, after = rmse(img / np.float32(a.spp), ref), rmse(out / np.float32(a.spp), ref)
        print(f"{name:20s} {a.width}x{a.height}x{a.spp}: render {render_ms:7.3f} ms, features {feat_ms:6.3f} ms, filter {t[1]:6.3f} ms, "
              f"RMSE vs {ref_spp} spp {before:.5f} -> {after:.5f} (x{after / before:.3f})", flush=True)
        frames.append((name, img, feats, ref, before))
    if not a.sweep:
        return
    rows = []
    for it, sc_, sn, sd in itertools.product((2, 3, 4, 5), (0.125, 0.25, 0.5, 1.0, 2.0, 4.0), (0.125, 0.25, 0.5), (0.05, 0.2, 1.0)):
        ratios = []
        for name, img, feats, ref, before in frames:
            out = rtmi.denoise(img, a.spp, *feats, a.spp, iterations=it, sigma_color=sc_, sigma_normal=sn, sigma_depth=sd)
            ratios.append(rmse(out / np.float32(a.spp), ref) / before)
        rows.append((float(np.mean(ratios)), it, sc_, sn, sd, ratios))
    rows.sort()
    print("mean ratio  iterations sigma_color sigma_normal sigma_depth   per scene")
    for r in rows[:25] + rows[-3:]:
        print(f"{r[0]:.4f}      {r[1]}          {r[2]:<8g}    {r[3]:<8g}     {r[4]:<8g}      " + " ".join(f"{x:.3f}" for x in r[5]))


if __name__ == "__main__":
    main()
