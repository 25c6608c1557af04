#!/usr/bin/env python3
"""Motion-blur probe of DESIGN 7g (MI355X): the fixed price of the movers' loop and the shipped scene.
usage: tools/gpu_motion.py [--width 1280] [--height 720] [--reps 5]
Fixed price: tests/media_scenes.mixed_scene with 1, 8 and 64 movers buried under its opaque floor (no ray reaches them: the
frame's bytes are the plain scene's) through the motion kernel of each layout, against the plain EXT kernel of that layout
(RTMI_FORCE_EXT) on the scene without movers, alternating, rt_stats.kernel_ms, median and minimum of --reps.
Shipped scene: scenes/motion_balls.json with and without its movers."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("RTMI_FORCE_EXT", "1")  # (the plain side runs the EXT twin of its layout, as the motion kernels are EXT)
from __graft_entry__ import load_package  # noqa: E402


def ms(rtmi, sc, variant, reps, seed=7):
    st = rtmi.Stats()
    out = []
    for _ in range(reps):
        sc.render(rtmi.Opts(seed=seed, variant=variant), st)
        out.append(st.kernel_ms)
    return out, st.kernel_variant


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rtmi = load_package()
    import media_scenes as MS
    import motion_scenes as MO
    fmt = lambda v: f"median {statistics.median(v):8.3f} ms, min {min(v):8.3f} ms"
    plain = MS.mixed_scene(rtmi, w=a.width, h=a.height, spp=16)
    scenes = {}
    for n in (1, 8, 64):
        scenes[n] = MS.mixed_scene(rtmi, w=a.width, h=a.height, spp=16)
        MO.bury_mover_mixed(scenes[n], n)
    for variant in (36, 44, 16):
        ms(rtmi, plain, variant, 1)  # (warm-up: tables, first launch)
        rows = {k: [] for k in ("plain", 1, 8, 64)}
        for _ in range(a.reps):  # alternating
            rows["plain"] += ms(rtmi, plain, variant, 1)[0]
            for n in (1, 8, 64):
                t, kv = ms(rtmi, scenes[n], variant, 1)
                assert kv == variant | 4096, kv
                rows[n] += t
        base = statistics.median(rows["plain"])
        print(f"layout {variant}: plain EXT {fmt(rows['plain'])}")
        for n in (1, 8, 64):
            print(f"layout {variant}: {n:2d} buried movers {fmt(rows[n])}  ({100 * (statistics.median(rows[n]) / base - 1):+.1f} %)")
    sc = rtmi.Scene.load(os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "motion_balls.json"))
    sc.override(width=a.width, height=a.height)
    still = sc.clone()
    still.clear_moving_spheres()
    ms(rtmi, sc, 0, 1)
    t_m, kv_m = ms(rtmi, sc, 0, a.reps)
    t_s, kv_s = ms(rtmi, still, 0, a.reps)
    print(f"motion_balls.json {a.width}x{a.height} x {sc.spp} spp: with movers (variant {kv_m}) {fmt(t_m)}; without (variant {kv_s}) {fmt(t_s)}")


if __name__ == "__main__":
    main()
