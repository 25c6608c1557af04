#!/usr/bin/env python3
"""The table of DESIGN.md section 7i (needs a GPU): hipEvent times of the display stage's kernels -- prepare, the reduction of
auto exposure, every blur level (horizontal + vertical pass) and finish -- on a synthetic HDR frame, at 160x90 and 1920x1080,
with bloom off and with bloom on at 5 levels, and the stage as a share of the denoiser's 0.47 ms and of the 119.7 ms headline
frame (both at 1080p).  Both outputs are written.  Every row is the SECOND call of its configuration (buffers and code objects are there), the best of
--repeat such calls.
usage: tools/gpu_display.py [--sizes 160x90,1920x1080] [--levels 5] [--repeat 5]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

rtmi = load_package()
DENOISE_MS, HEADLINE_MS = 0.47, 119.7  # DESIGN 7d (1080p), the headline frame of bench.py


def frame(w, h, spp):
    rng = np.random.default_rng(7)
    mean = np.exp(3.0 * rng.standard_normal((h, w, 3), dtype=np.float32))
    mean[h // 2, w // 2] = 3e4
    return np.ascontiguousarray(mean * np.float32(spp))


def timed(img, spp, repeat, **kw):
    """per-kernel ms of the best (by total) of `repeat` calls after a first one"""
    st = rtmi.DisplayStats()
    rtmi.display(img, spp, stats=st, **kw)  # both outputs: finish writes the float frame and the bytes
    best = None
    for _ in range(repeat):
        rtmi.display(img, spp, stats=st, **kw)
        t = rtmi.display_timing()
        if best is None or sum(t) < sum(best):
            best = t
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="160x90,1920x1080")
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    spp = 16
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        img = frame(w, h, spp)
        full = (w, h) == (1920, 1080)
        for name, kw in (("bloom off", {}), (f"bloom on, {a.levels} levels", dict(bloom_strength=0.5, bloom_threshold=1.0, bloom_levels=a.levels))):
            for auto in (False, True):
                t = timed(img, spp, a.repeat, tonemap="aces", exposure=0.5, auto_key=0.18 if auto else 0.0, **kw)
                parts, total = [], sum(t)
                if auto:
                    parts.append(f"reduce {t[0]:.4f}")
                    t = t[1:]
                parts.append(f"prepare {t[0]:.4f}")
                for k in range((len(t) - 2) // 2):
                    parts.append(f"blur{k} {t[1 + 2 * k]:.4f}+{t[2 + 2 * k]:.4f}")
                parts.append(f"finish {t[-1]:.4f}")
                share = f" = {100 * total / DENOISE_MS:.0f} % of the denoiser, {100 * total / HEADLINE_MS:.2f} % of the headline frame" if full else ""
                print(f"{w}x{h} {name}{', auto exposure' if auto else ''}: total {total:.4f} ms{share}\n    " + "  ".join(parts), flush=True)


if __name__ == "__main__":
    main()
