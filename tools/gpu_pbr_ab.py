#!/usr/bin/env python3
"""What the metallic-roughness material costs the scenes that do not use it, this tree against another tree (the
parent commit, built), alternating on one machine, and what pbr_wear.json costs:
    tools/gpu_pbr_ab.py OTHER_TREE [rounds]
Each child process loads the package of ONE tree and renders, 1 warm-up + 5 timed frames each (rt_stats.kernel_ms, min and
median, CRC of the frame): the 20 000-triangle height field of tests/test_gpu_grid_all at 1280 x 720 x 16, and mixed_emissive,
cornell_box, bumpy_pond, frosted_glass, mesh_light (mesh lights on) and env_sun with light sampling, at 1280 x 720 x 16 -- the
seven scenes of 7s's table: they run the changed general (EXT) instances and hold no pbr material, so they must give the same
bytes in both trees.  The parent process prints the CRCs side by side and each scene's spread (the largest difference between
the minima of the other tree's rounds) beside the difference between the trees.
This tree's first child then renders pbr_wear.json at 1280 x 720 at its own spp with light sampling off and on, the same scene
with every pbr material replaced by plastic(base texture, ior, roughness factor) -- the price of the per-hit resolve -- and the
per-pixel noise at 160 x 90 over 4 seeds, with and without light sampling (the median over lit pixels of sd / mean, as
tools/gpu_nee.py computes it)."""
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH, N = 1280, 720, 16, 20, 100
SHIPPED = ("mixed_emissive", "cornell_box", "bumpy_pond", "frosted_glass", "mesh_light", "env_sun")
CHILD_LIMIT = 420  # seconds


def timed(rtmi, sc, seed=1):
    ts = []
    for k in range(6):
        st = rtmi.Stats()
        img = sc.render(rtmi.Opts(seed=seed), st)
        if k:
            ts.append(st.kernel_ms)
    ts.sort()
    return ts[0], ts[len(ts) // 2], zlib.crc32(img.tobytes()), st.kernel_variant


def as_plastic(rtmi, text):
    """the scene of the JSON text with every pbr material replaced by a plastic of its base texture, index and roughness factor"""
    d = json.loads(text)
    for k, m in enumerate(d["material"]["data"]):
        if m["type"] == "pbr":
            d["material"]["data"][k] = {"type": "plastic", "texture": m["texture"], "ior": m.get("ior", 1.5), "roughness": m["roughness"]}
    return rtmi.Scene.parse(json.dumps(d))


def child(tree, with_wear):
    import numpy as np
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from __graft_entry__ import load_package
    rtmi = load_package()
    assert os.path.abspath(rtmi.__file__).startswith(os.path.abspath(tree))
    from test_gpu_grid_all import height_field
    scenes = os.path.join(tree, "ray-tracing-in-cuda_amd", "scenes")
    rows = {"height_field": timed(rtmi, height_field(rtmi, N, W, H, SPP, depth=DEPTH))}
    for name in SHIPPED:
        sc = rtmi.Scene.load(os.path.join(scenes, name + ".json"))
        sc.override(W, H, SPP)
        sc.set_light_sampling(True)
        if name == "mesh_light":
            sc.set_mesh_lights(True)
        rows[name] = timed(rtmi, sc)
    for name, (lo, med, crc, kv) in rows.items():
        print("ROW " + json.dumps({"tree": tree, "scene": name, "min": lo, "median": med, "crc": "%08x" % crc, "variant": kv}), flush=True)
    if not with_wear:
        return
    out = {"scene": "pbr_wear"}
    text = open(os.path.join(scenes, "pbr_wear.json")).read()
    for nee in (False, True):
        for what, make in (("pbr", lambda: rtmi.Scene.parse(text)), ("plastic", lambda: as_plastic(rtmi, text))):
            tag = what + ("_nee" if nee else "_plain")
            sc = make()
            spp = sc.spp
            sc.override(W, H, spp)
            sc.set_light_sampling(nee)
            lo, med, _, kv = timed(rtmi, sc)
            out["ms_" + tag], out["variant_" + tag], out["spp"] = round(lo, 2), kv, spp
        sc = rtmi.Scene.parse(text)
        sc.override(160, 90, spp)
        sc.set_light_sampling(nee)
        m = np.stack([sc.render(rtmi.Opts(seed=100 + s)).astype(np.float64).mean(axis=2) / spp for s in range(4)])
        mean, sd = m.mean(axis=0), m.std(axis=0, ddof=1)
        lit = mean > 1e-4
        out["lit_share_" + ("nee" if nee else "plain")] = round(float(lit.mean()), 3)
        out["rel_noise_" + ("nee" if nee else "plain")] = float(np.median(sd[lit] / mean[lit]))
    print("WEAR " + json.dumps(out), flush=True)


def main():
    other, rounds = os.path.abspath(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 2
    seen = {}  # (tree, scene) -> [(min, crc)]
    for r in range(rounds):
        print("round", r, flush=True)
        for tree in (ROOT, other):
            # (each child under its own time limit; its lines are passed on as they come)
            p = subprocess.Popen(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "child", tree,
                                  "wear" if r == 0 and tree == ROOT else "-"],
                                 stdout=subprocess.PIPE, text=True)
            for line in p.stdout:
                sys.stdout.write(line)
                sys.stdout.flush()
                if line.startswith("ROW "):
                    row = json.loads(line[4:])
                    seen.setdefault((tree, row["scene"]), []).append((row["min"], row["crc"]))
            if p.wait() != 0:
                sys.exit(p.returncode)
    print("%-16s %10s %10s %9s %9s  %s" % ("scene", "this (ms)", "other (ms)", "diff", "spread", "bytes"))
    for scene in [s for (t, s) in seen if t == ROOT]:
        a, b = seen[(ROOT, scene)], seen[(other, scene)]
        mine, theirs = min(x[0] for x in a), min(x[0] for x in b)
        spread = max(x[0] for x in b) - min(x[0] for x in b)
        same = {x[1] for x in a} == {x[1] for x in b} and len({x[1] for x in a}) == 1
        print("%-16s %10.2f %10.2f %+8.2f%% %8.2f%%  %s" % (scene, mine, theirs, 100 * (mine - theirs) / theirs, 100 * spread / theirs,
                                                          "same" if same else "DIFFERENT"))
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2], sys.argv[3] == "wear")
    else:
        main()
