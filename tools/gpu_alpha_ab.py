#!/usr/bin/env python3
"""What alpha cutouts cost the scenes that do not use them, this tree against another tree (the parent commit,
built), alternating on one machine, and what cutout_garden.json costs beside its twin without masks:
    tools/gpu_alpha_ab.py OTHER_TREE [rounds]
The method of tools/gpu_normal_map_ab.py.  Each child process loads the package of ONE tree and renders, 1 warm-up + 5 timed
frames each (rt_stats.kernel_ms, min and median, CRC of the frame): the 20 000-triangle height field of tests/test_gpu_grid_all,
and mixed_emissive and env_sun with light sampling, fog_room, motion_balls, smooth_mesh, marble_hall, bumpy_pond, pbr_wear and
normal_map_wall, all at 1280 x 720 x 16.  A scene without a mask must give the same bytes in both trees; the parent prints the
CRCs side by side and each scene's spread (the largest difference between the minima of the other tree's rounds) beside the
difference between the trees: a difference outside the spread is a finding.
Every child of this tree then renders cutout_garden.json at 1280 x 720 x 16 and its twin (every mask removed), each with and
without light sampling."""
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH, N = 1280, 720, 16, 20, 100
SHIPPED = (("mixed_emissive", True), ("env_sun", True), ("fog_room", False), ("motion_balls", False), ("smooth_mesh", False), ("marble_hall", False),
           ("bumpy_pond", False), ("pbr_wear", False), ("normal_map_wall", False))
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


def twin_of(rtmi, path):
    """cutout_garden.json with every mask removed"""
    sc = rtmi.Scene.load(path)
    for m in range(len(sc.materials())):
        if sc.alpha(m) is not None:
            sc.set_alpha(m, -1)
    return sc


def child(tree, label, with_masks):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from __graft_entry__ import load_package
    rtmi = load_package()
    assert os.path.abspath(rtmi.__file__).startswith(os.path.abspath(tree))
    from test_gpu_grid_all import height_field
    scenes = os.path.join(tree, "ray-tracing-in-cuda_amd", "scenes")
    rows = {}
    rows["height_field"] = timed(rtmi, height_field(rtmi, N, W, H, SPP, depth=DEPTH))
    for name, nee in SHIPPED:
        sc = rtmi.Scene.load(os.path.join(scenes, name + ".json"))
        sc.override(W, H, SPP)
        sc.set_light_sampling(nee)
        rows[name] = timed(rtmi, sc)
    if with_masks:
        path = os.path.join(scenes, "cutout_garden.json")
        for name, make in (("cutout_garden", lambda: rtmi.Scene.load(path)), ("garden_twin", lambda: twin_of(rtmi, path))):
            for nee in (False, True):
                sc = make()
                sc.override(W, H, SPP)
                sc.set_light_sampling(nee)
                rows[name + (" nee" if nee else "")] = timed(rtmi, sc)
    for name, (lo, med, crc, kv) in rows.items():
        print("ROW " + json.dumps({"tree": label, "scene": name, "min": lo, "median": med, "crc": "%08x" % crc, "variant": kv}), flush=True)


def main():
    other, rounds = os.path.abspath(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 2
    contestants = [("this", ROOT), ("other", other)]
    seen = {}  # (label, scene) -> [(min, crc)]
    for r in range(rounds):
        print("round", r, flush=True)
        for label, tree in contestants:
            # (each child under its own time limit; its lines are passed on as they come)
            p = subprocess.Popen(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "child", tree, label,
                                  "masks" if tree == ROOT else "-"], stdout=subprocess.PIPE, text=True)
            for line in p.stdout:
                sys.stdout.write(line)
                sys.stdout.flush()
                if line.startswith("ROW "):
                    row = json.loads(line[4:])
                    seen.setdefault((label, row["scene"]), []).append((row["min"], row["crc"]))
            if p.wait() != 0:
                sys.exit(p.returncode)
    labels = [c[0] for c in contestants]
    print("%-18s" % "scene" + "".join("%12s" % (l + " (ms)") for l in labels) + "%10s%9s  %s" % ("this diff", "spread", "bytes"))
    ok = True
    for scene in [s for (t, s) in seen if t == "this"]:
        best = {l: min(x[0] for x in seen[(l, scene)]) for l in labels if (l, scene) in seen}
        line = "%-18s" % scene + "".join("%12s" % ("%.2f" % best[l] if l in best else "-") for l in labels)
        if "other" in best:
            b = seen[("other", scene)]
            spread = max(x[0] for x in b) - min(x[0] for x in b)
            line += "%+9.2f%%" % (100 * (best["this"] - best["other"]) / best["other"])
            same = len({x[1] for l in labels for x in seen[(l, scene)]}) == 1
            line += "%8.2f%%  %s" % (100 * spread / best["other"], "same" if same else "DIFFERENT")
            ok = ok and same
        else:
            line += "  crc " + " ".join(sorted({x[1] for l in labels if (l, scene) in seen for x in seen[(l, scene)]}))
        print(line)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2], sys.argv[3], sys.argv[4] == "masks")
    else:
        main()
