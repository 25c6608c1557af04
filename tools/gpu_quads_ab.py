#!/usr/bin/env python3
"""What the quads cost the scenes that have none, this tree against another tree (the parent commit, built),
alternating on one machine, and what a quad buys beside the two triangles it replaces:
    tools/gpu_quads_ab.py OTHER_TREE [rounds]
Each child process loads the package of ONE tree and renders, 1 warm-up + 5 timed frames each (rt_stats.kernel_ms, min and
median, CRC of the frame), the scene set of tools/gpu_glossy_ab.py: the 20 000-triangle height field of
tests/test_gpu_grid_all at 1280 x 720 x 16, and mixed_emissive and env_sun with light sampling, fog_room, motion_balls and
smooth_mesh at 1280 x 720 x 16.  A scene without a quad must give the same bytes in both trees; the parent prints the CRCs side
by side and each scene's spread (the largest difference between the minima of the other tree's rounds) beside the difference
between the trees.
This tree's first child then renders scenes/cornell_box.json (without and with light sampling) and a floor of n x n quads, each beside its
twin in which every quad is its two triangles, at 1280 x 720 x 16: kernel time and, from the counting kernel where the scene's
family has one, the list entries a lane examined per query and the primitives tested for every query."""
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH, N = 1280, 720, 16, 20, 100
SHIPPED = (("mixed_emissive", True), ("env_sun", True), ("fog_room", False), ("motion_balls", False), ("smooth_mesh", False))
FLOOR_N = 64
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


def as_triangles(rtmi, sc):
    """the scene with every quad as the triangles (Q, Q + u, Q + u + v) and (Q, Q + u + v, Q + v)"""
    import numpy as np
    doc = json.loads(sc.to_json())
    out = []
    for o in doc["object"]["data"]:
        if o["type"] != "quad":
            out.append(o)
            continue
        q, u, v = (np.array(o[k], np.float64) for k in ("q", "u", "v"))
        a, b, c, d = q, q + u, q + u + v, q + v
        for tri in ((a, b, c), (a, c, d)):
            out.append({"type": "triangle", "v1": list(tri[0]), "v2": list(tri[1]), "v3": list(tri[2]), "material": o["material"]})
    doc["object"]["data"] = out
    twin = rtmi.Scene.parse(json.dumps(doc))
    twin.set_mesh_lights(True)  # (a quad light is always sampled; its triangles are only with the switch on)
    return twin


def floor_of_quads(rtmi, n):
    """n x n slightly tilted quads tiling a floor under two spheres, the sky above"""
    import numpy as np
    sc = rtmi.Scene.new(W, H, SPP, DEPTH)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((0.0, 3.0, 8.0), (0.0, 0.3, 0.0), (0, 1, 0), 40.0)
    rng = np.random.default_rng(5)
    mats = [sc.lambertian((0.7, 0.7, 0.65)), sc.lambertian((0.3, 0.35, 0.5)), sc.metal((0.8, 0.8, 0.8), 0.2)]
    s = 12.0 / n
    for i in range(n):
        for j in range(n):
            tilt = rng.uniform(-0.1, 0.1, 2) * s
            sc.quad((-6 + i * s, float(rng.uniform(0, 0.05)), -6 + j * s), (0, float(tilt[0]), s), (s, float(tilt[1]), 0), mats[(i + j) % 3])
    sc.sphere((-1.2, 0.9, 0.0), 0.8, sc.dielectric(1.5))
    sc.sphere((1.2, 0.9, 0.0), 0.8, sc.metal((0.9, 0.7, 0.5), 0.0))
    return sc


def examined(rtmi, sc):
    """(list entries examined per lane and query, primitives tested for every query) of the scene's grid walk, or None where the
    scene's kernel family has no counting kernel"""
    import numpy as np
    info = sc.table_info()
    img = sc.table_image().reshape(-1, 4)
    listed = set()
    if info.grid_cells > 0 and info.grid_wide == 1:
        cells = img[info.off_grid_cells:info.off_grid_items].view(np.uint32).reshape(-1)[:2 * info.grid_cells].reshape(-1, 2)
        items = img[info.off_grid_items:].view(np.uint32).reshape(-1)
        for first, h in cells:
            listed.update(int(x) for x in items[first + ((h >> 10) & 1023):first + ((h >> 10) & 1023) + (h >> 20)])
    others = int((sc.prims()["type"] != rtmi.PRIM_SPHERE).sum())
    always = info.np + others - len(listed)
    try:
        st = sc.count(rtmi.Opts(seed=1, sample_count=1))
    except rtmi.RtmiError:
        return None, always
    return st.lane_clusters / max(1, st.queries), always


def child(tree, with_quads):
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
    for name, (lo, med, crc, kv) in rows.items():
        print("ROW " + json.dumps({"tree": tree, "scene": name, "min": lo, "median": med, "crc": "%08x" % crc, "variant": kv}), flush=True)
    if not with_quads:
        return
    def cornell(nee):
        sc = rtmi.Scene.load(os.path.join(scenes, "cornell_box.json"))
        sc.override(W, H, SPP)
        sc.set_light_sampling(nee)
        return sc
    for label, sc in (("cornell_box", cornell(False)), ("cornell_box --nee", cornell(True)),
                      ("floor %d x %d" % (FLOOR_N, FLOOR_N), floor_of_quads(rtmi, FLOOR_N))):
        out = {"scene": label}
        for tag, s in (("quads", sc), ("triangles", as_triangles(rtmi, sc))):
            lo, med, _, kv = timed(rtmi, s)
            per_query, always = examined(rtmi, s)
            out[tag] = {"ms": round(lo, 2), "variant": kv, "prims": len(s.prims()), "always_tested": always,
                        "entries_per_query": None if per_query is None else round(per_query, 2)}
        print("QUADS " + json.dumps(out), flush=True)


def main():
    other, rounds = os.path.abspath(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 2
    seen = {}  # (tree, scene) -> [(min, crc)]
    for r in range(rounds):
        print("round", r, flush=True)
        for tree in (ROOT, other):
            # (each child under its own time limit; its lines are passed on as they come)
            p = subprocess.Popen(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "child", tree,
                                  "quads" if r == 0 and tree == ROOT else "-"],
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
        child(sys.argv[2], sys.argv[3] == "quads")
    else:
        main()
