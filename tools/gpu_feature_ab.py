#!/usr/bin/env python3
"""What a feature costs the scenes that do not use it, this tree against another tree (the parent commit, built), alternating
on one machine, and what the feature's own shipped scene costs beside its twin without the feature:
    tools/gpu_feature_ab.py FEATURE OTHER_TREE [rounds] [NAME=LIBRARY ...]
    tools/gpu_feature_ab.py --list
FEATURE is a key of FEATURES below; --list prints, without a device, what each would run.
Each child process loads the package of ONE tree and renders, 1 warm-up + 5 timed frames each (rt_stats.kernel_ms, min and
median, CRC of the frame): the 20 000-triangle height field of tests/test_gpu_grid_all and the feature's shared scenes -- the
scenes shipped before it, with or without light sampling -- all at 1280 x 720 x 16.  A scene without the feature must give the
same bytes in both trees; the parent prints the CRCs side by side and each scene's spread (the largest difference between the
minima of the other tree's rounds) beside the difference between the trees: a difference outside the spread is a finding.  The
exit status is 1 if a shared scene's bytes differ, and that of the first child that fails.
NAME=LIBRARY (where the feature accepts it): one more contestant per round, this tree's package over another build of its
library (RTMI_LIB), for a feature with two forms of its code.
A feature with a `twin`: every child of this tree (and of its other libraries) then renders the feature's scene and its twin at
1280 x 720 x 16, each with and without light sampling, as rows of the same table.  A feature with `extra`: this tree's first
child then prints one line of figures of its own (FEATURES says which)."""
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH, N = 1280, 720, 16, 20, 100
CHILD_LIMIT = 420  # seconds
# the shipped scenes a feature must not change, in order of arrival, each with its light-sampling flag: a feature names the
# prefix that was there before it
SHIPPED = (("mixed_emissive", True), ("env_sun", True), ("fog_room", False), ("motion_balls", False), ("smooth_mesh", False),
           ("marble_hall", False), ("bumpy_pond", False), ("pbr_wear", False), ("normal_map_wall", False))
# the scenes with something to sample, all with light sampling (mesh_light: mesh lights on): what a change to the light sample
# must not move
LIT = (("mixed_emissive", True), ("cornell_box", True), ("bumpy_pond", True), ("frosted_glass", True), ("mesh_light", True, "mesh lights"),
       ("env_sun", True))


def timed(rtmi, sc, seed=1):
    ts = []
    for k in range(6):
        st = rtmi.Stats()
        img = sc.render(rtmi.Opts(seed=seed), st)
        if k:
            ts.append(st.kernel_ms)
    ts.sort()
    return ts[0], ts[len(ts) // 2], zlib.crc32(img.tobytes()), st.kernel_variant


def rel_noise(rtmi, sc, spp):
    """(the median over lit pixels of sd / mean at 160 x 90 over 4 seeds, the share of lit pixels), as tools/gpu_nee.py computes it"""
    import numpy as np
    sc.override(160, 90, spp)
    m = np.stack([sc.render(rtmi.Opts(seed=100 + s)).astype(np.float64).mean(axis=2) / spp for s in range(4)])
    mean, sd = m.mean(axis=0), m.std(axis=0, ddof=1)
    lit = mean > 1e-4
    return float(np.median(sd[lit] / mean[lit])), round(float(lit.mean()), 3)


def own_spp(rtmi, out, tag, sc, nee):
    """times the scene at 1280 x 720 at its own spp into out's ms_ / variant_ / spp keys; returns the spp"""
    spp = sc.spp
    sc.override(W, H, spp)
    sc.set_light_sampling(nee)
    lo, _, _, kv = timed(rtmi, sc)
    out["ms_" + tag], out["variant_" + tag], out["spp"] = round(lo, 2), kv, spp
    return spp


def equal_noise(out, a, b):
    ratio = (out["rel_noise_" + a] / max(out["rel_noise_" + b], 1e-12)) ** 2
    out["variance_ratio"] = round(ratio, 2)
    out["equal_noise_speedup"] = round(out["ms_" + a] / (out["ms_" + b] / ratio), 2)


# ---------------------------------------------------------------------------------------------------------------- the twins
def _absolute_meshes(doc, path):
    for o in doc["object"]["data"]:
        if o.get("type") == "mesh":
            o["file"] = os.path.normpath(os.path.join(os.path.dirname(path), o["file"]))


def without(get, clear):
    """a twin: the file's scene with the side table `get` reads cleared on every material"""
    def twin(rtmi, path):
        sc = rtmi.Scene.load(path)
        for m in range(len(sc.materials())):
            if getattr(sc, get)(m) is not None:
                clear(sc, m)
        return sc
    return twin


def solid_noise(rtmi, path):
    """every noise texture as the solid colour between its two"""
    doc = json.load(open(path))
    for i, t in enumerate(doc["texture"]["data"]):
        if t["type"] == "noise":
            doc["texture"]["data"][i] = {"type": "solid_color", "color": [0.5 * (a + b) for a, b in zip(t["color0"], t["color1"])]}
    return rtmi.Scene.parse(json.dumps(doc))


def metal_and_lambertian(rtmi, path):
    """every rough_metal as metal(F0, fuzz = roughness) and every plastic as lambertian of its texture"""
    doc = json.load(open(path))
    for m in doc["material"]["data"]:
        if m["type"] == "rough_metal":
            m["type"], m["fuzz"] = "metal", m.pop("roughness")
        elif m["type"] == "plastic":
            m["type"] = "lambertian"
            m.pop("ior"), m.pop("roughness")
    _absolute_meshes(doc, path)
    return rtmi.Scene.parse(json.dumps(doc))


def dielectric(rtmi, path):
    """every rough_glass as dielectric of the same index (smooth and clear)"""
    doc = json.load(open(path))
    for m in doc["material"]["data"]:
        if m["type"] == "rough_glass":
            bump, ir = m.get("bump"), m["ir"]
            m.clear()
            m["type"], m["index_of_refraction"] = "dielectric", ir
            if bump:
                m["bump"] = bump
    _absolute_meshes(doc, path)
    return rtmi.Scene.parse(json.dumps(doc))


def plastic(rtmi, path):
    """every pbr material as a plastic of its base texture, index and roughness factor"""
    doc = json.load(open(path))
    for k, m in enumerate(doc["material"]["data"]):
        if m["type"] == "pbr":
            doc["material"]["data"][k] = {"type": "plastic", "texture": m["texture"], "ior": m.get("ior", 1.5), "roughness": m["roughness"]}
    return rtmi.Scene.parse(json.dumps(doc))


def two_triangles(rtmi, sc):
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


# ------------------------------------------------------------------------------------------- the features' own lines of figures
def noise_beside_the_twin(tag, scene, twin):
    """TAG lines: the scene and its twin at their own spp with and without light sampling, the per-pixel noise of the four and the
    equal-noise figure"""
    def extra(rtmi, scenes):
        path = os.path.join(scenes, scene + ".json")
        for label, make in ((scene, lambda: rtmi.Scene.load(path)), ("twin", lambda: twin(rtmi, path))):
            out = {"scene": label}
            for nee in (False, True):
                t = "nee" if nee else "plain"
                sc = make()
                out["rel_noise_" + t] = rel_noise(rtmi, sc, own_spp(rtmi, out, t, sc, nee))[0]
            equal_noise(out, "plain", "nee")
            print(tag + " " + json.dumps(out), flush=True)
    extra.__doc__ = (f"{tag} lines: {scene}.json and its twin ({twin.__doc__}) at their own spp with and without light sampling, the "
                     "per-pixel noise of the four and the equal-noise figure")
    return extra


def stage(rtmi, scenes):
    """STAGE: spot_stage.json at its own spp with light sampling off (the lights light nothing: the plain kernel's time) and on,
    and the per-pixel noise with it on"""
    out = {"scene": "spot_stage"}
    for nee in (False, True):
        sc = rtmi.Scene.load(os.path.join(scenes, "spot_stage.json"))
        spp = own_spp(rtmi, out, "nee" if nee else "plain", sc, nee)
    out["rel_noise_nee"], out["lit_share"] = rel_noise(rtmi, sc, spp)
    print("STAGE " + json.dumps(out), flush=True)


def benefit(rtmi, scenes):
    """BENEFIT: mesh_light.json at its own spp with light sampling, mesh lights off and on (off: the torus is no light, the scene
    has none and runs the plain kernel), the per-pixel noise of the two and the equal-noise figure"""
    out = {"scene": "mesh_light"}
    for on in (False, True):
        tag = "on" if on else "off"
        sc = rtmi.Scene.load(os.path.join(scenes, "mesh_light.json"))
        sc.set_mesh_lights(on)
        spp = own_spp(rtmi, out, tag, sc, True)
        out["lights_" + tag] = len(sc.lights())
        out["rel_noise_" + tag] = rel_noise(rtmi, sc, spp)[0]
    equal_noise(out, "off", "on")
    print("BENEFIT " + json.dumps(out), flush=True)


def wear(rtmi, scenes):
    """WEAR: pbr_wear.json and its plastic twin at their own spp without and with light sampling, and the scene's per-pixel noise"""
    out = {"scene": "pbr_wear"}
    path = os.path.join(scenes, "pbr_wear.json")
    for nee in (False, True):
        t = "nee" if nee else "plain"
        for what, make in (("pbr", lambda: rtmi.Scene.load(path)), ("plastic", lambda: plastic(rtmi, path))):
            spp = own_spp(rtmi, out, what + "_" + t, make(), nee)
        sc = rtmi.Scene.load(path)
        sc.set_light_sampling(nee)
        out["rel_noise_" + t], out["lit_share_" + t] = rel_noise(rtmi, sc, spp)
    print("WEAR " + json.dumps(out), flush=True)


FLOOR_N = 64


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


def quads(rtmi, scenes):
    """QUADS lines: cornell_box.json (without and with light sampling) and a floor of n x n quads, each beside its twin in which
    every quad is its two triangles, at 1280 x 720 x 16: kernel time and, from the counting kernel where the scene's family has
    one, the list entries a lane examined per query and the primitives tested for every query"""
    def cornell(nee):
        sc = rtmi.Scene.load(os.path.join(scenes, "cornell_box.json"))
        sc.override(W, H, SPP)
        sc.set_light_sampling(nee)
        return sc
    for label, sc in (("cornell_box", cornell(False)), ("cornell_box --nee", cornell(True)),
                      ("floor %d x %d" % (FLOOR_N, FLOOR_N), floor_of_quads(rtmi, FLOOR_N))):
        out = {"scene": label}
        for tag, s in (("quads", sc), ("triangles", two_triangles(rtmi, sc))):
            lo, med, _, kv = timed(rtmi, s)
            per_query, always = examined(rtmi, s)
            out[tag] = {"ms": round(lo, 2), "variant": kv, "prims": len(s.prims()), "always_tested": always,
                        "entries_per_query": None if per_query is None else round(per_query, 2)}
        print("QUADS " + json.dumps(out), flush=True)


def camera_views(rtmi, own):
    """rows of both trees: this tree's scenes/camera_views.json at 1280 x 720 x 16 through the perspective camera (the file's
    "projection" taken out), without and with light sampling; of this tree alone: the same through each projection"""
    doc = json.load(open(os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "camera_views.json")))
    doc["camera"].pop("projection")
    views = (("views perspective", None),)
    if own:
        views += (("views orthographic", ("orthographic", 5.0)), ("views panoramic", ("panoramic",)), ("views fisheye", ("fisheye", 180.0)))
    rows = {}
    for label, projection in views:
        for nee in (False, True):
            sc = rtmi.Scene.parse(json.dumps(doc))
            sc.override(W, H, SPP)
            sc.set_light_sampling(nee)
            if projection:
                sc.set_projection(*projection)
            rows[label + (" nee" if nee else "")] = timed(rtmi, sc)
    return rows


# feature -> shared: the scenes that must render the same bytes in both trees (behind the height field, unless height_field is
# False); scene: the feature's own shipped scene; twin: (its label, how it is made) where scene and twin are rows of the table;
# libraries: NAME=LIBRARY contestants are accepted; extra: the feature's own line of figures, printed by this tree's first child;
# views: rows(rtmi, is this tree) that every child adds to the table
FEATURES = {
    "glossy": dict(shared=SHIPPED[:5], scene="glossy_balls", extra=noise_beside_the_twin("GLOSSY", "glossy_balls", metal_and_lambertian)),
    "mesh_lights": dict(shared=SHIPPED[:2], height_field=False, scene="mesh_light", extra=benefit),
    "noise": dict(shared=SHIPPED[:5], scene="marble_hall", twin=("marble_twin", solid_noise), libraries=True),
    "bump": dict(shared=SHIPPED[:6], scene="bumpy_pond", twin=("pond_twin", without("bump", lambda sc, m: sc.set_bump(m, -1, 0.0))), libraries=True),
    "quads": dict(shared=SHIPPED[:5], scene="cornell_box", extra=quads),
    "glass": dict(shared=SHIPPED[:5] + (("cornell_box", True), ("bumpy_pond", True)), scene="frosted_glass",
                  extra=noise_beside_the_twin("GLASS", "frosted_glass", dielectric)),
    "lights": dict(shared=LIT, scene="spot_stage", extra=stage),
    "pbr": dict(shared=LIT, scene="pbr_wear", extra=wear),
    "normal_map": dict(shared=SHIPPED[:8], scene="normal_map_wall",
                       twin=("wall_twin", without("normal_map", lambda sc, m: sc.set_normal_map(m, -1, 0.0))), libraries=True),
    "alpha": dict(shared=SHIPPED[:9], scene="cutout_garden", twin=("garden_twin", without("alpha", lambda sc, m: sc.set_alpha(m, -1)))),
    "camera": dict(shared=SHIPPED[:9] + (("cutout_garden", True),), scene="camera_views", views=camera_views),
}


def child(feature, tree, label, first):
    f = FEATURES[feature]
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from __graft_entry__ import load_package
    rtmi = load_package()
    assert os.path.abspath(rtmi.__file__).startswith(os.path.abspath(tree))
    scenes = os.path.join(tree, "ray-tracing-in-cuda_amd", "scenes")
    rows = {}
    if f.get("height_field", True):
        from test_gpu_grid_all import height_field
        rows["height_field"] = timed(rtmi, height_field(rtmi, N, W, H, SPP, depth=DEPTH))
    for name, nee, *more in f["shared"]:
        sc = rtmi.Scene.load(os.path.join(scenes, name + ".json"))
        sc.override(W, H, SPP)
        sc.set_light_sampling(nee)
        if more:
            sc.set_mesh_lights(True)
        rows[name] = timed(rtmi, sc)
    if "twin" in f and tree == ROOT:
        path = os.path.join(scenes, f["scene"] + ".json")
        for name, make in ((f["scene"], lambda: rtmi.Scene.load(path)), (f["twin"][0], lambda: f["twin"][1](rtmi, path))):
            for nee in (False, True):
                sc = make()
                sc.override(W, H, SPP)
                sc.set_light_sampling(nee)
                rows[name + (" nee" if nee else "")] = timed(rtmi, sc)
    if "views" in f:
        rows.update(f["views"](rtmi, tree == ROOT))
    for name, (lo, med, crc, kv) in rows.items():
        print("ROW " + json.dumps({"tree": label, "scene": name, "min": lo, "median": med, "crc": "%08x" % crc, "variant": kv}), flush=True)
    if "extra" in f and first:
        f["extra"](rtmi, scenes)


def show():
    for feature, f in FEATURES.items():
        shared = (["height_field"] if f.get("height_field", True) else []) + [n + (" --nee" if nee else "") + "".join(" (%s)" % m for m in more)
                                                                              for n, nee, *more in f["shared"]]
        own = [f["scene"] + t for t in ("", " nee")] + [f["twin"][0] + t for t in ("", " nee")] if "twin" in f else []
        print(feature)
        print("  same bytes in both trees:", ", ".join(shared))
        print("  the feature's scene:", f["scene"] + ".json" + ("; rows: " + ", ".join(own) if own else ""))
        print("  contestants: this, other" + (", NAME=LIBRARY" if f.get("libraries") else ""))
        if "extra" in f:
            print("  extra:", " ".join((f["extra"].__doc__ or "").split()))
        if "views" in f:
            print("  views:", " ".join((f["views"].__doc__ or "").split()))


def main():
    feature, other = sys.argv[1], os.path.abspath(sys.argv[2])
    f = FEATURES[feature]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    libs = dict(a.split("=", 1) for a in sys.argv[4:])
    if libs and not f.get("libraries"):
        sys.exit(feature + " takes no NAME=LIBRARY contestants")
    contestants = [("this", ROOT, None), ("other", other, None)] + [(name, ROOT, os.path.abspath(lib)) for name, lib in libs.items()]
    seen = {}  # (label, scene) -> [(min, crc)]
    for r in range(rounds):
        print("round", r, flush=True)
        for label, tree, lib in contestants:
            # (each child under its own time limit; its lines are passed on as they come)
            env = dict(os.environ) if lib is None else dict(os.environ, RTMI_LIB=lib)
            p = subprocess.Popen(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "child", feature, tree, label,
                                  "first" if r == 0 and label == "this" else "-"], stdout=subprocess.PIPE, text=True, env=env)
            for line in p.stdout:
                sys.stdout.write(line)
                sys.stdout.flush()
                if line.startswith("ROW "):
                    row = json.loads(line[4:])
                    seen.setdefault((label, row["scene"]), []).append((row["min"], row["crc"]))
            if p.wait() != 0:
                sys.exit(p.returncode)
    labels = [c[0] for c in contestants]
    print("%-18s" % "scene" + "".join("%12s" % (l + " (ms)") for l in labels) + "".join("%10s" % (l + " diff") for l in labels if l != "other")
          + "%9s  %s" % ("spread", "bytes"))
    ok = True
    for scene in [s for (t, s) in seen if t == "this"]:
        best = {l: min(x[0] for x in seen[(l, scene)]) for l in labels if (l, scene) in seen}
        line = "%-18s" % scene + "".join("%12s" % ("%.2f" % best[l] if l in best else "-") for l in labels)
        if "other" in best:
            b = seen[("other", scene)]
            spread = max(x[0] for x in b) - min(x[0] for x in b)
            line += "".join("%+9.2f%%" % (100 * (best[l] - best["other"]) / best["other"]) for l in labels if l != "other")
            same = len({x[1] for l in labels for x in seen[(l, scene)]}) == 1
            line += "%8.2f%%  %s" % (100 * spread / best["other"], "same" if same else "DIFFERENT")
            ok = ok and same
        else:
            line += "  crc " + " ".join(sorted({x[1] for l in labels if (l, scene) in seen for x in seen[(l, scene)]}))
        print(line)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    if len(sys.argv) < 3 and sys.argv[1:] != ["--list"]:
        sys.exit(__doc__)
    if sys.argv[1] == "--list":
        show()
    elif sys.argv[1] == "child":
        child(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5] == "first")
    else:
        main()
