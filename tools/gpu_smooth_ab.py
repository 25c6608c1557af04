#!/usr/bin/env python3
"""What smooth shading costs on the 20 000-triangle mesh at 1280 x 720 x 16, this tree against another tree
(the parent commit, built), alternating on one machine:  tools/gpu_smooth_ab.py OTHER_TREE [rounds]
Each child process loads the package of ONE tree and renders the mesh of tests/test_gpu_grid_all.height_field without vertex
normals (1 warm-up + 5 timed frames, rt_stats.kernel_ms); this tree's child then renders it with generated normals (the mesh
through an OBJ file and normals="smooth").  The flat frames of both trees must be the same bytes."""
import os
import subprocess
import sys
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH, N = 1280, 720, 16, 20, 100


def timed(rtmi, sc):
    ts = []
    for k in range(6):
        st = rtmi.Stats()
        img = sc.render(rtmi.Opts(seed=1), st)
        if k:
            ts.append(st.kernel_ms)
    ts.sort()
    return ts[0], ts[len(ts) // 2], zlib.crc32(img.tobytes()), st.kernel_variant


def child(tree):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from __graft_entry__ import load_package
    rtmi = load_package()
    assert os.path.abspath(rtmi.__file__).startswith(os.path.abspath(tree))
    from test_gpu_grid_all import height_field
    sc = height_field(rtmi, N, W, H, SPP, depth=DEPTH)
    lo, med, crc, kv = timed(rtmi, sc)
    print(f"  {os.path.relpath(tree, ROOT):12s} flat    v{kv} min {lo:.2f} ms median {med:.2f} ms crc {crc:08x}", flush=True)
    if not hasattr(rtmi, "MESH_NORMALS"):
        return
    # the same mesh with generated normals: its triangles through an OBJ file, the rest of the scene as it was
    prims = sc.prims()
    tri = prims[prims["type"] == 5]
    sm = rtmi.Scene.new(W, H, SPP, DEPTH)
    sm.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    cam = (0.9 * 10.0, 0.55 * 10.0, 1.1 * 10.0)
    sm.camera(cam, (0, 0.3, 0), (0, 1, 0), 35.0)
    mats = [sm.lambertian((0.7, 0.3, 0.3)), sm.metal((0.8, 0.8, 0.8), 0.05), sm.lambertian((0.3, 0.6, 0.3)), sm.dielectric(1.5)]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "mesh.obj")
        with open(path, "w") as f:
            for p in tri:
                for c in range(3):
                    f.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in p["m"][3 * c:3 * c + 3]))
            for k in range(len(tri)):
                f.write("f %d %d %d\n" % (3 * k + 1, 3 * k + 2, 3 * k + 3))
        assert sm.add_obj(path, mats[0], normals="smooth", crease_angle=180.0) == len(tri)
    for p in prims[prims["type"] == 0]:
        sm.sphere(tuple(float(x) for x in p["f"][:3]), float(p["f"][3]), int(p["material"]))
    lo, med, crc, kv = timed(rtmi, sm)
    print(f"  {os.path.relpath(tree, ROOT):12s} smooth  v{kv} min {lo:.2f} ms median {med:.2f} ms (one lambertian material on the mesh)", flush=True)
    fl = rtmi.Scene.new(W, H, SPP, DEPTH)
    fl.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    fl.camera(cam, (0, 0.3, 0), (0, 1, 0), 35.0)
    mats = [fl.lambertian((0.7, 0.3, 0.3)), fl.metal((0.8, 0.8, 0.8), 0.05), fl.lambertian((0.3, 0.6, 0.3)), fl.dielectric(1.5)]
    for p in tri:
        fl.triangle(p["m"][0:3], p["m"][3:6], p["m"][6:9], mats[0])
    for p in prims[prims["type"] == 0]:
        fl.sphere(tuple(float(x) for x in p["f"][:3]), float(p["f"][3]), int(p["material"]))
    lo, med, crc, kv = timed(rtmi, fl)
    print(f"  {os.path.relpath(tree, ROOT):12s} flat'   v{kv} min {lo:.2f} ms median {med:.2f} ms (the same scene without the normals)", flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2])
    else:
        other, rounds = os.path.abspath(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 2
        for r in range(rounds):
            print("round", r, flush=True)
            for tree in (ROOT, other):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", tree], timeout=400)
                if p.returncode != 0:
                    sys.exit(p.returncode)
