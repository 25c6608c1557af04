#!/usr/bin/env python3
"""Writes tests/golden/camera_parent_tables.json: for every shipped scene (scenes/*.json) the SHA-256 of Scene.table_image() --
the packed tables the kernels read -- and the rt_table_info words, as the commit BEFORE the camera projections
packs them.  tests/test_camera.py holds every later commit to it: a perspective scene packs the parent's bytes.

usage: tools/make_camera_golden.py --root CHECKOUT     (a built checkout of that commit; the file is written into THIS tree)
No GPU needed: packing is host work."""
import argparse
import glob
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tables(root):
    sys.path.insert(0, root)
    from __graft_entry__ import load_package
    rtmi = load_package()
    out = {}
    for path in sorted(glob.glob(os.path.join(root, "ray-tracing-in-cuda_amd", "scenes", "*.json"))):
        sc = rtmi.Scene.load(path)
        info = sc.table_info()
        out[os.path.basename(path)] = {
            "sha256": hashlib.sha256(sc.table_image().tobytes()).hexdigest(),
            "info": {name: int(getattr(info, name)) for name, _ in info._fields_ if isinstance(getattr(info, name), int)},
        }
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    with open(os.path.join(HERE, "tests", "golden", "camera_parent_tables.json"), "w") as fh:
        json.dump(tables(os.path.abspath(a.root)), fh, indent=1, sort_keys=True)
        fh.write("\n")
