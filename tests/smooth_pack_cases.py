"""Scenes WITHOUT vertex normals whose packed tables must not change with smooth shading, and their digest:
tests/golden/smooth_pack_digests.json was written from these builders by the commit before the feature."""
import hashlib
import os

import ext_scenes as X
import trace_cases as TC

SHIPPED = ("three_sphere.json", "mixed_emissive.json", "env_sun.json", "fog_room.json", "motion_balls.json")


def _flat_obj(rtmi, tmp):
    """a small OBJ with vn lines and a/t/n corners through rt_scene_add_obj: flat, as before"""
    path = os.path.join(tmp, "flat.obj")
    with open(path, "w") as f:
        f.write("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nvt 0.1 0.2\nvt 0.9 0.3\nvt 0.4 0.8\nvn 0 0 1\nvn 0 1 0\n"
                "f 1/1/1 2/2/1 3/3/2\nf 1//2 2//1 4//2\nf 1 3 4\nf 2/1 3/2 4/3\n")
    sc = X._frame(rtmi)
    sc.xz_rect(-7, 7, -7, 7, 0.0, sc.lambertian((0.6, 0.6, 0.55)))
    assert sc.add_obj(path, sc.lambertian(sc.image_texture(X.image(3, 4, 12))), 1.5, [1, 0.2, 0, 0, 1, 0, 0.1, 0, 1], (0.2, 0.3, -0.4)) == 4
    return sc


def cases(rtmi, scenes_dir, tmp=None):
    """name -> builder of a scene"""
    out = {name: (lambda name=name: rtmi.Scene.load(os.path.join(scenes_dir, name))) for name in SHIPPED}
    out["trace mixed"] = lambda: TC.mixed(rtmi)
    out["trace clump nested"] = lambda: TC.nested_clump(rtmi)
    out["rtiow"] = lambda: TC.rtiow(rtmi)
    for name in X.CASES:
        out["ext " + name] = lambda name=name: X.scene(rtmi, name)
    if tmp is not None:
        out["flat obj"] = lambda: _flat_obj(rtmi, tmp)
    return out


def digest(sc):
    """sha256 of the packed image's bytes and of the rt_table_info record"""
    return {"image": hashlib.sha256(sc.table_image().tobytes()).hexdigest(), "info": hashlib.sha256(bytes(sc.table_info())).hexdigest()}
