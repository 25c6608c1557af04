"""Scenes of the mesh lights (emissive triangles among the sampled emitters, rt_scene_set_mesh_lights) shared by
test_mesh_lights.py (CPU) and test_gpu_mesh_lights.py, with their plain twins, and the digests of what the switch must leave
alone.

Every per-sample case uses the frame, sample count, seed and draw budget of nee_scenes.REF_* (48 x 27 pixels x 13 one-sample
frames = 16 848 samples).  A builder called with glossy=False builds the case's glossy-free geometry (glossy_scenes._Mats); the
plain twin is that with light sampling off and the environment cleared: what the plain kernel renders, the baseline of
criterion (b).  The reference of a case is ref64.reference on its RefScene.

What was fixed, and why (the fp64 and the fp32 reference were run on the CPU on every case before it was fixed; a case stays
only if the fp32 reference alone meets criterion (a) with at most 1 % of the samples flipping a branch):
  * no checker lies on y = 0 (a checker floor is lifted by nee_scenes.LIFT), and the checker-emissive quad is tilted, so that
    no plane of parity coincides with the emitter's own plane;
  * the lone triangle and the quad are large enough (about 1.9 and 3.3 square units, 2.5 above the floor) for a BSDF ray off
    a receiver to end on them a few hundred times in 16 848 samples: the MIS-weighted hits the cases pin;
  * the smooth emissive mesh is a 3-ring, 4-segment UV sphere (16 triangles, radius 0.65, close over the receivers: at
    radius 0.35 and further off only 33 BSDF rays ended on it with a light sample behind them) with exact radial vertex
    normals: each face's geometric normal is tens of degrees off its vertex normals, so a density stated with a vertex
    normal is far off;
  * under the environment the map is dimmed (ENV_SCALE), or the alias table picks a triangle 3 times in 13 784.

tests/golden/mesh_lights_off_digests.json was written from digest_cases() by the commit before the feature: lights() and the
packed image of every scene shipped then and of ext_scenes' "unlisted emitters", with light sampling as the scene has it and
switched on."""
import hashlib
import os

import numpy as np

import ext_scenes as X
import feature_scenes as FS
import glossy_scenes as GS
import nee_scenes as NS
import smooth_scenes as SM

NEE, ENV, FAMILIES = FS.NEE, FS.ENV, FS.FAMILIES
LIFT = NS.LIFT
SHIPPED_BEFORE = ("env_sun.json", "fog_room.json", "glossy_balls.json", "mixed_emissive.json", "motion_balls.json", "smooth_mesh.json",
                  "three_sphere.json")

# the lone triangle light, and the quad (a, b, c, d) that two triangles tile
TRI = ((-1.0, 2.4, -0.9), (1.1, 2.6, -0.7), (0.0, 2.9, 1.0))
QUAD = ((-0.9, 2.5, -0.9), (0.9, 2.7, -0.9), (0.9, 2.7, 0.9), (-0.9, 2.5, 0.9))
# the environment's scale in case (iv): the map's power is r^2 x scale x flux with r the radius of the scene's bound (the floor
# reaches 20 units out), so at the shipped scene's scale the alias table would all but never pick a triangle; at this one the
# environment takes about a third of the picks and the triangles about 45 %
ENV_SCALE = 0.0003


def _frame(rtmi, w=NS.REF_W, h=NS.REF_H, spp=1, depth=6, background=(0.02, 0.02, 0.03)):
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background(background, sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0)
    return sc


def _receivers(sc):
    """a lambertian floor, a checker-lambertian sphere and a fuzz-0.3 metal sphere"""
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.5, 0.4)))
    sc.sphere((-1.2, 0.6, 0.5), 0.6, sc.lambertian(sc.checker_texture((0.8, 0.8, 0.8), (0.1, 0.3, 0.1))))
    sc.sphere((1.3, 0.5, 0.8), 0.5, sc.metal((0.8, 0.7, 0.6), 0.3))


def lone(rtmi, glossy=True, **kw):
    """(i) a lone emissive triangle over a lambertian, a checker and a fuzz-0.3 metal receiver"""
    sc = _frame(rtmi, **kw)
    _receivers(sc)
    sc.triangle(TRI[0], TRI[1], TRI[2], sc.diffuse_light((6.0, 5.0, 4.0)))
    return sc


def checker_quad(rtmi, glossy=True, **kw):
    """(ii) a checker-emissive quad of two triangles, tilted"""
    sc = _frame(rtmi, **kw)
    _receivers(sc)
    X.quad(sc, QUAD[0], QUAD[1], QUAD[2], QUAD[3], sc.diffuse_light(sc.checker_texture((6.0, 1.0, 0.5), (0.5, 2.0, 6.0))), X.QUAD_UV)
    return sc


def emissive_mesh(sc, centre=(-0.3, 1.65, 0.6), radius=0.65, emission=(4.0, 5.0, 6.0), smooth=True):
    """a 3-ring, 4-segment UV sphere of 16 emissive triangles, with exact radial vertex normals"""
    v, n = SM.uv_sphere(centre, radius, 3, 4)
    mat = sc.diffuse_light(emission)
    for k in range(len(v)):
        sc.triangle(v[k][0], v[k][1], v[k][2], mat, normals=n[k] if smooth else None)
    return len(v)


def mixed(rtmi, glossy=True, env=False, **kw):
    """(iii) a small smooth-shaded emissive mesh beside a rectangle and a sphere light: the alias table mixes shapes;
    env=True, (iv): the same under scenes/env_sun.json's map"""
    sc = _frame(rtmi, background=(0.1, 0.2, 0.3) if env else (0.02, 0.02, 0.03), **kw)
    sc.xz_rect(-20, 20, -20, 20, LIFT, sc.lambertian(sc.checker_texture((0.8, 0.8, 0.8), (0.2, 0.4, 0.2))))
    sc.sphere((-1.2, 0.65, 0.5), 0.6, sc.lambertian((0.3, 0.5, 0.7)))
    sc.sphere((1.3, 0.55, 0.8), 0.5, sc.metal((0.8, 0.7, 0.6), 0.3))
    emissive_mesh(sc)
    sc.xz_rect(0.1, 1.1, -0.7, 0.3, 2.6, sc.diffuse_light((6.0, 5.0, 4.0)))
    sc.sphere((2.3, 1.9, 1.0), 0.25, sc.diffuse_light((5.0, 6.0, 7.0)))
    if env:
        e, _, rotate = NS._sun_map()
        sc.set_environment(e, ENV_SCALE, rotate)
    return sc


def mixed_env(rtmi, glossy=True, **kw):
    return mixed(rtmi, glossy, env=True, **kw)


def glossy(rtmi, glossy=True, **kw):
    """(v) a rough-metal and a plastic receiver under a triangle light"""
    sc = _frame(rtmi, **kw)
    m = GS._Mats(sc, glossy)
    sc.xz_rect(-20, 20, -20, 20, 0.0, sc.lambertian((0.6, 0.5, 0.4)))
    sc.sphere((-1.2, 0.6, 0.5), 0.6, m.rough((0.95, 0.64, 0.54), 0.4))
    sc.sphere((1.3, 0.6, 0.8), 0.6, m.plastic((0.7, 0.15, 0.1), 1.5, 0.15))
    sc.triangle(TRI[0], TRI[1], TRI[2], sc.diffuse_light((6.0, 5.0, 4.0)))
    return sc


# name -> (family bits the kernel must report, builder)
CASES = {
    "lone triangle": (NEE, lone),
    "checker quad": (NEE, checker_quad),
    "smooth mesh + rect + sphere": (NEE, mixed),
    "smooth mesh + rect + sphere, env": (ENV | NEE, mixed_env),
    "glossy under a triangle": (NEE, glossy),
}
MIXED = "smooth mesh + rect + sphere"
# the keys of ref64.tally() a mesh-light case is read by
TALLY_KEYS = ("triangle_picks", "other_picks", "triangle_shadow_stopped", "triangle_shadow_clear", "triangle_mis_hits", "triangle_full_weight_hits")

# What each case holds, read off the fp64 reference (ref64.tally on the 16 848 samples) and pinned: light samples
# that picked a triangle, those whose shadow ray was stopped, BSDF hits on a triangle light with an MIS weight below 1
PINNED = {
    "lone triangle": dict(triangle_picks=13862, triangle_shadow_stopped=1017, triangle_mis_hits=174),
    "checker quad": dict(triangle_picks=13862, triangle_shadow_stopped=928, triangle_mis_hits=297),
    "smooth mesh + rect + sphere": dict(triangle_picks=8742, other_picks=4664, triangle_shadow_stopped=5142, triangle_mis_hits=226),
    "smooth mesh + rect + sphere, env": dict(triangle_picks=5982, other_picks=7424, triangle_shadow_stopped=3511, triangle_mis_hits=226),
    "glossy under a triangle": dict(triangle_picks=14049, triangle_shadow_stopped=1346, triangle_mis_hits=191),
}


family, seed_of, inputs = FS.bindings(CASES.__getitem__)


def scene(rtmi, name, mesh_lights=True, **kw):
    sc = CASES[name][1](rtmi, True, **kw)
    sc.set_light_sampling(True)
    sc.set_mesh_lights(mesh_lights)
    return sc


def plain_twin(rtmi, name):
    return FS.cleared(CASES[name][1](rtmi, False))


def check_contents(name, tally):
    """the case holds what it is there for: the pinned counts, each at least nee_scenes.REQUIRED_EVENTS (1 % of the samples)"""
    want = PINNED[name]
    got = {k: tally[k] for k in want}
    assert got == want, (name, got, want)
    for k, v in want.items():
        assert v >= NS.REQUIRED_EVENTS, (name, k, v)


def analytic_twin(rtmi, w=64, h=36, spp=256):
    """nee_scenes.analytic_scene with its rectangle replaced by two emissive triangles tiling the same rectangle"""
    sc = rtmi.Scene.new(w, h, spp, 2)
    sc.set_background((0, 0, 0), sky_gradient=False, defocus_blur=False)
    sc.camera((2.5, 1.2, -1.5), (2.5, 0.0, 0.0), (0, 1, 0), 50.0)
    sc.xz_rect(-50, 50, -50, 50, 0.0, sc.lambertian((NS.RHO, NS.RHO, NS.RHO)))
    a, b, c, d = ((NS.LX[0], NS.H, NS.LZ[0]), (NS.LX[1], NS.H, NS.LZ[0]), (NS.LX[1], NS.H, NS.LZ[1]), (NS.LX[0], NS.H, NS.LZ[1]))
    X.quad(sc, a, b, c, d, sc.diffuse_light((NS.LE, NS.LE, NS.LE)), X.QUAD_UV)
    return sc


# ------------------------------------------------------------------------------------ what the switch leaves alone
def digest_cases(rtmi, scenes_dir):
    """name -> builder: every scene shipped before the feature and the "unlisted emitters" case, as they come and with light
    sampling switched on"""
    out = {}
    for name in SHIPPED_BEFORE:
        out[name] = lambda name=name: rtmi.Scene.load(os.path.join(scenes_dir, name))

        def lit(name=name):
            sc = rtmi.Scene.load(os.path.join(scenes_dir, name))
            sc.set_light_sampling(True)
            return sc
        out[name + " + light sampling"] = lit
    out["unlisted emitters"] = lambda: X._unlisted(rtmi)
    return out


def digest(sc):
    """sha256 of lights() and of the packed image"""
    return {"lights": hashlib.sha256(np.ascontiguousarray(sc.lights()).tobytes()).hexdigest(),
            "image": hashlib.sha256(sc.table_image().tobytes()).hexdigest()}
