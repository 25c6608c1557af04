"""Scenes, rays and references of the ray-query tests (rt_trace_hip), shared by test_trace.py (CPU) and
test_gpu_trace.py: built once per process, never changed.

Scenes   (a) "mixed": 23 primitives of all five kinds (sphere, the three rectangles, cylinder, triangle) with image textures on
             a frame -- ext_scenes.textured_objects + ext_scenes.mesh and a few more -- wide tables
         (b) "clump": the sphere clump of test_nested_grid.py with the nested grid on (nested_info().cells > 0)
         (c) "rtiow": Scene.rtiow(7), compact tables
Rays     4103 per scene from a fixed seed (64 x 64 + 7: whole work items and a ragged one): origins uniform in the primitives'
         bounding box scaled 1.5 x about its centre, half of them aimed at a uniform point of the box, half isotropic, |dir|
         log-uniform in [0.1, 10], t_max = +inf.
         Two scenes depart from that recipe, because with it the two references alone -- the fp32 restatement and ref64 in
         fp64 -- do not agree on t to 2e-5 relative (test_trace.py), which is what lets the GPU test cap its own disagreement
         with fp64 at 1 %.  What was measured with the plain recipe, references only, no kernel involved:
         (b) 11 hits in 4103 rays (spheres of radius 0.02 and 0.005 in a box 8 units wide), t apart by up to 8.5e-5: the
             discriminant of a tiny sphere seen from units away cancels.  Here the box is that of the 1100 CLUSTERED spheres
             (the nested cells: rays start inside the cluster, cross it or graze it), |dir| is log-uniform in [2, 10], and
             t_max is finite: the diagonal of the box the origins come from, in units of the ray's direction (a far sphere
             is out of reach).  993 hits on 653 primitives, t apart by at most 5.7e-6.
         (c) the ground sphere of radius 1000 makes the box 2000 units wide; nearly every ray meets the ground alone, from
             inside or from far away, and the two statements of its roots (|oc| ~ 1000) part by up to 2e-3.  Here the box is
             that of the primitives without the ground (which stays in the scene and is tested by every ray), origins are
             mirrored to lie above y = 0.01 and no ray descends, so the ground is never the winner.  612 hits on 218
             primitives, t apart by at most 1.1e-5.  test_gpu_trace.py holds the kernel to the restatement bit for bit on
             rays of the plain recipe as well ("rtiow, plain recipe": the ground wins there).
"""
import functools

import numpy as np

import ext_scenes as X
import ref64 as R
from test_nested_grid import clump

N_RAYS = 4103
SEED = 20240607
SCENES = ("mixed", "clump", "rtiow")
SPHERE, XY_RECT, XZ_RECT, YZ_RECT, CYLINDER, TRIANGLE = R.SPHERE, R.XY_RECT, R.XZ_RECT, R.YZ_RECT, R.CYLINDER, R.TRIANGLE


def mixed(rtmi):
    sc = X._frame(rtmi)
    X.textured_objects(sc)
    X.mesh(sc)
    sc.xy_rect(-3.0, 3.0, 0.01, 3.0, -3.2, sc.lambertian(sc.image_texture(X.image(5, 8, 17))))
    sc.sphere((0.4, 0.45, 1.6), 0.45, sc.metal((0.8, 0.7, 0.6), 0.1))
    sc.sphere((-2.3, 0.5, -0.9), 0.5, sc.dielectric(1.5))
    sc.sphere((2.4, 0.35, 2.0), 0.35, sc.lambertian(sc.checker_texture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))))
    sc.cylinder(0.25, -0.5, 0.5, sc.metal((0.7, 0.7, 0.9), 0.0), rotate=((0.0, 0.3, 1.0), 35.0), translate=(-0.4, 0.9, -1.2))
    return sc


def nested_clump(rtmi):
    sc = clump(rtmi)
    sc.set_nested_grid(True)
    assert sc.nested_info().cells > 0
    return sc


def rtiow(rtmi):
    return rtmi.Scene.rtiow(7, 64, 36, 1, 4)


BUILDERS = {"mixed": mixed, "clump": nested_clump, "rtiow": rtiow}


def prim_box(p):
    """bounding box of one rt_prim record"""
    ty, f = int(p["type"]), p["f"].astype(np.float64)
    if ty == SPHERE:
        return f[:3] - abs(f[3]), f[:3] + abs(f[3])
    if ty in (XY_RECT, XZ_RECT, YZ_RECT):
        ka, aa, ba = R._rect_axes(ty)
        lo, hi = np.zeros(3), np.zeros(3)
        lo[aa], hi[aa], lo[ba], hi[ba], lo[ka], hi[ka] = f[0], f[1], f[2], f[3], f[4], f[4]
        return lo, hi
    if ty == TRIANGLE:
        v = p["m"].astype(np.float64)[:9].reshape(3, 3)
        return v.min(axis=0), v.max(axis=0)
    m = p["m"].astype(np.float64).reshape(3, 4)  # cylinder: the corners of its object-space box through object-to-world
    r = abs(f[0])
    c = np.array([[x, y, z] for x in (-r, r) for y in (-r, r) for z in (f[1], f[2])])
    w = c @ m[:, :3].T + m[:, 3]
    return w.min(axis=0), w.max(axis=0)


def scene_box(sc, name):
    """the box the rays of a scene are drawn from (the module's docstring says where it is not that of all primitives)"""
    prims = sc.prims()
    if name == "rtiow":
        prims = prims[[not (int(p["type"]) == SPHERE and abs(p["f"][3]) >= 100.0) for p in prims]]
    if name == "clump":
        prims = prims[[abs(p["f"][3]) < 0.01 for p in prims]]
    boxes = [prim_box(p) for p in prims]
    return np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)


def make_rays(lo, hi, n=N_RAYS, seed=SEED, above=None, shortest=0.1):
    """(origins, directions) as float32, by the recipe of the module's docstring; above: origins are mirrored to lie above
    this height and no ray descends; shortest: the lower end of |dir|"""
    rng = np.random.default_rng(seed)
    centre, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    o = centre + 1.5 * half * rng.uniform(-1.0, 1.0, (n, 3))
    target = lo + (hi - lo) * rng.uniform(0.0, 1.0, (n, 3))
    iso = rng.normal(0.0, 1.0, (n, 3))
    if above is not None:
        o[:, 1] = above + np.abs(o[:, 1] - above)
    d = np.where((np.arange(n) % 2 == 0)[:, None], target - o, iso)
    if above is not None:
        d[:, 1] = np.abs(d[:, 1])
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    d *= np.exp(rng.uniform(np.log(shortest), np.log(10.0), (n, 1)))
    return o.astype(np.float32), d.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, origins, directions, t_max) of a test scene: one per process"""
    from __graft_entry__ import load_package
    rtmi = load_package()
    sc = BUILDERS[name](rtmi)
    lo, hi = scene_box(sc, name)
    o, d = make_rays(lo, hi, above=0.01 if name == "rtiow" else None, shortest=2.0 if name == "clump" else 0.1)
    t_max = np.full(len(o), np.inf, np.float32)
    if name == "clump":  # the far end: the diagonal of the box the origins come from, in units of the ray's own direction
        reach = 1.5 * np.sqrt(((hi - lo) ** 2).sum())
        t_max = (reach / np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))).astype(np.float32)
    for a in (o, d, t_max):
        a.setflags(write=False)
    return sc, o, d, t_max


@functools.lru_cache(maxsize=None)
def restatement(name):
    """rtcheck.oracle_hit_uv (fp32) of every ray: (prim or -1, t as float32, u, v).  The probe has no far end: its hit counts
    iff its t <= the ray's t_max."""
    import rtcheck
    sc, o, d, t_max = case(name)
    osc = rtcheck.OracleScene(sc)
    prim, t, uv = np.full(len(o), -1, np.int32), np.full(len(o), np.inf, np.float32), np.zeros((len(o), 2), np.float32)
    for i in range(len(o)):
        hit, (u, v), tt, p = rtcheck.oracle_hit_uv(osc, [float(x) for x in o[i]], [float(x) for x in d[i]])
        if hit and np.float32(tt) <= t_max[i]:
            prim[i], t[i], uv[i] = p, tt, (u, v)
    for a in (prim, t, uv):
        a.setflags(write=False)
    return prim, t, uv[:, 0], uv[:, 1]


@functools.lru_cache(maxsize=None)
def ref_scene(name):
    return R.RefScene(case(name)[0])


@functools.lru_cache(maxsize=None)
def fp64(name):
    """ref64.closest_hit in fp64 of every ray: (prim or -1, t; +inf on a miss)"""
    sc, o, d, t_max = case(name)
    t, idx = R.closest_hit(ref_scene(name), o.astype(np.float64), d.astype(np.float64), t_max.astype(np.float64), np.float64)
    idx, t = idx.astype(np.int32), np.where(idx >= 0, t, np.inf)
    idx.setflags(write=False), t.setflags(write=False)
    return idx, t


def rel_t(t, t_ref):
    """the tolerance form of test_primitives_fuzz.py: |t - t_ref| / max(1, |t_ref|)"""
    return np.abs(t.astype(np.float64) - t_ref) / np.maximum(1.0, np.abs(t_ref))


# ---- the guard's table: (what, origin, direction, t_max, valid)
_NAN, _INF, _DEN = float("nan"), float("inf"), 1e-40
GUARD_TABLE = [("plain", (0, 0, 0), (0, 0, 1), _INF, True),
               ("unnormalised", (1, 2, 3), (0.1, -7.0, 2.5), 12.5, True),
               ("axis-parallel", (5, 5, 5), (0, -1, 0), _INF, True),
               ("t_max -inf", (0, 0, 0), (0, 0, 1), -_INF, True),
               ("t_max negative", (0, 0, 0), (0, 0, 1), -3.0, True),
               ("t_max zero", (0, 0, 0), (0, 0, 1), 0.0, True),
               ("t_max NaN", (0, 0, 0), (0, 0, 1), _NAN, False),
               ("dir zero", (0, 0, 0), (0, 0, 0), _INF, False),
               ("dir negative zero", (0, 0, 0), (-0.0, 0.0, -0.0), _INF, False),
               ("dir denormal", (0, 0, 0), (_DEN, 0, 0), _INF, False),
               ("dir.dir denormal", (0, 0, 0), (1e-20, 1e-20, 0), _INF, False),
               ("dir.dir smallest normal side", (0, 0, 0), (2e-19, 0, 0), _INF, True),
               ("dir 1e30", (0, 0, 0), (1e30, 0, 0), _INF, False),
               ("dir 1e19 fits", (0, 0, 0), (1e19, 0, 0), _INF, True),
               ("origin large but finite", (1e30, 0, 0), (0, 1, 0), _INF, True)]
for _k in range(3):
    for _bad in (_NAN, _INF, -_INF):
        _o, _d = [0.5, 0.25, -1.0], [0.3, 0.4, 0.5]
        _o[_k] = _bad
        GUARD_TABLE.append(("origin[%d] %r" % (_k, _bad), tuple(_o), (0.3, 0.4, 0.5), _INF, False))
        _d[_k] = _bad
        GUARD_TABLE.append(("dir[%d] %r" % (_k, _bad), (0.5, 0.25, -1.0), tuple(_d), _INF, False))


def check_guard(rtmi):
    """rt_ray_valid on the table; the GPU test of invalid rays runs this first"""
    for what, o, d, t_max, valid in GUARD_TABLE:
        rec = rtmi.pack_rays([o], [d], t_max)
        assert rtmi.ray_valid(rec[0]) == valid, what
        assert rtmi.ray_valid((o, d, t_max)) == valid, what
    assert not rtmi._lib.rt_ray_valid(None)
    return [row for row in GUARD_TABLE if not row[4]]


@functools.lru_cache(maxsize=None)
def rtiow_plain_recipe():
    """(scene, origins, directions, restatement's prim, t, u, v) of scene (c) under the plain recipe: the box of ALL its primitives"""
    import rtcheck
    sc = case("rtiow")[0]
    boxes = [prim_box(p) for p in sc.prims()]
    o, d = make_rays(np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0), seed=SEED + 1)
    osc = rtcheck.OracleScene(sc)
    prim, t, uv = np.full(len(o), -1, np.int32), np.full(len(o), np.inf, np.float32), np.zeros((len(o), 2), np.float32)
    for i in range(len(o)):
        hit, (u, v), tt, p = rtcheck.oracle_hit_uv(osc, [float(x) for x in o[i]], [float(x) for x in d[i]])
        if hit:
            prim[i], t[i], uv[i] = p, tt, (u, v)
    return sc, o, d, prim, t, uv[:, 0], uv[:, 1]
