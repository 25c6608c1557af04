"""Smooth shading: meshes with vertex normals, the scenes of test_smooth.py (CPU) and test_gpu_smooth.py, built
once per process, and independent_normal(), a second statement of the shading normal.

The first statement is ref64.shading_normal, which ref64.hit_record applies on every triangle that carries vertex normals
(the geometric normal at emitters): ref64.trace and ref64.reference need nothing from this file, and the flat form is their
"flat_normals" perturbation.  independent_normal() shares nothing with ref64: it is what the first statement is checked
against."""
import functools

import numpy as np

import ext_scenes as X
import nee_scenes as NS
import ref64 as R

W, H, K = 48, 27, 4          # frames of the per-sample comparison: 48 x 27, four one-sample frames
SEED = NS.REF_SEED
DRAWS = NS.REF_DRAWS


# ---------------------------------------------------------------------------------------------------------------- meshes
def uv_sphere(centre, radius, rings, segs):
    """A closed UV sphere of 2 segs (rings - 1) triangles: (corners [n][3][3] float32, wound outward; normals [n][3][3]
    float64: the unit radial direction of each fp32 corner from the centre, the exact vertex normal of the sphere through it)"""
    c = np.asarray(centre, np.float64)

    def P(i, j):  # ring i of 0..rings (poles at the ends), segment j
        th, ph = np.pi * i / rings, 2 * np.pi * (j % segs) / segs
        return (c + radius * np.array([np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)])).astype(np.float32)
    tris = []
    for j in range(segs):
        tris.append((P(0, 0), P(1, j + 1), P(1, j)))
        tris.append((P(rings, 0), P(rings - 1, j), P(rings - 1, j + 1)))
        for i in range(1, rings - 1):
            tris.append((P(i, j), P(i, j + 1), P(i + 1, j + 1)))
            tris.append((P(i, j), P(i + 1, j + 1), P(i + 1, j)))
    v = np.array(tris, np.float32)
    n = v.astype(np.float64) - c
    n /= np.sqrt((n * n).sum(axis=-1))[..., None]
    return v, n


def add_mesh(sc, v, n, mats, smooth=True):
    """the triangles v with the vertex normals n (smooth) or without; triangle k takes mats[k % len(mats)]"""
    mats = mats if isinstance(mats, (list, tuple)) else [mats]
    for k in range(len(v)):
        sc.triangle(v[k][0], v[k][1], v[k][2], mats[k % len(mats)], normals=n[k] if smooth else None)


def write_obj(path, v, n=None, corner="a//n"):
    """v [m][3][3] (and normals n) as an OBJ file with one v (and vn) line per corner; corner: "a", "a//n" or "a/t/n" """
    with open(path, "w") as f:
        for tri in v:
            for p in tri:
                f.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in p))
        if corner == "a/t/n":
            f.write("vt 0.25 0.75\n")
        if n is not None:
            for tri in n:
                for p in tri:
                    f.write("vn %.17g %.17g %.17g\n" % tuple(float(x) for x in p))
        for k in range(len(v)):
            ids = [3 * k + 1, 3 * k + 2, 3 * k + 3]
            f.write("f " + " ".join({"a": "%d" % i, "a//n": "%d//%d" % (i, i), "a/t/n": "%d/1/%d" % (i, i)}[corner] for i in ids) + "\n")


# ---------------------------------------------------------------------------------------------------------------- scenes
def _tilted(n, k):
    """a unit normal near n, leaning a little another way for each k"""
    t = np.asarray(n, np.float64) + 0.35 * np.array([np.cos(2.1 * k), np.sin(1.3 * k), np.cos(0.7 * k + 1.0)])
    return t / np.sqrt((t * t).sum())


def query_scene(rtmi, smooth=True):
    """the ray-query scene: an 80-triangle closed smooth sphere mesh in three materials, a smooth image-textured triangle pair,
    a smooth emissive triangle, four flat triangles, a sphere and a rectangle"""
    sc = X._frame(rtmi)
    sc.xz_rect(-7, 7, -7, 7, 0.0, sc.lambertian((0.6, 0.6, 0.55)))
    sc.sphere((-1.9, 0.6, 0.6), 0.6, sc.metal((0.8, 0.7, 0.6), 0.1))
    v, n = uv_sphere((0.1, 1.1, 0.0), 0.9, 6, 8)
    add_mesh(sc, v, n, [sc.lambertian((0.7, 0.4, 0.3)), sc.metal((0.8, 0.8, 0.7), 0.2), sc.dielectric(1.5)], smooth)
    X.pyramid(sc, (2.0, 1.3, 0.8), 0.5, 0.8, sc.lambertian((0.3, 0.5, 0.7)))
    tex = sc.lambertian(sc.image_texture(X.image(7, 5, 15)))
    a, b, c, d = (0.9, 0.05, -2.0), (3.3, 0.05, -1.5), (3.2, 2.4, -1.1), (1.0, 2.2, -1.5)
    face = np.cross(np.subtract(b, a), np.subtract(c, a))
    na, nb, nc, nd = (_tilted(face / np.sqrt((face * face).sum()), k) for k in range(4))
    uv = X.QUAD_UV
    sc.triangle(a, b, c, tex, uv[0], uv[1], uv[2], normals=(na, nb, nc) if smooth else None)
    sc.triangle(a, c, d, tex, uv[0], uv[2], uv[3], normals=(na, nc, nd) if smooth else None)
    e = ((-2.9, 0.3, -1.8), (-1.3, 0.3, -2.2), (-2.1, 2.0, -2.0))
    sc.triangle(*e, sc.diffuse_light((3.0, 2.5, 2.0)), normals=[_tilted((0.2, 0.0, 1.0), 5 + k) for k in range(3)] if smooth else None)
    return sc


def nested_scene(rtmi, smooth=True, w=W, h=H):
    """a 720-triangle smooth sphere of radius 0.15 among 100 small spheres spread over [-4, 4]^3, the nested grid on: the mesh is
    a clump that the flat grid cannot list"""
    sc = rtmi.Scene.new(w, h, 1, 5)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((-1.0, 0.7, 1.9), (-1.0, 0.5, 1.0), (0, 1, 0), 35.0)
    rng = np.random.default_rng(3)
    m = [sc.lambertian((0.7, 0.3, 0.3)), sc.metal((0.8, 0.8, 0.8), 0.15), sc.dielectric(1.5)]
    for k in range(100):
        c = rng.uniform(-4, 4, 3)
        sc.sphere((float(c[0]), float(c[1]), float(c[2])), 0.02, m[k % 2])
    v, n = uv_sphere((-1.0, 0.5, 1.0), 0.15, 16, 24)
    # (a wedge of 30 triangles per material)
    for k in range(len(v)):
        sc.triangle(v[k][0], v[k][1], v[k][2], m[(k // 30) % 3], normals=n[k] if smooth else None)
    sc.set_nested_grid(True)
    return sc


def _room(rtmi, smooth, depth=6):
    """the stage of every render case but the nested one: a floor, a back wall, a rectangle emitter and three 36-triangle smooth
    sphere meshes -- lambertian, metal(0.3), glass -- that fill a third of the frame, under the sky gradient (a direction a
    normal changes then changes what comes back).  The plain twin of every family's case is this scene."""
    sc = rtmi.Scene.new(W, H, 1, depth)
    sc.set_background((0.0, 0.0, 0.0), sky_gradient=True, defocus_blur=False)
    sc.camera((0.0, 1.4, 3.6), (0.0, 0.85, 0.0), (0, 1, 0), 40.0)
    sc.xz_rect(-7, 7, -7, 7, 0.0, sc.lambertian((0.6, 0.6, 0.55)))
    sc.xy_rect(-4, 4, 0.0, 4.0, -2.5, sc.lambertian((0.5, 0.55, 0.6)))
    sc.xz_rect(-1.2, 1.2, -0.6, 1.0, 3.2, sc.diffuse_light((6.0, 5.0, 4.0)))
    m = [sc.lambertian((0.7, 0.4, 0.3)), sc.metal((0.8, 0.8, 0.7), 0.3), sc.dielectric(1.5)]
    for x, mat in ((-1.5, m[0]), (0.0, m[1]), (1.5, m[2])):
        v, n = uv_sphere((x, 0.9, 0.0), 0.68, 4, 6)
        add_mesh(sc, v, n, mat, smooth)
    return sc


def plain_scene(rtmi, smooth=True):
    return _room(rtmi, smooth)


def nee_scene(rtmi, smooth=True):
    sc = _room(rtmi, smooth)
    sc.set_light_sampling(True)
    return sc


def env_scene(rtmi, smooth=True):
    sc = _room(rtmi, smooth)
    env, scale, rotate = NS._sun_map()
    sc.set_environment(env, scale, rotate)
    return sc


def fog_scene(rtmi, smooth=True):
    sc = _room(rtmi, smooth)
    sc.add_medium_box((-12, -1, -12), (12, 8, 12), 0.08, (0.9, 0.9, 0.9))
    return sc


def motion_scene(rtmi, smooth=True):
    sc = _room(rtmi, smooth)
    sc.add_moving_sphere((-2.2, 0.4, 1.6), (1.8, 0.4, 1.2), 0.4, sc.lambertian((0.3, 0.6, 0.3)))
    return sc


NEE, ENV, MEDIA, MOTION = X.NEE, X.ENV, X.MEDIA, X.MOTION
FAMILIES = NEE | ENV | MEDIA | MOTION
# name -> (builder, family bits the kernel must report, layouts to render in (0: the scene's own))
RENDER_CASES = {
    "plain": (plain_scene, 0, (16, 36, 44)),
    "light sampling": (nee_scene, NEE, (0,)),
    "environment": (env_scene, ENV, (0,)),
    "fog": (fog_scene, MEDIA, (0,)),
    "mover": (motion_scene, MOTION, (0,)),
    "nested": (nested_scene, 0, (52,)),
}


def plain_twin(rtmi, name):
    sc = RENDER_CASES[name][0](rtmi, True)
    sc.set_light_sampling(False)
    sc.set_environment(None)
    sc.clear_media()
    sc.clear_moving_spheres()
    return sc


@functools.lru_cache(maxsize=None)
def words(rtmi):
    a = R.uniforms(rtmi, SEED, W, H, 0, K, DRAWS)
    a.setflags(write=False)
    return a


def shutter(rtmi):
    import motion_scenes as MO
    return MO.shutter_times(rtmi, SEED, W, H, 0, K)


# ---------------------------------------------------------------------------------------------------------------- rays
@functools.lru_cache(maxsize=None)
def query_case():
    """(smooth scene, the same scene flat, origins, directions): 4103 rays by the recipe of trace_cases.make_rays"""
    import trace_cases as TC
    from __graft_entry__ import load_package
    rtmi = load_package()
    sc, flat = query_scene(rtmi, True), query_scene(rtmi, False)
    boxes = [TC.prim_box(p) for p in sc.prims() if not (int(p["type"]) == R.XZ_RECT)]
    lo, hi = np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)
    o, d = TC.make_rays(lo, hi)
    o.setflags(write=False), d.setflags(write=False)
    return sc, flat, o, d


def independent_normal(pr, o, d):
    """the definition of DESIGN 7l in fp64, written without ref64: the plane point from t = (v1 - o).n / d.n with the face normal
    of the corners, the weight of a corner as the area of the sub-triangle opposite it over the whole.
    -> (shading normal, face-turned geometric normal g, front: the ray meets the side the face normal (v2 - v1) x (v3 - v1) points to)"""
    m = pr["m"].astype(np.float64)
    v1, v2, v3 = m[0:3], m[3:6], m[6:9]
    n1, n2, n3 = np.concatenate([pr["f"][:6], pr["m_inv"][6:9]]).reshape(3, 3).astype(np.float64)  # the record's vertex normals
    nf = np.cross(v2 - v1, v3 - v1)
    area = np.sqrt(nf @ nf)
    nf = nf / area
    t = ((v1 - o) @ nf) / (d @ nf)
    r = o + t[:, None] * d
    g = np.where(((d @ nf) < 0)[:, None], nf, -nf)
    half = lambda a, b: np.sqrt((np.cross(a, b) ** 2).sum(axis=1))
    a1, a2, a3 = half(v2 - r, v3 - r) / area, half(v3 - r, v1 - r) / area, half(v1 - r, v2 - r) / area  # opposite 1, 2, 3
    s = a1[:, None] * n1 + a2[:, None] * n2 + a3[:, None] * n3
    length = np.sqrt((s * s).sum(axis=1))
    ok = np.isfinite(length) & (length > 0)
    with np.errstate(all="ignore"):
        s = s / length[:, None]
    s = np.where(((s * g).sum(axis=1) < 0)[:, None], -s, s)
    return np.where(ok[:, None], s, g), g, (d @ nf) < 0
