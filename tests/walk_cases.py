"""Random scenes that put a GRID under every kernel group, shared by test_walk_cases.py (CPU: the premises, the host coverage
checks) and test_gpu_walk_families.py (every layout of every group against the group's linear scan, byte for byte).

The feature suites' hand-built cases mostly pack to tables without a grid (16 primitives or fewer outside the sphere prefix:
pack.hip lists nothing, and layouts 36 / 44 run the scan's per-query loops), so their "same bytes in every layout" says
nothing about the walk.  scene(rtmi, seed, family, shape) is one generator for all groups:

  geometry   drawn from (seed, shape) alone -- every group of a seed sees the same primitives.  150 to 900 primitives of every
             kind the packer knows: spheres (small ones, a few large ones), the three rectangles, turned cylinders, flat and
             smooth triangles, quads with arbitrary edges, turned boxes (six quads each).  shape: "sheet" (all near y = 0),
             "volume", or "clump" (a volume plus a few hundred small primitives of mixed kinds within a cell's worth of space: with
             set_nested_grid(True) the tables nest)
  materials  cycle through lambertian (solid, checker, image), metal, dielectric, rough metal, plastic, rough glass, twice over;
             a diffuse_light lies on one sphere, rectangle, cylinder, quad and triangle each
  built in   a 3 x 3 arrangement of abutting axis-aligned rectangles, triangles and quads on multiples of 0.5 (their boxes end
             on common planes; the grid's own planes follow from the packed scene and cannot be fixed from here); one long thin
             cylinder and one long thin quad across the whole cloud; one oversized wall; by the seed's number: a far mirror
             behind the cloud ((seed // 2) even; an xy_rect or a turned quad by (seed // 4)), the ground sphere of radius 1000
             (seed % 5 != 0), the camera inside the cloud (seed % 3 == 0, the feature-pass groups excepted), roulette
             (seed % 4 == 1)
  frame      40 x 24 to 96 x 56, spp 1 to 3, max_depth 2 to 8

`family` names a row of GROUPS and dresses the scene for one kernel group, within what render_host.hip combines (no alpha with
media or a projection, no nested grid or media or movers with light sampling or an environment, no masked mover).
"""
import collections

import numpy as np

import alpha_scenes as AS
import nee_scenes as NS

NEE, FEATURE, ENV, MEDIA, MOTION, TRACE = 256, 512, 1024, 2048, 4096, 8192  # the family bits of rt_stats.kernel_variant
FAMILIES = NEE | FEATURE | ENV | MEDIA | MOTION | TRACE
SHAPES = ("sheet", "volume", "clump")
N_RAYS = 4103                        # of the trace groups (trace_cases.make_rays: whole work items and a ragged one)
LDS_BYTES = 160 * 1024               # kCuLdsBytes (kernels.h)
LDS_BESIDE_TABLES = 4 * 1536 + 5120  # four wave accumulators and the alpha state (kWaveAccBytes, kAlphaLdsBytes)

Group = collections.namedtuple("Group", "bits nee env media motion nested alpha camera passes trace", defaults=(False,) * 6 + (None, False, False))
# name -> (family bits of a frame, what the scene is dressed with).  passes: the group's frames are the three feature passes
# (bits: FEATURE and the scene's environment); trace: its "frames" are the closest-hit records of N_RAYS rays
GROUPS = {
    "plain": Group(0),
    "nee": Group(NEE, nee=True),
    "env": Group(ENV, env=True),
    "env_nee": Group(ENV | NEE, nee=True, env=True),
    "media": Group(MEDIA, media=True),
    "motion": Group(MOTION, motion=True),
    "feature": Group(FEATURE, passes=True),
    "feature_env": Group(FEATURE | ENV, env=True, passes=True),
    "nested": Group(0, nested=True),
    "alpha": Group(0, alpha=True),
    "alpha_nested": Group(0, nested=True, alpha=True),
    "alpha_feature": Group(FEATURE, alpha=True, passes=True),
    "alpha_motion": Group(MOTION, motion=True, alpha=True),
    "alpha_nee": Group(NEE, nee=True, alpha=True),
    "alpha_env_nee": Group(ENV | NEE, nee=True, env=True, alpha=True),
    "camera": Group(0, camera="orthographic"),
    "camera_nested": Group(0, nested=True, camera="panoramic"),
    "camera_feature": Group(FEATURE, camera="fisheye", passes=True),
    "camera_motion": Group(MOTION, motion=True, camera="orthographic"),
    "camera_nee": Group(NEE, nee=True, camera="fisheye"),
    "camera_env": Group(ENV, env=True, camera="panoramic"),
    "camera_media": Group(MEDIA, media=True, camera="panoramic"),
    "trace": Group(TRACE, trace=True),
    "trace_nested": Group(TRACE, nested=True, trace=True),
}
# two seeds per group, none shared between groups: a sheet and a volume, or two clumps where the group's tables nest
CASES = [(name, 100 + 2 * i + k, "clump" if g.nested else SHAPES[k]) for i, (name, g) in enumerate(GROUPS.items()) for k in range(2)]


def twin_family(family):
    """the group whose scene is this group's without the alpha masks / the projection / the media / the movers: what a frame
    of `family` must differ from, or the feature does not show in the case.  None: the group adds none of them"""
    g = GROUPS[family]
    if not (g.alpha or g.camera or g.media or g.motion):
        return None
    want = g._replace(alpha=False, camera=None) if (g.alpha or g.camera) else g._replace(media=False, motion=False, bits=g.bits & ~(MEDIA | MOTION))
    return next(name for name, other in GROUPS.items() if other == want)


def layouts(family):
    """the layouts a group's frames are rendered in beside the scan 16, as render_host.hip allows: the walks over LDS and global
    tables and the scene's own choice -- or, on nested tables, the nested walk and the scene's own choice (52 again) -- and the
    scan over global tables where the family has that build (plain, feature on the plain scene, trace)"""
    g = GROUPS[family]
    out = (52, 0) if g.nested else (36, 44, 0)
    has_24 = not (g.alpha or g.camera) and g.bits in (0, FEATURE, TRACE)
    return out + ((24,) if has_24 else ())


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _f3(v):
    return tuple(float(x) for x in v)


def _materials(sc):
    """two rounds of the eight scattering materials (the image: in memory, 6 x 5 texels), and the emitter"""
    px = (np.arange(6 * 5 * 3, dtype=np.uint32).reshape(6, 5, 3) * 37 % 251).astype(np.uint8)
    mats = []
    for r in range(2):
        a = 0.25 * r
        mats += [sc.lambertian((0.7 - a, 0.3 + a, 0.3)), sc.lambertian(sc.checker_texture((0.2, 0.3, 0.1 + a), (0.9, 0.9, 0.9 - a))),
                 sc.lambertian(sc.image_texture(px if r == 0 else px[::-1].copy())), sc.metal((0.9, 0.85 - a, 0.8), 0.2 * r), sc.dielectric(1.5 + 0.2 * r),
                 sc.rough_metal((0.9, 0.7 + a, 0.4), 0.3 - 0.2 * r), sc.plastic((0.2 + a, 0.4, 0.8 - a), 1.5, 0.3),
                 sc.rough_glass(1.5, 0.2 + 0.2 * r, (0.3, 0.1, 0.05) if r else None)]
    return mats, sc.diffuse_light((3.0, 2.5, 2.0))


class _Adder:
    """adds one primitive of a kind at a point: `s` is its size, `rng` draws its edges and its turn"""
    KINDS = ("sphere", "rect", "cylinder", "triangle", "smooth", "quad", "box")

    def __init__(self, sc, rng):
        self.sc, self.rng, self.n_rect = sc, rng, 0

    def __call__(self, kind, c, s, m):
        sc, rng = self.sc, self.rng
        c = np.asarray(c, np.float64)
        if kind == "sphere":
            sc.sphere(_f3(c), 0.6 * s, m)
        elif kind == "rect":
            self.n_rect += 1
            a, b, k = {0: (0, 1, 2), 1: (0, 2, 1), 2: (1, 2, 0)}[self.n_rect % 3]
            [sc.xy_rect, sc.xz_rect, sc.yz_rect][self.n_rect % 3](float(c[a]), float(c[a] + 2 * s), float(c[b]), float(c[b] + 2 * s), float(c[k]), m)
        elif kind == "cylinder":
            sc.cylinder(0.4 * s, -s, s, m, rotate=(_f3(_unit(rng.normal(size=3))), float(rng.uniform(0, 180))), translate=_f3(c))
        elif kind in ("triangle", "smooth"):
            a, b = rng.normal(size=3) * s, rng.normal(size=3) * s
            normals = None
            if kind == "smooth":  # the face normal, tilted differently at every vertex
                n = _unit(np.cross(a, b))
                normals = [_unit(n + 0.4 * rng.normal(size=3)) for _ in range(3)]
            sc.triangle(_f3(c), _f3(c + a), _f3(c + b), m, (0.0, 0.0), (1.0, 0.0), (0.0, 1.0), normals=normals)
        elif kind == "quad":
            sc.quad(_f3(c), _f3(rng.normal(size=3) * s), _f3(rng.normal(size=3) * s), m)
        elif kind == "box":
            e = rng.uniform(0.3, 0.8, 3) * s
            sc.box(_f3(-e), _f3(e), m, rotate=(_f3(_unit(rng.normal(size=3))), float(rng.uniform(0, 90))), translate=_f3(c))
        else:
            raise ValueError(kind)


def scene(rtmi, seed, family, shape):
    """the scene of (seed, shape), dressed for the group `family` (the module's text)"""
    g = GROUPS[family]
    if shape not in SHAPES or (g.nested and shape != "clump"):
        raise ValueError((family, shape))
    seed = int(seed)
    rng = np.random.default_rng([seed, SHAPES.index(shape)])  # the geometry's stream: every draw below is made for every family
    sheet = shape == "sheet"
    w, h, spp, depth = int(rng.integers(40, 97)), int(rng.integers(24, 57)), int(rng.integers(1, 4)), int(rng.integers(2, 9))
    half = float(rng.uniform(2.0, 6.0))
    n_units = int(rng.integers(140, 340 if shape == "clump" else 560))
    size = float(rng.uniform(1.8, 2.6)) * half / np.sqrt(n_units)
    top = 2.0 * size if sheet else half  # the cloud: [-half, half] x [sheet: 0, volume: -half, top] x [-half, half]
    mid = 0.5 * top if sheet else 0.0
    inside, mirror, mirror_quad, ground = seed % 3 == 0, (seed // 2) % 2 == 0, (seed // 4) % 2 == 1, seed % 5 != 0
    if g.passes:  # a feature pass ends at its first hit: from inside the cloud that lies in the first cell or two, and the
        inside = False  # pass would say little about the walk (measured: DESIGN 7x) -- the passes look on from outside
    lens = g.camera == "fisheye"
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background(_f3(rng.uniform(0.3, 1.0, 3)), sky_gradient=bool(rng.random() < 0.5), defocus_blur=lens)
    sc.set_russian_roulette(0.9 if seed % 4 == 1 else 0.0)
    # the camera: on the +x, +z side of the cloud (the wall stands behind it at -x, the mirror at -z), or inside it
    eye_in = np.array([0.4 * half * rng.uniform(-1, 1), mid + (0.5 * top if sheet else 0.3 * half * rng.uniform(-1, 1)), 0.4 * half * rng.uniform(-1, 1)])
    eye_out = rng.uniform(1.6, 2.4) * half * np.array([rng.uniform(0.3, 1.0), 0.5, 1.0])
    at = np.array([0.2 * half * rng.uniform(-1, 1), mid, 0.2 * half * rng.uniform(-1, 1)])
    fill = float(rng.uniform(0.7, 1.0))
    eye = eye_in if inside else eye_out
    # from outside, the frame's width spans `fill` of the cloud's: most camera rays meet the cloud, not the ground around it
    fov = 35.0 if inside else float(np.degrees(2.0 * np.arctan(fill * half * h / (w * np.linalg.norm(eye_out - at)))))
    if g.camera == "orthographic":    # exactly along -z: every direction has two zero components
        at = np.array([np.float32(at[0]), np.float32(mid if sheet else at[1] + 0.1 * half), 0.0], np.float64)
        eye = np.array([at[0], at[1], np.float32(2.5 * half)], np.float64)
    elif g.camera == "panoramic":     # from inside the cloud
        eye = eye_in
    elif g.camera == "fisheye":       # towards the cloud's centre from halfway out, through a lens
        eye = np.array([0.3 * half, mid + 0.5 * top, 0.6 * half])
    sc.camera(_f3(eye), _f3(at), (0, 1, 0), fov, 0.0, 0.08 * half if lens else 0.0, float(np.linalg.norm(eye - at)) if lens else 0.0)
    if g.camera == "orthographic":
        sc.set_projection("orthographic", (4.0 * size if sheet else 1.6 * half))
    elif g.camera == "panoramic":
        sc.set_projection("panoramic", 360.0, 180.0)
    elif g.camera == "fisheye":
        sc.set_projection("fisheye", 180.0)
    mats, light = _materials(sc)
    add = _Adder(sc, rng)

    def point():
        c = rng.uniform(-half, half, 3)
        if sheet:
            c[1] = rng.uniform(0.0, top)
        return c

    # ---- the always-tested ones: the ground, the wall, the far mirror, a few large spheres, the two long thin ones
    if ground:
        sc.sphere((0.0, -1000.0 - (0.0 if sheet else half), 0.0), 1000.0, mats[1])
    sc.yz_rect(-2.0 * half, 4.0 * half, -4.0 * half, 4.0 * half, -1.5 * half, mats[0])
    far = float(rng.choice([5.0, 12.0, 30.0])) * half
    if mirror and mirror_quad:
        sc.quad((-500.0, -500.0, 0.0), (1000.0, 0.0, 0.0), (0.0, 1000.0, 0.0), sc.metal((0.95, 0.95, 0.95), 0.0), rotate=((0.0, 1.0, 0.0), 8.0),
                translate=(0.0, 0.0, -far))
    elif mirror:
        sc.xy_rect(-500.0, 500.0, -500.0, 500.0, -far, sc.metal((0.95, 0.95, 0.95), 0.0))
    for k in range(3):
        r = (0.5 * top if sheet else 0.12 * half) * float(rng.uniform(0.7, 1.0))
        c = np.array([-0.9 * half, (r if sheet else rng.uniform(-0.5, 0.5) * half), (k - 1) * 0.8 * half])
        sc.sphere(_f3(c), r, mats[3 + k])
    sc.cylinder(0.05 * size, -1.2 * half, 1.2 * half, mats[3], rotate=((0.0, 1.0, 0.0), 75.0), translate=(0.0, mid, 0.1 * half))
    sc.quad((-1.2 * half, mid + 0.2 * size, 0.4 * half), (2.4 * half, 0.0, -0.9 * half), (0.0, 0.06 * size, 0.02 * size), mats[6])
    # ---- boxes that end on common planes: abutting axis-aligned primitives on multiples of 0.5
    y0 = 0.0 if sheet else 0.5
    for i in range(3):
        for j in range(3):
            x, z, m, k = 0.5 * i - 0.5, 0.5 * j - 1.0, mats[(3 * i + j) % len(mats)], (3 * i + j) % 4
            if k == 0:
                sc.xz_rect(x, x + 0.5, z, z + 0.5, y0, m)
            elif k == 1:
                sc.triangle((x, y0, z), (x + 0.5, y0, z), (x, y0, z + 0.5), m, (0.0, 0.0), (1.0, 0.0), (0.0, 1.0))
            elif k == 2:
                sc.quad((x, y0, z), (0.5, 0.0, 0.0), (0.0, 0.0, 0.5), m)
            else:
                sc.xy_rect(x, x + 0.5, y0, y0 + 0.5, z, m)
    # ---- one emitter of every kind that can be one
    for kind in ("sphere", "rect", "cylinder", "quad", "triangle"):
        add(kind, point(), size * float(rng.uniform(0.5, 1.0)), light)
    # ---- the cloud
    kinds = rng.choice(len(add.KINDS), size=n_units, p=[0.34, 0.12, 0.12, 0.11, 0.09, 0.17, 0.05])
    for i in range(n_units):
        add(add.KINDS[kinds[i]], point(), size * float(rng.uniform(0.3, 1.0)), mats[i % len(mats)])
    if shape == "clump":  # a few hundred small ones of mixed kinds within what is about one cell
        centre = np.array([0.3 * half, 0.2 * half, -0.2 * half])
        reach = 0.4 * 2.0 * half / n_units ** (1.0 / 3.0)
        n_clump = int(rng.integers(200, 260))
        ckinds = rng.choice(len(add.KINDS), size=n_clump, p=[0.3, 0.1, 0.1, 0.15, 0.1, 0.2, 0.05])
        for i in range(n_clump):
            add(add.KINDS[ckinds[i]], centre + reach * rng.uniform(-1, 1, 3), 0.12 * reach * float(rng.uniform(0.5, 1.0)), mats[(i + 5) % len(mats)])

    # ---- the family's dress (a stream of its own: the geometry above is every family's)
    fr = np.random.default_rng([seed, 99])
    if g.alpha:  # masks on a third of the static materials; the movers' materials, made below, keep none
        planes = list(AS.PLANES)[:7]
        for k, m in enumerate(mats[::3]):
            plane = AS.PLANES[planes[k % len(planes)]]
            sc.set_alpha(m, sc.image_texture(AS.colours(plane), alpha=plane), 0.5)
    if g.nee:
        sc.set_light_sampling(True)
        sc.set_mesh_lights(True)
        sc.point_light((0.1 * half, mid + 0.25 * top, 0.15 * half), _f3(np.array([1.0, 0.9, 0.8]) * 0.5 * half * half))
        sc.spot_light((-0.3 * half, top + 0.8 * half, 0.2 * half), (0.1, -1.0, -0.05), _f3(np.array([0.8, 0.9, 1.0]) * half * half), 20.0, 35.0)
        sc.distant_light((-0.3, -1.0, -0.2), (1.2, 1.1, 1.0), 1.5)
    if g.env:
        sc.set_environment(*NS._sun_map())
    if g.media:
        sc.add_medium_box((-1.1 * half, -0.05 if sheet else -1.1 * half, -1.1 * half), (1.1 * half, top + 0.5 * half, 1.1 * half), 0.12 / half, (0.9, 0.9, 0.95))
        sc.add_medium_sphere((0.1 * half, mid, -0.1 * half), 0.45 * half, 0.6 / half, (0.8, 0.85, 0.9))
    if g.motion:  # three movers whose paths cross many cells
        mm = [sc.lambertian((0.9, 0.9, 0.2)), sc.metal((0.8, 0.8, 0.8), 0.2), sc.plastic((0.8, 0.2, 0.2), 1.5, 0.3)]
        for k in range(3):
            a, b = fr.uniform(-1, 1, 3) * half, fr.uniform(-1, 1, 3) * half
            a[k], b[k] = -0.9 * half, 0.9 * half
            if sheet:
                a[1], b[1] = (0.5 * top, 0.8 * top) if k != 1 else (0.3 * top, 2.5 * top)
            sc.add_moving_sphere(_f3(a), _f3(b), float(fr.uniform(0.8, 1.6)) * size, mm[k])
    if g.nested:
        sc.set_nested_grid(True)
    return sc


def listed_prims(sc):
    """list indices of the primitives the grid's cells list (every other one is tested for every query)"""
    t, img = sc.table_info(), sc.table_image()
    if t.grid_cells == 0:
        return set()
    word = lambda rec, k: int(img[rec].view(np.uint32)[k])
    out = {word(t.off_sph_cold + slot, 2) for slot in range(t.np, t.ns) if not np.isneginf(img[slot, 3])}
    out |= {word(t.off_rect_cold + j, 1) for j in range(t.nr_a, t.nr)}
    out |= {word(t.off_cyl_cold + 4 * k + 3, 1) for k in range(t.nc_a, t.nc)}
    out |= {word(t.off_tri_cold + 2 * k, 1) for k in range(t.nt_a, t.nt)}
    nq, nq_a = sc.quad_counts()
    out |= {word(t.off_tri_cold + 2 * (t.nt + k), 1) for k in range(nq_a, nq)}
    return out


def cloud_box(sc):
    """the bounds of the listed primitives: where the grid is"""
    from test_tables import other_box
    P, lo, hi = sc.prims(), [], []
    for i in listed_prims(sc):
        if int(P["type"][i]) == 0:
            c, r = P["f"][i][:3].astype(np.float64), abs(float(P["f"][i][3]))
            a, b = c - r, c + r
        else:
            a, b = other_box(P[i])
        lo.append(a), hi.append(b)
    return np.min(lo, axis=0), np.max(hi, axis=0)


def rays(sc, seed):
    """(origins, directions, t_max) of a trace group: N_RAYS rays of trace_cases.make_rays over the cloud's box; every other
    ray has a finite far end, 0.3 to 3 times the box's diagonal away (t_max is in units of the ray's direction)"""
    import trace_cases as TC
    lo, hi = cloud_box(sc)
    o, d = TC.make_rays(lo, hi, n=N_RAYS, seed=int(seed))
    reach = np.random.default_rng([int(seed), 7]).uniform(0.3, 3.0, N_RAYS) * np.sqrt(((hi - lo) ** 2).sum())
    t_max = np.where(np.arange(N_RAYS) % 2 == 0, reach / np.sqrt((d.astype(np.float64) ** 2).sum(axis=1)), np.inf).astype(np.float32)
    return o, d, t_max


def camera_rays(sc):
    """(origins, directions) of Scene.camera_ray at the frame's pixel centres, without those a fisheye leaves outside its circle"""
    w, h = sc.width, sc.height
    o, d = [], []
    for y in range(h):
        for x in range(w):
            a, b, ok = sc.camera_ray((x + 0.5) / (w - 1), (y + 0.5) / (h - 1))
            if ok:
                o.append(a), d.append(b)
    return np.array(o, np.float64), np.array(d, np.float64)
