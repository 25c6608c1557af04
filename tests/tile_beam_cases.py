"""Scenes and the fp32 restatement shared by tests/test_tile_beams.py (CPU) and tests/test_gpu_tile_beams.py (GPU): the camera
ray as render_burst.h forms it and the candidate predicate RT_CAND of the sphere test (render_query.h, render_device.h), in
numpy float32, operation by operation.  fmaf(a, b, c) is evaluated as float32(float64(a) * float64(b) + float64(c)): the
product is exact in fp64, so the value differs from the fused one only where the fp64 sum lands on a float32 tie (a double
rounding, one case in 2^29) -- by one ulp, four orders of magnitude inside the bound's margins."""
import sys

import numpy as np

F = np.float32


def fmaf(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def camera_records(sc):
    """The six camera records of the packed image, the sphere table's slots [n][4], and whether the lens is on."""
    ti, img = sc.table_info(), sc.table_image()
    assert ti.grid_wide == 0 and ti.nr + ti.nc + ti.nt == 0, "a sphere-only scene with compact tables"
    off_cam = ti.off_tri_hot + 5 * ti.nt
    cv = img[off_cam:off_cam + 6].astype(F)
    nslots = ti.np + 9 * ti.ncl
    return cv, img[:nslots].astype(F), bool(sc.info.flags & sys.modules[type(sc).__module__].FLAG_DEFOCUS_BLUR)


def burst_rays(sc, bx, by, ju, jv, lx, ly):
    """o, d of the burst's camera rays (render_burst.h): pixel (bx, by), jitter (ju, jv) in [0, 1), lens sample (lx, ly) in
    the unit disk; arrays of one length, float32 results."""
    cv, _, defocus = camera_records(sc)
    w, h = sc.width, sc.height
    inv_wm1, inv_hm1 = F(1.0) / F(w - 1), F(1.0) / F(h - 1)
    bu = (bx.astype(F) + ju.astype(F)) * inv_wm1
    bv = (by.astype(F) + jv.astype(F)) * inv_hm1
    org, ll, hor, ver, cu, cw = cv[0], cv[1], cv[2], cv[3], cv[4], cv[5]
    off = [np.zeros_like(bu) for _ in range(3)]
    if defocus:
        rdx, rdy = org[3] * lx.astype(F), org[3] * ly.astype(F)
        off = [fmaf(cu[a], rdx, cw[a] * rdy) for a in range(3)]
    d = [fmaf(bv, ver[a], fmaf(bu, hor[a], ll[a])) for a in range(3)]
    d = [((d[a] - org[a]) - off[a]).astype(F) for a in range(3)]
    o = [(org[a] + off[a]).astype(F) for a in range(3)]
    return o, d


def flagged(o, d, slots):
    """[ray][slot]: RT_CAND of RT_SPHERE_TEST for every ray against every slot of the sphere table"""
    ox, oy, oz = (v[:, None] for v in o)
    dx, dy, dz = (v[:, None] for v in d)
    sx, sy, sz, sw = (slots[None, :, k] for k in range(4))
    with np.errstate(invalid="ignore", over="ignore"):
        ocx, ocy, ocz = (ox - sx).astype(F), (oy - sy).astype(F), (oz - sz).astype(F)
        hb = fmaf(ocx, dx, fmaf(ocy, dy, (ocz * dz).astype(F)))
        cc = fmaf(ocx, ocx, fmaf(ocy, ocy, fmaf(ocz, ocz, -sw)))
        ra = fmaf(dx, dx, fmaf(dy, dy, (dz * dz).astype(F)))
        disc = fmaf(hb, hb, -((ra * cc).astype(F)))
        return ~(disc < 0) & ~((hb >= 0) & (cc >= 0))


def tile_samples(sc, tx, ty, n, rng):
    """n random samples of tile (tx, ty) plus the extremes: the tile's corner pixels with the jitter's end values, and the
    rim of the lens."""
    w, h = sc.width, sc.height
    x1, y1 = min(8 * tx + 8, w), min(8 * ty + 8, h)
    bx = rng.integers(8 * tx, x1, n)
    by = rng.integers(8 * ty, y1, n)
    top = 1.0 - 2.0 ** -24
    ju = rng.integers(0, 1 << 24, n) * 2.0 ** -24
    jv = rng.integers(0, 1 << 24, n) * 2.0 ** -24
    lx = np.empty(n)
    ly = np.empty(n)
    for i in range(n):  # random_in_unit_disk's rejection, on the generator's grid of values
        while True:
            a, b = rng.integers(0, 1 << 24, 2) * 2.0 ** -23 - 1.0
            if F(a) * F(a) + F(b) * F(b) < 1.0:
                break
        lx[i], ly[i] = a, b
    th = rng.uniform(0, 2 * np.pi, 64)
    cbx, cby, cju, cjv, clx, cly = [], [], [], [], [], []
    for px, ju_e in ((8 * tx, 0.0), (x1 - 1, top)):
        for py, jv_e in ((8 * ty, 0.0), (y1 - 1, top)):
            for t in th[:16]:
                cbx.append(px), cby.append(py), cju.append(ju_e), cjv.append(jv_e)
                clx.append(np.cos(t) * (1 - 1e-6)), cly.append(np.sin(t) * (1 - 1e-6))
    return (np.concatenate([bx, cbx]), np.concatenate([by, cby]), np.concatenate([ju, cju]), np.concatenate([jv, cjv]),
            np.concatenate([lx, clx]), np.concatenate([ly, cly]))


def film_tile(sc, p):
    """the tile whose beam's middle passes nearest the point p (None: behind the camera or off the frame)"""
    cv, _, _ = camera_records(sc)
    org, ll, hor, ver = (cv[k, :3].astype(np.float64) for k in range(4))
    m = np.stack([hor, ver, -(np.asarray(p, np.float64) - org)], axis=1)
    u, v, mu = np.linalg.solve(m, org - ll)
    if mu <= 0:
        return None
    x, y = u * (sc.width - 1), v * (sc.height - 1)
    if not (0 <= x < sc.width and 0 <= y < sc.height):
        return None
    return int(x) // 8, int(y) // 8


# ---- scenes ----------------------------------------------------------------------------------------------------------

def _mats(sc):
    return [sc.lambertian((0.6, 0.5, 0.4)), sc.metal((0.8, 0.8, 0.9), 0.1), sc.dielectric(1.5),
            sc.lambertian(sc.checker_texture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))]


def layer_scene(rtmi, w, h, spp, eye, lookat, aperture, focus, defocus=True, vfov=30.0, n=120, half=6.0, seed=3, ground=True):
    """a sheet of small spheres on a big ground sphere, two large ones in it: RTIOW's shape, small enough for a quick test"""
    rng = np.random.default_rng(seed)
    sc = rtmi.Scene.new(w, h, spp, 8)
    sc.camera(tuple(eye), tuple(lookat), (0, 1, 0), vfov, 0.0, aperture, focus)
    sc.set_background((0.6, 0.7, 0.9), sky_gradient=True, defocus_blur=defocus)
    m = _mats(sc)
    if ground:
        sc.sphere((0.0, -1000.0, 0.0), 1000.0, m[3])
    sc.sphere((0.0, 1.0, 0.0), 1.0, m[2])
    sc.sphere((-3.0, 1.0, 0.5), 1.0, m[1])
    for i in range(n):
        r = float(rng.uniform(0.1, 0.25))
        c = rng.uniform(-half, half, 3)
        c[1] = r
        sc.sphere(tuple(c), r, m[i % 3])
    return sc


def fuzz_scene(rtmi, seed, sheet):
    """the sheet and volume generators of tests/test_gpu_fuzz.py, at sizes whose tables stay compact"""
    rng = np.random.default_rng(seed)
    n = int(rng.choice([20, 70, 300]))
    half = float(rng.uniform(2.0, 12.0))
    w, h, spp = int(rng.integers(40, 110)), int(rng.integers(24, 60)), int(rng.integers(1, 4))
    sc = rtmi.Scene.new(w, h, spp, int(rng.integers(2, 12)))
    inside = rng.random() < 0.3
    eye = rng.uniform(-0.5, 0.5, 3) * half if inside else rng.uniform(1.5, 3.0) * half * np.array([rng.choice([-1, 1]), 0.4, rng.choice([-1, 1])])
    sc.camera(tuple(eye), tuple(rng.uniform(-0.2, 0.2, 3) * half), (0, 1, 0), float(rng.uniform(25, 70)), 0.0,
              float(rng.choice([0.0, 0.1])), 0.0)
    sc.set_background(tuple(rng.uniform(0.3, 1.0, 3)), sky_gradient=bool(rng.random() < 0.5), defocus_blur=bool(rng.random() < 0.5))
    m = _mats(sc)
    if rng.random() < 0.7:
        sc.sphere((0.0, -1000.0 - (0.0 if sheet else half), 0.0), 1000.0, m[-1])
    for _ in range(int(rng.integers(0, 4))):
        sc.sphere(tuple(rng.uniform(-0.5, 0.5, 3) * half), float(rng.uniform(0.8, 1.5)), m[int(rng.integers(0, len(m)))])
    rmax = float(rng.uniform(0.05, 0.3))
    for i in range(n):
        r = float(rng.uniform(0.3 * rmax, rmax))
        c = rng.uniform(-half, half, 3)
        if sheet:
            c[1] = r
        sc.sphere(tuple(c), r, m[i % len(m)])
    return sc


def row_scene(rtmi, w=64, h=40, spp=8):
    """40 spheres along one line of sight: the middle tiles' lists overflow"""
    sc = rtmi.Scene.new(w, h, spp, 6)
    sc.camera((0.0, 0.0, 10.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0, 0.0, 0.0, 10.0)
    sc.set_background((0.6, 0.7, 0.9), sky_gradient=True, defocus_blur=False)
    m = _mats(sc)
    for i in range(40):
        sc.sphere((0.0, 0.0, 5.0 - 1.0 * i), 0.3 + 0.012 * i, m[i % 3])
    return sc


def sky_scene(rtmi, w=64, h=40, spp=8):
    """the camera looks away from everything: every list is empty"""
    sc = layer_scene(rtmi, w, h, spp, (0.0, 3.0, 12.0), (0.0, 40.0, 60.0), 0.1, 10.0, vfov=20.0, n=40)
    return sc
