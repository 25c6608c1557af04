"""An independent statement of the path estimators of DESIGN 7a (light sampling + MIS), 7e (environment maps), 7f (homogeneous
participating media with isotropic scattering), 7g (motion blur: linearly moving spheres over a per-sample shutter time), 7l
(smooth shading), 7m (the glossy materials), 7n-7u (triangle lights, noise textures, bumps, quads, rough glass, point / spot /
distant lights, the metallic-roughness material, normal maps), 7v (alpha cutouts), 7y (anisotropic media) and 7z (light sampling
in participating media), in NumPy, vectorised over a batch of samples, at a floating type of the caller's choice (float64: the
reference; float32: the same formulas at the kernel's precision, used to measure how many samples sit on a branch).

Test infrastructure only.  It is written from the definitions -- DESIGN 2 (the integrator, the order of the draws), the
sections above, include/rtmi.h's text of the records, and the reference's primitive, material and texture definitions -- with
libm's arccos / arctan2 / log, plain closest-hit loops over the primitive, mover and media lists and no fused operations.  It
shares no code with the kernels or with oracle/.

There is ONE integrator loop, trace(), one hit record, hit_record(), one texture lookup, texture_value(), and one light sample,
sample_light().  An extension joins them with records on RefScene, read ONCE from the product scene (lights, media, movers,
the media's asymmetries, noise parameters, bumps, normal maps, pbr maps, analytic lights, alpha masks: each empty unless the scene
has them) or records the scene's tables already hold (a triangle's vertex normals, a primitive's or a material's type), a branch
in those functions or a block
in the loop, columns or event codes in the signature, counters in trace()'s `log` for what the signature has no column for,
and keys in tally(); its deliberate mistakes are names in trace()'s one `perturb`.  A model large enough for a file of its own
is imported HERE, holds no loop and imports nothing of this file (ref64_base.py holds what they share):
    ref64_glossy            7m  the GGX lobe, rough metal's and plastic's sample and evaluation
    ref64_noise             7o  the lattice noise and the three styles' scalar and colour
    ref64_bump              7p  the analytic gradient of that scalar and the rule that tilts the normal
    ref64_glass             7r  the exact Fresnel term, rough glass's sample and evaluation, the tint
    ref64_analytic_lights   7s  the light records, the three lights' samples
    ref64_pbr               7t  the bytes of a hit, the choice between metal and plastic
    ref64_normal_map        7u  the texel's decoding, every primitive's tangents, the frame and the rule
    ref64_phase             7y  the Henyey-Greenstein distribution, its inverse and density, the frame, a vertex's direction
(triangle lights, 7n, quads, 7q, alpha cutouts, 7v -- opaque_hit(), the query trace() makes -- and a shadow ray's optical depth,
7z -- optical_depth() -- are short enough to stand here).  No module restates trace(), and none swaps a function of this one.  The
reference evaluates the scene it is given: which combinations the product renders is the product's to refuse and test_refusals'
to assert.  Where two extensions meet and DESIGN defines no order -- a shadow ray past a mover, a shadow ray towards the
environment light in a scene with media -- trace() raises NotImplementedError.

Inputs are the product's exported tables (Scene.prims / materials / textures / lights / media / moving_spheres / get_camera /
info / environment / noise / bump / normal_map / pbr_map / analytic_lights / alpha / get_image_alpha / medium_phase), the light
alias table and the environment's CDF tables as the packed image stores them (table_image, found by content), the uniforms of rtmi.sample_stream and, for movers, the
shutter times of rtmi.shutter_time (one per sample: the time is no draw of the stream) and the pixels of the image textures
(Scene.get_image).  Out of scope: the nested grid (a candidate search, which this reference has none of: it scans the lists).

trace() returns, per sample, the radiance, an event signature (one row of integers: per vertex the primitive hit, the mover
that took over, the set of media that took a free-flight draw and the medium whose event won, what the material did, the
checker parity, the image texel read, the roulette outcome, the light and texel picked and whether through the alias, the
shadow ray's verdict, the primitive that stopped it and the media it stayed in, how an emitter hit was weighted; columns a scene
does not exercise stay NONE; two samples took the same branches iff their rows are equal; tally() counts the special vertices of a batch from
it) and the number of draws consumed.
"""
import numpy as np

import ref64_analytic_lights as AL
import ref64_bump as BU
import ref64_glass as GL
import ref64_noise as NO
import ref64_normal_map as NM
import ref64_pbr as PB
import ref64_phase as PH
from ref64_base import SPHERE, XY_RECT, XZ_RECT, YZ_RECT, CYLINDER, TRIANGLE, QUAD, _affine, _cross, _dot, _rect_axes, _unit
from ref64_glossy import (ROUGH_METAL, PLASTIC, GLOSSY_MIN_ROUGHNESS, GLOSSY_EVENTS, EV_ROUGH, EV_COAT, EV_BODY, EV_BELOW,
                          EV_ROUGH_ABSORBED, EV_COAT_ABSORBED, alpha_of, r0_of, glossy_sample, glossy_eval, glossy_tally)

LAMBERTIAN, METAL, DIELECTRIC, DIFFUSE_LIGHT = range(4)  # (ref64_glossy: ROUGH_METAL, PLASTIC = 4, 5)
ROUGH_GLASS, PBR = 6, 7
SOLID, CHECKER, IMAGE, NOISE = range(4)
ENVIRONMENT = 100
POINT, SPOT, DISTANT = AL.POINT, AL.SPOT, AL.DISTANT
DELTA_LIGHTS = (POINT, SPOT, DISTANT)
# the counters of trace()'s `log`: what the signature has no column for.  bump_* / nm_*: perturbed vertices in all, on back faces,
# (nm) whose texel tilts, and where a guard kept n (nm: the texel tilts and the frame was built).  alpha_*: opaque_hit()'s counters.
# ended_by_depth: the paths that scattered with no depth left
ALPHA_COUNTERS = ("masked_hits", "passes", "opaque", "max_passes", "shadow_through", "shadow_queries", "path_queries")
LOG_KEYS = (("bump_bumped", "bump_back", "bump_kept", "nm_mapped", "nm_back", "nm_tilting", "nm_kept", "quad_back_hits", "ended_by_depth")
            + GL.LOG_KEYS + AL.LOG_KEYS + PB.LOG_KEYS + tuple("alpha_" + k for k in ALPHA_COUNTERS))


def new_log():
    """the counters at 0 and alpha_masked_samples, the set of the samples that met a masked hit"""
    return dict(dict.fromkeys(LOG_KEYS, 0), alpha_masked_samples=set())
MEDIUM_SPHERE, MEDIUM_BOX = 0, 1
T_MIN = 0.001           # hittable_list::hit's t_min of every query
SHADOW_T_MAX = 0.999    # a shadow ray ends just short of its light point
METAL_MIN_FUZZ = 0.05   # metal vertices below this fuzz take no light sample

# event codes of the signature
EV_MISS, EV_EMIT, EV_LAMBERT, EV_METAL, EV_METAL_ABSORBED, EV_REFLECT, EV_REFRACT = range(7)
EV_MEDIUM, EV_MEDIUM_HG = 20, 21  # a medium vertex whose stored g is 0 (the rejection loop) / is not (two draws)
MEDIUM_EVENTS = (EV_MEDIUM, EV_MEDIUM_HG)
NONE = -9
# the signature's columns: two per sample (draws consumed, the first roulette), then one block per vertex.  C_PRIM is the static
# winner; C_MOVER the mover that took over (-1: none) in a scene with movers; C_DREW the set of media that took a free-flight
# draw and C_MEDIUM the medium whose event won (-1: none) in a scene with media
SAMPLE_COLUMNS = 2
# C_IMAGE_TEXEL the flat index (row x cols + col) of the image texel the vertex's material read; C_BLOCKER the primitive that
# stopped the shadow ray.  C_TEXEL is the texel the environment light's sample picked and, in a scene with media, the set of
# media the shadow ray stayed in (C_STAYS): a shadow ray towards the environment in a scene with media raises, so the column is
# NONE at every vertex of such a scene until the stays are written
(C_PRIM, C_MISS_TEXEL, C_PARITY, C_EVENT, C_ROULETTE, C_LIGHT, C_TEXEL, C_SHADOW, C_HIT_WEIGHT, C_ALIAS,
 C_MOVER, C_DREW, C_MEDIUM, C_IMAGE_TEXEL, C_BLOCKER) = range(15)
VERTEX_COLUMNS = 15
C_STAYS = C_TEXEL
# C_SHADOW: the light sample reached its light / was occluded / had zero weight (no shadow ray) / was not made because the
# vertex lies inside the sphere light it picked
SHADOW_CLEAR, SHADOW_OCCLUDED, SHADOW_NONE, SHADOW_INSIDE = range(4)
# C_HIT_WEIGHT, on an emitter hit: weighted by MIS / full weight because the ray's vertex took no light sample (a camera ray, a
# dielectric, a near-mirror, an emitter that is no listed light) / full weight because the ray started inside the sphere light
HIT_MIS, HIT_UNSAMPLED, HIT_FROM_INSIDE = range(3)


# ---------------------------------------------------------------------------------------------------------------- tables
def find_alias_table(image, lights):
    """(threshold[nl], alias[nl]) of the packed image: the light records are found by their content (selection probability and
    emission of every light at the record stride of 7 x 4 words), the alias table follows the last record."""
    nl = len(lights)
    w = np.ascontiguousarray(image, np.float32).reshape(-1)
    bits = w.view(np.int32)
    stride = 28
    prob = lights["probability"].astype(np.float32)
    cand = np.flatnonzero(w[2::4] == prob[0]) * 4
    starts = []
    for k in cand:
        if k + stride * nl + 4 * nl > w.size:
            continue
        rec = w[k:k + stride * nl].reshape(nl, stride)
        area = lights["shape"] != ENVIRONMENT  # (the environment's record holds no emission)
        if (np.array_equal(rec[:, 2], prob) and np.array_equal(rec[area, 4:7], lights["emission"][area])
                and np.array_equal(rec[area, 8:11], lights["emission_odd"][area])
                and np.allclose(rec[:, 3], 1.0 / lights["area"].astype(np.float64), rtol=1e-6)):
            starts.append(int(k))
    if len(starts) != 1:
        raise AssertionError(f"light records found {len(starts)} times in the packed image")
    at = starts[0] + stride * nl
    thr = w[at:at + 4 * nl:4].copy()
    ali = bits[at + 1:at + 4 * nl:4].copy()
    return thr, ali


def find_env_tables(image, texels):
    """(marg, cond, band, ct) as the packed image holds them behind the texels (fp32)"""
    rows, cols = texels.shape[:2]
    w = np.ascontiguousarray(image, np.float32).reshape(-1)
    env = texels.reshape(-1)
    n = env.size
    tail = (rows + 1) + rows * (cols + 1) + rows + (rows + 1)
    starts = []
    for k in np.flatnonzero(w[:w.size - n - tail + 1] == env[0]):
        if k % 4 or not np.array_equal(w[k:k + n], env):
            continue
        at = k + n
        # (a 1 x 1 map is three words: the tables behind it decide which match is the environment)
        if w[at] == 0 and w[at + rows] == 1 and w[at + tail - rows - 1] == 1 and w[at + tail - 1] == -1:
            starts.append(int(at))
    if len(starts) != 1:
        raise AssertionError(f"environment texels found {len(starts)} times in the packed image")
    at = starts[0]
    marg = w[at:at + rows + 1].copy(); at += rows + 1
    cond = w[at:at + rows * (cols + 1)].reshape(rows, cols + 1).copy(); at += rows * (cols + 1)
    band = w[at:at + rows].copy(); at += rows
    ct = w[at:at + rows + 1].copy()
    return marg, cond, band, ct


class RefScene:
    """What trace() reads, taken from a product Scene.  nee=False, movers=False, media=False take the plain twin's view: the
    scene with that extension left out."""

    def __init__(self, sc, nee=None, movers=True, media=True):
        info = sc.info
        self.width, self.height, self.max_depth = info.width, info.height, info.max_depth
        self.flags, self.background, self.rr = info.flags, np.array(info.background[:], np.float32), np.float32(info.russian_roulette)
        cam = sc.get_camera()
        self.cam = {k: np.array(getattr(cam, k)[:], np.float32) for k in ("origin", "lower_left", "horizontal", "vertical", "u", "v")}
        self.lens_radius = np.float32(cam.lens_radius)
        self.prims, self.mats, self.texs = sc.prims(), sc.materials(), sc.textures()
        self.images = {ti: sc.get_image(ti) for ti, t in enumerate(self.texs) if t["type"] == IMAGE}  # (rows, cols, 3) uint8
        self.env = None
        environment = sc.environment
        self.nee = sc.light_sampling if nee is None else bool(nee)
        self.lights = sc.lights() if self.nee else sc.lights()[:0]
        image = sc.table_image() if (environment is not None or len(self.lights)) else None
        if environment is not None:
            tex, scale, rotate = environment
            t = float(rotate) / 360.0
            t -= np.floor(t)
            uoff = np.float32(t)
            marg, cond, band, ct = find_env_tables(image, tex)
            self.env = dict(tex=tex, scale=np.float32(scale), uoff=uoff if uoff < 1 else np.float32(0), marg=marg, cond=cond, band=band, ct=ct)
        self.thr = self.alias = None
        if len(self.lights):
            if not sc.light_sampling:
                raise ValueError("the alias table only exists while the scene's light sampling is on")
            self.thr, self.alias = find_alias_table(image, self.lights)
        self.light_of_prim = {int(l["prim"]): i for i, l in enumerate(self.lights) if l["prim"] >= 0}
        self.movers = sc.moving_spheres() if movers else sc.moving_spheres()[:0]
        self.media = sc.media() if media else sc.media()[:0]
        self.media_g = np.array([sc.medium_phase(i) for i in range(len(self.media))], np.float32)  # the stored asymmetries (7y)
        # the extensions' records, each empty unless the scene has them.  noise: texture -> the dict of Scene.noise; bumps:
        # material -> (the height field's noise parameters, strength); normal_maps: material -> (image texture, scale); pbr_maps:
        # pbr material -> its metallic-roughness map's texture or -1; analytic: index into lights -> ref64_analytic_lights.record;
        # alpha_masks: material -> (the mask's alpha plane [rows][cols] uint8, c8)
        materials = range(len(self.mats))
        self.noise = {ti: sc.noise(ti) for ti, t in enumerate(self.texs) if t["type"] == NOISE}
        self.bumps = {m: (self.noise[int(b[0])], np.float32(b[1])) for m in materials for b in [sc.bump(m)] if b is not None}
        self.normal_maps = {m: (int(b[0]), np.float32(b[1])) for m in materials for b in [sc.normal_map(m)] if b is not None}
        self.pbr_maps = {m: -1 if mp is None else int(mp) for m in materials if self.mats["type"][m] == PBR for mp in [sc.pbr_map(m)]}
        self.alpha_masks = {m: (sc.get_image_alpha(int(a[0])), cutoff_byte(a[1])) for m in materials for a in [sc.alpha(m)] if a is not None}
        self.analytic = {}
        at = [i for i, l in enumerate(self.lights) if l["shape"] in DELTA_LIGHTS]
        if at:  # (a light whose weight is not positive and finite is in neither list)
            radius = AL.bound_radius(self.prims)
            recs = [r for r in (AL.record(al, radius) for al in sc.analytic_lights()) if r["weight"] > 0 and np.isfinite(r["weight"])]
            assert [self.lights[i]["shape"] for i in at] == [r["type"] for r in recs], (at, [r["type"] for r in recs])
            self.analytic = dict(zip(at, recs))


def uniforms(rtmi, seed, width, height, first, count, n):
    """uint32 words [count * height * width][n] of rtmi.sample_stream, samples ordered (sample, y, x)"""
    out = np.empty((count, height * width, n), np.uint32)
    for k in range(count):
        for pix in range(height * width):
            out[k, pix] = rtmi.sample_stream(seed, pix, first + k, n)
    return out.reshape(-1, n)


# ---------------------------------------------------------------------------------------------------------------- geometry
def quad_record(pr, T):
    """(Q, u, v, n, A, B) of a quad's rt_prim record: the corner, the edges and, derived by the host in fp64 and rounded
    once, the unit normal n = c / |c| (c = u x v) and A = v x w, B = w x u with w = c / (c.c)"""
    m, mi = pr["m"].astype(T), pr["m_inv"].astype(T)
    return m[0:3], m[3:6], m[6:9], m[9:12], mi[0:3], mi[3:6]


def quad_ab(pr, o, d, t, T):
    """a = A.(p - Q), b = B.(p - Q) of the point p = o + t d: the quad holds p iff both lie in [0, 1]; its record's (u, v)"""
    Q, _, _, _, A, B = quad_record(pr, T)
    r = o + t[:, None] * d - Q
    return _dot(A[None, :], r), _dot(B[None, :], r)


def quad_t(pr, o, d, T):
    """t = n.(Q - o) / n.d where den = n.d is finite and not zero and the quad holds the point (any t: the caller applies the
    range), NaN elsewhere"""
    Q, _, _, n, _, _ = quad_record(pr, T)
    with np.errstate(all="ignore"):
        den = _dot(d, n[None, :])
        t = _dot(n[None, :], Q - o) / den
        a, b = quad_ab(pr, o, d, t, T)
        ok = (den != 0) & np.isfinite(den) & (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
    return np.where(ok, t, T(np.nan)).astype(T)


def _triangle_plane(p, o, d, dd, T):
    """hit_triangle up to its range test: (the plane point r, theta = d.n / |d| with the stored normal n turned to the origin's
    side, (o - v1).n, the four same-side tests all > 0).  The ray is rejected unless theta < 0."""
    m = p["m"].astype(T)
    v1, v2, v3, n0 = m[0:3], m[3:6], m[6:9], m[9:12]
    oc = o - v1
    n = np.where((_dot(oc, n0) < 0)[:, None], -n0, n0)
    a = np.sqrt(dd)
    with np.errstate(all="ignore"):
        theta = _dot(d, n) / a
        ocn = _dot(oc, n)
        r = o - d / a[:, None] * ocn[:, None] / theta[:, None]
        n1 = _dot(_cross(r - v1, v2 - v1), _cross(v3 - v1, v2 - v1))
        n2 = _dot(_cross(r - v2, v1 - v2), _cross(v3 - v2, v1 - v2))
        n3 = _dot(_cross(r - v1, v3 - v1), _cross(v2 - v1, v3 - v1))
        n4 = _dot(_cross(r - v2, v3 - v2), _cross(v1 - v2, v3 - v2))
        inside = (n1 > 0) & (n2 > 0) & (n3 > 0) & (n4 > 0)
    return r, theta, ocn, inside


def _prim_t(p, o, d, dd, t_min, best, T):
    """ray parameter at which the primitive's own hit() accepts the ray within [t_min, best], NaN where it does not"""
    nan = T(np.nan)
    ty = int(p["type"])
    f = p["f"].astype(T)
    with np.errstate(all="ignore"):
        if ty == SPHERE:
            oc = o - f[:3]
            hb = _dot(oc, d)
            disc = hb * hb - dd * (_dot(oc, oc) - f[3] * f[3])
            sq = np.sqrt(np.maximum(disc, 0))
            r1, r2 = (-hb - sq) / dd, (-hb + sq) / dd
            first = (r1 >= t_min) & (r1 <= best)
            return np.where(disc < 0, nan, np.where(first, r1, r2))
        if ty in (XY_RECT, XZ_RECT, YZ_RECT):
            ka, aa, ba = _rect_axes(ty)
            t = (f[4] - o[:, ka]) / d[:, ka]
            a, b = o[:, aa] + t * d[:, aa], o[:, ba] + t * d[:, ba]
            inside = (a >= f[0]) & (a <= f[1]) & (b >= f[2]) & (b <= f[3])
            return np.where(inside, t, nan)
        if ty == TRIANGLE:
            _, theta, ocn, inside = _triangle_plane(p, o, d, dd, T)
            return np.where((theta < 0) & inside, -ocn / theta / np.sqrt(dd), nan)
        if ty == QUAD:
            return quad_t(p, o, d, T)
        # open tube about the object-space z axis
        R, tr = _affine(p["m_inv"], T)
        oo, od = o @ R.T + tr, d @ R.T
        A = od[:, 0] ** 2 + od[:, 1] ** 2
        B = 2 * (od[:, 0] * oo[:, 0] + od[:, 1] * oo[:, 1])
        Cq = oo[:, 0] ** 2 + oo[:, 1] ** 2 - f[0] * f[0]
        delta = B * B - 4 * A * Cq
        sq = np.sqrt(np.maximum(delta, 0))
        ta, tb = -0.5 * (B - sq) / A, -0.5 * (B + sq) / A
        t0, t1 = np.minimum(ta, tb), np.maximum(ta, tb)
        in_z = lambda t: (oo[:, 2] + t * od[:, 2] >= f[1]) & (oo[:, 2] + t * od[:, 2] <= f[2])
        near_ok = (t0 >= t_min) & (t0 <= best) & in_z(t0)   # the near wall, within range and between the ends
        far_ok = (t1 >= t_min) & (t1 <= best) & in_z(t1)    # else the far wall (seen through an open end, or from inside)
        t = np.where(near_ok, t0, np.where(far_ok, t1, nan))
        # the near root beyond the range ends the test (cylinder::hit returns before it tries the far one)
        t = np.where((delta < 0) | (t0 > best) | (t1 < t_min), nan, t)
        return t


def closest_hit(S, o, d, t_max, T):
    """hittable_list::hit: primitives in list order, a hit is accepted while t_min <= t <= the closest so far (ties: the later)"""
    n = len(o)
    best = np.full(n, t_max, T) if np.isscalar(t_max) else t_max.astype(T).copy()
    idx = np.full(n, -1, np.int64)
    dd = _dot(d, d)
    t_min = T(T_MIN)
    for i, p in enumerate(S.prims):
        t = _prim_t(p, o, d, dd, t_min, best, T)
        with np.errstate(invalid="ignore"):
            ok = (t >= t_min) & (t <= best)
        best = np.where(ok, t, best)
        idx = np.where(ok, i, idx)
    return best, idx


def prim_normals(p):
    """(n1, n2, n3) [3][3] of an rt_prim record: f[0..5] and m_inv[6..8]; all zero on a triangle without vertex normals"""
    return np.concatenate([p["f"][:6], p["m_inv"][6:9]]).reshape(3, 3)


def has_normals(p):
    return bool(np.any(prim_normals(p) != 0))


def shading_normal(pr, o, d, g, T):
    """s = a1 n1 + a2 n2 + a3 n3, each corner's normal by the area of the sub-triangle opposite it over the whole (the
    weight that is 1 at the corner): the three area weights of hit_uv, where w1 = (r, v1, v2) is corner 3's, w2 = (r, v1, v3)
    corner 2's and w3 = (r, v3, v2) corner 1's.  Normalised, turned into the hemisphere of the face-turned geometric normal g;
    s zero or not finite: g.  In dtype T, the plane point as the triangle test derives it."""
    m = pr["m"].astype(T)
    v1, v2, v3 = m[0:3], m[3:6], m[6:9]
    n1, n2, n3 = prim_normals(pr).astype(T)
    r, _, _, _ = _triangle_plane(pr, o, d, _dot(d, d), T)
    norm = lambda a: np.sqrt(_dot(a, a))
    with np.errstate(all="ignore"):
        w1 = norm(_cross(r - v1, r - v2)) / norm(_cross(v3 - v1, v3 - v2))
        w2 = norm(_cross(r - v1, r - v3)) / norm(_cross(v2 - v1, v2 - v3))
        w3 = norm(_cross(r - v3, r - v2)) / norm(_cross(v1 - v3, v1 - v2))
        s = w3[:, None] * n1 + w2[:, None] * n2 + w1[:, None] * n3
        l2 = _dot(s, s)
        ok = np.isfinite(l2) & (l2 > 0)
        s = s / np.sqrt(l2)[:, None]
        s = np.where((_dot(s, g) < 0)[:, None], -s, s)
    return np.where(ok[:, None], s, g).astype(T)


def hit_record(S, o, d, t, idx, T, perturb=(), log=None):
    """point and face-turned normal of accepted hits; front = the ray meets the outward side.  On a triangle that carries vertex
    normals and whose material is no emitter the normal is the shading normal (front stays the geometric side); "flat_normals"
    leaves the geometric normal there too.  Then the material's bump or its normal map (7u) tilts that normal about
    the geometric one: the product refuses both on one material, so the order in which they stand here is no statement.  Movers
    do not come here: the product refuses a bumped or mapped mover."""
    p = o + t[:, None] * d
    n_out = np.zeros_like(o)
    quad = np.zeros(len(o), bool)
    for i in np.unique(idx):
        m = idx == i
        pr = S.prims[i]
        ty, f = int(pr["type"]), pr["f"].astype(T)
        if ty == QUAD:
            n_out[m], quad[m] = quad_record(pr, T)[3], True
        elif ty == SPHERE:
            n_out[m] = (p[m] - f[:3]) / f[3]
        elif ty == CYLINDER:
            R, tr = _affine(pr["m_inv"], T)
            op = p[m] @ R.T + tr
            radial = np.stack([op[:, 0], op[:, 1], np.zeros_like(op[:, 0])], axis=1)
            radial /= np.sqrt(_dot(radial, radial))[:, None]
            n_out[m] = radial @ R  # apply_normal: the transpose of the inverse
        elif ty == TRIANGLE:
            n_out[m] = pr["m"][9:12].astype(T)  # the stored unit normal
        else:
            n_out[m, _rect_axes(ty)[0]] = 1
    front = _dot(d, n_out) < 0
    g = np.where(front[:, None], n_out, -n_out)
    if "quad_front_flipped" in perturb:
        front = front ^ quad
    if log is not None:
        log["quad_back_hits"] += int((quad & ~front).sum())
    n = g.copy()
    for i in (() if "flat_normals" in perturb else np.unique(idx)):
        pr = S.prims[i]
        if int(pr["type"]) == TRIANGLE and has_normals(pr) and int(S.mats["type"][pr["material"]]) != DIFFUSE_LIGHT:
            m = idx == i
            n[m] = shading_normal(pr, o[m], d[m], n[m], T)
    mat = S.prims["material"][idx]
    for m in (() if "bump_off" in perturb else np.unique(mat[np.isin(mat, list(S.bumps))])):
        sel = mat == m
        par, k = S.bumps[int(m)]
        n[sel], ok = BU.bump(n[sel], g[sel], d[sel], front[sel], k, BU.gradient_of(p[sel], par, T, perturb), T, perturb)
        if log is not None:
            log["bump_bumped"] += int(sel.sum())
            log["bump_back"] += int((~front[sel]).sum())
            log["bump_kept"] += int((~ok).sum())
    mapped = np.isin(mat, list(S.normal_maps))
    if mapped.any() and "nm_off" not in perturb:
        u, v = hit_uv(S, o, d, t, idx, T, perturb=perturb)
        for i in np.unique(idx[mapped]):
            sel = idx == i
            tex, s = S.normal_maps[int(S.prims["material"][i])]
            img = S.images[tex]
            row, col = image_texel(img, u[sel], v[sel], T, perturb)
            xyz, active = NM.decode(img[row, col], T, perturb)
            Tr, Br = NM.raw_tangents(S.prims[i], p[sel], T)
            parts = {}
            n[sel], ok = NM.normal(n[sel], g[sel], d[sel], front[sel], s, Tr, Br, xyz, active, T, perturb, parts)
            if log is not None:
                log["nm_mapped"] += int(sel.sum())
                log["nm_back"] += int((~front[sel]).sum())
                log["nm_tilting"] += int(active.sum())
                log["nm_kept"] += int((active & parts["usable"] & ~ok).sum())
    return p, n, front


def mover_centre(m, s, T):
    """c(s) = center0 + s v, with v = center1 - center0 as the scene keeps it: one fp32 subtraction per component"""
    v = (m["center1"].astype(np.float32) - m["center0"].astype(np.float32)).astype(T)
    return m["center0"].astype(T) + s.astype(T)[:, None] * v


def mover_t(m, s, o, d, dd, t_min, best, T):
    """sphere::hit against (c(s), radius): the near root where it lies in [t_min, best], else the far one; NaN without a real root"""
    oc = o - mover_centre(m, s, T)
    r = T(m["radius"])
    with np.errstate(all="ignore"):
        hb = _dot(oc, d)
        disc = hb * hb - dd * (_dot(oc, oc) - r * r)
        sq = np.sqrt(np.maximum(disc, 0))
        r1, r2 = (-hb - sq) / dd, (-hb + sq) / dd
        first = (r1 >= t_min) & (r1 <= best)
        return np.where(disc < 0, T(np.nan), np.where(first, r1, r2))


def medium_interval(m, o, d, t_s, T):
    """[a, b]: the stay of the rays o + t d inside the boundary of medium m, clipped to [0.001, t_s]; non-empty where a < b"""
    f = m["f"].astype(T)
    a = np.full(len(o), T(T_MIN), T)
    b = t_s.astype(T).copy()
    with np.errstate(all="ignore"):
        if int(m["shape"]) == MEDIUM_SPHERE:
            oc = o - f[:3]
            A = _dot(d, d)
            hb = _dot(oc, d)
            disc = hb * hb - A * (_dot(oc, oc) - f[3] * f[3])
            sq = np.sqrt(np.maximum(disc, 0))
            a = np.maximum(a, (-hb - sq) / A)
            b = np.minimum(b, (-hb + sq) / A)
            ok = (disc > 0) & (a < b)
        else:
            for k in range(3):
                inv = T(1) / d[:, k]
                t0, t1 = (f[k] - o[:, k]) * inv, (f[3 + k] - o[:, k]) * inv
                lo, hi = np.where(inv < 0, t1, t0), np.where(inv < 0, t0, t1)
                a = np.where(lo > a, lo, a)
                b = np.where(hi < b, hi, b)
            ok = a < b
    return a, b, ok


def optical_depth(S, o, d, t_max, T):
    """(tau, the set of media with a non-empty stay) of the segments o + t d, t in [0.001, t_max]: every medium of
    positive density, in list order, adds sigma (b - a) |d| of its stay [a, b].  No draw is taken"""
    tau = np.zeros(len(o), T)
    stays = np.zeros(len(o), np.int64)
    length = np.sqrt(_dot(d, d))
    far = np.full(len(o), t_max, T)
    for mi, m in enumerate(S.media):
        sigma = T(m["density"])
        if not sigma > 0:
            continue
        a, b, ok = medium_interval(m, o, d, far, T)
        tau = np.where(ok, tau + sigma * (b - a) * length, tau)
        stays |= np.where(ok, 1 << mi, 0)
    return tau, stays


def phase_density(g, c, T):
    """the phase function's density per steradian at cos t = c, per vertex: 1 / (4 pi) where the asymmetry g (fp64) is 0"""
    out = np.full(len(g), T(1.0 / (4.0 * np.pi)), T)
    k = g != 0
    if k.any():
        out[k] = PH.hg_density(g[k], c[k])
    return out


def checker_odd(p, T):
    """sign of sin(10x) sin(10y) sin(10z) < 0, as the parity of the three floors (a zero factor: even)"""
    k = np.floor(T(10) * p / T(np.pi)).astype(np.int64).sum(axis=1)
    return (k % 2 != 0) & ~(p == 0).any(axis=1)


def sphere_uv(n, T):
    """get_sphere_uv of a unit outward normal: u from the azimuth atan2(-z, x) + pi, v from the polar angle acos(-y)"""
    pi = T(np.pi)
    return (np.arctan2(-n[:, 2], n[:, 0]) + pi) / (2 * pi), np.arccos(-n[:, 1]) / pi


def hit_uv(S, o, d, t, idx, T, mov=None, time=None, perturb=()):
    """the hit record's (u, v) of accepted hits: of the static primitive idx, or of mover mov >= 0 at the samples' shutter times"""
    u, v = np.zeros(len(o), T), np.zeros(len(o), T)
    static = np.ones(len(o), bool) if mov is None else mov < 0
    with np.errstate(all="ignore"):
        for mi in (() if mov is None else np.unique(mov[~static])):
            k = mov == mi
            mv = S.movers[mi]
            n_out = (o[k] + t[k][:, None] * d[k] - mover_centre(mv, time[k], T)) / T(mv["radius"])
            u[k], v[k] = sphere_uv(n_out, T)
        for i in np.unique(idx[static]):
            k = static & (idx == i)
            pr = S.prims[i]
            ty, f = int(pr["type"]), pr["f"].astype(T)
            oo, dd, tt = o[k], d[k], t[k]
            if ty == SPHERE:
                u[k], v[k] = sphere_uv((oo + tt[:, None] * dd - f[:3]) / f[3], T)
            elif ty in (XY_RECT, XZ_RECT, YZ_RECT):
                _, aa, ba = _rect_axes(ty)
                u[k] = (oo[:, aa] + tt * dd[:, aa] - f[0]) / (f[1] - f[0])
                v[k] = (oo[:, ba] + tt * dd[:, ba] - f[2]) / (f[3] - f[2])
            elif ty == CYLINDER:
                R, tr = _affine(pr["m_inv"], T)
                op = (oo @ R.T + tr) + tt[:, None] * (dd @ R.T)
                u[k] = (np.arctan2(op[:, 1], op[:, 0]) + 2 * T(np.pi)) / (4 * T(np.pi))
                v[k] = (op[:, 2] - f[1]) / (f[2] - f[1])
            elif ty == QUAD:
                a, b = quad_ab(pr, oo, dd, tt, T)
                u[k], v[k] = (b, a) if "quad_uv_swapped" in perturb else (a, b)
            else:
                # the area weights of the plane point, each with the corner the reference pairs it with: the sub-triangle
                # (r, v1, v2) over the whole goes with u1, (r, v1, v3) with u2, (r, v3, v2) with u3
                m = pr["m"].astype(T)
                v1, v2, v3 = m[0:3], m[3:6], m[6:9]
                c = pr["m_inv"].astype(T)
                uv1, uv2, uv3 = c[0:2], c[2:4], c[4:6]
                if "tri_natural_pairing" in perturb:  # each weight with the corner opposite its sub-triangle
                    uv1, uv3 = uv3, uv1
                r, _, _, _ = _triangle_plane(pr, oo, dd, _dot(dd, dd), T)
                norm = lambda a: np.sqrt(_dot(a, a))
                w1 = norm(_cross(r - v1, r - v2)) / norm(_cross(v3 - v1, v3 - v2))
                w2 = norm(_cross(r - v1, r - v3)) / norm(_cross(v2 - v1, v2 - v3))
                w3 = norm(_cross(r - v3, r - v2)) / norm(_cross(v1 - v3, v1 - v2))
                u[k] = uv1[0] * w1 + uv2[0] * w2 + uv3[0] * w3
                v[k] = uv1[1] * w1 + uv2[1] * w2 + uv3[1] * w3
    return u, v


def image_texel(img, u, v, T, perturb=()):
    """(row, col) of texel[int(frac(u) rows)][int(frac(v) cols)]: u indexes ROWS; clamped to the last row and column"""
    rows, cols = img.shape[:2]
    if "uv_transposed" in perturb:
        u, v = v, u
    with np.errstate(invalid="ignore"):
        row = np.nan_to_num((u - np.floor(u)) * T(rows)).astype(np.int64).clip(0, rows - 1)
        col = np.nan_to_num((v - np.floor(v)) * T(cols)).astype(np.int64).clip(0, cols - 1)
    return row, col


def texture_value(S, tex, p, T, o=None, d=None, t=None, idx=None, mov=None, time=None, perturb=()):
    """(colour, flat index of the image texel read or NONE) of the textures `tex` at the hits: a solid colour, the checker's
    parity at the point p, the noise texture's colour at p, or the image's texel at the hit record's (u, v), which needs the ray (o, d), its parameter t, the
    static primitive idx, and the mover that took over with the samples' shutter times"""
    out = np.zeros_like(p)
    texel = np.full(len(p), NONE, np.int64)
    for ti in np.unique(tex):
        m = tex == ti
        tx = S.texs[ti]
        c0, c1 = tx["c0"].astype(T), tx["c1"].astype(T)
        if tx["type"] == IMAGE:
            img = S.images[int(ti)]
            u, v = hit_uv(S, o[m], d[m], t[m], idx[m], T, None if mov is None else mov[m], None if time is None else time[m], perturb)
            row, col = image_texel(img, u, v, T, perturb)
            out[m] = img[row, col].astype(T) / T(255)
            texel[m] = row * img.shape[1] + col
        elif tx["type"] == NOISE:
            out[m] = NO.colour(p[m], tx["c0"], tx["c1"], S.noise[int(ti)], T, perturb)
        else:
            out[m] = np.where(checker_odd(p[m], T)[:, None], c1, c0) if tx["type"] == CHECKER else c0
    return out, texel


def metal_pdf(w, r, f, T):
    """solid-angle density at unit w of d = r + f s, s uniform in the unit ball: the length of the ray t w inside the ball of
    radius f about r, weighted by t^2 and normalised by the ball's volume"""
    wr = _dot(w, r)
    disc = wr * wr - (1 - f * f)
    sq = np.sqrt(np.maximum(disc, 0))
    t1, t0 = wr + sq, np.maximum(wr - sq, 0)
    pdf = (t1 ** 3 - t0 ** 3) / (4 * T(np.pi) * f ** 3)
    return np.where((disc >= 0) & (t1 > 0), pdf, 0).astype(T)


# ---------------------------------------------------------------------------------------------------------------- alpha cutouts
CAP = 64  # one query passes through at most this many transparent hits


def cutoff_byte(cutoff):
    """c8 = clamp(ceil(255 cutoff), 1, 255), in fp64"""
    return int(min(max(np.ceil(255.0 * np.float64(cutoff)), 1.0), 255.0))


def opaque_hit(S, o, d, t_max, T, perturb=(), log=None, samples=None, depth=None, on_pass=None):
    """DESIGN 7v, from the model's text in include/rtmi.h: the closest hit that is no hole, as (total t from o, the opaque winner
    or -1); a scalar t_max is a path query, an array of far ends a shadow query.  A material's mask is read at the hit record's
    (u, v) with image_texel's nearest texel; with a8 the alpha byte there the hit is transparent iff a8 < c8.  A transparent hit is
    no vertex: the query goes on from o + t d in the same direction with the usual t_min and t_max - t left of its range, and
    nothing else happens.  One query passes through at most CAP transparent hits: the next masked hit counts as opaque whatever
    its texel says.  Without masks this is closest_hit()'s result as it stands.
    log: counts into its alpha_* keys; samples: the rays' sample indices (for the log); depth: trace()'s counters, for
    "al_counts_bounce"; on_pass(samples or None, points, directions): called with the hole points of every round of passes"""
    shadow = not np.isscalar(t_max)
    masks = {} if "al_off" in perturb or (shadow and "al_shadow_opaque" in perturb) else S.alpha_masks
    n = len(o)
    if log is not None:
        log["alpha_shadow_queries" if shadow else "alpha_path_queries"] += n
    if not masks:
        return closest_hit(S, o, d, t_max, T)
    left = np.asarray(t_max).astype(T).copy() if shadow else np.full(n, t_max, T)
    at = np.array(o, T, copy=True)
    total = np.zeros(n, T)
    passes = np.zeros(n, np.int64)
    out_t = left.copy()
    out_idx = np.full(n, -1, np.int64)
    todo = np.arange(n)
    material = S.prims["material"]
    while len(todo):
        t, idx = closest_hit(S, at[todo], d[todo], left[todo], T)
        through = np.zeros(len(todo), bool)
        mat = np.where(idx >= 0, material[np.clip(idx, 0, None)], -1)
        for m, (plane, c8) in masks.items():
            k = np.flatnonzero(mat == m)
            if len(k) == 0:
                continue
            u, v = hit_uv(S, at[todo[k]], d[todo[k]], t[k], idx[k], T)
            if "al_uv_swapped" in perturb:
                u, v = v, u
            row, col = image_texel(plane, u, v, T)
            a8 = plane[row, col].astype(np.int64)
            clear = (a8 >= c8) if "al_inverted" in perturb else (a8 < c8)
            clear &= passes[todo[k]] < CAP  # the 65th masked hit of a query is opaque whatever its texel says
            through[k] = clear
            if log is not None:
                log["alpha_masked_hits"] += len(k)
                log["alpha_passes"] += int(clear.sum())
                log["alpha_opaque"] += int((~clear).sum())
                if samples is not None:
                    log["alpha_masked_samples"].update(samples[todo[k]].tolist())
        done = todo[~through]
        out_t[done] = total[done] + t[~through]
        out_idx[done] = idx[~through]
        go = todo[through]
        at[go] = at[go] + t[through][:, None] * d[go]
        total[go] += t[through]
        left[go] -= t[through]
        passes[go] += 1
        if on_pass is not None and len(go):
            on_pass(None if samples is None else samples[go], at[go], d[go])
        todo = go
    if log is not None:
        log["alpha_max_passes"] = max(log["alpha_max_passes"], int(passes.max()) if n else 0)
        if shadow:
            log["alpha_shadow_through"] += int((passes > 0).sum())
    if depth is not None and "al_counts_bounce" in perturb and not shadow and samples is not None:
        depth[samples] -= passes
    return out_t, out_idx


# ---------------------------------------------------------------------------------------------------------------- environment
def env_texel(E, d, T):
    rows, cols = E["tex"].shape[:2]
    pi = T(np.pi)
    v = np.arccos(np.clip(d[:, 1], -1, 1)) / pi
    row = np.clip((v * rows).astype(np.int64), 0, rows - 1)
    u = (np.arctan2(-d[:, 2], d[:, 0]) + pi) / (2 * pi) + T(E["uoff"])
    u = u - np.floor(u)
    col = np.clip((u * cols).astype(np.int64), 0, cols - 1)
    return row, col


def env_eval(E, d, T):
    """radiance and sampling density of unit directions, through the one lookup both strategies use"""
    row, col = env_texel(E, d, T)
    rad = T(E["scale"]) * E["tex"][row, col].astype(T)
    pm = E["marg"].astype(T)[row + 1] - E["marg"].astype(T)[row]
    cond = E["cond"].astype(T)
    pc = cond[row, col + 1] - cond[row, col]
    return rad, pm * pc / E["band"].astype(T)[row], row * E["tex"].shape[1] + col


def env_sample(E, u1, u2, T):
    rows, cols = E["tex"].shape[:2]
    marg, cond, ct = E["marg"].astype(T), E["cond"].astype(T), E["ct"].astype(T)
    row = np.clip(np.searchsorted(marg[:rows], u1, side="right") - 1, 0, rows - 1)  # the last entry <= u1
    m0, m1 = marg[row], marg[row + 1]
    with np.errstate(all="ignore"):
        a1 = np.where(m1 > m0, (u1 - m0) / (m1 - m0), T(0.5))
        col = np.zeros(len(row), np.int64)
        for r in np.unique(row):
            col[row == r] = np.searchsorted(cond[r, :cols], u2[row == r], side="right") - 1
        col = col.clip(0, cols - 1)
        c0, c1 = cond[row, col], cond[row, col + 1]
        a2 = np.where(c1 > c0, (u2 - c0) / (c1 - c0), T(0.5))
    cth = ct[row] + a1 * (ct[row + 1] - ct[row])
    sth = np.sqrt(np.maximum(0, 1 - cth * cth))
    u = (col + a2) / cols - T(E["uoff"])
    u = u - np.floor(u)
    phi = 2 * T(np.pi) * u - T(np.pi)
    return np.stack([sth * np.cos(phi), cth, -sth * np.sin(phi)], axis=1).astype(T)


# ---------------------------------------------------------------------------------------------------------------- light sampling
def inside_sphere_light(S, li, p, T):
    """is p inside (or on) sphere light li: c^2 <= r^2, where the cone of directions towards it is the whole sphere"""
    f = S.prims[S.lights[li]["prim"]]["f"].astype(T)
    return ~(_dot(f[:3] - p, f[:3] - p) > f[3] * f[3])


def light_pdf_of_hit(S, li, o, d, t, n, T):
    """the light strategy's solid-angle density of the direction of a ray from o that hit light li at parameter t (normal n): a
    sphere's by the cone it subtends; every other shape's -- rectangle, cylinder, triangle, quad -- by area with the hit's normal,
    which on an emitter is the geometric one"""
    L = S.lights[li]
    sel = T(L["probability"])
    if L["shape"] == SPHERE:
        f = S.prims[L["prim"]]["f"].astype(T)
        c2, r2 = _dot(f[:3] - o, f[:3] - o), f[3] * f[3]
        with np.errstate(all="ignore"):
            cos_max = np.sqrt(np.maximum(0, 1 - r2 / c2))
            pdf = sel / (2 * T(np.pi) * (r2 / c2) / (1 + cos_max))
        return np.where(inside_sphere_light(S, li, o, T), 0, pdf)
    dist2 = t * t * _dot(d, d)
    cos_l = np.abs(_dot(n, d)) / np.sqrt(_dot(d, d))
    with np.errstate(all="ignore"):
        return sel / T(L["area"]) * dist2 / cos_l


def triangle_light_record(pr):
    """(v1, e1, e2, n) as the light record of a triangle holds them: fp32, the edges fp32 differences of the fp32
    vertices, n the GEOMETRIC unit normal whatever vertex normals the triangle carries (an emitter hit keeps it)"""
    m = pr["m"].astype(np.float32)
    return m[0:3], m[3:6] - m[0:3], m[6:9] - m[0:3], m[9:12]


def triangle_area(pr):
    """|e1 x e2| / 2 in fp64 from the stored vertices"""
    m = pr["m"].astype(np.float64)
    return 0.5 * float(np.linalg.norm(np.cross(m[3:6] - m[0:3], m[6:9] - m[0:3])))


def sample_triangle(pr, u1, u2, T, perturb=()):
    """(the point uniform by area y = v1 + (1 - s) e1 + u2 s e2 with s = sqrt(u1), the normal the density is stated with)"""
    v1, e1, e2, n = (a.astype(T) for a in triangle_light_record(pr))
    if "tri_vertex_normal" in perturb:  # (a triangle without vertex normals: n tilted by 0.5 about e1, so the name never does nothing)
        n1 = prim_normals(pr)[0].astype(T)
        if not np.any(n1 != 0):
            t = e1 / np.sqrt((e1 * e1).sum())
            n1 = (np.cos(T(0.5)) * n + np.sin(T(0.5)) * np.cross(t, n)).astype(T)
        n = n1
    s = u1 if "tri_no_sqrt" in perturb else np.sqrt(u1)
    return v1 + (1 - s)[:, None] * e1 + (u2 * s)[:, None] * e2, n


def sample_quad(pr, u1, u2, T):
    """(the point uniform by area y = Q + u1 u + u2 v, the quad's unit normal)"""
    Q, u, v, n, _, _ = quad_record(pr, T)
    return Q + u1[:, None] * u + u2[:, None] * v, n


def sample_light(S, li, p, u1, u2, T, perturb=(), log=None):
    """for the vertices p that picked light li: (vector from p to the light point (a unit direction for the environment),
    the light strategy's solid-angle density there, the emitted radiance towards p, the texel picked or NONE, delta: the light is
    a point, spot or distant light, whose sample no BSDF ray can find: it counts at weight 1)"""
    L = S.lights[li]
    sel, pi = T(L["probability"]), T(np.pi)
    n = len(p)
    texel = np.full(n, NONE, np.int64)
    if L["shape"] == ENVIRONMENT:
        ld = env_sample(S.env, u1, u2, T)
        rad, pe, texel = env_eval(S.env, ld, T)
        return ld, sel * pe, rad, texel, False
    if L["shape"] in DELTA_LIGHTS:
        return AL.sample(L, S.analytic[li], p, u1, u2, T, perturb, log) + (texel, True)
    pr = S.prims[L["prim"]]
    f = pr["f"].astype(T)
    if L["shape"] == SPHERE:
        # a direction uniform in the cone the sphere subtends (u1: the polar angle, u2: the azimuth, in the frame of
        # Duff et al. 2017 about the axis), then the nearer intersection
        w = f[:3] - p
        c2, r2 = _dot(w, w), f[3] * f[3]
        with np.errstate(all="ignore"):
            q = r2 / c2
            omc = q / (1 + np.sqrt(np.maximum(0, 1 - q)))
            cth = 1 - u1 * omc
            sth2 = np.maximum(0, 1 - cth * cth)
            sth = np.sqrt(sth2)
            phi = 2 * pi * u2
            c = np.sqrt(c2)
            a = w / c[:, None]
            sg = np.copysign(T(1), a[:, 2])
            fa = -1 / (sg + a[:, 2])
            fb = a[:, 0] * a[:, 1] * fa
            t1 = np.stack([1 + sg * a[:, 0] ** 2 * fa, sg * fb, -sg * a[:, 0]], axis=1)
            t2 = np.stack([fb, sg + a[:, 1] ** 2 * fa, -a[:, 1]], axis=1)
            e = (sth * np.cos(phi))[:, None] * t1 + (sth * np.sin(phi))[:, None] * t2 + cth[:, None] * a
            dist = c * cth - np.sqrt(np.maximum(0, r2 - c2 * sth2))
            ld = dist[:, None] * e
            pl = sel / (2 * pi * omc)
        outside = ~inside_sphere_light(S, li, p, T)  # a vertex inside the sphere takes no sample of it
        ld, pl = np.where(outside[:, None], ld, 0), np.where(outside, pl, 0)
    else:  # a point y uniform by area, with the normal ln there: p_l = selection / area x |ld|^2 / |ln . ld / |ld||
        area = T(L["area"])
        if L["shape"] == CYLINDER:
            R, tr = _affine(pr["m"], T)
            phi = 2 * pi * u1
            q = np.stack([np.abs(f[0]) * np.cos(phi), np.abs(f[0]) * np.sin(phi), f[1] + u2 * (f[2] - f[1])], axis=1)
            y = q @ R.T + tr
            ln = np.stack([np.cos(phi), np.sin(phi), np.zeros_like(phi)], axis=1) @ R.T
        elif L["shape"] == TRIANGLE:
            y, ln = sample_triangle(pr, u1, u2, T, perturb)
        elif L["shape"] == QUAD:
            y, ln = sample_quad(pr, u1, u2, T)
            if "quad_light_half_area" in perturb:
                area = area * T(0.5)
        else:
            ka, aa, ba = _rect_axes(L["shape"])
            y = np.zeros((n, 3), T)
            y[:, aa], y[:, ba], y[:, ka] = f[0] + u1 * (f[1] - f[0]), f[2] + u2 * (f[3] - f[2]), f[4]
            ln = np.zeros((n, 3), T)
            ln[:, ka] = 1
        ld = (y - p).astype(T)
        d2 = _dot(ld, ld)
        with np.errstate(all="ignore"):
            cos_l = np.abs(_dot(ln, ld)) / np.sqrt(d2)
            if "no_cos" in perturb:
                cos_l = np.ones_like(cos_l)
            pl = sel / area * d2 / cos_l
    odd = checker_odd(p + ld, T)
    rad = np.where(odd[:, None], L["emission_odd"].astype(T), L["emission"].astype(T))
    return ld.astype(T), pl.astype(T), rad, texel, False


# ---------------------------------------------------------------------------------------------------------------- the integrator
class _Draws:
    """the per-sample cursor over the uniforms of the sample's own stream"""

    def __init__(self, words, T):
        self.u = (words >> 8).astype(T) * T(2.0 ** -24)
        self.at = np.zeros(len(words), np.int64)
        self.limit = words.shape[1]

    def next(self, who):
        """one uniform for the samples `who` (indices)"""
        v = self.u[who, np.minimum(self.at[who], self.limit - 1)]
        self.at[who] += 1
        return v

    def reject(self, who, dims, T):
        """rejection sampling from (-1, 1)^dims to the open unit ball, for the samples `who`"""
        out = np.zeros((len(who), 3), T)
        todo = np.arange(len(who))
        while len(todo):
            c = np.stack([2 * self.next(who[todo]) - 1 for _ in range(dims)], axis=1)
            ok = _dot(c, c) < 1
            out[todo[ok], :dims] = c[ok]
            todo = todo[~ok]
            if (self.at[who] > self.limit + 64).any():
                raise RuntimeError("a rejection loop ran far beyond the requested draws")
        return out


def trace(S, words, first_pixel=0, dtype=np.float64, perturb=(), shutter=None, probe=None, log=None, on_pass=None):
    """One sample per row of `words` (the sample's stream as uint32 words), pixel ids first_pixel, first_pixel + 1, ... modulo the
    frame; `shutter`: the samples' shutter times, required where the scene has movers.  Returns (rgb [N][3], signature [N][*]
    int64, draws consumed [N]).  probe: a dict that receives the FIRST vertex of every sample (what a feature pass shows):
    "glossy" (bool: it lies on a glossy material, rough glass and pbr among them), "albedo" (F0 or rho there; pbr: the base colour
    c8 / 255), "normal" (the shading normal), "texture_value" (the colour an emitter, a lambertian or a plastic read from its
    texture: zeros elsewhere), "first_t" / "first_idx" (the first path query's total t and its opaque winner; NaN / -1 where the
    sample made no query).  log: a dict of new_log() that counts what the signature has no column for (LOG_KEYS).  on_pass:
    handed to opaque_hit(), in an fp64 run alone.
    perturb names deliberate mistakes, for the tests that show the comparison can fail.  Every name, in one place (the model
    files' docstrings say what each of theirs does):
      ref64_noise.PERTURBATIONS, ref64_bump.PERTURBATIONS, ref64_normal_map.PERTURBATIONS, ref64_glass.PERTURBATIONS
      ("fresnel_draw_last" is glass's name for "lobe_draw_last"), ref64_pbr.PERTURBATIONS, ref64_analytic_lights.PERTURBATIONS,
      ref64_phase.PERTURBATIONS ("phase_isotropic": g ignored altogether, every medium vertex runs the rejection loop);
      of 7z (media_nee_scenes.MISTAKES says which case shows which): "no_transmittance": the shadow ray ignores the media
      (T = 1);  "isotropic_pdf": pdf_b = 1 / (4 pi) at a vertex with g != 0, for the light's direction and the continuation's (the
      direction is still drawn with g);
      "shadow_flight_draw": a free-flight draw taken for every non-empty stay of a shadow ray (and thrown away);
      "medium_full_weight": a medium vertex's continuation arrives at an emitter at full weight (as if it took no light sample);
      "tri_no_sqrt": a triangle light's barycentrics taken without the square root (s = u1): points crowd towards v2;
      "tri_vertex_normal": a triangle light's density stated with its first vertex normal in place of the geometric one;
      "quad_uv_swapped": a quad's (u, v) = (b, a);  "quad_light_half_area": a quad light's density stated with half the area;
      "quad_front_flipped": a quad's front = den > 0 (the normal stays turned against the ray);
      "skip_draw", "no_cos", "mis_unsquared", "no_rr_light": at the light sample;
      "skip_flight": the free-flight draw left out (the distance is taken from the NEXT position instead: a wrong order of draws);
      "half_time": every sample at s = 0.5 (a renderer that ignores the shutter time);
      "uv_transposed": the image lookup with u indexing columns;
      "tri_natural_pairing": each area weight of a triangle with the corner opposite its sub-triangle;
      "flat_normals": the geometric normal where a triangle carries vertex normals (a renderer without smooth shading);
      "g1_for_g2": a glossy vertex's attenuation with G1(wo) in place of G2 (without the factor G2 / G1);
      "lobe_draw_last": plastic's lobe draw taken after u1, u2 instead of in front of them;
      "nee_albedo_pdf": a glossy vertex's light sample with f cos taken as albedo x pdf_b, the shortcut that holds for
      lambertian and metal;
      "delta_power_heuristic": the power heuristic applied to the sample of a point, spot or distant light;
      "al_off": masks ignored;  "al_inverted": a masked hit is transparent iff a8 >= c8;  "al_uv_swapped": the mask read with
      the row from v and the column from u;  "al_shadow_opaque": shadow rays do not pass;  "al_counts_bounce": a pass uses up
      a bounce."""
    T = dtype
    N = len(words)
    log = new_log() if log is None else log
    ul_last = "lobe_draw_last" in perturb or "fresnel_draw_last" in perturb
    D = _Draws(words, T)
    W, H = S.width, S.height
    pix = (first_pixel + np.arange(N)) % (W * H)
    everyone = np.arange(N)
    rr, pi = T(S.rr), T(np.pi)
    if len(S.movers):
        if shutter is None:
            raise ValueError("a scene with movers needs the samples' shutter times")
        time = np.full(N, 0.5, T) if "half_time" in perturb else np.asarray(shutter, np.float64).astype(T)
    cam = {k: v.astype(T) for k, v in S.cam.items()}
    sig = [np.full((N, SAMPLE_COLUMNS), NONE, np.int64)]
    media_g = S.media_g.astype(np.float64) * (0 if "phase_isotropic" in perturb else -1 if "phase_backward" in perturb else 1)

    def note(column, who, values):
        sig[-1][who, column] = values

    # camera::get_ray: the jitter, then the lens sample where blur is on
    s = ((pix % W).astype(T) + D.next(everyone)) / T(W - 1)
    t = ((pix // W).astype(T) + D.next(everyone)) / T(H - 1)
    off = np.zeros((N, 3), T)
    if S.flags & 2:
        lens = T(S.lens_radius) * D.reject(everyone, 2, T)
        off = lens[:, :1] * cam["u"] + lens[:, 1:2] * cam["v"]
    o = cam["origin"] + off
    d = cam["lower_left"] + s[:, None] * cam["horizontal"] + t[:, None] * cam["vertical"] - cam["origin"] - off
    beta = np.ones((N, 3), T)
    rgb = np.zeros((N, 3), T)
    depth = np.full(N, S.max_depth, np.int64)
    mis = np.full(N, -1, T)  # density of the BSDF sample that made the ray; < 0: its vertex took no light sample
    alive = depth > 0
    if rr > 0:  # roulette before the first query as before every other
        lost = D.next(everyone) > rr
        note(1, everyone, lost)
        alive &= ~lost
        beta = beta / rr

    while alive.any():
        who = np.flatnonzero(alive)
        oo, dd = o[who], d[who]
        t_hit, idx = opaque_hit(S, oo, dd, np.inf, T, perturb, log, who, depth, on_pass if T is np.float64 else None)
        if probe is not None and len(sig) == 1:
            probe.update(first_t=np.full(N, np.nan), first_idx=np.full(N, -1, np.int64))
            probe["first_t"][who], probe["first_idx"][who] = t_hit, idx
        sig.append(np.full((N, VERTEX_COLUMNS), NONE, np.int64))
        note(C_PRIM, who, idx)
        # ---- the movers (7g), in list order, behind every static primitive: accepted while t_min <= t <= the closest so far
        mov = np.full(len(who), -1, np.int64)
        if len(S.movers):
            a = _dot(dd, dd)
            t_min = T(T_MIN)
            for mi, m in enumerate(S.movers):
                tt = mover_t(m, time[who], oo, dd, a, t_min, t_hit, T)
                with np.errstate(invalid="ignore"):
                    ok = (tt >= t_min) & (tt <= t_hit)
                t_hit = np.where(ok, tt, t_hit)
                mov = np.where(ok, mi, mov)
            note(C_MOVER, who, mov)
        # ---- the media walk (7f), in list order: a non-empty stay in a medium of positive density takes one draw
        t_m = np.full(len(who), np.inf, T)
        med = np.full(len(who), -1, np.int64)
        if len(S.media):
            drew = np.zeros(len(who), np.int64)
            length = np.sqrt(_dot(dd, dd))
            for mi, m in enumerate(S.media):
                sigma = T(m["density"])
                if not sigma > 0:
                    continue
                a, b, ok = medium_interval(m, oo, dd, t_hit, T)
                k = np.flatnonzero(ok)
                if len(k) == 0:
                    continue
                if "skip_flight" in perturb:
                    D.at[who[k]] += 1
                u = D.next(who[k])
                if "skip_flight" in perturb:
                    D.at[who[k]] -= 1
                tt = a[k] + (-np.log(1 - u) / sigma) / length[k]
                drew[k] |= 1 << mi
                win = (tt < b[k]) & (tt < t_m[k])
                t_m[k[win]] = tt[win]
                med[k[win]] = mi
            note(C_DREW, who, drew)
            note(C_MEDIUM, who, med)
        vol = med >= 0  # a medium event nearer than the surface: a vertex of the volume
        t_hit = np.where(vol, t_m, t_hit)
        # ---- a miss ends the path with the background
        miss = (idx < 0) & (mov < 0) & ~vol
        if miss.any():
            m = who[miss]
            ud = _unit(dd[miss])
            if S.env is not None:
                bg, pe, texel = env_eval(S.env, ud, T)
                note(C_MISS_TEXEL, m, texel)
                if len(S.lights) and S.lights[-1]["shape"] == ENVIRONMENT:
                    pl = T(S.lights[-1]["probability"]) * pe
                    bg = bg * _mis_bsdf(mis[m], pl, perturb)[:, None]
            elif S.flags & 1:
                tt = 0.5 * (ud[:, 1] + 1)
                bg = (1 - tt)[:, None] * np.ones(3, T) + tt[:, None] * np.array([0.5, 0.7, 1.0], T)
            else:
                bg = np.broadcast_to(S.background.astype(T), (len(m), 3))
            rgb[m] += beta[m] * bg
            alive[m] = False
        if miss.all():
            continue
        who, oo, dd, t_hit, idx, mov, med, vol = (x[~miss] for x in (who, oo, dd, t_hit, idx, mov, med, vol))
        # ---- the hit record: a static winner's; a mover's is the sphere's about c(s); a medium event has a point and no normal
        p = oo + t_hit[:, None] * dd
        n = np.zeros_like(dd)
        front = np.zeros(len(who), bool)
        mat = np.full(len(who), -1, np.int64)
        st = np.flatnonzero((mov < 0) & ~vol)
        p[st], n[st], front[st] = hit_record(S, oo[st], dd[st], t_hit[st], idx[st], T, perturb, log)
        mat[st] = S.prims["material"][idx[st]]
        for mi, m in enumerate(S.movers):
            q = np.flatnonzero((mov == mi) & ~vol)
            if len(q):
                n_out = (p[q] - mover_centre(m, time[who[q]], T)) / T(m["radius"])
                f = _dot(dd[q], n_out) < 0
                n[q], front[q], mat[q] = np.where(f[:, None], n_out, -n_out), f, int(m["material"])
        surface = np.flatnonzero(~vol)
        kind = np.full(len(who), NONE, np.int64)
        tex = np.full(len(who), -1, np.int64)
        kind[surface], tex[surface] = S.mats["type"][mat[surface]], S.mats["texture"][mat[surface]]
        listed = np.where(mov < 0, idx, -1)  # the static winner where it is the vertex's surface: the key of a listed light
        checker = np.isin(kind, (LAMBERTIAN, DIFFUSE_LIGHT, PLASTIC)) & (S.texs["type"][np.maximum(tex, 0)] == CHECKER)
        note(C_PARITY, who, np.where(checker, checker_odd(p, T), NONE))
        event = np.full(len(who), NONE, np.int64)
        shutter_of = time[who] if len(S.movers) else None

        tex_read = np.zeros_like(dd)

        def textured(k, of=None):  # the value at the vertices k of their material's texture (or of texture `of`), the image texel noted
            value, texel = texture_value(S, tex[k] if of is None else np.full(len(k), of), p[k], T, oo[k], dd[k], t_hit[k], idx[k], mov[k],
                                         None if shutter_of is None else shutter_of[k], perturb)
            if of is None:
                note(C_IMAGE_TEXEL, who[k], texel)
                tex_read[k] = value
            return value
        # ---- an emitter ends the path with what it emits
        em = kind == DIFFUSE_LIGHT
        if em.any():
            m = who[em]
            Le = textured(em)
            wgt = np.ones(em.sum(), T)
            how = np.full(em.sum(), HIT_UNSAMPLED, np.int64)
            for li in {S.light_of_prim.get(int(i), -1) for i in np.unique(listed[em])} - {-1}:
                sel = listed[em] == S.lights[li]["prim"]
                pl = light_pdf_of_hit(S, li, oo[em][sel], dd[em][sel], t_hit[em][sel], n[em][sel], T)
                wgt[sel] = _mis_bsdf(mis[m][sel], pl, perturb)
                inside = inside_sphere_light(S, li, oo[em][sel], T) if S.lights[li]["shape"] == SPHERE else np.zeros(sel.sum(), bool)
                how[sel] = np.where(mis[m][sel] < 0, HIT_UNSAMPLED, np.where(inside, HIT_FROM_INSIDE, HIT_MIS))
            note(C_HIT_WEIGHT, m, how)
            rgb[m] += beta[m] * Le * wgt[:, None]
            alive[m] = False
            event[em] = EV_EMIT
        # ---- the scatter step
        new_d = np.zeros_like(dd)
        att = np.ones_like(dd)
        scattered = ~em
        pdf_b = np.full(len(who), -1, T)
        refl_dir = np.zeros_like(dd)       # metal: the mirror direction of its lobe
        fuzz = np.zeros(len(who), T)       # metal: its fuzz (0: a lambertian vertex)
        takes_light = np.zeros(len(who), bool)
        travel = np.zeros_like(dd)             # a medium vertex: the unit direction of travel that arrived
        g_v = np.zeros(len(who), np.float64)   # ... and its medium's asymmetry as the light sample and the continuation see it
        if vol.any():  # a medium event: a vertex without a normal that emits nothing -- albedo, then a direction by its medium's g
            k = np.flatnonzero(vol)
            travel[k] = _unit(dd[k])
            iso, hg = k[media_g[med[k]] == 0], k[media_g[med[k]] != 0]
            new_d[iso] = _unit(D.reject(who[iso], 3, T))  # g = 0 (7f): uniform, by the rejection loop
            event[iso] = EV_MEDIUM
            if len(hg):  # g != 0 (7y): two draws, the polar angle about the direction of travel from u1, the azimuth from u2
                u1, u2 = D.next(who[hg]), D.next(who[hg])
                if "phase_swapped_draws" in perturb:
                    u1, u2 = u2, u1
                for mi in np.unique(med[hg]):
                    sel = med[hg] == mi
                    new_d[hg[sel]] = PH.hg_direction(media_g[mi], travel[hg[sel]], u1[sel], u2[sel], T)
                event[hg] = EV_MEDIUM_HG
            att[k] = S.media["albedo"][med[k]].astype(T)
            if S.nee and len(S.lights):  # (7z) it takes a light sample: f = albedo x pdf_b, no cosine and no hemisphere
                g_v[k] = 0.0 if "isotropic_pdf" in perturb else media_g[med[k]]
                takes_light[k] = True
                pdf_b[k] = phase_density(g_v[k], _dot(_unit(new_d[k]), travel[k]), T)
        lam = kind == LAMBERTIAN
        if lam.any():
            sph = D.reject(who[lam], 3, T)
            nd = n[lam] + _unit(sph)
            tiny = (np.abs(nd) < 1e-8).all(axis=1)
            nd[tiny] = n[lam][tiny]
            new_d[lam], att[lam] = nd, textured(lam)
            event[lam] = EV_LAMBERT
            takes_light[lam] = True
            pdf_b[lam] = np.maximum(0, _dot(_unit(nd), n[lam])) / pi
        met = kind == METAL
        if met.any():
            ud = _unit(dd[met])
            r = ud - 2 * _dot(ud, n[met])[:, None] * n[met]
            fz = S.mats["fuzz"][mat[met]].astype(T)
            nd = r + fz[:, None] * D.reject(who[met], 3, T)
            up = _dot(nd, n[met]) > 0
            new_d[met], att[met] = nd, S.mats["albedo"][mat[met]].astype(T)
            scattered[met] = up
            event[met] = np.where(up, EV_METAL, EV_METAL_ABSORBED)
            refl_dir[met], fuzz[met] = r, fz
            takes_light[met] = S.mats["fuzz"][mat[met]] >= np.float32(METAL_MIN_FUZZ)
            for f in np.unique(fz[takes_light[met]]):
                sel = np.flatnonzero(met)[(fz == f) & up]
                pdf_b[sel] = metal_pdf(_unit(new_d[sel]), refl_dir[sel], f, T)
        die = kind == DIELECTRIC
        if die.any():
            ir = S.mats["ir"][mat[die]].astype(T)
            ratio = np.where(front[die], 1 / ir, ir)
            ud, nn = _unit(dd[die]), n[die]
            cos_t = np.minimum(-_dot(ud, nn), 1)
            sin_t = np.sqrt(np.maximum(0, 1 - cos_t * cos_t))
            reflect = ratio * sin_t > 1
            can = np.flatnonzero(~reflect)
            if len(can):  # the uniform is drawn only where refraction is possible
                r0 = ((1 - ratio[can]) / (1 + ratio[can])) ** 2
                schlick = r0 + (1 - r0) * (1 - cos_t[can]) ** 5
                reflect[can] = schlick > D.next(who[die][can])
            perp = ratio[:, None] * (ud + cos_t[:, None] * nn)
            refracted = perp - np.sqrt(np.abs(1 - _dot(perp, perp)))[:, None] * nn
            new_d[die] = np.where(reflect[:, None], ud - 2 * _dot(ud, nn)[:, None] * nn, refracted)
            event[die] = np.where(reflect, EV_REFLECT, EV_REFRACT)
        # ---- the glossy materials: their draws where dielectric takes its Fresnel draw; none where wo.z <= 0
        # Beside them rough glass (7r) and pbr (7t).  What the light sample needs again stands in the g_* arrays, per vertex: the
        # lobe's alpha, whether the row is a plastic's (pbr: what ul chose), F0 (plastic: r0), rho (plastic and pbr: the body or base
        # colour; rough glass: its tint Tr over the segment, 1 on a front hit) and, for rough glass, eta
        glo = np.isin(kind, (ROUGH_METAL, PLASTIC, ROUGH_GLASS, PBR))
        g_alpha, g_f0, g_rho = np.zeros(len(who), T), np.zeros((len(who), 3), T), np.zeros((len(who), 3), T)
        g_plastic, g_ud = np.zeros(len(who), bool), np.zeros_like(dd)
        g_eta = np.zeros(len(who), T)
        if glo.any():
            k = np.flatnonzero(glo)
            kn, kg, kq = k[kind[k] != ROUGH_GLASS], k[kind[k] == ROUGH_GLASS], k[kind[k] == PBR]
            rec = S.mats[mat[k]]
            g_plastic[k] = rec["type"] == PLASTIC
            g_alpha[k] = alpha_of(rec["fuzz"]).astype(T)
            g_f0[k] = np.where(np.isin(rec["type"], (PLASTIC, PBR))[:, None], r0_of(rec["ir"]).astype(T)[:, None], rec["albedo"].astype(T))
            rough = np.zeros(len(who), np.float32)  # the roughness that decides on the light sample: the material's; pbr: the hit's
            rough[k] = rec["fuzz"]
            kp = k[g_plastic[k]]
            if len(kp):
                g_rho[kp] = textured(kp)
            if len(kg):  # the side from the hit record, the tint over t |d| with the material's sigma (its albedo words)
                g_eta[kg] = GL.eta_of(S.mats["ir"][mat[kg]], front[kg], T, perturb)
                sigma = S.mats["albedo"][mat[kg]]
                tr = GL.tint(sigma, t_hit[kg] * np.sqrt(_dot(dd[kg], dd[kg])), T)
                g_rho[kg] = np.where(front[kg][:, None] | ("no_absorption" in perturb), T(1), tr)
                log["glass_tinted_back_hits"] += int((~front[kg] & (sigma > 0).any(axis=1)).sum())
            m8 = np.zeros(len(who), T)
            for pm in np.unique(mat[kq]):  # the bytes of the hit: from the base texture and the map under the factors rf, mf
                q = kq[mat[kq] == pm]
                base, mp = textured(q), np.ones((len(q), 3), T)
                if S.pbr_maps[int(pm)] >= 0:
                    mp = textured(q, S.pbr_maps[int(pm)])
                c8, r8, m8[q] = PB.params(base, mp[:, 0] if "roughness_from_r" in perturb else mp[:, 1], mp[:, 2], S.mats["fuzz"][pm],
                                          S.mats["albedo"][pm][0], T)
                g_rho[q], rough[q], g_alpha[q] = PB.unit(c8, T), PB.unit(r8, np.float32), PB.alpha_of(PB.unit(r8, T), T)
                for key, which in (("map", S.pbr_maps[int(pm)]), ("base", int(S.mats["texture"][pm]))):
                    name = {IMAGE: "image", NOISE: "noise", CHECKER: "checker"}.get(int(S.texs["type"][which]) if which >= 0 else -1)
                    if f"pbr_{name}_{key}_hits" in log:
                        log[f"pbr_{name}_{key}_hits"] += len(q)
            g_ud[k] = _unit(dd[k])
            wo_z = -_dot(g_ud[k], n[k])
            dr = k[wo_z > 0]  # the vertices that draw
            ul, u1, u2 = np.zeros(len(who), T), np.zeros(len(who), T), np.zeros(len(who), T)
            pd = dr[kind[dr] != ROUGH_METAL]  # ul: plastic's lobe draw, rough glass's Fresnel draw, pbr's choice
            if not ul_last:
                ul[pd] = D.next(who[pd])
            u1[dr] = D.next(who[dr])
            u2[dr] = D.next(who[dr])
            if ul_last:
                ul[pd] = D.next(who[pd])
            # pbr: ul < m is a rough metal of F0 = c, else a plastic of body c under the coat's r0, with ul rescaled
            if len(kq):
                metal, ul[kq] = PB.choose(m8[kq], ul[kq], T, perturb)
                g_plastic[kq] = ~metal
                g_f0[kq] = np.where(metal[:, None], T(0.04) if "metal_f0_004" in perturb else g_rho[kq], g_f0[kq])
            wi, at, pdf = np.zeros_like(dd), np.zeros_like(dd), np.zeros(len(who), T)
            below, absorbed_wi, lobe = np.zeros(len(who), bool), np.zeros(len(who), bool), np.zeros(len(who), bool)
            if len(kn):
                wi[kn], at[kn], pdf[kn], below[kn], absorbed_wi[kn], lobe[kn] = glossy_sample(
                    n[kn], g_ud[kn], g_alpha[kn], g_plastic[kn], g_f0[kn], g_rho[kn], ul[kn], u1[kn], u2[kn], T, perturb)
            if len(kg):  # (lobe: the ray was reflected)
                wi[kg], at[kg], pdf[kg], below[kg], absorbed_wi[kg], lobe[kg] = GL.glass_sample(
                    n[kg], g_ud[kg], g_alpha[kg], g_eta[kg], g_rho[kg], ul[kg], u1[kg], u2[kg], T, perturb, log)
            if len(kq):
                lobe[kq] |= metal  # (a pbr metal choice is signed EV_COAT)
            new_d[k], att[k] = wi[k], at[k]
            scattered[k] = ~below[k] & ~absorbed_wi[k]
            event[k] = np.where(below[k], EV_BELOW, np.where(kind[k] != ROUGH_METAL,
                                                             np.where(lobe[k], np.where(absorbed_wi[k], EV_COAT_ABSORBED, EV_COAT), EV_BODY),
                                                             np.where(absorbed_wi[k], EV_ROUGH_ABSORBED, EV_ROUGH)))
            takes_light[k] = (rough[k] >= np.float32(GLOSSY_MIN_ROUGHNESS)) & ~below[k]
            pdf_b[k] = np.where(scattered[k], pdf[k], -1)
            if len(kq):
                log["pbr_vertices"] += len(kq)
                log["pbr_below"] += int(below[kq].sum())
                log["pbr_metal_choices"] += int((metal & ~below[kq]).sum())
                log["pbr_plastic_choices"] += int((~metal & ~below[kq]).sum())
                log["pbr_smooth_vertices"] += int((~takes_light[kq] & ~below[kq]).sum())
        if probe is not None and len(sig) == 2:
            probe.update(glossy=np.zeros(N, bool), albedo=np.zeros((N, 3), T), normal=np.zeros((N, 3), T), texture_value=np.zeros((N, 3), T))
            probe["glossy"][who] = glo
            probe["albedo"][who] = np.where(g_plastic[:, None], g_rho, g_f0)
            probe["normal"][who] = n
            probe["texture_value"][who] = tex_read
        note(C_EVENT, who, event)
        if not S.nee or len(S.lights) == 0:
            takes_light[:] = False
        # ---- what goes on: depth, then the roulette of the next query
        go = ~em & scattered
        if glo.any():
            before = beta[who].copy()                  # the throughput in front of the vertex (a glossy vertex's light sample)
        carried = beta[who] * att                      # the throughput the continuation carries
        depth[who[go]] -= 1
        go_on = go & (depth[who] > 0)
        log["ended_by_depth"] += int((go & ~go_on).sum())
        absorbed = ~em & ~scattered                    # (a metal direction below the surface)
        # an absorbed metal vertex samples its light where its continuation would have been traced, with a roulette draw of its own
        draws_rr = go_on | (absorbed & takes_light & (depth[who] > 1))
        survived = draws_rr.copy()
        if rr > 0 and draws_rr.any():
            k = np.flatnonzero(draws_rr)
            lost = D.next(who[k]) > rr
            note(C_ROULETTE, who[k], lost)
            survived[k] = ~lost
            carried[k] = carried[k] / rr
            if glo.any():
                before[k] = before[k] / rr
        alive[who] = go_on & survived
        beta[who] = carried
        o[who], d[who] = p, new_d
        mis[who] = np.where(takes_light, pdf_b, -1)
        if "medium_full_weight" in perturb:
            mis[who[vol]] = -1
        # ---- the light sample
        ls = np.flatnonzero(takes_light & survived & draws_rr & (len(S.lights) > 0))
        if len(ls) == 0:
            continue
        m = who[ls]
        if "skip_draw" in perturb:
            D.at[m] += 1
        u0, u1, u2 = D.next(m), D.next(m), D.next(m)
        nl = len(S.lights)
        xs = u0 * nl
        pick = np.minimum(xs.astype(np.int64), nl - 1)
        aliased = xs - pick >= S.thr.astype(T)[pick]
        pick = np.where(aliased, S.alias[pick], pick)
        note(C_LIGHT, m, pick)
        note(C_ALIAS, m, aliased)
        ld = np.zeros((len(m), 3), T)
        pl = np.zeros(len(m), T)
        Le = np.zeros((len(m), 3), T)
        texel = np.full(len(m), NONE, np.int64)
        inside = np.zeros(len(m), bool)
        delta = np.zeros(len(m), bool)
        for li in np.unique(pick):
            sel = pick == li
            ld[sel], pl[sel], Le[sel], texel[sel], delta[sel] = sample_light(S, li, p[ls][sel], u1[sel], u2[sel], T, perturb, log)
            if S.lights[li]["shape"] == SPHERE:
                inside[sel] = inside_sphere_light(S, li, p[ls][sel], T)
        note(C_TEXEL, m, texel)
        d2 = _dot(ld, ld)
        gl = glo[ls]
        with np.errstate(all="ignore"):
            w = ld / np.sqrt(d2)[:, None]
            wn = _dot(w, n[ls])
            pb = np.where(fuzz[ls] > 0, 0, wn / pi)
            for f in np.unique(fuzz[ls][fuzz[ls] > 0]):
                sel = fuzz[ls] == f
                pb[sel] = metal_pdf(w[sel], refl_dir[ls][sel], f, T)
            pb = np.where(wn > 0, pb, 0)
            mv = vol[ls]  # a medium vertex: the phase function's density of the light's direction, no cosine and no hemisphere
            pb[mv] = phase_density(g_v[ls][mv], _dot(w[mv], travel[ls][mv]), T)
            if gl.any():
                # f cos is not albedo x pdf_b at a glossy vertex: both are evaluated for the light's direction
                q, wl = ls[gl], w[gl]
                fc, pg = np.zeros((len(q), 3), T), np.zeros(len(q), T)
                a = g_alpha[q]
                if "light_step_from_factors" in perturb:
                    a = np.where(kind[q] == PBR, alpha_of(S.mats["fuzz"][mat[q]]).astype(T), a)
                r, e = kind[q] != ROUGH_GLASS, kind[q] == ROUGH_GLASS
                if r.any():  # (a pbr row as the material its vertex chose)
                    fc[r], pg[r] = glossy_eval(n[q[r]], g_ud[q[r]], a[r], g_plastic[q[r]], g_f0[q[r]], g_rho[q[r]], wl[r], T)
                if e.any():
                    fc[e], pg[e] = GL.glass_eval(n[q[e]], g_ud[q[e]], a[e], g_eta[q[e]], g_rho[q[e]], wl[e], T)
                log["glass_light_evaluations"] += int(e.sum())
                log["pbr_light_evaluations"] += int((kind[q] == PBR).sum())
                log["pbr_lit"] += int((fc[kind[q] == PBR] > 0).any(axis=1).sum())
                if "nee_albedo_pdf" in perturb:
                    fc = np.where(g_plastic[q][:, None], g_rho[q], g_f0[q]) * pg[:, None]
                pb[gl] = pg
                fcos = np.zeros((len(ls), 3), T)
                fcos[gl] = fc
            # f cos / p_l times the power heuristic's p_l^2 / (p_l^2 + pdf_b^2); f cos = albedo x pdf_b for lambertian and metal
            weight = pb * pl / (pl + pb if "mis_unsquared" in perturb else pl * pl + pb * pb)
            if gl.any():  # the glossy vertices' scalar part: p_l / (p_l^2 + pdf_b^2); f cos joins per channel below
                weight = np.where(gl, pl / (pl + pb if "mis_unsquared" in perturb else pl * pl + pb * pb), weight)
            if "delta_power_heuristic" not in perturb:  # a delta sample counts at weight 1: f cos x colour / p_l
                weight = np.where(delta, np.where(gl, 1 / pl, pb / pl), weight)
        usable = (pl > 0) & (pb > 0) & (d2 > 0) & np.isfinite(weight) & (weight > 0)
        verdict = np.where(inside, SHADOW_INSIDE, SHADOW_NONE)
        if usable.any():
            k = np.flatnonzero(usable)
            is_env = S.lights["shape"][pick[k]] == ENVIRONMENT
            if len(S.movers) or (len(S.media) and is_env.any()):
                raise NotImplementedError("a shadow ray past a mover, or towards the environment in a scene with media: DESIGN defines none")
            far = np.where(is_env, T(np.inf), T(SHADOW_T_MAX))
            _, blocker = opaque_hit(S, p[ls][k], ld[k], far, T, perturb, log, m[k])
            verdict[k] = np.where(blocker >= 0, SHADOW_OCCLUDED, SHADOW_CLEAR)
            note(C_BLOCKER, m[k], np.where(blocker >= 0, blocker, NONE))
            clear = k[blocker < 0]
            reach = weight[clear]  # the sample's weight as it reaches the vertex
            if len(S.media):  # (7z) the shadow ray takes no draw; any opaque hit occludes; a clear sample is dimmed by exp(-tau)
                tau, stays = optical_depth(S, p[ls][k], ld[k], T(SHADOW_T_MAX), T)
                if "shadow_flight_draw" in perturb:
                    for mi in range(len(S.media)):
                        D.next(m[k][(stays >> mi) & 1 == 1])
                note(C_STAYS, m[k], stays)
                if "no_transmittance" not in perturb:
                    reach = reach * np.exp(-tau[blocker < 0])
            through = carried[ls][clear]
            if gl.any():
                through = np.where(gl[clear][:, None], before[ls][clear] * fcos[clear], through)
            if "no_rr_light" in perturb and rr > 0:
                through = through * rr
            rgb[m[clear]] += through * Le[clear] * reach[:, None]
        note(C_SHADOW, m, verdict)

    sig[0][:, 0] = D.at
    return rgb, np.concatenate(sig, axis=1), D.at.copy()


def same_signature(a, b):
    """per sample: did two runs over the same draws take the same branches (rows equal, the shorter one padded)"""
    w = max(a.shape[1], b.shape[1])
    pad = lambda s: np.pad(s, ((0, 0), (0, w - s.shape[1])), constant_values=NONE)
    return (pad(a) == pad(b)).all(axis=1)


def tally(sig, S=None, log=None):
    """How often the special vertices of DESIGN 7a occurred in a batch, read from its signatures, so that a test of such a case can
    assert that the case was there: light samples not made because the vertex lies inside the sphere light it picked, and BSDF
    hits on that light from inside kept at weight 1; absorbed metal vertices that took a light sample all the same; dielectric
    vertices, the light samples they took (none, by definition) and the emitter hits of their rays at full weight; light picks
    that went to the bucket's own light and to its alias.  Of 7f (MEDIA_KEYS): medium events, those on paths that met a surface
    vertex later, those behind a refraction, and the media that had one.  Of 7y: medium events by whether the medium's g is 0,
    paths that met a surface after an anisotropic one, paths with both kinds.  Of 7z: light samples at medium and at surface
    vertices, the medium ones that were clear, shadow rays that stayed in a medium by verdict, emitter hits straight behind a
    medium vertex and those of them weighted by MIS.  Of 7g (MOTION_KEYS): vertices on movers, which movers
    were hit, and the paths that went from a mover to a static surface and the other way.  Of triangles and image textures
    (EXT_KEYS): vertices that read an image texel, those that took a light sample, those on a mover, the samples with such a
    vertex, and the samples that met one after a medium event; emitter hits at full weight behind a vertex that took a light
    sample (the emitter is no listed light); and, where the RefScene S says which primitives are triangles and which carry
    an image texture, vertices on triangles, those that took a light sample, and shadow rays stopped by either kind.  Of 7m
    (ref64_glossy.GLOSSY_KEYS and more): what ref64_glossy.glossy_tally() counts (by the material's roughness: a pbr vertex's is
    its hit's, which the log counts as pbr_smooth_vertices).  Of 7n-7u, with S: _extension_tally()'s counts.  With the `log` that
    trace() filled: its counters (LOG_KEYS), which hold what the signature has no column for, and of 7v the shares the alpha cases
    assert (alpha_masked_share, alpha_pass_share, alpha_opaque_share)."""
    v = sig[:, SAMPLE_COLUMNS:].reshape(len(sig), -1, VERTEX_COLUMNS)
    event, light, shadow, how, alias, mover = (v[:, :, c] for c in (C_EVENT, C_LIGHT, C_SHADOW, C_HIT_WEIGHT, C_ALIAS, C_MOVER))
    prim, blocker = v[:, :, C_PRIM], v[:, :, C_BLOCKER]
    image = v[:, :, C_IMAGE_TEXEL] != NONE
    is_tri, is_image = np.zeros(1, bool), np.zeros(1, bool)
    if S is not None and len(S.prims):
        is_tri = S.prims["type"] == TRIANGLE
        mat = S.mats[S.prims["material"]]
        is_image = np.isin(mat["type"], (LAMBERTIAN, DIFFUSE_LIGHT)) & (S.texs["type"][mat["texture"]] == IMAGE)
    of = lambda flags, i: (i >= 0) & flags[np.clip(i, 0, len(flags) - 1)]
    glass = np.isin(event, (EV_REFLECT, EV_REFRACT))
    later = lambda x: np.flip(np.cumsum(np.flip(x, axis=1), axis=1), axis=1) - x > 0
    med, hg = np.isin(event, MEDIUM_EVENTS), event == EV_MEDIUM_HG
    took, emit = light != NONE, event == EV_EMIT
    nxt = lambda x: np.concatenate([x[:, 1:], np.zeros((len(x), 1), bool)], axis=1)
    # C_STAYS shares its column with the environment light's texel: it is a set of media where the scene has media (C_DREW is set)
    through = (v[:, :, C_DREW] != NONE) & (v[:, :, C_STAYS] != NONE) & (v[:, :, C_STAYS] > 0)
    surface = np.isin(event, (EV_LAMBERT, EV_METAL, EV_METAL_ABSORBED, EV_REFLECT, EV_REFRACT, EV_EMIT))
    glass_before = np.cumsum(np.isin(event, (EV_REFRACT,)), axis=1) > 0
    vertex = event != NONE
    on_mover, on_static = vertex & (mover >= 0), vertex & (mover < 0)
    on_tri = on_static & ~med & of(is_tri, prim)
    env_light = len(S.lights) - 1 if S is not None and len(S.lights) and S.lights[-1]["shape"] == ENVIRONMENT else -1
    roughness = None
    if S is not None:  # a material's roughness; pbr: the byte of its factor, as every hit has it, where no map scales it
        roughness = S.mats["fuzz"].astype(np.float64)
        for m, mp in S.pbr_maps.items():
            roughness[m] = PB.unit(PB.byte(roughness[m], np.float64), np.float32) if mp < 0 else np.nan
    glossy = glossy_tally(event, dict(prim=prim, light=light, env_light=env_light, took_light=light != NONE, roughness=roughness,
                                      clear=shadow == SHADOW_CLEAR, medium=med, on_mover=mover >= 0,
                                      full_weight_emitter=(event == EV_EMIT) & (how == HIT_UNSAMPLED),
                                      missed_to_texel=v[:, :, C_MISS_TEXEL] != NONE, lost=v[:, :, C_ROULETTE] == 1), S)
    ext = _extension_tally(v, S) if S is not None else {}
    if log:  # alpha cutouts: the shares of samples that met a masked hit, and of masked hits that passed / were opaque
        hits = max(log["alpha_masked_hits"], 1)
        log = dict(log, alpha_masked_samples=len(log["alpha_masked_samples"]), alpha_masked_share=len(log["alpha_masked_samples"]) / max(len(sig), 1),
                   alpha_pass_share=log["alpha_passes"] / hits, alpha_opaque_share=log["alpha_opaque"] / hits)
    return dict(glossy, **ext, **(log or {}),
                inside_no_sample=int((shadow == SHADOW_INSIDE).sum()), inside_full_weight_hits=int((how == HIT_FROM_INSIDE).sum()),
                absorbed_metal_light_samples=int(((event == EV_METAL_ABSORBED) & (light != NONE)).sum()),
                dielectric_vertices=int(glass.sum()), dielectric_light_samples=int((glass & (light != NONE)).sum()),
                dielectric_full_weight_hits=int((glass[:, :-1] & (how[:, 1:] == HIT_UNSAMPLED)).sum()),
                bucket_picks=int((alias == 0).sum()), alias_picks=int((alias == 1).sum()),
                medium_events=int(med.sum()), medium_then_surface=int((med & later(surface)).any(axis=1).sum()),
                medium_behind_glass=int((med & glass_before).sum()),
                media_with_events=sorted(int(i) for i in np.unique(v[:, :, C_MEDIUM][med])),
                anisotropic_events=int(hg.sum()), isotropic_events=int((med & ~hg).sum()),
                surface_after_anisotropic=int((hg & later(surface)).any(axis=1).sum()),
                both_on_one_path=int((hg.any(axis=1) & (med & ~hg).any(axis=1)).sum()),
                medium_light_samples=int((med & took).sum()), surface_light_samples=int((~med & took).sum()),
                medium_samples_clear=int((med & (shadow == SHADOW_CLEAR)).sum()),
                clear_through_media=int(((shadow == SHADOW_CLEAR) & through).sum()),
                occluded_through_media=int(((shadow == SHADOW_OCCLUDED) & through).sum()),
                medium_then_emitter=int((med & nxt(emit)).sum()),
                medium_then_emitter_mis=int((med & took & nxt(emit & (how == HIT_MIS))).sum()),
                mover_vertices=int(on_mover.sum()), movers_hit=sorted(int(i) for i in np.unique(mover[on_mover])),
                mover_then_static=int((on_mover & later(on_static)).any(axis=1).sum()),
                static_then_mover=int((on_static & later(on_mover)).any(axis=1).sum()),
                image_vertices=int(image.sum()), image_vertices_with_light_sample=int((image & (light != NONE)).sum()),
                image_samples=int(image.any(axis=1).sum()), image_mover_vertices=int((image & on_mover).sum()),
                medium_then_image_surface=int((med & later(image)).any(axis=1).sum()),
                unlisted_emitter_hits_after_light_sample=int(((light[:, :-1] != NONE) & (event[:, 1:] == EV_EMIT)
                                                              & (how[:, 1:] == HIT_UNSAMPLED)).sum()),
                triangle_vertices=int(on_tri.sum()),
                triangle_vertices_with_light_sample=int((on_tri & (light != NONE)).sum()),
                shadow_stopped_by_triangle=int(of(is_tri, blocker).sum()),
                shadow_stopped_by_image_prim=int(of(is_image, blocker).sum()))


def _extension_tally(v, S):
    """tally()'s counts of DESIGN 7n-7u from the signature's vertex blocks v [N][vertices][columns], by the RefScene's records: what
    the cases of each extension are there for.  Triangle lights (triangle_*) and quads (quad_*): light samples that picked one,
    their shadow rays' verdicts, BSDF hits on one by weight (C_FRONT is no column: the two sides of a cube are told apart by the
    event that follows); other_picks: light samples of a light that is neither.  Noise (noise_*): surface vertices whose material's
    texture is a noise texture, by material type, and the share of samples with one.  Bumps (bump_*) and normal maps (nm_*): the
    static surface vertices whose material carries one, by material and (nm) primitive type.  Rough glass (glass_*): its vertices
    by event, with a light sample, the emitter hits behind them by weight, the roughnesses met.  Point, spot and distant lights:
    picks per type, their shadow rays, glossy vertices one of them lit, emitter hits weighted by MIS."""
    N = len(v)
    event, light, shadow, how, prim, blocker, mover = (v[:, :, c] for c in (C_EVENT, C_LIGHT, C_SHADOW, C_HIT_WEIGHT, C_PRIM, C_BLOCKER, C_MOVER))
    pick = lambda flags, i: (i >= 0) & np.asarray(flags, bool)[np.clip(i, 0, max(len(flags) - 1, 0))] if len(flags) else np.zeros(i.shape, bool)
    count = lambda x: int(x.sum())
    nxt = lambda x: np.concatenate([x[:, 1:], np.zeros((N, 1), bool)], axis=1)
    took, emit = light != NONE, event == EV_EMIT
    # ---- the lights by shape
    shape = S.lights["shape"]
    of = lambda kind: pick(shape == kind, light)
    tri_pick, quad_pick = of(TRIANGLE), of(QUAD)
    delta = of(POINT) | of(SPOT) | of(DISTANT)
    light_prim = lambda kind: np.isin(np.arange(len(S.prims)), S.lights["prim"][shape == kind])
    on_tri_light, on_quad = emit & pick(light_prim(TRIANGLE), prim), pick(S.prims["type"] == QUAD, prim)
    glossy = np.isin(event, GLOSSY_EVENTS)
    out = dict(triangle_picks=count(tri_pick), quad_picks=count(quad_pick), other_picks=count((light >= 0) & ~tri_pick & ~quad_pick),
               triangle_shadow_stopped=count(tri_pick & (shadow == SHADOW_OCCLUDED)), triangle_shadow_clear=count(tri_pick & (shadow == SHADOW_CLEAR)),
               triangle_mis_hits=count(on_tri_light & (how == HIT_MIS)), triangle_full_weight_hits=count(on_tri_light & (how == HIT_UNSAMPLED)),
               quad_vertices=count(on_quad), quad_shadow_stops=count((shadow == SHADOW_OCCLUDED) & pick(S.prims["type"] == QUAD, blocker)),
               quad_refractions=count(on_quad & (event == EV_REFRACT)), quad_reflections=count(on_quad & (event == EV_REFLECT)),
               quad_emitter_hits=count(on_quad & emit), quad_mis_hits=count(on_quad & emit & (how == HIT_MIS)),
               point_picks=count(of(POINT)), spot_picks=count(of(SPOT)), distant_picks=count(of(DISTANT)), area_picks=count((light >= 0) & ~delta),
               analytic_shadow_occluded=count(delta & (shadow == SHADOW_OCCLUDED)), analytic_shadow_clear=count(delta & (shadow == SHADOW_CLEAR)),
               analytic_no_shadow_ray=count(delta & (shadow == SHADOW_NONE)), glossy_lit_by_analytic=count(glossy & delta & (shadow == SHADOW_CLEAR)),
               emitter_mis_hits=count(emit & (how == HIT_MIS)))
    # ---- the material under every surface vertex: a mover's is its own; a medium event is no surface
    surface = (event != NONE) & (event != EV_MISS) & ~np.isin(event, MEDIUM_EVENTS)
    on_mover = mover >= 0 if len(S.movers) else np.zeros(event.shape, bool)
    static = surface & (prim >= 0) & ~on_mover
    mat = np.where(prim >= 0, S.prims["material"][np.clip(prim, 0, max(len(S.prims) - 1, 0))], -1) if len(S.prims) else np.full(event.shape, -1)
    if len(S.movers):
        mat = np.where(on_mover, S.movers["material"][np.clip(mover, 0, len(S.movers) - 1)], mat)
    mat = np.where(surface, mat, -1)
    mtype = np.where(mat >= 0, S.mats["type"][np.clip(mat, 0, len(S.mats) - 1)], -1)
    tex = np.where(mat >= 0, S.mats["texture"][np.clip(mat, 0, len(S.mats) - 1)], -1)
    noisy = np.isin(mtype, (LAMBERTIAN, DIFFUSE_LIGHT, PLASTIC)) & (tex >= 0) & (S.texs["type"][np.clip(tex, 0, len(S.texs) - 1)] == NOISE)
    out.update(noise_vertices=count(noisy), noise_share=float(noisy.any(axis=1).mean()), noise_lambertian=count(noisy & (mtype == LAMBERTIAN)),
               noise_plastic=count(noisy & (mtype == PLASTIC)), noise_emitter=count(noisy & (mtype == DIFFUSE_LIGHT)),
               noise_plastic_light_samples=count(noisy & (mtype == PLASTIC) & took), noise_mover=count(noisy & on_mover),
               noise_textures=sorted(int(t) for t in np.unique(tex[noisy])))
    kinds = (("lambertian", LAMBERTIAN), ("metal", METAL), ("dielectric", DIELECTRIC), ("rough_metal", ROUGH_METAL), ("plastic", PLASTIC))
    for prefix, carriers, more in (("bump_", S.bumps, ()), ("nm_", S.normal_maps, (("rough_glass", ROUGH_GLASS), ("pbr", PBR)))):
        on = static & np.isin(mat, list(carriers))
        out.update({prefix + "vertices": count(on), prefix + "share": float(on.any(axis=1).mean()), prefix + "light_samples": count(on & took)})
        out.update({prefix + name: count(on & (mtype == kind)) for name, kind in kinds + more})
    on = static & np.isin(mat, list(S.normal_maps))
    ptype = np.where(on, S.prims["type"][np.clip(prim, 0, max(len(S.prims) - 1, 0))], -1) if len(S.prims) else np.full(event.shape, -1)
    for name, shapes in (("sphere", (SPHERE,)), ("rect", (XY_RECT, XZ_RECT, YZ_RECT)), ("cylinder", (CYLINDER,)), ("triangle", (TRIANGLE,)), ("quad", (QUAD,))):
        out["nm_on_" + name] = count(np.isin(ptype, shapes))
    # ---- rough glass
    on = glossy & (mtype == ROUGH_GLASS)
    emit_full, emit_mis = emit & (how == HIT_UNSAMPLED), emit & (how == HIT_MIS)
    rough = S.mats["fuzz"][np.clip(mat, 0, len(S.mats) - 1)][on & ~on_mover]
    out.update(glass_vertices=count(on), glass_mover_vertices=count(on & on_mover), glass_reflect_events=count(on & (event == EV_COAT)),
               glass_refract_events=count(on & (event == EV_BODY)), glass_below_events=count(on & (event == EV_BELOW)),
               glass_light_samples=count(on & took), glass_below_light_samples=count(on & (event == EV_BELOW) & took),
               glass_full_weight_hits_behind_refraction=count(on & (event == EV_BODY) & took & nxt(emit_full)),
               glass_mis_hits_behind_reflection=count(on & (event == EV_COAT) & nxt(emit_mis)),
               glass_then_medium=count((np.cumsum(on & (event == EV_BODY), axis=1) > 0) & np.isin(event, MEDIUM_EVENTS)),
               glass_roughnesses=sorted(float(np.float32(x)) for x in np.unique(rough)))
    return out


MEDIA_KEYS = ("medium_events", "medium_then_surface", "medium_behind_glass", "media_with_events")
MOTION_KEYS = ("mover_vertices", "movers_hit", "mover_then_static", "static_then_mover")
EXT_KEYS = ("image_vertices", "image_vertices_with_light_sample", "image_samples", "triangle_vertices",
            "triangle_vertices_with_light_sample", "shadow_stopped_by_triangle", "shadow_stopped_by_image_prim",
            "unlisted_emitter_hits_after_light_sample", "medium_then_image_surface", "image_mover_vertices")


def _mis_bsdf(pdf_b, pl, perturb=()):
    """weight of a BSDF ray's emitter hit or escape: pdf_b^2 / (pdf_b^2 + p_l^2); 1 where the vertex took no light sample
    (pdf_b < 0) or the light strategy cannot produce the direction"""
    with np.errstate(all="ignore"):
        if "mis_unsquared" in perturb:
            w = pdf_b / (pdf_b + pl)
        else:
            w = pdf_b * pdf_b / (pdf_b * pdf_b + pl * pl)
    w = np.where(pdf_b > 0, w, 0)
    return np.where((pdf_b >= 0) & (pl > 0), w, 1).astype(pl.dtype)


def implied_alias_probability(thr, alias):
    """(thr_i + sum over j with alias_j = i of (1 - thr_j)) / n: the probability with which one uniform draw picks light i"""
    thr = thr.astype(np.float64)
    n = len(thr)
    p = thr.copy()
    np.add.at(p, alias, 1.0 - thr)
    return p / n


# ---------------------------------------------------------------------------------------------------------------- the comparison
def reference(S, words, shutter=None):
    """the fp64 radiance, which samples took the same branches at fp32 (the stable ones), the draws consumed, and the tally of the
    fp64 run's special vertices, its log among them"""
    log = new_log()
    rgb, sig64, draws = trace(S, words, shutter=shutter, log=log)
    _, sig32, _ = trace(S, words, dtype=np.float32, shutter=shutter)
    return rgb, same_signature(sig64, sig32), draws, tally(sig64, S, log)


def judge(got, ref, stable):
    """The figures the per-sample assertions read.  got / ref: [N][3].
    share: samples within 1e-4 max(1, |ref|) in every channel (gate G2's number, scaled for emitters brighter than 1);
    z: per channel, mean(got - ref) in units of std(got - ref) / sqrt(N); bias_ok: |mean| < 5 std / sqrt(N) + 1e-6"""
    diff = got.astype(np.float64) - ref
    within = (np.abs(diff) <= 1e-4 * np.maximum(1.0, np.abs(ref))).all(axis=1)
    n = len(ref)
    mean, se = diff.mean(axis=0), diff.std(axis=0) / np.sqrt(n)
    return dict(share=float(within.mean()), median=float(np.median(np.abs(diff).max(axis=1))),
                share_stable=float(within[stable].mean()), flips=float(1 - stable.mean()),
                z=(mean / np.maximum(se, 1e-300)) * (np.abs(mean) > 0), bias_ok=bool((np.abs(mean) < 5 * se + 1e-6).all()),
                mean_diff=mean)


def row(name, j, base=None):
    z = " ".join(f"{v:+.2f}" for v in j["z"])
    b = "" if base is None else f" | plain stable {100 * base:7.3f} %"
    return (f"{name:40s} | within {100 * j['share']:7.3f} % | median {j['median']:.2e} | flips {100 * j['flips']:.3f} % | "
            f"stable within {100 * j['share_stable']:7.3f} %{b} | max |mean diff| {np.abs(j['mean_diff']).max():.1e}, z {z}")
