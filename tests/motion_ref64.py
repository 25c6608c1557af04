"""An independent statement of the path estimator of DESIGN 7g (motion blur: linearly moving spheres over a per-sample shutter
time), in NumPy, vectorised over a batch of samples, at a floating type of the caller's choice (float64: the reference; float32:
the same formulas at the kernel's precision, used to measure how many samples sit on a branch).

Test infrastructure only, under the contract of nee_ref64.py and media_ref64.py: written from the definitions -- DESIGN 2 (the
integrator, the order of the draws) and 7g (the shutter time, the movers' query and its tie rule) -- with plain loops over the
primitive and mover lists and no fused operations; it shares no code with the kernels or with oracle/.  The static primitives'
tests, hit records, textures and the cursor over a sample's draws are nee_ref64's, which are such statements themselves.

Inputs are the product's exported tables (Scene.prims / materials / textures / moving_spheres / get_camera / info), the uniforms
of rtmi.sample_stream and the shutter times of rtmi.shutter_time (one per sample: the time is no draw of the stream).  Out of
scope: triangles, image textures, light sampling, environment maps, media (which movers do not combine with).

trace() returns, per sample, the radiance, an event signature (per vertex: the static winner, the mover that took over, the
checker parity, what the material did, the roulette outcome; two samples took the same branches iff their rows are equal) and
the number of draws consumed.
"""
import numpy as np

import nee_ref64 as R

NONE = R.NONE
SAMPLE_COLUMNS = 2
C_PRIM, C_MOVER, C_PARITY, C_EVENT, C_ROULETTE = range(5)
VERTEX_COLUMNS = 5


class RefScene(R.RefScene):
    """nee_ref64's view of a scene (light sampling off), and its movers in list order"""

    def __init__(self, sc, movers=True):
        super().__init__(sc, nee=False)
        if sc.environment is not None or len(sc.media()):
            raise ValueError("movers do not combine with an environment map or with media")
        self.movers = sc.moving_spheres() if movers else sc.moving_spheres()[:0]


def mover_centre(m, s, T):
    """c(s) = center0 + s v, with v = center1 - center0 as the scene keeps it: one fp32 subtraction per component"""
    v = (m["center1"].astype(np.float32) - m["center0"].astype(np.float32)).astype(T)
    return m["center0"].astype(T) + s.astype(T)[:, None] * v


def mover_t(m, s, o, d, dd, t_min, best, T):
    """sphere::hit against (c(s), radius): the near root where it lies in [t_min, best], else the far one; NaN without a real root"""
    oc = o - mover_centre(m, s, T)
    r = T(m["radius"])
    with np.errstate(all="ignore"):
        hb = R._dot(oc, d)
        disc = hb * hb - dd * (R._dot(oc, oc) - r * r)
        sq = np.sqrt(np.maximum(disc, 0))
        r1, r2 = (-hb - sq) / dd, (-hb + sq) / dd
        first = (r1 >= t_min) & (r1 <= best)
        return np.where(disc < 0, T(np.nan), np.where(first, r1, r2))


def trace(S, words, shutter, first_pixel=0, dtype=np.float64, perturb=()):
    """One sample per row of `words` with its shutter time in `shutter`, pixel ids first_pixel, first_pixel + 1, ... modulo the
    frame.  Returns (rgb [N][3], signature [N][*] int64, draws consumed [N]).  perturb: "half_time" puts every sample at s = 0.5
    (a renderer that ignores the shutter time)."""
    T = dtype
    N = len(words)
    D = R._Draws(words, T)
    W, H = S.width, S.height
    pix = (first_pixel + np.arange(N)) % (W * H)
    everyone = np.arange(N)
    rr = T(S.rr)
    time = np.full(N, 0.5, T) if "half_time" in perturb else np.asarray(shutter, np.float64).astype(T)
    cam = {k: v.astype(T) for k, v in S.cam.items()}
    sig = [np.full((N, SAMPLE_COLUMNS), NONE, np.int64)]

    def note(column, who, values):
        sig[-1][who, column] = values

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
    alive = depth > 0
    if rr > 0:
        lost = D.next(everyone) > rr
        note(1, everyone, lost)
        alive &= ~lost
        beta = beta / rr

    while alive.any():
        who = np.flatnonzero(alive)
        oo, dd = o[who], d[who]
        best, idx = R.closest_hit(S, oo, dd, np.inf, T)
        sig.append(np.full((N, VERTEX_COLUMNS), NONE, np.int64))
        note(C_PRIM, who, idx)
        # ---- the movers, in list order, behind every static primitive: accepted while t_min <= t <= the closest so far
        mov = np.full(len(who), -1, np.int64)
        a = R._dot(dd, dd)
        t_min = T(R.T_MIN)
        for mi, m in enumerate(S.movers):
            tt = mover_t(m, time[who], oo, dd, a, t_min, best, T)
            with np.errstate(invalid="ignore"):
                ok = (tt >= t_min) & (tt <= best)
            best = np.where(ok, tt, best)
            mov = np.where(ok, mi, mov)
        note(C_MOVER, who, mov)
        on_mover = mov >= 0
        # ---- a miss ends the path with the background
        miss = (idx < 0) & ~on_mover
        if miss.any():
            m = who[miss]
            if S.flags & 1:
                ud = R._unit(dd[miss])
                tt = 0.5 * (ud[:, 1] + 1)
                bg = (1 - tt)[:, None] * np.ones(3, T) + tt[:, None] * np.array([0.5, 0.7, 1.0], T)
            else:
                bg = np.broadcast_to(S.background.astype(T), (len(m), 3))
            rgb[m] += beta[m] * bg
            alive[m] = False
        new_d = np.zeros_like(dd)
        att = np.ones_like(dd)
        p = np.zeros_like(dd)
        event = np.full(len(who), NONE, np.int64)
        scattered = np.zeros(len(who), bool)
        k = np.flatnonzero(~miss)
        if len(k):
            # ---- the hit record: a static winner's is nee_ref64's; a mover's is the sphere's about c(s)
            ps = oo[k] + best[k][:, None] * dd[k]
            n = np.zeros_like(ps)
            front = np.zeros(len(k), bool)
            mat = np.zeros(len(k), np.int64)
            st = np.flatnonzero(~on_mover[k])
            if len(st):
                ps[st], n[st], front[st] = R.hit_record(S, oo[k[st]], dd[k[st]], best[k[st]], idx[k[st]], T)
                mat[st] = S.prims["material"][idx[k[st]]]
            for mi, m in enumerate(S.movers):
                q = np.flatnonzero(mov[k] == mi)
                if len(q):
                    n_out = (ps[q] - mover_centre(m, time[who[k[q]]], T)) / T(m["radius"])
                    f = R._dot(dd[k[q]], n_out) < 0
                    n[q], front[q], mat[q] = np.where(f[:, None], n_out, -n_out), f, int(m["material"])
            p[k] = ps
            kind = S.mats["type"][mat]
            tex = S.mats["texture"][mat]
            checker = np.isin(kind, (R.LAMBERTIAN, R.DIFFUSE_LIGHT)) & (S.texs["type"][np.maximum(tex, 0)] == R.CHECKER)
            note(C_PARITY, who[k], np.where(checker, R.checker_odd(ps, T), NONE))
            em = kind == R.DIFFUSE_LIGHT
            if em.any():
                m = who[k[em]]
                rgb[m] += beta[m] * R.texture_value(S, tex[em], ps[em], T)
                alive[m] = False
                event[k[em]] = R.EV_EMIT
            lam = kind == R.LAMBERTIAN
            if lam.any():
                nd = n[lam] + R._unit(D.reject(who[k[lam]], 3, T))
                tiny = (np.abs(nd) < 1e-8).all(axis=1)
                nd[tiny] = n[lam][tiny]
                new_d[k[lam]], att[k[lam]] = nd, R.texture_value(S, tex[lam], ps[lam], T)
                event[k[lam]] = R.EV_LAMBERT
                scattered[k[lam]] = True
            met = kind == R.METAL
            if met.any():
                ud = R._unit(dd[k[met]])
                r = ud - 2 * R._dot(ud, n[met])[:, None] * n[met]
                fz = S.mats["fuzz"][mat[met]].astype(T)
                nd = r + fz[:, None] * D.reject(who[k[met]], 3, T)
                up = R._dot(nd, n[met]) > 0
                new_d[k[met]], att[k[met]] = nd, S.mats["albedo"][mat[met]].astype(T)
                scattered[k[met]] = up
                event[k[met]] = np.where(up, R.EV_METAL, R.EV_METAL_ABSORBED)
            die = kind == R.DIELECTRIC
            if die.any():
                ir = S.mats["ir"][mat[die]].astype(T)
                ratio = np.where(front[die], 1 / ir, ir)
                ud, nn = R._unit(dd[k[die]]), n[die]
                cos_t = np.minimum(-R._dot(ud, nn), 1)
                sin_t = np.sqrt(np.maximum(0, 1 - cos_t * cos_t))
                reflect = ratio * sin_t > 1
                can = np.flatnonzero(~reflect)
                if len(can):  # the uniform is drawn only where refraction is possible
                    r0 = ((1 - ratio[can]) / (1 + ratio[can])) ** 2
                    schlick = r0 + (1 - r0) * (1 - cos_t[can]) ** 5
                    reflect[can] = schlick > D.next(who[k[die]][can])
                perp = ratio[:, None] * (ud + cos_t[:, None] * nn)
                refracted = perp - np.sqrt(np.abs(1 - R._dot(perp, perp)))[:, None] * nn
                new_d[k[die]] = np.where(reflect[:, None], ud - 2 * R._dot(ud, nn)[:, None] * nn, refracted)
                event[k[die]] = np.where(reflect, R.EV_REFLECT, R.EV_REFRACT)
                scattered[k[die]] = True
        note(C_EVENT, who, event)
        # ---- what goes on: one unit of depth per vertex, then the roulette of the next query
        go = scattered & alive[who]
        carried = beta[who] * att
        depth[who[go]] -= 1
        go_on = go & (depth[who] > 0)
        survived = go_on.copy()
        if rr > 0 and go_on.any():
            k = np.flatnonzero(go_on)
            lost = D.next(who[k]) > rr
            note(C_ROULETTE, who[k], lost)
            survived[k] = ~lost
            carried[k] = carried[k] / rr
        alive[who] = go_on & survived
        beta[who] = carried
        o[who], d[who] = p, new_d

    sig[0][:, 0] = D.at
    return rgb, np.concatenate(sig, axis=1), D.at.copy()


def tally(sig):
    """from the signatures: which movers were hit, and the paths that went from a mover to a static surface and the other way"""
    v = sig[:, SAMPLE_COLUMNS:].reshape(len(sig), -1, VERTEX_COLUMNS)
    vertex = v[:, :, C_EVENT] != NONE
    on_mover = vertex & (v[:, :, C_MOVER] >= 0)
    on_static = vertex & (v[:, :, C_MOVER] < 0)
    later = lambda x: np.flip(np.cumsum(np.flip(x, axis=1), axis=1), axis=1) - x > 0
    return dict(mover_vertices=int(on_mover.sum()), movers_hit=sorted(int(i) for i in np.unique(v[:, :, C_MOVER][on_mover])),
                mover_then_static=int((on_mover & later(on_static)).any(axis=1).sum()),
                static_then_mover=int((on_static & later(on_mover)).any(axis=1).sum()))


def reference(S, words, shutter):
    """the fp64 radiance, which samples took the same branches at fp32 (the stable ones), the draws consumed, the tally"""
    rgb, sig64, draws = trace(S, words, shutter)
    _, sig32, _ = trace(S, words, shutter, dtype=np.float32)
    return rgb, R.same_signature(sig64, sig32), draws, tally(sig64)
