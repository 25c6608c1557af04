"""An independent statement of the path estimator of DESIGN 7f (homogeneous participating media with isotropic scattering), in
NumPy, vectorised over a batch of samples, at a floating type of the caller's choice (float64: the reference; float32: the
same formulas at the kernel's precision, used to measure how many samples sit on a branch).

Test infrastructure only, under the contract of nee_ref64.py: written from the definitions -- DESIGN 2 (the integrator, the
order of the draws) and 7f (the media walk) -- with plain loops over the primitive and media lists, libm's log and no fused
operations; it shares no code with the kernels or with oracle/.  The primitive tests, hit records, textures and the cursor
over a sample's draws are nee_ref64's, which are such statements themselves.

Inputs are the product's exported tables (Scene.prims / materials / textures / media / get_camera / info) and the uniforms of
rtmi.sample_stream.  Out of scope: triangles, image textures, light sampling, environment maps (which media do not combine
with).

trace() returns, per sample, the radiance, an event signature (per vertex: the surface winner, the set of media that took a
free-flight draw, the medium whose event won, the checker parity, what the material did, the roulette outcome; two samples
took the same branches iff their rows are equal) and the number of draws consumed.
"""
import numpy as np

import nee_ref64 as R

MEDIUM_SPHERE, MEDIUM_BOX = 0, 1
EV_MEDIUM = 20  # beside nee_ref64's EV_* codes
NONE = R.NONE
SAMPLE_COLUMNS = 2
C_PRIM, C_DREW, C_MEDIUM, C_PARITY, C_EVENT, C_ROULETTE = range(6)
VERTEX_COLUMNS = 6


class RefScene(R.RefScene):
    """nee_ref64's view of a scene (light sampling off), and its media in list order"""

    def __init__(self, sc, media=True):
        super().__init__(sc, nee=False)
        if sc.environment is not None:
            raise ValueError("media do not combine with an environment map")
        self.media = sc.media() if media else sc.media()[:0]


def medium_interval(m, o, d, t_s, T):
    """[a, b]: the stay of the rays o + t d inside the boundary of medium m, clipped to [0.001, t_s]; non-empty where a < b"""
    f = m["f"].astype(T)
    a = np.full(len(o), T(R.T_MIN), T)
    b = t_s.astype(T).copy()
    with np.errstate(all="ignore"):
        if int(m["shape"]) == MEDIUM_SPHERE:
            oc = o - f[:3]
            A = R._dot(d, d)
            hb = R._dot(oc, d)
            disc = hb * hb - A * (R._dot(oc, oc) - f[3] * f[3])
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


def trace(S, words, first_pixel=0, dtype=np.float64, perturb=()):
    """One sample per row of `words`, pixel ids first_pixel, first_pixel + 1, ... modulo the frame.
    Returns (rgb [N][3], signature [N][*] int64, draws consumed [N]).  perturb: "skip_flight" leaves the free-flight draw out
    (the distance is taken from the NEXT position instead: a wrong order of draws)."""
    T = dtype
    N = len(words)
    D = R._Draws(words, T)
    W, H = S.width, S.height
    pix = (first_pixel + np.arange(N)) % (W * H)
    everyone = np.arange(N)
    rr = T(S.rr)
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
    if rr > 0:  # the roulette comes before the query, the media draws after it
        lost = D.next(everyone) > rr
        note(1, everyone, lost)
        alive &= ~lost
        beta = beta / rr

    while alive.any():
        who = np.flatnonzero(alive)
        oo, dd = o[who], d[who]
        t_s, idx = R.closest_hit(S, oo, dd, np.inf, T)
        sig.append(np.full((N, VERTEX_COLUMNS), NONE, np.int64))
        note(C_PRIM, who, idx)
        # ---- the media walk, in list order: a non-empty stay in a medium of positive density takes one draw
        t_m = np.full(len(who), np.inf, T)
        i_m = np.full(len(who), -1, np.int64)
        drew = np.zeros(len(who), np.int64)
        length = np.sqrt(R._dot(dd, dd))
        for mi, m in enumerate(S.media):
            sigma = T(m["density"])
            if not sigma > 0:
                continue
            a, b, ok = medium_interval(m, oo, dd, t_s, T)
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
            i_m[k[win]] = mi
        note(C_DREW, who, drew)
        note(C_MEDIUM, who, i_m)
        in_medium = i_m >= 0
        # ---- a miss ends the path with the background
        miss = (idx < 0) & ~in_medium
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
        # ---- a medium event: a vertex without a normal that emits nothing -- albedo, then a uniform direction
        if in_medium.any():
            k = np.flatnonzero(in_medium)
            p[k] = oo[k] + t_m[k][:, None] * dd[k]
            new_d[k] = R._unit(D.reject(who[k], 3, T))
            att[k] = S.media["albedo"][i_m[k]].astype(T)
            event[k] = EV_MEDIUM
            scattered[k] = True
        surf = (idx >= 0) & ~in_medium
        if surf.any():
            k = np.flatnonzero(surf)
            ps, n, front = R.hit_record(S, oo[k], dd[k], t_s[k], idx[k], T)
            p[k] = ps
            mat = S.prims["material"][idx[k]]
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
    """from the signatures: medium events, and medium events on paths that met a surface vertex later"""
    v = sig[:, SAMPLE_COLUMNS:].reshape(len(sig), -1, VERTEX_COLUMNS)
    event = v[:, :, C_EVENT]
    med = event == EV_MEDIUM
    surface = np.isin(event, (R.EV_LAMBERT, R.EV_METAL, R.EV_METAL_ABSORBED, R.EV_REFLECT, R.EV_REFRACT, R.EV_EMIT))
    later_surface = np.flip(np.cumsum(np.flip(surface, axis=1), axis=1), axis=1) - surface > 0
    glass_before = np.cumsum(np.isin(event, (R.EV_REFRACT,)), axis=1) > 0
    return dict(medium_events=int(med.sum()), medium_then_surface=int((med & later_surface).any(axis=1).sum()),
                medium_behind_glass=int((med & glass_before).sum()),
                media_with_events=sorted(int(i) for i in np.unique(v[:, :, C_MEDIUM][med])))


def reference(S, words):
    """the fp64 radiance, which samples took the same branches at fp32 (the stable ones), the draws consumed, the tally"""
    rgb, sig64, draws = trace(S, words)
    _, sig32, _ = trace(S, words, dtype=np.float32)
    return rgb, R.same_signature(sig64, sig32), draws, tally(sig64)
