"""Quads for ref64.py, in NumPy at a floating type of the caller's choice.

Test infrastructure only, written from the definition of the primitive (include/rtmi.h, RT_PRIM_QUAD), not from csrc/rt_quad.h.
A quad is the parallelogram with corner Q and edges u, v.  Its record holds Q, u, v and, derived by the host in fp64 and
rounded once, the unit normal n = c / |c| (c = u x v) and A = v x w, B = w x u with w = c / (c.c).  A ray o + t d
    den = n.d                      zero or not finite: a miss
    t   = n.(Q - o) / den          accepted within [t_min, best], ties to the later primitive (closest_hit's rule)
    p   = o + t d,  a = A.(p - Q),  b = B.(p - Q)
    hit iff 0 <= a <= 1 and 0 <= b <= 1;  the record's (u, v) = (a, b), its normal n turned against the ray, front = den < 0.
As a light (a diffuse_light with a solid or checker texture): the point y = Q + u1 u + u2 v, uniform by area, and the light
strategy's solid-angle density of ld = y - p,
    p_l = selection / |c| x |ld|^2 / |n.ld / |ld||,
with |c| the light record's area; emission, checker parity at y and light_pdf_of_hit from the hit's side follow the rectangle's
rules.  Everything runs at dtype T with plain (unfused) operations on the record's fp32 words.

ref64.py is not edited.  Its _prim_t takes an unknown type for a cylinder, its hit_record and hit_uv for a rectangle, and its
sample_light reads a rectangle's `f` words.  installed() puts wrappers in their places while a trace runs -- each handles type
6 itself and hands every other primitive, and every sample that hit one, to the function it replaced -- and takes them out
again.  trace() and reference() are ref64's, called inside installed().

Deliberate mistakes (names in `perturb`, as ref64.trace takes them; hit_record takes none, so installed(perturb) carries them):
  quad_uv_swapped        the record's (u, v) = (b, a)
  quad_light_half_area   the density stated with half the area
  quad_front_flipped     front = den > 0 (the normal stays turned against the ray)
"""
import contextlib

import numpy as np

import ref64 as R

QUAD = 6
PERTURBATIONS = ("quad_uv_swapped", "quad_light_half_area", "quad_front_flipped")


def record(pr, T):
    """(Q, u, v, n, A, B) of a quad's rt_prim record at dtype T"""
    m, mi = pr["m"].astype(T), pr["m_inv"].astype(T)
    return m[0:3], m[3:6], m[6:9], m[9:12], mi[0:3], mi[3:6]


def is_quad(pr):
    return int(pr["type"]) == QUAD


def quad_t(pr, o, d, T):
    """the ray parameter at which the quad accepts the ray (any t: the caller applies the range), NaN where it does not"""
    Q, _, _, n, A, B = record(pr, T)
    with np.errstate(all="ignore"):
        den = R._dot(d, n[None, :])
        t = R._dot(n[None, :], Q - o) / den
        r = o + t[:, None] * d - Q
        a, b = R._dot(A[None, :], r), R._dot(B[None, :], r)
        ok = (den != 0) & np.isfinite(den) & (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
    return np.where(ok, t, T(np.nan)).astype(T)


def quad_ab(pr, o, d, t, T):
    Q, _, _, _, A, B = record(pr, T)
    r = o + t[:, None] * d - Q
    return R._dot(A[None, :], r), R._dot(B[None, :], r)


def sample_quad(S, li, p, u1, u2, T, perturb=()):
    """ref64.sample_light's contract for a quad light: (ld, p_l, emitted radiance, texel = NONE)"""
    L = S.lights[li]
    Q, u, v, n, _, _ = record(S.prims[L["prim"]], T)
    y = Q + u1[:, None] * u + u2[:, None] * v
    ld = (y - p).astype(T)
    d2 = R._dot(ld, ld)
    area = T(L["area"]) * (T(0.5) if "quad_light_half_area" in perturb else T(1))
    with np.errstate(all="ignore"):
        cos_l = np.abs(R._dot(n[None, :], ld)) / np.sqrt(d2)
        pl = T(L["probability"]) / area * d2 / cos_l
    odd = R.checker_odd(p + ld, T)
    rad = np.where(odd[:, None], L["emission_odd"].astype(T), L["emission"].astype(T))
    return ld, pl.astype(T), rad, np.full(len(p), R.NONE, np.int64)


@contextlib.contextmanager
def installed(perturb=()):
    """ref64's _prim_t, hit_record, hit_uv, sample_light and light_pdf_of_hit with quads, for the length of the block"""
    orig = {k: getattr(R, k) for k in ("_prim_t", "hit_record", "hit_uv", "sample_light", "light_pdf_of_hit")}

    def _prim_t(p, o, d, dd, t_min, best, T):
        if is_quad(p):
            return quad_t(p, o, d, T)
        return orig["_prim_t"](p, o, d, dd, t_min, best, T)

    def quads_of(S, idx):
        kinds = np.array([is_quad(p) for p in S.prims], bool)
        return (idx >= 0) & kinds[np.clip(idx, 0, len(kinds) - 1)]

    def hit_record(S, o, d, t, idx, T, flat=False):
        q = quads_of(S, idx)
        if not q.any():
            return orig["hit_record"](S, o, d, t, idx, T, flat)
        p = o + t[:, None] * d
        n = np.zeros_like(o)
        front = np.zeros(len(o), bool)
        if (~q).any():
            p[~q], n[~q], front[~q] = orig["hit_record"](S, o[~q], d[~q], t[~q], idx[~q], T, flat)
        for i in np.unique(idx[q]):
            m = q & (idx == i)
            n_out = record(S.prims[i], T)[3]
            f = R._dot(d[m], n_out[None, :]) < 0
            n[m] = np.where(f[:, None], n_out, -n_out)
            front[m] = ~f if "quad_front_flipped" in perturb else f
        return p, n, front

    def hit_uv(S, o, d, t, idx, T, mov=None, time=None, perturb_=()):
        static = np.ones(len(o), bool) if mov is None else mov < 0
        q = static & quads_of(S, idx)
        if not q.any():
            return orig["hit_uv"](S, o, d, t, idx, T, mov, time, perturb_)
        u, v = np.zeros(len(o), T), np.zeros(len(o), T)
        if (~q).any():
            r = ~q
            u[r], v[r] = orig["hit_uv"](S, o[r], d[r], t[r], idx[r], T, None if mov is None else mov[r],
                                        None if time is None else time[r], perturb_)
        for i in np.unique(idx[q]):
            m = q & (idx == i)
            a, b = quad_ab(S.prims[i], o[m], d[m], t[m], T)
            u[m], v[m] = (b, a) if "quad_uv_swapped" in tuple(perturb_) + tuple(perturb) else (a, b)
        return u, v

    def sample_light(S, li, p, u1, u2, T, perturb_=()):
        if S.lights[li]["shape"] == QUAD:
            return sample_quad(S, li, p, u1, u2, T, tuple(perturb_) + tuple(perturb))
        return orig["sample_light"](S, li, p, u1, u2, T, perturb_)

    def light_pdf_of_hit(S, li, o, d, t, n, T):
        L = S.lights[li]
        if L["shape"] == QUAD:  # by area, from the hit's side: the rectangle's rule with the quad's unit normal
            nq = record(S.prims[L["prim"]], T)[3]
            dist2 = t * t * R._dot(d, d)
            with np.errstate(all="ignore"):
                cos_l = np.abs(R._dot(nq[None, :], d)) / np.sqrt(R._dot(d, d))
                return T(L["probability"]) / T(L["area"]) * dist2 / cos_l
        return orig["light_pdf_of_hit"](S, li, o, d, t, n, T)

    new = dict(_prim_t=_prim_t, hit_record=hit_record, hit_uv=hit_uv, sample_light=sample_light, light_pdf_of_hit=light_pdf_of_hit)
    for k, f in new.items():
        setattr(R, k, f)
    try:
        yield
    finally:
        for k, f in orig.items():
            setattr(R, k, f)


def trace(S, words, perturb=(), **kw):
    with installed(perturb):
        return R.trace(S, words, perturb=tuple(perturb), **kw)


def reference(S, words, shutter=None):
    with installed():
        return R.reference(S, words, shutter)


def tally(sig, S):
    """What a quad case is there for, from the reference's signatures: vertices on a quad, light samples that picked a quad
    light, shadow rays a quad stopped, refractions at a quad (C_FRONT is no column: the two sides of a cube are told apart by the
    event that follows), and BSDF hits on a quad light weighted by MIS"""
    v = sig[:, R.SAMPLE_COLUMNS:].reshape(len(sig), -1, R.VERTEX_COLUMNS)
    event, light, shadow, how, prim, blocker = (v[:, :, c] for c in (R.C_EVENT, R.C_LIGHT, R.C_SHADOW, R.C_HIT_WEIGHT, R.C_PRIM, R.C_BLOCKER))
    kinds = np.array([is_quad(p) for p in S.prims], bool)
    on_quad = (prim >= 0) & kinds[np.clip(prim, 0, len(kinds) - 1)]
    quad_light = S.lights["shape"] == QUAD if len(S.lights) else np.zeros(1, bool)
    picked = (light >= 0) & quad_light[np.clip(light, 0, len(quad_light) - 1)]
    stopped = (shadow == R.SHADOW_OCCLUDED) & (blocker >= 0) & kinds[np.clip(blocker, 0, len(kinds) - 1)]
    return dict(quad_vertices=int(on_quad.sum()), quad_picks=int(picked.sum()), other_picks=int(((light >= 0) & ~picked).sum()),
                quad_shadow_stops=int(stopped.sum()), quad_refractions=int((on_quad & (event == R.EV_REFRACT)).sum()),
                quad_reflections=int((on_quad & (event == R.EV_REFLECT)).sum()),
                quad_emitter_hits=int((on_quad & (event == R.EV_EMIT)).sum()),
                quad_mis_hits=int((on_quad & (event == R.EV_EMIT) & (how == R.HIT_MIS)).sum()))
