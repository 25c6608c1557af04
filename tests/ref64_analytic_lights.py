"""Point, spot and distant lights for ref64.py, in NumPy at a floating type of the caller's choice.

Test infrastructure only, written from the definition of the lights (include/rtmi.h, rt_analytic_light), not from
csrc/rt_lights.h: plain (unfused) operations on the fp32 words the light record holds.  At a vertex p, with psel the light's
selection probability, a sample is the vector ld towards the light, a "density" pl and a colour, and contributes
f cos x colour / pl at MIS weight 1:
    point    ld = x - p, pl = psel |ld|^2, colour I;  |ld|^2 = 0: no sample
    spot     the point light's, its colour times falloff;  c = a.(-ld / |ld|), s = clamp((c - cos_o) inv, 0, 1), falloff = s^2 (3 - 2 s);
             falloff 0: no sample (pl = 0)
    distant  ld = D w with w uniform in the cone of 1 - cos(alpha) = omc about t -- the sphere light's expressions: 1 - cos(theta)
             = u1 omc, azimuth 2 pi u2, the frame of Duff et al. 2017 about t -- pl = psel, colour E x 2 / (1 + cos alpha)
What the host derives in fp64 and rounds once is derived here the same way from Scene.analytic_lights(): the unit axes (a
distant light's negated: towards the light), cos_o, inv = min(1 / (cos_i - cos_o), FLT_MAX), omc, the folded colour, and D = 4 x
the half diagonal of the primitives' bounding box (bound_radius, restated here).

This file holds the model alone and imports nothing of ref64.  RefScene keeps record() of every analytic light;
ref64.sample_light calls sample() and tells trace() that the sample is a delta sample, and trace() adds f cos x colour / pl
without the power heuristic.  The shadow ray's far end of 0.999 is what ref64 gives every light that is not the environment.
sample() counts the spot samples by falloff into trace()'s log, under LOG_KEYS.

Deliberate mistakes (names in `perturb`):
  point_no_inverse_square   pl = psel for point and spot lights
  spot_linear_falloff       falloff = s
  distant_unfolded          the colour E without 2 / (1 + cos alpha)
  delta_power_heuristic     the power heuristic applied to the sample (trace()'s own)
"""
import numpy as np

from ref64_base import SPHERE, XY_RECT, XZ_RECT, YZ_RECT, CYLINDER, TRIANGLE, _dot, _rect_axes

POINT, SPOT, DISTANT = 101, 102, 103
PERTURBATIONS = ("point_no_inverse_square", "spot_linear_falloff", "distant_unfolded", "delta_power_heuristic")
FLT_MAX = float(np.finfo(np.float32).max)
LOG_KEYS = tuple("analytic_" + k for k in ("point_samples", "spot_samples", "distant_samples", "spot_falloff_zero", "spot_falloff_partial",
                                           "spot_falloff_one", "distant_alpha_zero_samples"))


def luminance(c):
    c = np.asarray(c, np.float64)
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def bound_radius(prims):
    """half the diagonal of the box around the primitives' boxes, in fp64 from the records (0 without primitives)"""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)

    def add(*pts):
        nonlocal lo, hi
        for p in pts:
            lo, hi = np.minimum(lo, p), np.maximum(hi, p)
    for p in prims:
        f, m, t = p["f"].astype(np.float64), p["m"].astype(np.float64), int(p["type"])
        if t == SPHERE:
            add(f[:3] - abs(f[3]), f[:3] + abs(f[3]))
        elif t in (XY_RECT, XZ_RECT, YZ_RECT):
            ka, aa, ba = _rect_axes(t)
            for a, b in ((f[0], f[2]), (f[1], f[3])):
                q = np.zeros(3)
                q[aa], q[ba], q[ka] = a, b, f[4]
                add(q)
        elif t == CYLINDER:
            r = abs(f[0])
            for k in range(8):
                q = np.array([r if k & 1 else -r, r if k & 2 else -r, f[2] if k & 4 else f[1], 1.0])
                add(m.reshape(3, 4) @ q)
        elif t == TRIANGLE:
            add(m[0:3], m[3:6], m[6:9])
        else:  # a quad: Q, Q + u, Q + u + v, Q + v
            add(m[0:3], m[0:3] + m[3:6], m[0:3] + m[3:6] + m[6:9], m[0:3] + m[6:9])
    if not (hi >= lo).all():
        return 0.0
    return 0.5 * float(np.sqrt(((hi - lo) ** 2).sum()))


def record(al, radius):
    """what the light record and rt_light hold for one rt_analytic_light, derived in fp64 and rounded once to fp32:
    dict(type, x, axis, cos_o, inv, omc, dist, colour, measure, weight)"""
    t = int(al["type"])
    colour = al["color"].astype(np.float64)
    out = dict(type=t, x=al["position"].astype(np.float32), axis=np.zeros(3, np.float32), cos_o=np.float32(0), inv=np.float32(0),
               omc=np.float32(0), dist=np.float32(0), fold=1.0)
    if t != POINT:
        d = al["direction"].astype(np.float64)
        d = d / np.sqrt((d * d).sum())
        out["axis"] = ((-d if t == DISTANT else d) + 0.0).astype(np.float32)
    if t == POINT:
        out["measure"] = 4 * np.pi
    elif t == SPOT:
        ci, co = np.cos(np.radians(float(al["angle"][0]))), np.cos(np.radians(float(al["angle"][1])))
        with np.errstate(all="ignore"):
            out["cos_o"], out["inv"] = np.float32(co), np.float32(min(np.float64(1) / (ci - co), FLT_MAX))
        out["measure"] = 2 * np.pi * (1 - (ci + co) / 2)
    else:
        ca = np.cos(np.radians(float(al["angle"][0])))
        out["omc"], out["dist"], out["fold"] = np.float32(1 - ca), np.float32(4 * radius), 2 / (1 + ca)
        out["measure"] = np.pi * radius * radius
    out["colour"] = (colour * out["fold"]).astype(np.float32)
    out["weight"] = out["measure"] * float(luminance(colour)) / np.pi
    return out


def falloff_of(rec, ld, T, perturb=()):
    """the spot's falloff towards the vertex at -ld from it"""
    a = np.atleast_2d(np.asarray(rec["axis"]).astype(T))  # (one axis, or one per vertex)
    with np.errstate(all="ignore"):
        c = -_dot(a, ld) / np.sqrt(_dot(ld, ld))
        s = np.clip((c - np.asarray(rec["cos_o"]).astype(T)) * np.asarray(rec["inv"]).astype(T), 0, 1)
    s = np.where(np.isnan(s), 0, s).astype(T)
    return s if "spot_linear_falloff" in perturb else s * s * (3 - 2 * s)


def cone_direction(t, omc, u1, u2, T):
    """uniform in the cone of 1 - cos(half-angle) = omc about the unit vector t: the sphere light's expressions"""
    n = len(u1)
    a = np.broadcast_to(np.asarray(t).astype(T), (n, 3))  # (one axis and one omc, or one per vertex)
    cth = 1 - u1 * np.asarray(omc).astype(T)
    sth = np.sqrt(np.maximum(0, 1 - cth * cth))
    phi = 2 * T(np.pi) * u2
    sg = np.copysign(T(1), a[:, 2])
    fa = -1 / (sg + a[:, 2])
    fb = a[:, 0] * a[:, 1] * fa
    t1 = np.stack([1 + sg * a[:, 0] ** 2 * fa, sg * fb, -sg * a[:, 0]], axis=1)
    t2 = np.stack([fb, sg + a[:, 1] ** 2 * fa, -a[:, 1]], axis=1)
    return ((sth * np.cos(phi))[:, None] * t1 + (sth * np.sin(phi))[:, None] * t2 + cth[:, None] * a).astype(T)


def sample(L, rec, p, u1, u2, T, perturb=(), log=None):
    """(ld, pl, colour) at the vertices p of the analytic light with the light record L and the record() rec"""
    sel = T(L["probability"])
    n = len(p)
    colour = np.broadcast_to(L["emission"].astype(T), (n, 3)).copy()
    if rec["type"] == DISTANT:
        ld = (T(rec["dist"]) * cone_direction(rec["axis"], rec["omc"], u1, u2, T)).astype(T)
        pl = np.full(n, sel, T)
        if "distant_unfolded" in perturb:
            colour = (colour / T(rec["fold"])).astype(T)
        if log is not None:
            log["analytic_distant_samples"] += n
            log["analytic_distant_alpha_zero_samples"] += n if rec["omc"] == 0 else 0
        return ld, pl, colour
    ld = (rec["x"].astype(T) - p).astype(T)
    d2 = _dot(ld, ld)
    pl = np.full(n, sel, T) if "point_no_inverse_square" in perturb else (sel * d2).astype(T)
    if rec["type"] == SPOT:
        fall = falloff_of(rec, ld, T, perturb)
        # (the falloff on the colour, not under pl: the same product, and pl stays in range at a falloff of 1e-30)
        pl = np.where(fall > 0, pl, 0).astype(T)
        colour = (colour * fall[:, None]).astype(T)
        if log is not None:
            log["analytic_spot_samples"] += n
            log["analytic_spot_falloff_zero"] += int((fall == 0).sum())
            log["analytic_spot_falloff_one"] += int((fall == 1).sum())
            log["analytic_spot_falloff_partial"] += int(((fall > 0) & (fall < 1)).sum())
    elif log is not None:
        log["analytic_point_samples"] += n
    return ld, np.where(d2 > 0, pl, 0).astype(T), colour
