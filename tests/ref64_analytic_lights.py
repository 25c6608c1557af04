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

ref64.py is not edited and its loop is not restated.  ref64.trace applies the power heuristic pb pl / (pl^2 + pb^2) to every
light sample; installed() states weight 1 through it by returning (ld, K pl, K colour) with a power of two K: the product
pb (K pl) (K colour) / ((K pl)^2 + pb^2) is pb colour / pl up to the relative term pb^2 / (K pl)^2.  K = 2^100 at float64 and
2^40 at float32; both conditions -- (K pl)^2 finite, and pb_max^2 / (K pl)^2 below a quarter of the type's epsilon, with pb_max
a bound of the scene's BSDF densities (pb_bound) -- are checked on every call, and a violation raises ArithmeticError (with a
`report` dict, a term that does not vanish is counted there instead: a run whose radiance is discarded, the fp32 signatures).
The shadow ray's far end of 0.999 is what ref64 gives every light that is not the environment.

Deliberate mistakes (names in `perturb`):
  point_no_inverse_square   pl = psel for point and spot lights
  spot_linear_falloff       falloff = s
  distant_unfolded          the colour E without 2 / (1 + cos alpha)
  delta_power_heuristic     K = 1: the power heuristic applied to the sample
"""
import contextlib

import numpy as np

import ref64 as R
import ref64_glass as RG

POINT, SPOT, DISTANT = 101, 102, 103
PERTURBATIONS = ("point_no_inverse_square", "spot_linear_falloff", "distant_unfolded", "delta_power_heuristic")
FLT_MAX = float(np.finfo(np.float32).max)
K_OF = {np.dtype(np.float64): 2.0 ** 100, np.dtype(np.float32): 2.0 ** 40}
LOG_KEYS = ("point_samples", "spot_samples", "distant_samples", "spot_falloff_zero", "spot_falloff_partial", "spot_falloff_one",
            "distant_alpha_zero_samples")


def new_log():
    return dict.fromkeys(LOG_KEYS, 0)


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
        if t == R.SPHERE:
            add(f[:3] - abs(f[3]), f[:3] + abs(f[3]))
        elif t in (R.XY_RECT, R.XZ_RECT, R.YZ_RECT):
            ka, aa, ba = R._rect_axes(t)
            for a, b in ((f[0], f[2]), (f[1], f[3])):
                q = np.zeros(3)
                q[aa], q[ba], q[ka] = a, b, f[4]
                add(q)
        elif t == R.CYLINDER:
            r = abs(f[0])
            for k in range(8):
                q = np.array([r if k & 1 else -r, r if k & 2 else -r, f[2] if k & 4 else f[1], 1.0])
                add(m.reshape(3, 4) @ q)
        elif t == R.TRIANGLE:
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


def attach(S, sc):
    """give the RefScene the records of the scene's analytic lights, by index into S.lights (a light whose weight is not
    positive and finite is in neither list)"""
    radius = bound_radius(sc.prims())
    recs = [record(al, radius) for al in sc.analytic_lights()]
    recs = [r for r in recs if r["weight"] > 0 and np.isfinite(r["weight"])]
    at = [i for i, l in enumerate(S.lights) if l["shape"] in (POINT, SPOT, DISTANT)]
    assert len(at) == len(recs) and all(S.lights[i]["shape"] == r["type"] for i, r in zip(at, recs)), (at, [r["type"] for r in recs])
    S.analytic = dict(zip(at, recs))
    return S


def pb_bound(S):
    """a bound of the BSDF densities a light sample can meet: lambertian 1 / pi; metal of fuzz f: 3 (1 + f)^2 / (2 pi f^2); a
    GGX lobe of alpha = max(r^2, 1e-3): G1 D / (4 wo.z) <= 1 / (2 pi alpha^3)"""
    b = 1 / np.pi
    for m in S.mats:
        f = float(m["fuzz"])
        if m["type"] == R.METAL and f >= R.METAL_MIN_FUZZ:
            b = max(b, 3 * (1 + f) ** 2 / (2 * np.pi * f * f))
        elif m["type"] in (R.ROUGH_METAL, R.PLASTIC, RG.ROUGH_GLASS) and f >= R.GLOSSY_MIN_ROUGHNESS:
            b = max(b, 1 / (2 * np.pi * max(f * f, 1e-3) ** 3) + 1 / np.pi)
    return b


def falloff_of(rec, ld, T, perturb=()):
    """the spot's falloff towards the vertex at -ld from it"""
    a = np.atleast_2d(np.asarray(rec["axis"]).astype(T))  # (one axis, or one per vertex)
    with np.errstate(all="ignore"):
        c = -R._dot(a, ld) / np.sqrt(R._dot(ld, ld))
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


def sample(S, li, p, u1, u2, T, perturb=(), log=None):
    """(ld, pl, colour) of the analytic light li at the vertices p, at its true scale (no K)"""
    L, rec = S.lights[li], S.analytic[li]
    sel = T(L["probability"])
    n = len(p)
    colour = np.broadcast_to(L["emission"].astype(T), (n, 3)).copy()
    if rec["type"] == DISTANT:
        ld = (T(rec["dist"]) * cone_direction(rec["axis"], rec["omc"], u1, u2, T)).astype(T)
        pl = np.full(n, sel, T)
        if "distant_unfolded" in perturb:
            colour = (colour / T(rec["fold"])).astype(T)
        if log is not None:
            log["distant_samples"] += n
            log["distant_alpha_zero_samples"] += n if rec["omc"] == 0 else 0
        return ld, pl, colour
    ld = (rec["x"].astype(T) - p).astype(T)
    d2 = R._dot(ld, ld)
    pl = np.full(n, sel, T) if "point_no_inverse_square" in perturb else (sel * d2).astype(T)
    if rec["type"] == SPOT:
        fall = falloff_of(rec, ld, T, perturb)
        # (the falloff on the colour, not under pl: the same product, and K pl stays in range at a falloff of 1e-30)
        pl = np.where(fall > 0, pl, 0).astype(T)
        colour = (colour * fall[:, None]).astype(T)
        if log is not None:
            log["spot_samples"] += n
            log["spot_falloff_zero"] += int((fall == 0).sum())
            log["spot_falloff_one"] += int((fall == 1).sum())
            log["spot_falloff_partial"] += int(((fall > 0) & (fall < 1)).sum())
    elif log is not None:
        log["point_samples"] += n
    return ld, np.where(d2 > 0, pl, 0).astype(T), colour


@contextlib.contextmanager
def installed(perturb=(), log=None, report=None):
    """ref64.sample_light with the analytic lights of an attach()ed RefScene, for the length of the block"""
    original = R.sample_light

    def sample_light(S, li, p, u1, u2, T, perturb_=()):
        if S.lights[li]["shape"] not in (POINT, SPOT, DISTANT):
            return original(S, li, p, u1, u2, T, perturb_)
        ld, pl, colour = sample(S, li, p, u1, u2, T, tuple(perturb) + tuple(perturb_), log)
        K = 1.0 if "delta_power_heuristic" in perturb else K_OF[np.dtype(T)]
        with np.errstate(all="ignore"):
            kpl = (T(K) * pl).astype(T)
            made = kpl[pl > 0]
            if K != 1.0 and len(made):
                if not np.isfinite(made * made).all():
                    raise ArithmeticError(f"(K pl)^2 overflows {np.dtype(T)} at K = 2^{int(np.log2(K))}")
                late = int((pb_bound(S) ** 2 / (made.astype(np.float64) ** 2) > np.finfo(T).eps / 4).sum())
                if late and report is None:
                    raise ArithmeticError(f"pb^2 / (K pl)^2 does not vanish at {np.dtype(T)} for {late} samples (K = 2^{int(np.log2(K))})")
                if late:
                    report["not_vanishing"] = report.get("not_vanishing", 0) + late
        return ld, kpl, (T(K) * colour).astype(T), np.full(len(p), R.NONE, np.int64)
    R.sample_light = sample_light
    try:
        yield
    finally:
        R.sample_light = original


def trace(S, words, perturb=(), log=None, report=None, sc=None, **kw):
    """ref64.trace through ref64_glass (rough glass, quads and, with sc, bumps) with the analytic lights installed"""
    rest = tuple(x for x in perturb if x not in PERTURBATIONS)
    with installed(perturb, log, report):
        return RG.trace(S, words, perturb=rest, sc=sc, **kw)


def reference(S, words, sc=None):
    """ref64.reference's four results, the tally extended by tally() and the log of the fp64 run"""
    log, glass_log = new_log(), RG.new_log()
    with installed((), log):
        rgb, sig64, draws = RG.trace(S, words, log=glass_log, sc=sc)
    with installed((), None, {}):  # (the fp32 run's radiance is discarded: its signatures say which samples are stable)
        _, sig32, _ = RG.trace(S, words, dtype=np.float32, sc=sc)
    P = RG.present(S)
    return rgb, R.same_signature(sig64, sig32), draws, dict(R.tally(sig64, P), **RG.tally(sig64, P, glass_log), **tally(sig64, S, log))


def tally(sig, S, log):
    """What an analytic-light case is there for.  From the signatures: light samples per type, their shadow rays occluded and
    clear, glossy vertices (rough metal, plastic, rough glass events) that took a sample of an analytic light and had it arrive,
    emitter hits weighted by MIS.  From the wrapper's log: the spot samples by falloff (LOG_KEYS)."""
    v = sig[:, R.SAMPLE_COLUMNS:].reshape(len(sig), -1, R.VERTEX_COLUMNS)
    event, light, shadow, how = (v[:, :, c] for c in (R.C_EVENT, R.C_LIGHT, R.C_SHADOW, R.C_HIT_WEIGHT))
    shape = S.lights["shape"] if len(S.lights) else np.zeros(1, np.int32)
    of = lambda kind: (light >= 0) & (shape[np.clip(light, 0, len(shape) - 1)] == kind)
    delta = of(POINT) | of(SPOT) | of(DISTANT)
    glossy = np.isin(event, RG.G.GLOSSY_EVENTS)
    out = {"analytic_" + k: v for k, v in log.items()}
    out.update(point_picks=int(of(POINT).sum()), spot_picks=int(of(SPOT).sum()), distant_picks=int(of(DISTANT).sum()),
               area_picks=int(((light >= 0) & ~delta).sum()),
               analytic_shadow_occluded=int((delta & (shadow == R.SHADOW_OCCLUDED)).sum()),
               analytic_shadow_clear=int((delta & (shadow == R.SHADOW_CLEAR)).sum()),
               analytic_no_shadow_ray=int((delta & (shadow == R.SHADOW_NONE)).sum()),
               glossy_lit_by_analytic=int((glossy & delta & (shadow == R.SHADOW_CLEAR)).sum()),
               emitter_mis_hits=int(((event == R.EV_EMIT) & (how == R.HIT_MIS)).sum()))
    return out
