"""The glossy materials of DESIGN 7m -- GGX rough metal and coated plastic -- stated in NumPy at a floating type of the caller's
choice: the model that ref64.trace()'s glossy block evaluates.

Test infrastructure only, written from the definitions of DESIGN 7m (which repeat the issue's): the distribution D, Smith's
Lambda, the visible-normal sample of Heitz 2018, the two materials' f cos, pdf_b and attenuation.  Plain operations, no fused
ones; it shares no code with csrc/rt_glossy.h.

This file holds no integrator and imports none: ref64 imports it, never the other way round.  The order of the materials' draws
and the light sample's weight are ref64.trace()'s to state; the perturbations that concern them are named here (PERTURBATIONS)
and listed with every other in ref64.trace()'s docstring.

The signature's C_EVENT gains: EV_ROUGH (a rough-metal vertex that scattered), EV_COAT / EV_BODY (plastic: the lobe taken),
EV_BELOW (absorbed because wo.z <= 0), EV_ROUGH_ABSORBED / EV_COAT_ABSORBED (absorbed because wi.z <= 0).  A glossy vertex that
took a light sample is one of those with C_LIGHT set: glossy_tally() counts them, as a part of ref64.tally()."""
import numpy as np

from ref64_base import _cross, _dot, _unit

ROUGH_METAL, PLASTIC = 4, 5
GLOSSY_MIN_ROUGHNESS = 0.05  # vertices of a glossy material below this roughness take no light sample
EV_ROUGH, EV_COAT, EV_BODY, EV_BELOW, EV_ROUGH_ABSORBED, EV_COAT_ABSORBED = range(30, 36)
GLOSSY_EVENTS = (EV_ROUGH, EV_COAT, EV_BODY, EV_BELOW, EV_ROUGH_ABSORBED, EV_COAT_ABSORBED)
PERTURBATIONS = ("g1_for_g2", "lobe_draw_last", "nee_albedo_pdf")
# the counts of glossy_tally()
GLOSSY_KEYS = ("rough_vertices", "coat_vertices", "body_vertices", "below_vertices", "absorbed_wi_vertices", "glossy_light_samples",
               "absorbed_wi_light_samples", "smooth_glossy_vertices", "smooth_glossy_full_weight_hits", "glossy_env_picks",
               "glossy_escapes_after_light_sample", "medium_then_glossy", "glossy_then_medium", "glossy_mover_vertices", "roulette_losses")


# ------------------------------------------------------------------------------------------------- the model (local frame)
def alpha_of(r):
    """alpha = max(r^2, 1e-3) as the packer stores it (fp32)"""
    r = np.asarray(r, np.float32)
    return np.maximum(r * r, np.float32(1e-3))


def r0_of(ior):
    """r0 = ((ior - 1) / (ior + 1))^2 as the packer stores it (fp32)"""
    ior = np.asarray(ior, np.float32)
    q = (ior - np.float32(1)) / (ior + np.float32(1))
    return q * q


def frame(n, T):
    """(t1, t2): the orthonormal frame of Duff et al. 2017 about the unit vectors n, the one the sphere-light sampler uses"""
    sg = np.copysign(T(1), n[:, 2])
    fa = -1 / (sg + n[:, 2])
    fb = n[:, 0] * n[:, 1] * fa
    t1 = np.stack([1 + sg * n[:, 0] ** 2 * fa, sg * fb, -sg * n[:, 0]], axis=1)
    t2 = np.stack([fb, sg + n[:, 1] ** 2 * fa, -n[:, 1]], axis=1)
    return t1.astype(T), t2.astype(T)


def to_local(v, n, t1, t2):
    return np.stack([_dot(v, t1), _dot(v, t2), _dot(v, n)], axis=1)


def to_world(l, n, t1, t2):
    return l[:, 0:1] * t1 + l[:, 1:2] * t2 + l[:, 2:3] * n


def schlick(f0, c):
    return f0 + (1 - f0) * (1 - c) ** 5


def ggx_d(alpha, h, T):
    a2 = alpha * alpha
    return a2 / (T(np.pi) * (a2 * h[:, 2] ** 2 + h[:, 0] ** 2 + h[:, 1] ** 2) ** 2)


def ggx_lambda(alpha, w):
    return (np.sqrt(1 + alpha * alpha * (w[:, 0] ** 2 + w[:, 1] ** 2) / w[:, 2] ** 2) - 1) / 2


def sample_h(alpha, wo, u1, u2, T):
    """a visible normal of the lobe seen from wo (Heitz 2018), steps 1-7 of DESIGN 7m"""
    vh = _unit(np.stack([alpha * wo[:, 0], alpha * wo[:, 1], wo[:, 2]], axis=1))
    l = np.sqrt(vh[:, 0] ** 2 + vh[:, 1] ** 2)
    with np.errstate(all="ignore"):
        T1 = np.where((l > 0)[:, None], np.stack([-vh[:, 1], vh[:, 0], np.zeros_like(l)], axis=1) / l[:, None],
                      np.array([1, 0, 0], T))
    T2 = _cross(vh, T1)
    rr, phi = np.sqrt(u1), 2 * T(np.pi) * u2
    t1, t2 = rr * np.cos(phi), rr * np.sin(phi)
    s = (1 + vh[:, 2]) / 2
    t2 = (1 - s) * np.sqrt(np.maximum(0, 1 - t1 * t1)) + s * t2
    nh = t1[:, None] * T1 + t2[:, None] * T2 + np.sqrt(np.maximum(0, 1 - t1 * t1 - t2 * t2))[:, None] * vh
    return _unit(np.stack([alpha * nh[:, 0], alpha * nh[:, 1], np.maximum(0, nh[:, 2])], axis=1)).astype(T)


def lobe_terms(alpha, wo, wi, h, T):
    """(D G2 / (4 wo.z), pdf_s = G1(wo) D / (4 wo.z), G2 / G1(wo)) of local directions above the surface"""
    lo, li = ggx_lambda(alpha, wo), ggx_lambda(alpha, wi)
    g1, g2 = 1 / (1 + lo), 1 / (1 + lo + li)
    dq = ggx_d(alpha, h, T) / (4 * wo[:, 2])
    return dq * g2, dq * g1, g2 / g1


def _plastic_terms(alpha, r0, rho, wo, wi, h, T, g1_for_g2=False):
    spec, pdf_s, _ = lobe_terms(alpha, wo, wi, h, T)
    if g1_for_g2:
        spec = pdf_s
    fo, fi = schlick(r0, wo[:, 2]), schlick(r0, wi[:, 2])
    ps = T(0.25) + T(0.75) * fo
    cpi = wi[:, 2] / T(np.pi)
    fcos = (schlick(r0, _dot(wo, h)) * spec)[:, None] + ((1 - fo) * (1 - fi) * cpi)[:, None] * rho
    return fcos, ps * pdf_s + (1 - ps) * cpi


def glossy_sample(n, ud, alpha, plastic, f0, rho, ul, u1, u2, T, perturb=()):
    """Both materials' scatter step, vectorised over vertices: n the unit shading normal, ud = unit(d) of the arriving ray, alpha,
    plastic (bool per vertex), f0 [N][3] (rough metal: F0; plastic: r0 in every channel), rho [N][3] (plastic's body colour), the
    uniforms (ul only read where plastic).  -> (unit wi in world space, attenuation, pdf_b, below: wo.z <= 0, absorbed: wi.z <= 0,
    lobe: the microfacet lobe was drawn).  Rows that are below or absorbed hold zeros."""
    N = len(n)
    t1, t2 = frame(n, T)
    wo = to_local(-ud, n, t1, t2)
    below = ~(wo[:, 2] > 0)
    wi_w, att, pdf = np.zeros((N, 3), T), np.zeros((N, 3), T), np.zeros(N, T)
    absorbed, lobe = np.zeros(N, bool), np.zeros(N, bool)
    k = np.flatnonzero(~below)
    if len(k) == 0:
        return wi_w, att, pdf, below, absorbed, lobe
    a, w, pl = alpha[k], wo[k], plastic[k]
    r0 = f0[k, 0]
    ps = T(0.25) + T(0.75) * schlick(r0, w[:, 2])
    take = ~pl | (ul[k] < ps)
    with np.errstate(all="ignore"):
        h = sample_h(a, w, u1[k], u2[k], T)
        wi = 2 * _dot(w, h)[:, None] * h - w
        phi = 2 * T(np.pi) * u2[k]
        body = np.stack([np.sqrt(u1[k]) * np.cos(phi), np.sqrt(u1[k]) * np.sin(phi), np.sqrt(1 - u1[k])], axis=1)
        wi = np.where(take[:, None], wi, body)
        h = np.where(take[:, None], h, _unit(w + wi))
        up = wi[:, 2] > 0
        spec, pdf_s, ratio = lobe_terms(a, w, wi, h, T)
        if "g1_for_g2" in perturb:
            ratio = np.ones_like(ratio)
        at_m = schlick(f0[k], _dot(w, h)[:, None]) * ratio[:, None]
        fc_p, pdf_p = _plastic_terms(a, r0, rho[k], w, wi, h, T, "g1_for_g2" in perturb)
        at = np.where(pl[:, None], fc_p / pdf_p[:, None], at_m)
        pd = np.where(pl, pdf_p, pdf_s)
    g = k[up]
    wi_w[g] = to_world(wi[up], n[g], t1[g], t2[g])
    att[g], pdf[g] = at[up], pd[up]
    absorbed[k] = ~up
    lobe[k] = take
    return wi_w, att, pdf, below, absorbed, lobe


def glossy_eval(n, ud, alpha, plastic, f0, rho, wl, T):
    """(f cos [N][3], pdf_b [N]) of the unit world directions wl; zeros where wo.z <= 0 or wl.z <= 0"""
    N = len(n)
    t1, t2 = frame(n, T)
    wo, wi = to_local(-ud, n, t1, t2), to_local(wl, n, t1, t2)
    ok = (wo[:, 2] > 0) & (wi[:, 2] > 0)
    fcos, pdf = np.zeros((N, 3), T), np.zeros(N, T)
    k = np.flatnonzero(ok)
    if len(k):
        with np.errstate(all="ignore"):
            h = _unit(wo[k] + wi[k])
            spec, pdf_s, _ = lobe_terms(alpha[k], wo[k], wi[k], h, T)
            fc_m = schlick(f0[k], _dot(wo[k], h)[:, None]) * spec[:, None]
            fc_p, pdf_p = _plastic_terms(alpha[k], f0[k, 0], rho[k], wo[k], wi[k], h, T)
        fcos[k] = np.where(plastic[k][:, None], fc_p, fc_m)
        pdf[k] = np.where(plastic[k], pdf_p, pdf_s)
    return fcos, pdf


# ------------------------------------------------------------------------------------------------- the tally
def glossy_tally(event, at, S):
    """how often the vertices a glossy case is there for occurred: by event, with a light sample, by material roughness, and in
    sequence with emitters, media and the environment.  event [N][vertices]: the signature's C_EVENT; `at`: what ref64.tally()
    read from the other columns, per vertex -- prim, light (the light picked), env_light (the environment's index among the
    lights, -1: none) and the flags took_light, clear (the shadow ray's verdict), medium, on_mover, full_weight_emitter (an
    emitter hit at full weight), missed_to_texel (an escape that read an environment texel), lost (the roulette) -- and, per
    MATERIAL, roughness (NaN where the material has no single one: a pbr material under a map), so that
    this file knows the glossy event codes and no others.  S: the RefScene, or None (no count by roughness then)."""
    prim, light, took_light, med, on_mover = at["prim"], at["light"], at["took_light"], at["medium"], at["on_mover"]
    glossy = np.isin(event, GLOSSY_EVENTS)
    sampled = glossy & took_light
    later = lambda x: np.flip(np.cumsum(np.flip(x, axis=1), axis=1), axis=1) - x > 0
    # the roughness of the material under each static glossy vertex (movers: by their own material, counted separately)
    rough = np.full(event.shape, np.nan)
    if S is not None and len(S.prims):
        r_of_prim = at["roughness"][S.prims["material"]]
        on_static = glossy & (prim >= 0) & ~on_mover
        rough[on_static] = r_of_prim[prim[on_static]]
    with np.errstate(invalid="ignore"):
        smooth = glossy & (rough < GLOSSY_MIN_ROUGHNESS)
    nxt_emit_full = np.zeros_like(glossy)
    nxt_emit_full[:, :-1] = at["full_weight_emitter"][:, 1:]
    env_pick = sampled & (light == at["env_light"])
    # a BSDF ray from a glossy vertex that took a light sample and escapes: its miss is the next block's C_MISS_TEXEL
    escaped = np.zeros_like(glossy)
    escaped[:, :-1] = sampled[:, :-1] & at["missed_to_texel"][:, 1:]
    absorbed_wi = np.isin(event, (EV_ROUGH_ABSORBED, EV_COAT_ABSORBED))
    return dict(rough_vertices=int((event == EV_ROUGH).sum()), coat_vertices=int((event == EV_COAT).sum()),
                body_vertices=int((event == EV_BODY).sum()), below_vertices=int((event == EV_BELOW).sum()),
                absorbed_wi_vertices=int(absorbed_wi.sum()),
                glossy_light_samples=int(sampled.sum()),
                glossy_light_samples_clear=int((sampled & at["clear"]).sum()),
                absorbed_wi_light_samples=int((absorbed_wi & took_light).sum()),
                below_light_samples=int(((event == EV_BELOW) & took_light).sum()),
                smooth_glossy_vertices=int(smooth.sum()), smooth_glossy_light_samples=int((smooth & took_light).sum()),
                smooth_glossy_full_weight_hits=int((smooth & nxt_emit_full).sum()),
                roughnesses=sorted(float(np.float32(x)) for x in np.unique(rough[~np.isnan(rough)])),
                glossy_env_picks=int(env_pick.sum()), glossy_escapes_after_light_sample=int(escaped.sum()),
                medium_then_glossy=int((med & later(glossy)).any(axis=1).sum()),
                glossy_then_medium=int((glossy & later(med)).any(axis=1).sum()),
                glossy_mover_vertices=int((glossy & on_mover).sum()),
                glossy_static_vertices=int((glossy & ~on_mover).sum()),
                roulette_losses=int(at["lost"].sum()))
