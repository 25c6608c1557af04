"""Rough glass for ref64.py, in NumPy at a floating type of the caller's choice.

Test infrastructure only, written from the definition of the material (include/rtmi.h, rt_scene_add_rough_glass), not from
csrc/rt_glass.h: plain operations, no fused ones.  All vectors are local to the frame of Duff et al. about the face-turned
shading normal n, wo = -unit(d), alpha = max(r^2, 1e-3), eta = front ? 1 / ir : ir (1 / ir as the packer rounds it, in fp32).
    wo.z <= 0                      absorbed: no draws, no light sample
    draws uf, u1, u2;  h = the visible normal of the GGX lobe from (u1, u2);  c = wo.h
    s2 = eta^2 (1 - c^2);  F = 1 where s2 >= 1, else with ct = sqrt(1 - s2):
    rs = (eta c - ct) / (eta c + ct),  rp = (c - eta ct) / (c + eta ct),  F = (rs^2 + rp^2) / 2
    uf < F:  wi = 2 c h - wo, absorbed if wi.z <= 0;  pdf_b = F G1(wo) D(h) / (4 wo.z)
    else:    wi = (eta c - ct) h - eta wo, absorbed if wi.z >= 0;  pdf_b = -1: an emitter behind it counts at full weight
    attenuation = Tr G2(wo, wi) / G1(wo);  Tr = 1 on a front hit, exp(-sigma t |d|) per channel on a back hit
    light sample (r >= 0.05, wo.z > 0), wl.z > 0, h_l = unit(wo + wl):  f cos = Tr F(wo.h_l) D(h_l) G2 / (4 wo.z),
    pdf_b = F(wo.h_l) G1(wo) D(h_l) / (4 wo.z);  both zero for wl.z <= 0

This file holds the model alone and imports nothing of ref64.  ref64.trace()'s glossy block states the vertex: the side from the
hit record, eta_of() and tint() over t |d|, the draws uf, u1, u2 in the model's order, glass_sample(), the r >= 0.05 and
absorbed-vertex rules, pdf_b = -1 as a full-weight emitter hit, glass_eval() times the throughput in front of the vertex for the
light sample.  A reflection is signed EV_COAT (EV_COAT_ABSORBED), a refraction EV_BODY, wo.z <= 0 EV_BELOW.  glass_sample()
counts what the signatures keep neither (the critical angle, the side) into trace()'s log, under LOG_KEYS.

Deliberate mistakes (names in `perturb`, as ref64.trace takes them):
  fresnel_draw_last        uf taken after u1, u2 (glass's name for lobe_draw_last)
  g1_for_g2                the attenuation without G2 / G1 (the glossy materials' name: it applies to glass rows too)
  eta_from_wrong_side      eta = front ? ir : 1 / ir
  no_absorption            Tr = 1 on every hit
  refraction_mis_weighted  a refracted direction carries the density (1 - F) G1 D / (4 wo.z) instead of -1: an emitter behind it
                           is weighted by MIS
"""
import numpy as np

import ref64_glossy as G

ROUGH_GLASS = 6
PERTURBATIONS = ("fresnel_draw_last", "g1_for_g2", "eta_from_wrong_side", "no_absorption", "refraction_mis_weighted")
LOG_KEYS = tuple("glass_" + k for k in ("reflections", "refractions", "tir", "absorbed_reflections", "absorbed_refractions", "below",
                                        "tinted_back_hits", "light_evaluations"))


# ------------------------------------------------------------------------------------------------- the model (local frame)
def fresnel(eta, c):
    """(F, ct, beyond the critical angle) of the exact unpolarised Fresnel term at c = wo.h for the ratio eta"""
    s2 = eta * eta * (1 - c * c)
    tir = s2 >= 1
    with np.errstate(all="ignore"):
        ct = np.sqrt(np.maximum(0, 1 - s2))
        rs = (eta * c - ct) / (eta * c + ct)
        rp = (c - eta * ct) / (c + eta * ct)
        F = np.where(tir, 1, (rs * rs + rp * rp) / 2)
    return F.astype(c.dtype), np.where(tir, 0, ct).astype(c.dtype), tir


def eta_of(ir, front, T, perturb=()):
    """eta per vertex: 1 / ir (rounded to fp32, as the packer stores it) on a front hit, ir on a back hit"""
    ir32 = np.asarray(ir, np.float32)
    inv = (np.float32(1) / ir32).astype(T)
    if "eta_from_wrong_side" in perturb:
        front = ~front
    return np.where(front, inv, ir32.astype(T))


def tint(sigma, dist, T):
    """Tr per channel over the distance dist"""
    return np.exp(-(sigma.astype(T) * dist[:, None])).astype(T)


def refract(wo, h, eta, c, ct):
    return (eta * c - ct)[:, None] * h - eta[:, None] * wo


def glass_sample(n, ud, alpha, eta, tr, uf, u1, u2, T, perturb=(), log=None):
    """The scatter step, vectorised over vertices: n the unit shading normal, ud = unit(d) of the arriving ray, eta and the tint
    tr [N][3] of each.  -> (unit wi in world space, attenuation, pdf_b, below: wo.z <= 0, absorbed: wi on the wrong side,
    reflected).  Rows that are below or absorbed hold zeros."""
    N = len(n)
    t1, t2 = G.frame(n, T)
    wo = G.to_local(-ud, n, t1, t2)
    below = ~(wo[:, 2] > 0)
    wi_w, att, pdf = np.zeros((N, 3), T), np.zeros((N, 3), T), np.zeros(N, T)
    absorbed, reflected = np.zeros(N, bool), np.zeros(N, bool)
    k = np.flatnonzero(~below)
    if log is not None:
        log["glass_below"] += int(below.sum())
    if len(k) == 0:
        return wi_w, att, pdf, below, absorbed, reflected
    a, w, e = alpha[k], wo[k], eta[k]
    with np.errstate(all="ignore"):
        h = G.sample_h(a, w, u1[k], u2[k], T)
        c = G._dot(w, h)
        F, ct, tir = fresnel(e, c)
        refl = uf[k] < F
        wi = np.where(refl[:, None], 2 * c[:, None] * h - w, refract(w, h, e, c, ct))
        ok = np.where(refl, wi[:, 2] > 0, wi[:, 2] < 0)
        lo, li = G.ggx_lambda(a, w), G.ggx_lambda(a, wi)
        g1, g2 = 1 / (1 + lo), 1 / (1 + lo + li)
        ratio = np.ones_like(g1) if "g1_for_g2" in perturb else g2 / g1
        pdf_s = G.ggx_d(a, h, T) / (4 * w[:, 2]) * g1
        pd = np.where(refl, F * pdf_s, (1 - F) * pdf_s if "refraction_mis_weighted" in perturb else T(-1))
    g = k[ok]
    wi_w[g] = G.to_world(wi[ok], n[g], t1[g], t2[g])
    att[g] = tr[g] * ratio[ok][:, None]
    pdf[g] = pd[ok]
    absorbed[k] = ~ok
    reflected[k] = refl
    if log is not None:
        log["glass_reflections"] += int((refl & ok).sum())
        log["glass_refractions"] += int((~refl & ok).sum())
        log["glass_tir"] += int(tir.sum())
        log["glass_absorbed_reflections"] += int((refl & ~ok).sum())
        log["glass_absorbed_refractions"] += int((~refl & ~ok).sum())
    return wi_w, att, pdf, below, absorbed, reflected


def glass_eval(n, ud, alpha, eta, tr, wl, T):
    """(f cos [N][3], pdf_b [N]) of the unit world directions wl: the reflection hemisphere alone"""
    N = len(n)
    t1, t2 = G.frame(n, T)
    wo, wi = G.to_local(-ud, n, t1, t2), G.to_local(wl, n, t1, t2)
    ok = (wo[:, 2] > 0) & (wi[:, 2] > 0)
    fcos, pdf = np.zeros((N, 3), T), np.zeros(N, T)
    k = np.flatnonzero(ok)
    if len(k):
        with np.errstate(all="ignore"):
            h = G._unit(wo[k] + wi[k])
            spec, pdf_s, _ = G.lobe_terms(alpha[k], wo[k], wi[k], h, T)
            F, _, _ = fresnel(eta[k], G._dot(wo[k], h))
        fcos[k] = tr[k] * (F * spec)[:, None]
        pdf[k] = F * pdf_s
    return fcos, pdf
