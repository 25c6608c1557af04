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

ref64.py is not edited and its path loop is not restated.  present() hands ref64.trace a COPY of the RefScene in which every
rough_glass is a plastic: its `ir` negated (the mark), its texture one of the sentinel textures appended to S.texs (a solid
texture whose c0 is the material's sigma).  installed() replaces, for the length of a trace,
    r0_of          a negative ir comes back as |ir|: the "r0" of a glass row is its index (> 1, which no r0 is)
    texture_value  a sentinel texture's value is +1 on a front hit and -Tr on a back hit (the sign bit carries the side; the
                   wrapper gets o, d, t, idx, the mover and the shutter time, which is what the tint and the side need)
    glossy_sample  rows with r0 > 1 are glass: (wi, attenuation, pdf_b, below, absorbed, lobe = reflected)
    glossy_eval    likewise
and trace() does the rest: ul, u1, u2 in the model's order, the r >= 0.05 and absorbed-vertex rules, pdf_b = -1 as a full-weight
emitter hit, the light sample times the throughput in front of the vertex.  A reflection is signed EV_COAT (EV_COAT_ABSORBED), a
refraction EV_BODY, wo.z <= 0 EV_BELOW.  Bumps and quads come with ref64_bump / ref64_quads, entered by installed(sc=...).

Deliberate mistakes (names in `perturb`):
  fresnel_draw_last        uf taken after u1, u2 (ref64's lobe_draw_last)
  g1_for_g2                the attenuation without G2 / G1 (ref64's own name; honoured here for the glass rows)
  eta_from_wrong_side      eta = front ? ir : 1 / ir
  no_absorption            Tr = 1 on every hit
  refraction_mis_weighted  a refracted direction carries the density (1 - F) G1 D / (4 wo.z) instead of -1: an emitter behind it
                           is weighted by MIS
"""
import contextlib
import copy

import numpy as np

import ref64 as R
import ref64_bump as B
import ref64_glossy as G
import ref64_quads as Q

ROUGH_GLASS = 6
PERTURBATIONS = ("fresnel_draw_last", "g1_for_g2", "eta_from_wrong_side", "no_absorption", "refraction_mis_weighted")
LOG_KEYS = ("reflections", "refractions", "tir", "absorbed_reflections", "absorbed_refractions", "below", "tinted_back_hits",
            "light_evaluations")


def new_log():
    """what installed() counts over the calls of one trace (the signatures keep neither the critical angle nor the side)"""
    return dict.fromkeys(LOG_KEYS, 0)


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
        log["below"] += int(below.sum())
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
        log["reflections"] += int((refl & ok).sum())
        log["refractions"] += int((~refl & ok).sum())
        log["tir"] += int(tir.sum())
        log["absorbed_reflections"] += int((refl & ~ok).sum())
        log["absorbed_refractions"] += int((~refl & ~ok).sum())
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


# ------------------------------------------------------------------------------------------------- presenting it to ref64
def is_glass_scene(S):
    return bool((S.mats["type"] == ROUGH_GLASS).any())


def present(S):
    """a copy of the RefScene with every rough_glass shown as a plastic (see the module's docstring); S itself where it has none"""
    if not is_glass_scene(S):
        return S
    P = copy.copy(S)
    P.mats, first = S.mats.copy(), len(S.texs)
    glass = np.flatnonzero(S.mats["type"] == ROUGH_GLASS)
    extra = np.zeros(len(glass), S.texs.dtype)
    extra["type"] = R.SOLID
    extra["c0"] = S.mats["albedo"][glass]
    P.texs = np.concatenate([S.texs, extra])
    P.mats["type"][glass] = G.PLASTIC
    P.mats["texture"][glass] = first + np.arange(len(glass))
    P.mats["ir"][glass] = -S.mats["ir"][glass]
    P.glass_textures = (first, first + len(glass))
    P.glass_materials = glass
    return P


def _front(S, p, o, d, t, idx, mov, time, T):
    """the side of the hits: a static primitive's by ref64.hit_record, a mover's from its centre at the sample's time"""
    front = np.zeros(len(o), bool)
    st = np.flatnonzero(mov < 0) if mov is not None else np.arange(len(o))
    if len(st):
        front[st] = R.hit_record(S, o[st], d[st], t[st], idx[st], T)[2]
    if mov is not None:
        for mi in np.unique(mov[mov >= 0]):
            q = np.flatnonzero(mov == mi)
            m = S.movers[mi]
            n_out = (p[q] - R.mover_centre(m, time[q], T)) / T(m["radius"])
            front[q] = R._dot(d[q], n_out) < 0
    return front


@contextlib.contextmanager
def installed(perturb=(), log=None, sc=None):
    """ref64's r0_of, texture_value, glossy_sample and glossy_eval with rough glass, for the length of the block; with the product
    scene sc, its bumps (ref64_bump) too, and quads (ref64_quads) always.  A scene that was not present()ed has no row these
    wrappers keep: every call goes to the function it replaced."""
    orig = {k: getattr(R, k) for k in ("r0_of", "texture_value", "glossy_sample", "glossy_eval")}

    def r0_of(ior):
        ior = np.asarray(ior, np.float32)
        with np.errstate(all="ignore"):
            return np.where(ior < 0, -ior, orig["r0_of"](np.abs(ior))).astype(np.float32)

    def texture_value(S, tex, p, T, o=None, d=None, t=None, idx=None, mov=None, time=None, perturb_=()):
        lo, hi = getattr(S, "glass_textures", (0, 0))
        g = (tex >= lo) & (tex < hi)
        if not g.any():
            return orig["texture_value"](S, tex, p, T, o, d, t, idx, mov, time, perturb_)
        out, texel = np.zeros_like(p), np.full(len(p), R.NONE, np.int64)
        if (~g).any():
            r = ~g
            sub = lambda x: None if x is None else x[r]
            out[r], texel[r] = orig["texture_value"](S, tex[r], p[r], T, sub(o), sub(d), sub(t), sub(idx), sub(mov), sub(time), perturb_)
        front = _front(S, p[g], o[g], d[g], t[g], idx[g], None if mov is None else mov[g], None if time is None else time[g], T)
        sigma = S.texs["c0"][tex[g]]
        tr = tint(sigma, t[g] * np.sqrt(R._dot(d[g], d[g])), T)
        if "no_absorption" in perturb:
            tr = np.ones_like(tr)
        if log is not None:
            log["tinted_back_hits"] += int((~front & (sigma > 0).any(axis=1)).sum())
        out[g] = np.where(front[:, None], T(1), -tr)
        return out, texel

    def split(f0, plastic):
        return plastic & (f0[:, 0] > 1)

    def side_and_tint(rho):
        front = ~np.signbit(rho[:, 0])
        return front, np.where(front[:, None], 1, np.abs(rho)).astype(rho.dtype)

    def glossy_sample(n, ud, alpha, plastic, f0, rho, ul, u1, u2, T, perturb_=()):
        g = split(f0, plastic)
        if not g.any():
            return orig["glossy_sample"](n, ud, alpha, plastic, f0, rho, ul, u1, u2, T, perturb_)
        N = len(n)
        outs = [np.zeros((N, 3), T), np.zeros((N, 3), T), np.zeros(N, T), np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, bool)]
        r = ~g
        if r.any():
            for dst, src in zip(outs, orig["glossy_sample"](n[r], ud[r], alpha[r], plastic[r], f0[r], rho[r], ul[r], u1[r], u2[r], T, perturb_)):
                dst[r] = src
        front, tr = side_and_tint(rho[g])
        eta = eta_of(f0[g, 0], front, T, perturb)
        for dst, src in zip(outs, glass_sample(n[g], ud[g], alpha[g], eta, tr, ul[g], u1[g], u2[g], T, tuple(perturb) + tuple(perturb_), log)):
            dst[g] = src
        return tuple(outs)

    def glossy_eval(n, ud, alpha, plastic, f0, rho, wl, T):
        g = split(f0, plastic)
        if not g.any():
            return orig["glossy_eval"](n, ud, alpha, plastic, f0, rho, wl, T)
        N = len(n)
        fcos, pdf = np.zeros((N, 3), T), np.zeros(N, T)
        r = ~g
        if r.any():
            fcos[r], pdf[r] = orig["glossy_eval"](n[r], ud[r], alpha[r], plastic[r], f0[r], rho[r], wl[r], T)
        front, tr = side_and_tint(rho[g])
        fcos[g], pdf[g] = glass_eval(n[g], ud[g], alpha[g], eta_of(f0[g, 0], front, T, perturb), tr, wl[g], T)
        if log is not None:
            log["light_evaluations"] += int(g.sum())
        return fcos, pdf

    new = dict(r0_of=r0_of, texture_value=texture_value, glossy_sample=glossy_sample, glossy_eval=glossy_eval)
    with contextlib.ExitStack() as stack:
        stack.enter_context(Q.installed())
        if sc is not None and any(sc.bump(m) is not None for m in range(len(sc.materials()))):
            stack.enter_context(B.installed(sc))
        for k, f in new.items():
            setattr(R, k, f)
        try:
            yield
        finally:
            for k, f in orig.items():
                setattr(R, k, f)


def _rest(perturb):
    """the names ref64.trace itself reads: fresnel_draw_last is its lobe_draw_last"""
    out = tuple(x for x in perturb if x not in PERTURBATIONS or x == "g1_for_g2")
    return out + (("lobe_draw_last",) if "fresnel_draw_last" in perturb else ())


def trace(S, words, perturb=(), log=None, sc=None, **kw):
    with installed(perturb, log, sc):
        return R.trace(present(S), words, perturb=_rest(perturb), **kw)


def reference(S, words, shutter=None, sc=None):
    """ref64.reference's four results and the log of the fp64 run"""
    P, log = present(S), new_log()
    with installed((), log, sc):
        rgb, sig64, draws = R.trace(P, words, shutter=shutter)
    with installed((), None, sc):
        _, sig32, _ = R.trace(P, words, dtype=np.float32, shutter=shutter)
    return rgb, R.same_signature(sig64, sig32), draws, dict(R.tally(sig64, P), **tally(sig64, P, log))


def tally(sig, P, log):
    """What a glass case is there for.  From the reference's signatures, on the vertices whose surface is a rough glass: by event,
    with a light sample, the emitter hits at full weight behind a refraction and weighted below 1 behind a reflection, and the
    roughnesses met.  From the wrapper's log: what the signatures do not keep (LOG_KEYS)."""
    v = sig[:, R.SAMPLE_COLUMNS:].reshape(len(sig), -1, R.VERTEX_COLUMNS)
    event, prim, mover, light, how = (v[:, :, c] for c in (R.C_EVENT, R.C_PRIM, R.C_MOVER, R.C_LIGHT, R.C_HIT_WEIGHT))
    glass_mat = np.zeros(len(P.mats), bool)
    glass_mat[getattr(P, "glass_materials", [])] = True
    of_prim = glass_mat[P.prims["material"]] if len(P.prims) else np.zeros(1, bool)
    of_mover = glass_mat[P.movers["material"]] if len(P.movers) else np.zeros(1, bool)
    pick = lambda flags, i: (i >= 0) & flags[np.clip(i, 0, len(flags) - 1)]
    on = np.isin(event, G.GLOSSY_EVENTS) & np.where(mover >= 0, pick(of_mover, mover), pick(of_prim, prim))
    nxt = lambda x: np.concatenate([x[:, 1:], np.zeros((len(x), 1), bool)], axis=1)
    emit_full, emit_mis = (event == R.EV_EMIT) & (how == R.HIT_UNSAMPLED), (event == R.EV_EMIT) & (how == R.HIT_MIS)
    rough = np.full(event.shape, np.nan)
    static = on & (mover < 0)
    rough[static] = P.mats["fuzz"][P.prims["material"]][prim[static]]
    return dict({"glass_" + k: v for k, v in log.items()},
                glass_vertices=int(on.sum()), glass_mover_vertices=int((on & (mover >= 0)).sum()),
                glass_reflect_events=int((on & (event == G.EV_COAT)).sum()), glass_refract_events=int((on & (event == G.EV_BODY)).sum()),
                glass_below_events=int((on & (event == G.EV_BELOW)).sum()),
                glass_light_samples=int((on & (light != R.NONE)).sum()),
                glass_below_light_samples=int((on & (event == G.EV_BELOW) & (light != R.NONE)).sum()),
                glass_full_weight_hits_behind_refraction=int((on & (event == G.EV_BODY) & (light != R.NONE) & nxt(emit_full)).sum()),
                glass_mis_hits_behind_reflection=int((on & (event == G.EV_COAT) & nxt(emit_mis)).sum()),
                glass_then_medium=int(((np.cumsum(on & (event == G.EV_BODY), axis=1) > 0) & (event == R.EV_MEDIUM)).sum()),
                glass_roughnesses=sorted(float(np.float32(x)) for x in np.unique(rough[~np.isnan(rough)])))
