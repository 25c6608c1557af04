"""The glossy materials of DESIGN 7m -- GGX rough metal and coated plastic -- stated in NumPy at a floating type of the caller's
choice, and ref64.trace restated with them.

Test infrastructure only, written from the definitions of DESIGN 7m (which repeat the issue's): the distribution D, Smith's
Lambda, the visible-normal sample of Heitz 2018, the two materials' f cos, pdf_b and attenuation, the order of their draws and
the light sample's weight.  Plain operations, no fused ones; it shares no code with csrc/rt_glossy.h.

trace() is ref64.trace's loop with the two materials added.  Everything else -- the hit queries, the hit record (taken through
the module attribute ref64.hit_record, so that smooth_scenes.smooth_reference() still swaps it), textures, lights, the
environment, media, movers, the MIS weight, judge -- is ref64's, imported.  On a scene without glossy materials it returns
exactly what ref64.trace returns (test_glossy.py asserts it on three cases): that licenses the restatement.

The signature's C_EVENT gains: EV_ROUGH (a rough-metal vertex that scattered), EV_COAT / EV_BODY (plastic: the lobe taken),
EV_BELOW (absorbed because wo.z <= 0), EV_ROUGH_ABSORBED / EV_COAT_ABSORBED (absorbed because wi.z <= 0).  A glossy vertex that
took a light sample is one of those with C_LIGHT set: glossy_tally() counts them."""
import numpy as np

import ref64 as R
from ref64 import (NONE, C_PRIM, C_MISS_TEXEL, C_PARITY, C_EVENT, C_ROULETTE, C_LIGHT, C_TEXEL, C_SHADOW, C_HIT_WEIGHT, C_ALIAS,
                   C_MOVER, C_DREW, C_MEDIUM, C_IMAGE_TEXEL, C_BLOCKER, VERTEX_COLUMNS, SAMPLE_COLUMNS, _dot, _unit)

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
    T2 = R._cross(vh, T1)
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


# ------------------------------------------------------------------------------------------------- the integrator
def trace(S, words, first_pixel=0, dtype=np.float64, perturb=(), shutter=None, probe=None):
    """ref64.trace with rough_metal and plastic vertices.  probe: a dict that receives the FIRST vertex of every sample (what a
    feature pass shows): "glossy" (bool: it lies on a glossy material), "albedo" (F0 or rho there), "normal" (the shading normal).  perturb: ref64.trace's names, and "g1_for_g2" (the attenuation with
    G1(wo) in place of G2: without the factor G2 / G1), "lobe_draw_last" (plastic's lobe draw taken after u1, u2 instead of in
    front of them), "nee_albedo_pdf" (the light sample's f cos taken as albedo x pdf_b, the shortcut that holds for lambertian
    and metal)."""
    T = dtype
    N = len(words)
    D = R._Draws(words, T)
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
    mis = np.full(N, -1, T)
    alive = depth > 0
    if rr > 0:
        lost = D.next(everyone) > rr
        note(1, everyone, lost)
        alive &= ~lost
        beta = beta / rr

    while alive.any():
        who = np.flatnonzero(alive)
        oo, dd = o[who], d[who]
        t_hit, idx = R.closest_hit(S, oo, dd, np.inf, T)
        sig.append(np.full((N, VERTEX_COLUMNS), NONE, np.int64))
        note(C_PRIM, who, idx)
        mov = np.full(len(who), -1, np.int64)
        if len(S.movers):
            a = _dot(dd, dd)
            t_min = T(R.T_MIN)
            for mi, m in enumerate(S.movers):
                tt = R.mover_t(m, time[who], oo, dd, a, t_min, t_hit, T)
                with np.errstate(invalid="ignore"):
                    ok = (tt >= t_min) & (tt <= t_hit)
                t_hit = np.where(ok, tt, t_hit)
                mov = np.where(ok, mi, mov)
            note(C_MOVER, who, mov)
        t_m = np.full(len(who), np.inf, T)
        med = np.full(len(who), -1, np.int64)
        if len(S.media):
            drew = np.zeros(len(who), np.int64)
            length = np.sqrt(_dot(dd, dd))
            for mi, m in enumerate(S.media):
                sigma = T(m["density"])
                if not sigma > 0:
                    continue
                a, b, ok = R.medium_interval(m, oo, dd, t_hit, T)
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
        vol = med >= 0
        t_hit = np.where(vol, t_m, t_hit)
        miss = (idx < 0) & (mov < 0) & ~vol
        if miss.any():
            m = who[miss]
            ud = _unit(dd[miss])
            if S.env is not None:
                bg, pe, texel = R.env_eval(S.env, ud, T)
                note(C_MISS_TEXEL, m, texel)
                if len(S.lights) and S.lights[-1]["shape"] == R.ENVIRONMENT:
                    pl = T(S.lights[-1]["probability"]) * pe
                    bg = bg * R._mis_bsdf(mis[m], pl, perturb)[:, None]
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
        p = oo + t_hit[:, None] * dd
        n = np.zeros_like(dd)
        front = np.zeros(len(who), bool)
        mat = np.full(len(who), -1, np.int64)
        st = np.flatnonzero((mov < 0) & ~vol)
        p[st], n[st], front[st] = R.hit_record(S, oo[st], dd[st], t_hit[st], idx[st], T)
        mat[st] = S.prims["material"][idx[st]]
        for mi, m in enumerate(S.movers):
            q = np.flatnonzero((mov == mi) & ~vol)
            if len(q):
                n_out = (p[q] - R.mover_centre(m, time[who[q]], T)) / T(m["radius"])
                f = _dot(dd[q], n_out) < 0
                n[q], front[q], mat[q] = np.where(f[:, None], n_out, -n_out), f, int(m["material"])
        surface = np.flatnonzero(~vol)
        kind = np.full(len(who), NONE, np.int64)
        tex = np.full(len(who), -1, np.int64)
        kind[surface], tex[surface] = S.mats["type"][mat[surface]], S.mats["texture"][mat[surface]]
        listed = np.where(mov < 0, idx, -1)
        checker = np.isin(kind, (R.LAMBERTIAN, R.DIFFUSE_LIGHT, PLASTIC)) & (S.texs["type"][np.maximum(tex, 0)] == R.CHECKER)
        note(C_PARITY, who, np.where(checker, R.checker_odd(p, T), NONE))
        event = np.full(len(who), NONE, np.int64)
        shutter_of = time[who] if len(S.movers) else None

        def textured(k):
            value, texel = R.texture_value(S, tex[k], p[k], T, oo[k], dd[k], t_hit[k], idx[k], mov[k],
                                           None if shutter_of is None else shutter_of[k], perturb)
            note(C_IMAGE_TEXEL, who[k], texel)
            return value
        em = kind == R.DIFFUSE_LIGHT
        if em.any():
            m = who[em]
            Le = textured(em)
            wgt = np.ones(em.sum(), T)
            how = np.full(em.sum(), R.HIT_UNSAMPLED, np.int64)
            for li in {S.light_of_prim.get(int(i), -1) for i in np.unique(listed[em])} - {-1}:
                sel = listed[em] == S.lights[li]["prim"]
                pl = R.light_pdf_of_hit(S, li, oo[em][sel], dd[em][sel], t_hit[em][sel], n[em][sel], T)
                wgt[sel] = R._mis_bsdf(mis[m][sel], pl, perturb)
                inside = R.inside_sphere_light(S, li, oo[em][sel], T) if S.lights[li]["shape"] == R.SPHERE else np.zeros(sel.sum(), bool)
                how[sel] = np.where(mis[m][sel] < 0, R.HIT_UNSAMPLED, np.where(inside, R.HIT_FROM_INSIDE, R.HIT_MIS))
            note(C_HIT_WEIGHT, m, how)
            rgb[m] += beta[m] * Le * wgt[:, None]
            alive[m] = False
            event[em] = R.EV_EMIT
        new_d = np.zeros_like(dd)
        att = np.ones_like(dd)
        scattered = ~em
        pdf_b = np.full(len(who), -1, T)
        refl_dir = np.zeros_like(dd)
        fuzz = np.zeros(len(who), T)
        takes_light = np.zeros(len(who), bool)
        if vol.any():
            if len(S.lights):
                raise NotImplementedError("a light sample at a medium vertex: DESIGN defines none")
            k = np.flatnonzero(vol)
            new_d[k] = _unit(D.reject(who[k], 3, T))
            att[k] = S.media["albedo"][med[k]].astype(T)
            event[k] = R.EV_MEDIUM
        lam = kind == R.LAMBERTIAN
        if lam.any():
            sph = D.reject(who[lam], 3, T)
            nd = n[lam] + _unit(sph)
            tiny = (np.abs(nd) < 1e-8).all(axis=1)
            nd[tiny] = n[lam][tiny]
            new_d[lam], att[lam] = nd, textured(lam)
            event[lam] = R.EV_LAMBERT
            takes_light[lam] = True
            pdf_b[lam] = np.maximum(0, _dot(_unit(nd), n[lam])) / pi
        met = kind == R.METAL
        if met.any():
            ud = _unit(dd[met])
            r = ud - 2 * _dot(ud, n[met])[:, None] * n[met]
            fz = S.mats["fuzz"][mat[met]].astype(T)
            nd = r + fz[:, None] * D.reject(who[met], 3, T)
            up = _dot(nd, n[met]) > 0
            new_d[met], att[met] = nd, S.mats["albedo"][mat[met]].astype(T)
            scattered[met] = up
            event[met] = np.where(up, R.EV_METAL, R.EV_METAL_ABSORBED)
            refl_dir[met], fuzz[met] = r, fz
            takes_light[met] = S.mats["fuzz"][mat[met]] >= np.float32(R.METAL_MIN_FUZZ)
            for f in np.unique(fz[takes_light[met]]):
                sel = np.flatnonzero(met)[(fz == f) & up]
                pdf_b[sel] = R.metal_pdf(_unit(new_d[sel]), refl_dir[sel], f, T)
        die = kind == R.DIELECTRIC
        if die.any():
            ir = S.mats["ir"][mat[die]].astype(T)
            ratio = np.where(front[die], 1 / ir, ir)
            ud, nn = _unit(dd[die]), n[die]
            cos_t = np.minimum(-_dot(ud, nn), 1)
            sin_t = np.sqrt(np.maximum(0, 1 - cos_t * cos_t))
            reflect = ratio * sin_t > 1
            can = np.flatnonzero(~reflect)
            if len(can):
                r0 = ((1 - ratio[can]) / (1 + ratio[can])) ** 2
                sch = r0 + (1 - r0) * (1 - cos_t[can]) ** 5
                reflect[can] = sch > D.next(who[die][can])
            perp = ratio[:, None] * (ud + cos_t[:, None] * nn)
            refracted = perp - np.sqrt(np.abs(1 - _dot(perp, perp)))[:, None] * nn
            new_d[die] = np.where(reflect[:, None], ud - 2 * _dot(ud, nn)[:, None] * nn, refracted)
            event[die] = np.where(reflect, R.EV_REFLECT, R.EV_REFRACT)
        # ---- the glossy materials: their draws where dielectric takes its Fresnel draw; none where wo.z <= 0
        glo = np.isin(kind, (ROUGH_METAL, PLASTIC))
        g_alpha, g_f0, g_rho = np.zeros(len(who), T), np.zeros((len(who), 3), T), np.zeros((len(who), 3), T)
        g_plastic, g_ud = np.zeros(len(who), bool), np.zeros_like(dd)
        if glo.any():
            k = np.flatnonzero(glo)
            rec = S.mats[mat[k]]
            g_plastic[k] = rec["type"] == PLASTIC
            g_alpha[k] = alpha_of(rec["fuzz"]).astype(T)
            g_f0[k] = np.where(g_plastic[k][:, None], r0_of(rec["ir"]).astype(T)[:, None], rec["albedo"].astype(T))
            kp = k[g_plastic[k]]
            if len(kp):
                g_rho[kp] = textured(kp)
            g_ud[k] = _unit(dd[k])
            wo_z = -_dot(g_ud[k], n[k])
            dr = k[wo_z > 0]  # the vertices that draw
            ul, u1, u2 = np.zeros(len(who), T), np.zeros(len(who), T), np.zeros(len(who), T)
            pd = dr[g_plastic[dr]]
            if "lobe_draw_last" not in perturb:
                ul[pd] = D.next(who[pd])
            u1[dr] = D.next(who[dr])
            u2[dr] = D.next(who[dr])
            if "lobe_draw_last" in perturb:
                ul[pd] = D.next(who[pd])
            wi, at, pdf, below, absorbed_wi, lobe = glossy_sample(n[k], g_ud[k], g_alpha[k], g_plastic[k], g_f0[k], g_rho[k], ul[k], u1[k],
                                                                  u2[k], T, perturb)
            new_d[k], att[k] = wi, at
            scattered[k] = ~below & ~absorbed_wi
            event[k] = np.where(below, EV_BELOW, np.where(g_plastic[k], np.where(lobe, np.where(absorbed_wi, EV_COAT_ABSORBED, EV_COAT), EV_BODY),
                                                         np.where(absorbed_wi, EV_ROUGH_ABSORBED, EV_ROUGH)))
            takes_light[k] = (rec["fuzz"] >= np.float32(GLOSSY_MIN_ROUGHNESS)) & ~below
            pdf_b[k] = np.where(scattered[k], pdf, -1)
        if probe is not None and len(sig) == 2:
            probe["glossy"], probe["albedo"], probe["normal"] = np.zeros(N, bool), np.zeros((N, 3), T), np.zeros((N, 3), T)
            probe["glossy"][who] = glo
            probe["albedo"][who] = np.where(g_plastic[:, None], g_rho, g_f0)
            probe["normal"][who] = n
        note(C_EVENT, who, event)
        if not S.nee or len(S.lights) == 0:
            takes_light[:] = False
        go = ~em & scattered
        before = beta[who].copy()                      # the throughput in front of the vertex (a glossy vertex's light sample)
        carried = beta[who] * att
        depth[who[go]] -= 1
        go_on = go & (depth[who] > 0)
        absorbed = ~em & ~scattered
        draws_rr = go_on | (absorbed & takes_light & (depth[who] > 1))
        survived = draws_rr.copy()
        if rr > 0 and draws_rr.any():
            k = np.flatnonzero(draws_rr)
            lost = D.next(who[k]) > rr
            note(C_ROULETTE, who[k], lost)
            survived[k] = ~lost
            carried[k] = carried[k] / rr
            before[k] = before[k] / rr
        alive[who] = go_on & survived
        beta[who] = carried
        o[who], d[who] = p, new_d
        mis[who] = np.where(takes_light, pdf_b, -1)
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
        for li in np.unique(pick):
            sel = pick == li
            ld[sel], pl[sel], Le[sel], texel[sel] = R.sample_light(S, li, p[ls][sel], u1[sel], u2[sel], T, perturb)
            if S.lights[li]["shape"] == R.SPHERE:
                inside[sel] = R.inside_sphere_light(S, li, p[ls][sel], T)
        note(C_TEXEL, m, texel)
        d2 = _dot(ld, ld)
        gl = glo[ls]
        with np.errstate(all="ignore"):
            w = ld / np.sqrt(d2)[:, None]
            wn = _dot(w, n[ls])
            pb = np.where(fuzz[ls] > 0, 0, wn / pi)
            for f in np.unique(fuzz[ls][fuzz[ls] > 0]):
                sel = fuzz[ls] == f
                pb[sel] = R.metal_pdf(w[sel], refl_dir[ls][sel], f, T)
            pb = np.where(wn > 0, pb, 0)
            fcos = None
            if gl.any():
                # f cos is not albedo x pdf_b here: both are evaluated for the light's direction
                q = ls[gl]
                fc, pg = glossy_eval(n[q], g_ud[q], g_alpha[q], g_plastic[q], g_f0[q], g_rho[q], w[gl], T)
                if "nee_albedo_pdf" in perturb:
                    fc = np.where(g_plastic[q][:, None], g_rho[q], g_f0[q]) * pg[:, None]
                pb[gl] = pg
                fcos = np.zeros((len(ls), 3), T)
                fcos[gl] = fc
            weight = pb * pl / (pl + pb if "mis_unsquared" in perturb else pl * pl + pb * pb)
            if gl.any():  # the glossy vertices' scalar part: p_l / (p_l^2 + pdf_b^2); f cos joins per channel below
                weight = np.where(gl, pl / (pl + pb if "mis_unsquared" in perturb else pl * pl + pb * pb), weight)
        usable = (pl > 0) & (pb > 0) & (d2 > 0) & np.isfinite(weight) & (weight > 0)
        verdict = np.where(inside, R.SHADOW_INSIDE, R.SHADOW_NONE)
        if usable.any():
            if len(S.media) or len(S.movers):
                raise NotImplementedError("a shadow ray through a medium or past a mover: DESIGN defines none")
            k = np.flatnonzero(usable)
            is_env = S.lights["shape"][pick[k]] == R.ENVIRONMENT
            far = np.where(is_env, T(np.inf), T(R.SHADOW_T_MAX))
            _, blocker = R.closest_hit(S, p[ls][k], ld[k], far, T)
            verdict[k] = np.where(blocker >= 0, R.SHADOW_OCCLUDED, R.SHADOW_CLEAR)
            note(C_BLOCKER, m[k], np.where(blocker >= 0, blocker, NONE))
            clear = k[blocker < 0]
            through = carried[ls][clear]
            if fcos is not None:
                through = np.where(gl[clear][:, None], before[ls][clear] * fcos[clear], through)
            if "no_rr_light" in perturb and rr > 0:
                through = through * rr
            rgb[m[clear]] += through * Le[clear] * weight[clear][:, None]
        note(C_SHADOW, m, verdict)

    sig[0][:, 0] = D.at
    return rgb, np.concatenate(sig, axis=1), D.at.copy()


def reference(S, words, shutter=None):
    """ref64.reference through this trace: the fp64 radiance, the samples whose branches do not depend on the precision, the draws
    consumed, ref64's tally and glossy_tally of the fp64 run"""
    rgb, sig64, draws = trace(S, words, shutter=shutter)
    _, sig32, _ = trace(S, words, dtype=np.float32, shutter=shutter)
    t = R.tally(sig64, S)
    t.update(glossy_tally(sig64, S))
    return rgb, R.same_signature(sig64, sig32), draws, t


def glossy_tally(sig, S):
    """how often the vertices a glossy case is there for occurred: by event, with a light sample, by material roughness, and in
    sequence with emitters, media and the environment"""
    v = sig[:, SAMPLE_COLUMNS:].reshape(len(sig), -1, VERTEX_COLUMNS)
    event, light, how, prim, mover, shadow, miss_texel = (v[:, :, c] for c in (C_EVENT, C_LIGHT, C_HIT_WEIGHT, C_PRIM, C_MOVER, C_SHADOW,
                                                                                 C_MISS_TEXEL))
    glossy = np.isin(event, GLOSSY_EVENTS)
    sampled = glossy & (light != NONE)
    later = lambda x: np.flip(np.cumsum(np.flip(x, axis=1), axis=1), axis=1) - x > 0
    med = event == R.EV_MEDIUM
    # the roughness of the material under each static glossy vertex (movers: by their own material, counted separately)
    rough = np.full(event.shape, np.nan)
    if len(S.prims):
        r_of_prim = S.mats["fuzz"][S.prims["material"]].astype(np.float64)
        on_static = glossy & (prim >= 0) & ~(mover >= 0)
        rough[on_static] = r_of_prim[prim[on_static]]
    with np.errstate(invalid="ignore"):
        smooth = glossy & (rough < GLOSSY_MIN_ROUGHNESS)
    nxt_emit_full = np.zeros_like(glossy)
    nxt_emit_full[:, :-1] = (event[:, 1:] == R.EV_EMIT) & (how[:, 1:] == R.HIT_UNSAMPLED)
    env_pick = np.zeros_like(glossy)
    if len(S.lights) and S.lights[-1]["shape"] == R.ENVIRONMENT:
        env_pick = sampled & (light == len(S.lights) - 1)
    # a BSDF ray from a glossy vertex that took a light sample and escapes: its miss is the next block's C_MISS_TEXEL
    escaped = np.zeros_like(glossy)
    escaped[:, :-1] = sampled[:, :-1] & (miss_texel[:, 1:] != NONE)
    return dict(rough_vertices=int((event == EV_ROUGH).sum()), coat_vertices=int((event == EV_COAT).sum()),
                body_vertices=int((event == EV_BODY).sum()), below_vertices=int((event == EV_BELOW).sum()),
                absorbed_wi_vertices=int(np.isin(event, (EV_ROUGH_ABSORBED, EV_COAT_ABSORBED)).sum()),
                glossy_light_samples=int(sampled.sum()),
                glossy_light_samples_clear=int((sampled & (shadow == R.SHADOW_CLEAR)).sum()),
                absorbed_wi_light_samples=int((np.isin(event, (EV_ROUGH_ABSORBED, EV_COAT_ABSORBED)) & (light != NONE)).sum()),
                below_light_samples=int(((event == EV_BELOW) & (light != NONE)).sum()),
                smooth_glossy_vertices=int(smooth.sum()), smooth_glossy_light_samples=int((smooth & (light != NONE)).sum()),
                smooth_glossy_full_weight_hits=int((smooth & nxt_emit_full).sum()),
                roughnesses=sorted(float(np.float32(x)) for x in np.unique(rough[~np.isnan(rough)])),
                glossy_env_picks=int(env_pick.sum()), glossy_escapes_after_light_sample=int(escaped.sum()),
                medium_then_glossy=int((med & later(glossy)).any(axis=1).sum()),
                glossy_then_medium=int((glossy & later(med)).any(axis=1).sum()),
                glossy_mover_vertices=int((glossy & (mover >= 0)).sum()),
                glossy_static_vertices=int((glossy & ~(mover >= 0)).sum()),
                roulette_losses=int((v[:, :, C_ROULETTE] == 1).sum()))
