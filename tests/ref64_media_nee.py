"""An independent fp64 statement of light sampling in participating media: a path tracer for scenes of lambertian,
metal, dielectric and diffuse_light surfaces on any primitive, homogeneous media with a Henyey-Greenstein asymmetry each, and the
sampled emitters of 7a without an environment (area lights and point / spot / distant lights) -- in NumPy, vectorised over a
batch of samples, at a floating type of the caller's choice, in the manner of ref64.py.

Test infrastructure only.  ref64.trace() raises NotImplementedError where a light sample meets a medium and stays so; this module
states what DESIGN 7z defines there.  It takes from ref64, unchanged, what is not the new step: RefScene, the draws, closest_hit
(through opaque_hit), hit_record, texture_value, medium_interval, sample_light, the light strategy's density of a hit and the
power heuristic of a BSDF hit; from ref64_phase the fp64 Henyey-Greenstein direction and density.  Its premises (tests/
test_media_nee.py): with every sigma = 0 its radiance is ref64.reference()'s with light sampling, with no lights it is
ref64.reference()'s of the media scene, both within 1e-12.

The estimator (7a's vocabulary and order of draws, plus):
  * a medium vertex takes a light sample where a surface vertex does -- after depth-- and a survived roulette draw, the three light
    draws behind the roulette draw.  pdf_b of the direction w_l to the light point is 1 / (4 pi) for the stored g = 0 and the phase
    function's density at w . w_l otherwise (w: the unit direction of travel); f = albedo x pdf_b, no cosine: the contribution is
    beta x albedo x Le x pdf_b p_l / (p_l^2 + pdf_b^2), a delta light's beta x albedo x Le x pdf_b / p_l;
  * its continuation carries pdf_b of the direction it drew, and an emitter it reaches is weighed pdf_b^2 / (pdf_b^2 + p_l^2);
  * a shadow ray takes no draw: every medium, in list order, adds sigma (b - a) |d| of its stay [a, b] over the shadow ray's own
    range [0.001, 0.999] to tau; an unoccluded sample is multiplied by exp(-tau); any surface occludes; T enters no weight.

Deliberate mistakes (`perturb`), for the tests that show the comparisons can fail:
    "no_transmittance"       the shadow ray ignores the media (T = 1)
    "isotropic_pdf"          pdf_b = 1 / (4 pi) at a vertex with g != 0, for the light's direction and the continuation's
    "shadow_flight_draw"     a free-flight draw taken for every non-empty stay of a shadow ray (and thrown away)
    "medium_full_weight"     a medium vertex's continuation arrives at an emitter at full weight (as if it took no light sample)
"""
import numpy as np

import ref64 as R
import ref64_phase as PH
from ref64 import RefScene, uniforms, judge, row  # noqa: F401 (re-exported to the tests)
from ref64_base import _dot, _unit

PERTURBATIONS = ("no_transmittance", "isotropic_pdf", "shadow_flight_draw", "medium_full_weight")
NONE = R.NONE
EV_MISS, EV_EMIT, EV_LAMBERT, EV_METAL, EV_METAL_ABSORBED, EV_REFLECT, EV_REFRACT, EV_MEDIUM_ISO, EV_MEDIUM_HG = range(9)
# per vertex: the surface winner, the media that took a free-flight draw, the medium whose event won, what happened, the checker
# parity, the roulette, the light picked and whether through the alias, the shadow ray's verdict, what stopped it, the media it
# stayed in, how an emitter hit was weighted
(C_PRIM, C_DREW, C_MEDIUM, C_EVENT, C_PARITY, C_ROULETTE, C_LIGHT, C_ALIAS, C_SHADOW, C_BLOCKER, C_STAYS, C_HIT_WEIGHT) = range(12)
VERTEX_COLUMNS = 12
SAMPLE_COLUMNS = 2
SHADOW_CLEAR, SHADOW_OCCLUDED, SHADOW_NONE, SHADOW_INSIDE = R.SHADOW_CLEAR, R.SHADOW_OCCLUDED, R.SHADOW_NONE, R.SHADOW_INSIDE
HIT_MIS, HIT_UNSAMPLED, HIT_FROM_INSIDE = R.HIT_MIS, R.HIT_UNSAMPLED, R.HIT_FROM_INSIDE
ISOTROPIC = 1.0 / (4.0 * np.pi)


def check_scene_class(S):
    assert np.isin(S.mats["type"], (R.LAMBERTIAN, R.METAL, R.DIELECTRIC, R.DIFFUSE_LIGHT)).all(), "lambertian / metal / dielectric / diffuse_light only"
    assert S.env is None and len(S.movers) == 0, "no environment, no movers"
    assert not S.bumps and not S.normal_maps and not S.alpha_masks and not S.noise
    assert not len(S.lights) or (S.lights["shape"] != R.ENVIRONMENT).all()


def optical_depth(S, o, d, t_max, T):
    """(tau, the set of media with a non-empty stay) of the segments o + t d, t in [0.001, t_max]: sigma (b - a) |d| per stay"""
    tau = np.zeros(len(o), T)
    stays = np.zeros(len(o), np.int64)
    length = np.sqrt(_dot(d, d))
    far = np.full(len(o), t_max, T)
    for mi, m in enumerate(S.media):
        sigma = T(m["density"])
        if not sigma > 0:
            continue
        a, b, ok = R.medium_interval(m, o, d, far, T)
        tau = np.where(ok, tau + sigma * (b - a) * length, tau)
        stays |= np.where(ok, 1 << mi, 0)
    return tau, stays


def phase_density(g, c, T):
    """the phase function's density per steradian at cos t = c, per vertex (g: fp64 array of the stored asymmetries)"""
    return np.where(g == 0, T(ISOTROPIC), PH.hg_density(g, c)).astype(T)


def trace(S, g, words, dtype=np.float64, perturb=(), log=None):
    """One sample per row of `words`, pixels 0, 1, ... modulo the frame; g: the media's stored asymmetries in list order.
    Returns (rgb [N][3], signature [N][*], draws consumed [N]).  log: a dict whose "ended_by_depth" counts the paths that
    scattered with no depth left (the signature has no column for it)."""
    check_scene_class(S)
    assert not set(perturb) - set(PERTURBATIONS), perturb
    T = dtype
    g = np.asarray(g, np.float32).astype(np.float64)
    assert len(g) == len(S.media)
    N = len(words)
    D = R._Draws(words, T)
    W, H = S.width, S.height
    pix = np.arange(N) % (W * H)
    everyone = np.arange(N)
    rr, pi = T(S.rr), T(np.pi)
    cam = {k: v.astype(T) for k, v in S.cam.items()}
    sig = [np.full((N, SAMPLE_COLUMNS), NONE, np.int64)]
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
        sig[0][:, 1] = lost
        alive &= ~lost
        beta = beta / rr
    sampling = bool(S.nee) and len(S.lights) > 0

    while alive.any():
        who = np.flatnonzero(alive)
        oo, dd = o[who], d[who]
        t_hit, idx = R.opaque_hit(S, oo, dd, np.inf, T)
        row_ = np.full((N, VERTEX_COLUMNS), NONE, np.int64)
        sig.append(row_)
        row_[who, C_PRIM] = idx
        # ---- the media walk of a path query (7f): list order, one free-flight draw per non-empty stay
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
                tt = a[k] + (-np.log(1 - D.next(who[k])) / sigma) / length[k]
                drew[k] |= 1 << mi
                win = (tt < b[k]) & (tt < t_m[k])
                t_m[k[win]], med[k[win]] = tt[win], mi
            row_[who, C_DREW], row_[who, C_MEDIUM] = drew, med
        vol = med >= 0
        t_hit = np.where(vol, t_m, t_hit)
        miss = (idx < 0) & ~vol
        if miss.any():
            m = who[miss]
            ud = _unit(dd[miss])
            if S.flags & 1:
                tt = 0.5 * (ud[:, 1] + 1)
                bg = (1 - tt)[:, None] * np.ones(3, T) + tt[:, None] * np.array([0.5, 0.7, 1.0], T)
            else:
                bg = np.broadcast_to(S.background.astype(T), (len(m), 3))
            rgb[m] += beta[m] * bg
            alive[m] = False
            row_[m, C_EVENT] = EV_MISS
        if miss.all():
            continue
        who, oo, dd, t_hit, idx, med, vol = (x[~miss] for x in (who, oo, dd, t_hit, idx, med, vol))
        p = oo + t_hit[:, None] * dd
        n = np.zeros_like(dd)
        front = np.zeros(len(who), bool)
        mat = np.full(len(who), -1, np.int64)
        st = np.flatnonzero(~vol)
        p[st], n[st], front[st] = R.hit_record(S, oo[st], dd[st], t_hit[st], idx[st], T)
        mat[st] = S.prims["material"][idx[st]]
        kind = np.full(len(who), NONE, np.int64)
        tex = np.full(len(who), -1, np.int64)
        kind[st], tex[st] = S.mats["type"][mat[st]], S.mats["texture"][mat[st]]
        checker = np.isin(kind, (R.LAMBERTIAN, R.DIFFUSE_LIGHT)) & (S.texs["type"][np.maximum(tex, 0)] == R.CHECKER)
        row_[who, C_PARITY] = np.where(checker, R.checker_odd(p, T), NONE)
        event = np.full(len(who), NONE, np.int64)
        no_mover = np.full(len(who), -1, np.int64)

        def textured(k):
            return R.texture_value(S, tex[k], p[k], T, oo[k], dd[k], t_hit[k], idx[k], no_mover[k], None)[0]
        # ---- an emitter ends the path
        em = kind == R.DIFFUSE_LIGHT
        if em.any():
            m = who[em]
            Le = textured(em)
            wgt = np.ones(em.sum(), T)
            how = np.full(em.sum(), HIT_UNSAMPLED, np.int64)
            if sampling:
                for li in {S.light_of_prim.get(int(i), -1) for i in np.unique(idx[em])} - {-1}:
                    sel = idx[em] == S.lights[li]["prim"]
                    pl = R.light_pdf_of_hit(S, li, oo[em][sel], dd[em][sel], t_hit[em][sel], n[em][sel], T)
                    wgt[sel] = R._mis_bsdf(mis[m][sel], pl)
                    inside = R.inside_sphere_light(S, li, oo[em][sel], T) if S.lights[li]["shape"] == R.SPHERE else np.zeros(sel.sum(), bool)
                    how[sel] = np.where(mis[m][sel] < 0, HIT_UNSAMPLED, np.where(inside, HIT_FROM_INSIDE, HIT_MIS))
            row_[m, C_HIT_WEIGHT] = how
            rgb[m] += beta[m] * Le * wgt[:, None]
            alive[m] = False
            event[em] = EV_EMIT
        # ---- the scatter step
        new_d = np.zeros_like(dd)
        att = np.ones_like(dd)
        scattered = ~em
        pdf_b = np.full(len(who), -1, T)
        refl_dir = np.zeros_like(dd)
        fuzz = np.zeros(len(who), T)
        takes_light = np.zeros(len(who), bool)
        travel = np.zeros_like(dd)          # a medium vertex: the unit direction of travel that arrived
        g_v = np.zeros(len(who), np.float64)  # ... and its medium's asymmetry as the light sample and the continuation see it
        if vol.any():
            k = np.flatnonzero(vol)
            travel[k] = _unit(dd[k])
            g_true = g[med[k]]
            iso, hg = k[g_true == 0], k[g_true != 0]
            if len(iso):
                new_d[iso] = _unit(D.reject(who[iso], 3, T))
                event[iso] = EV_MEDIUM_ISO
            if len(hg):
                u1, u2 = D.next(who[hg]), D.next(who[hg])
                for mi in np.unique(med[hg]):
                    sel = med[hg] == mi
                    new_d[hg[sel]] = PH.hg_direction(g[mi], travel[hg[sel]], u1[sel], u2[sel], T)
                event[hg] = EV_MEDIUM_HG
            att[k] = S.media["albedo"][med[k]].astype(T)
            g_v[k] = 0.0 if "isotropic_pdf" in perturb else g_true
            takes_light[k] = True
            pdf_b[k] = phase_density(g_v[k], _dot(_unit(new_d[k]), travel[k]), T)
        lam = kind == R.LAMBERTIAN
        if lam.any():
            nd = n[lam] + _unit(D.reject(who[lam], 3, T))
            tiny = (np.abs(nd) < 1e-8).all(axis=1)
            nd[tiny] = n[lam][tiny]
            new_d[lam], att[lam] = nd, textured(lam)
            event[lam] = EV_LAMBERT
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
            event[met] = np.where(up, EV_METAL, EV_METAL_ABSORBED)
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
                schlick = r0 + (1 - r0) * (1 - cos_t[can]) ** 5
                reflect[can] = schlick > D.next(who[die][can])
            perp = ratio[:, None] * (ud + cos_t[:, None] * nn)
            refracted = perp - np.sqrt(np.abs(1 - _dot(perp, perp)))[:, None] * nn
            new_d[die] = np.where(reflect[:, None], ud - 2 * _dot(ud, nn)[:, None] * nn, refracted)
            event[die] = np.where(reflect, EV_REFLECT, EV_REFRACT)
        row_[who, C_EVENT] = event
        if not sampling:
            takes_light[:] = False
        # ---- what goes on: depth, then the roulette of the next query
        go = ~em & scattered
        carried = beta[who] * att
        depth[who[go]] -= 1
        go_on = go & (depth[who] > 0)
        if log is not None:
            log["ended_by_depth"] = log.get("ended_by_depth", 0) + int((go & ~go_on).sum())
        absorbed = ~em & ~scattered
        draws_rr = go_on | (absorbed & takes_light & (depth[who] > 1))
        survived = draws_rr.copy()
        if rr > 0 and draws_rr.any():
            k = np.flatnonzero(draws_rr)
            lost = D.next(who[k]) > rr
            row_[who[k], C_ROULETTE] = lost
            survived[k] = ~lost
            carried[k] = carried[k] / rr
        alive[who] = go_on & survived
        beta[who] = carried
        o[who], d[who] = p, new_d
        mis[who] = np.where(takes_light, pdf_b, -1)
        if "medium_full_weight" in perturb:
            mis[who[vol]] = -1
        # ---- the light sample
        ls = np.flatnonzero(takes_light & survived & draws_rr)
        if len(ls) == 0:
            continue
        m = who[ls]
        u0, u1, u2 = D.next(m), D.next(m), D.next(m)
        nl = len(S.lights)
        xs = u0 * nl
        pick = np.minimum(xs.astype(np.int64), nl - 1)
        aliased = xs - pick >= S.thr.astype(T)[pick]
        pick = np.where(aliased, S.alias[pick], pick)
        row_[m, C_LIGHT], row_[m, C_ALIAS] = pick, aliased
        ld = np.zeros((len(m), 3), T)
        pl = np.zeros(len(m), T)
        Le = np.zeros((len(m), 3), T)
        inside = np.zeros(len(m), bool)
        delta = np.zeros(len(m), bool)
        for li in np.unique(pick):
            sel = pick == li
            ld[sel], pl[sel], Le[sel], _, delta[sel] = R.sample_light(S, li, p[ls][sel], u1[sel], u2[sel], T)
            if S.lights[li]["shape"] == R.SPHERE:
                inside[sel] = R.inside_sphere_light(S, li, p[ls][sel], T)
        d2 = _dot(ld, ld)
        with np.errstate(all="ignore"):
            w = ld / np.sqrt(d2)[:, None]
            wn = _dot(w, n[ls])
            pb = np.where(fuzz[ls] > 0, 0, wn / pi)
            for f in np.unique(fuzz[ls][fuzz[ls] > 0]):
                sel = fuzz[ls] == f
                pb[sel] = R.metal_pdf(w[sel], refl_dir[ls][sel], f, T)
            pb = np.where(wn > 0, pb, 0)
            # a medium vertex: the phase function's density of the light's direction, no cosine and no hemisphere
            pb = np.where(vol[ls], phase_density(g_v[ls], _dot(w, travel[ls]), T), pb)
            weight = pb * pl / (pl * pl + pb * pb)
            weight = np.where(delta, pb / pl, weight)
        usable = (pl > 0) & (pb > 0) & (d2 > 0) & np.isfinite(weight) & (weight > 0)
        verdict = np.where(inside, SHADOW_INSIDE, SHADOW_NONE)
        if usable.any():
            k = np.flatnonzero(usable)
            far = np.full(len(k), R.SHADOW_T_MAX, T)
            _, blocker = R.opaque_hit(S, p[ls][k], ld[k], far, T)
            tau, stays = optical_depth(S, p[ls][k], ld[k], T(R.SHADOW_T_MAX), T)
            if "shadow_flight_draw" in perturb:
                for mi in range(len(S.media)):
                    D.next(m[k][(stays >> mi) & 1 == 1])
            verdict[k] = np.where(blocker >= 0, SHADOW_OCCLUDED, SHADOW_CLEAR)
            row_[m[k], C_BLOCKER] = np.where(blocker >= 0, blocker, NONE)
            row_[m[k], C_STAYS] = stays
            c = blocker < 0
            clear = k[c]
            Tr = np.ones(len(clear), T) if "no_transmittance" in perturb else np.exp(-tau[c])
            rgb[m[clear]] += carried[ls][clear] * Le[clear] * (weight[clear] * Tr)[:, None]
        row_[m, C_SHADOW] = verdict

    sig[0][:, 0] = D.at
    return rgb, np.concatenate(sig, axis=1), D.at.copy()


def tally(sig):
    """what the premises of the GPU comparison count, from a signature"""
    v = sig[:, SAMPLE_COLUMNS:].reshape(len(sig), -1, VERTEX_COLUMNS)
    ev, light, shadow, stays, how = (v[:, :, c] for c in (C_EVENT, C_LIGHT, C_SHADOW, C_STAYS, C_HIT_WEIGHT))
    med = np.isin(ev, (EV_MEDIUM_ISO, EV_MEDIUM_HG))
    took = light != NONE
    through = (stays != NONE) & (stays > 0)
    nxt = lambda x: np.concatenate([x[:, 1:], np.zeros((len(x), 1), bool)], axis=1)
    emit = ev == EV_EMIT
    return dict(medium_events=int(med.sum()), anisotropic_events=int((ev == EV_MEDIUM_HG).sum()),
                medium_light_samples=int((med & took).sum()), surface_light_samples=int((~med & took).sum()),
                medium_samples_clear=int((med & (shadow == SHADOW_CLEAR)).sum()),
                clear_through_media=int(((shadow == SHADOW_CLEAR) & through).sum()),
                occluded_through_media=int(((shadow == SHADOW_OCCLUDED) & through).sum()),
                medium_then_emitter=int((med & nxt(emit)).sum()),
                medium_then_emitter_mis=int((med & took & nxt(emit & (how == HIT_MIS))).sum()))


def reference(S, g, words):
    """the fp64 radiance, which samples took the same branches at fp32 (the stable ones), the draws consumed and the fp64 run's tally"""
    rgb, sig64, draws = trace(S, g, words)
    _, sig32, _ = trace(S, g, words, dtype=np.float32)
    w = max(sig64.shape[1], sig32.shape[1])
    pad = lambda a: np.pad(a, ((0, 0), (0, w - a.shape[1])), constant_values=NONE)
    return rgb, (pad(sig64) == pad(sig32)).all(axis=1), draws, tally(sig64)
