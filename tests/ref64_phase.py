"""An independent fp64 statement of anisotropic media: a small path tracer for the scene class of phase_scenes.py
-- spheres with solid lambertian and diffuse_light materials, a sky-gradient or constant background, Russian roulette, homogeneous
media with a Henyey-Greenstein asymmetry g each, a pinhole camera -- in NumPy, vectorised over a batch of samples, at a floating
type of the caller's choice, in the manner of ref64.py.

Test infrastructure only.  ref64.trace() fixes the direction of a medium vertex inside its loop, so the phase function cannot
join it as a model file; this module is a tracer of its own until it is folded into ref64.trace().  It takes from ref64,
unchanged, what is not the new step: RefScene, uniforms, _Draws, closest_hit, medium_interval, judge, row.  With every g = 0 its
radiance is ref64.reference()'s on the same words (tests/test_phase.py holds it to 1e-12), which pins this statement to the
established one everywhere but the new step.

The new step, from the definitions (include/rtmi.h): a vertex in a medium with g != 0 takes no attempt of the rejection
loop but two uniforms u1, u2.  The polar angle t about the unit direction of travel w has the distribution function
    F(cos t) = (1 - g^2) / (2 g) (1 / sqrt(1 + g^2 - 2 g cos t) - 1 / (1 + g)),
inverted in closed form at u1; the azimuth is 2 pi u2, measured in the frame of Duff et al. 2017 about w (the frame the product's
documents name: the azimuth of a sample means nothing without it).  Angles through libm's arccos / sin / cos, no fused operation.

trace() returns (rgb [N][3], signature [N][*], draws [N]); the signature holds, per vertex, the sphere hit, the set of media that
took a free-flight draw, the medium whose event won, whether the vertex was anisotropic, what happened and the roulette's outcome.

Deliberate mistakes (`perturb`), for the tests that show the comparison can fail:
    "phase_isotropic"       g ignored: every medium vertex runs the rejection loop
    "phase_backward"        g negated
    "phase_swapped_draws"   u2 drives the polar angle, u1 the azimuth
"""
import numpy as np

from ref64 import RefScene, uniforms, _Draws, closest_hit, medium_interval, judge, row  # noqa: F401 (re-exported to the tests)
from ref64_base import SPHERE, _dot, _unit

PERTURBATIONS = ("phase_isotropic", "phase_backward", "phase_swapped_draws")
LAMBERTIAN, DIFFUSE_LIGHT = 0, 3
SOLID = 0
NONE = -9
EV_MISS, EV_EMIT, EV_LAMBERT, EV_MEDIUM_ISO, EV_MEDIUM_HG = range(5)
C_PRIM, C_DREW, C_MEDIUM, C_ANISO, C_EVENT, C_ROULETTE = range(6)
VERTEX_COLUMNS = 6
SAMPLE_COLUMNS = 2


def stored_g(sc):
    """the asymmetries a product scene holds, in list order"""
    return np.array([sc.medium_phase(i) for i in range(len(sc.media()))], np.float32)


def check_scene_class(S):
    assert (S.prims["type"] == SPHERE).all(), "spheres only"
    assert np.isin(S.mats["type"], (LAMBERTIAN, DIFFUSE_LIGHT)).all() and (S.texs["type"] == SOLID).all(), "solid lambertian / diffuse_light only"
    assert not S.flags & 2 and S.env is None and len(S.lights) == 0 and len(S.movers) == 0, "pinhole camera, no environment, no light sampling, no movers"
    assert not S.bumps and not S.normal_maps and not S.alpha_masks


def hg_cdf(g, c):
    """F(cos t) of the phase function with asymmetry g != 0 (fp64)"""
    g, c = np.asarray(g, np.float64), np.asarray(c, np.float64)
    return (1 - g * g) / (2 * g) * (1 / np.sqrt(1 + g * g - 2 * g * c) - 1 / (1 + g))


def hg_density(g, c):
    """p(cos t) per steradian (fp64)"""
    g, c = np.asarray(g, np.float64), np.asarray(c, np.float64)
    return (1 - g * g) / (4 * np.pi * (1 + g * g - 2 * g * c) ** 1.5)


def hg_cos(g, u, T=np.float64):
    """cos t with F(cos t) = u: from F, 1 / sqrt(1 + g^2 - 2 g c) = 2 g u / (1 - g^2) + 1 / (1 + g) = (1 - g + 2 g u) / (1 - g^2)"""
    g, u = T(g), np.asarray(u, T)
    root = (1 - g * g) / (1 - g + 2 * g * u)  # sqrt(1 + g^2 - 2 g c)
    return np.clip((1 + g * g - root * root) / (2 * g), -1, 1)


def frame(w):
    """(t1, t2) with (t1, t2, w) orthonormal and right-handed, of Duff et al. 2017, 'Building an Orthonormal Basis, Revisited'"""
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    s = np.copysign(np.ones_like(z), z)
    a = -1 / (s + z)
    b = x * y * a
    return np.stack([1 + s * x * x * a, s * b, -s * x], axis=1), np.stack([b, s + y * y * a, -y], axis=1)


def hg_direction(g, w, u1, u2, T=np.float64):
    """the direction of a vertex with asymmetry g that arrived along the unit vector w"""
    theta = np.arccos(hg_cos(g, u1, T))
    phi = T(2 * np.pi) * u2
    t1, t2 = frame(w)
    return ((np.sin(theta) * np.cos(phi))[:, None] * t1 + (np.sin(theta) * np.sin(phi))[:, None] * t2 + np.cos(theta)[:, None] * w).astype(T)


def trace(S, g, words, dtype=np.float64, perturb=()):
    """One sample per row of `words`, pixels 0, 1, ... modulo the frame; g: the media's asymmetries in list order"""
    check_scene_class(S)
    assert not set(perturb) - set(PERTURBATIONS), perturb
    T = dtype
    g = np.asarray(g, np.float32).astype(np.float64)
    assert len(g) == len(S.media)
    if "phase_isotropic" in perturb:
        g = np.zeros_like(g)
    if "phase_backward" in perturb:
        g = -g
    N = len(words)
    D = _Draws(words, T)
    W, H = S.width, S.height
    pix = np.arange(N) % (W * H)
    everyone = np.arange(N)
    rr = T(S.rr)
    cam = {k: v.astype(T) for k, v in S.cam.items()}
    sig = [np.full((N, SAMPLE_COLUMNS), NONE, np.int64)]
    s = ((pix % W).astype(T) + D.next(everyone)) / T(W - 1)
    t = ((pix // W).astype(T) + D.next(everyone)) / T(H - 1)
    o = np.broadcast_to(cam["origin"], (N, 3)).copy()
    d = cam["lower_left"] + s[:, None] * cam["horizontal"] + t[:, None] * cam["vertical"] - cam["origin"]
    beta = np.ones((N, 3), T)
    rgb = np.zeros((N, 3), T)
    depth = np.full(N, S.max_depth, np.int64)
    alive = depth > 0
    if rr > 0:
        lost = D.next(everyone) > rr
        sig[0][:, 1] = lost
        alive &= ~lost
        beta = beta / rr
    albedo_of_mat = S.texs["c0"][S.mats["texture"]]
    while alive.any():
        who = np.flatnonzero(alive)
        oo, dd = o[who], d[who]
        t_hit, idx = closest_hit(S, oo, dd, np.inf, T)
        row_ = np.full((N, VERTEX_COLUMNS), NONE, np.int64)
        sig.append(row_)
        row_[who, C_PRIM] = idx
        # the media walk: list order, one free-flight draw per non-empty stay in a medium of positive density
        t_m = np.full(len(who), np.inf, T)
        med = np.full(len(who), -1, np.int64)
        drew = np.zeros(len(who), np.int64)
        length = np.sqrt(_dot(dd, dd))
        for mi, m in enumerate(S.media):
            sigma = T(m["density"])
            if not sigma > 0:
                continue
            a, b, ok = medium_interval(m, oo, dd, t_hit, T)
            k = np.flatnonzero(ok)
            if len(k) == 0:
                continue
            tt = a[k] + (-np.log(1 - D.next(who[k])) / sigma) / length[k]
            drew[k] |= 1 << mi
            win = (tt < b[k]) & (tt < t_m[k])
            t_m[k[win]], med[k[win]] = tt[win], mi
        vol = med >= 0
        row_[who, C_DREW], row_[who, C_MEDIUM] = drew, med
        t_hit = np.where(vol, t_m, t_hit)
        miss = (idx < 0) & ~vol
        event = np.full(len(who), NONE, np.int64)
        if miss.any():
            ud = _unit(dd[miss])
            if S.flags & 1:
                tt = 0.5 * (ud[:, 1] + 1)
                bg = (1 - tt)[:, None] * np.ones(3, T) + tt[:, None] * np.array([0.5, 0.7, 1.0], T)
            else:
                bg = np.broadcast_to(S.background.astype(T), (int(miss.sum()), 3))
            rgb[who[miss]] += beta[who[miss]] * bg
            alive[who[miss]] = False
            event[miss] = EV_MISS
        p = oo + np.where(miss, 0, t_hit)[:, None] * dd
        new_d = np.zeros_like(dd)
        att = np.ones_like(dd)
        surf = np.flatnonzero(~miss & ~vol)
        mat = S.prims["material"][idx[surf]]
        emits = S.mats["type"][mat] == DIFFUSE_LIGHT
        em, lam = surf[emits], surf[~emits]
        if len(em):
            rgb[who[em]] += beta[who[em]] * albedo_of_mat[mat[emits]].astype(T)
            alive[who[em]] = False
            event[em] = EV_EMIT
        # the scatter step: medium vertices first, then the lambertian ones (each sample is one or the other: the order is no statement)
        aniso = np.zeros(len(who), bool)
        aniso[vol] = g[med[vol]] != 0
        iso = np.flatnonzero(vol & ~aniso)
        if len(iso):
            new_d[iso] = _unit(D.reject(who[iso], 3, T))
            att[iso] = S.media["albedo"][med[iso]].astype(T)
            event[iso] = EV_MEDIUM_ISO
        hg = np.flatnonzero(aniso)
        if len(hg):
            u1, u2 = D.next(who[hg]), D.next(who[hg])
            if "phase_swapped_draws" in perturb:
                u1, u2 = u2, u1
            w = _unit(dd[hg])
            for mi in np.unique(med[hg]):
                sel = med[hg] == mi
                new_d[hg[sel]] = hg_direction(g[mi], w[sel], u1[sel], u2[sel], T)
            att[hg] = S.media["albedo"][med[hg]].astype(T)
            event[hg] = EV_MEDIUM_HG
        row_[who, C_ANISO] = np.where(vol, aniso, NONE)
        if len(lam):
            f = S.prims["f"][idx[lam]].astype(T)
            n_out = (p[lam] - f[:, :3]) / f[:, 3:4]
            front = _dot(dd[lam], n_out) < 0
            n = np.where(front[:, None], n_out, -n_out)
            nd = n + _unit(D.reject(who[lam], 3, T))
            tiny = (np.abs(nd) < 1e-8).all(axis=1)
            nd[tiny] = n[tiny]
            new_d[lam], att[lam] = nd, albedo_of_mat[mat[~emits]].astype(T)
            event[lam] = EV_LAMBERT
        row_[who, C_EVENT] = event
        go = np.isin(event, (EV_LAMBERT, EV_MEDIUM_ISO, EV_MEDIUM_HG))
        carried = beta[who] * att
        depth[who[go]] -= 1
        go_on = go & (depth[who] > 0)
        survived = go_on.copy()
        if rr > 0 and go_on.any():
            k = np.flatnonzero(go_on)
            lost = D.next(who[k]) > rr
            row_[who[k], C_ROULETTE] = lost
            survived[k] = ~lost
            carried[k] = carried[k] / rr
        alive[who] = survived
        beta[who] = carried
        o[who], d[who] = p, new_d
    sig[0][:, 0] = D.at
    return rgb, np.concatenate(sig, axis=1), D.at.copy()


def tally(sig):
    """what the premises of the GPU comparison count, from a signature"""
    v = sig[:, SAMPLE_COLUMNS:].reshape(len(sig), -1, VERTEX_COLUMNS)
    ev = v[:, :, C_EVENT]
    hg, iso = ev == EV_MEDIUM_HG, ev == EV_MEDIUM_ISO
    surface = np.isin(ev, (EV_LAMBERT, EV_EMIT))
    later_surface = np.zeros(len(sig), bool)
    seen = np.zeros(len(sig), bool)
    for k in range(v.shape[1]):
        later_surface |= seen & surface[:, k]
        seen |= hg[:, k]
    return dict(anisotropic_events=int(hg.sum()), isotropic_events=int(iso.sum()), surface_after_anisotropic=int(later_surface.sum()),
                both_on_one_path=int((hg.any(axis=1) & iso.any(axis=1)).sum()),
                media_with_events=sorted(int(m) for m in np.unique(v[:, :, C_MEDIUM][hg | iso])))


def reference(S, g, words):
    """the fp64 radiance, which samples took the same branches at fp32 (the stable ones), the draws consumed and the fp64 run's tally"""
    rgb, sig64, draws = trace(S, g, words)
    _, sig32, _ = trace(S, g, words, dtype=np.float32)
    w = max(sig64.shape[1], sig32.shape[1])
    pad = lambda a: np.pad(a, ((0, 0), (0, w - a.shape[1])), constant_values=NONE)
    return rgb, (pad(sig64) == pad(sig32)).all(axis=1), draws, tally(sig64)
