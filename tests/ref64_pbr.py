"""The metallic-roughness material for ref64.py, in NumPy at a floating type of the caller's choice.

Test infrastructure only, written from the definition of the material (include/rtmi.h, rt_scene_add_pbr), not from
csrc/rt_pbr.h: plain operations, no fused ones.  At a hit, with the base colour c and the map's channels G, B (1 without a map):
    byte(x) = floor(clip(x, 0, 1) 255 + 0.5);  c8 = byte(c),  r8 = byte(rf G),  m8 = byte(mf B)
    c = c8 / 255,  r = r8 / 255,  m = m8 / 255,  alpha = max(r r, 1e-3): these four are fp32 values BY DEFINITION (one fp32
    division, one fp32 product), formed at float32 whatever the caller's type, as ref64_glossy.alpha_of forms the packer's alpha
    draws ul, u1, u2 (plastic's order);  ul < m: a rough metal, F0 = c;  else a plastic, body c, r0 of the coat's index,
    lobe draw ul' = (ul - m) / (1 - m).  Everything else is that material's rule (ref64_glossy), for the scatter step and for the
    light sample, which both see the lobe the vertex chose.

ref64.py is not edited and its path loop is not restated.  present() hands ref64.trace a COPY of the RefScene (as ref64_glass
presents it) in which every pbr material is a plastic: its `ir` scaled by -2^-20 (the mark: a value in (-1, 0), exact in fp32;
ref64_glass marks its rows with ir < -1), its texture a sentinel texture appended to S.texs.  installed() replaces, for the
length of a trace,
    r0_of          a marked ir comes back as MINUS the coat's r0: a negative "r0" marks the row in the two calls below
    texture_value  a sentinel texture's value carries the hit's bytes: (c8.r + 256 r8, c8.g + 256 m8, c8.b + 256 slot), integers
                   below 2^24 (exact at float32), slot the material's place among the pbr materials; the base texture and the
                   map are evaluated by the function it replaced (images, checkers; noise through ref64_noise)
    glossy_sample  rows with r0 < 0: the choice, ul', alpha, then the function it replaced with the row as the material it chose;
                   what it chose is kept per vertex (keyed by the bits of n and unit(d)) for
    glossy_eval    which finds it again: trace() calls glossy_sample before glossy_eval for the same vertices.
A metal choice is signed EV_COAT, a plastic one EV_COAT / EV_BODY as its own lobe draw says.

What the hooks cannot express: ref64.trace decides whether a glossy vertex takes a light sample from the MATERIAL's roughness
(`rec["fuzz"] >= GLOSSY_MIN_ROUGHNESS`), not from a value of the hit.  present() therefore shows a roughness on the right side
of the threshold and raises for a material whose map can carry r = r8 / 255 across it (r8 >= 13 on one part, below on another):
the cases keep each material on one side, and every call checks that the hits are where the material was presented.

Deliberate mistakes (names in `perturb`):
  lobe_draw_not_rescaled   a plastic choice uses ul as it is
  metal_f0_004             a metal choice has F0 = 0.04 in place of the base colour
  roughness_from_r         the map's R channel scales the roughness
  light_step_from_factors  the light sample's alpha and r come from the factors rf, not from the hit
"""
import contextlib
import copy

import numpy as np

import ref64 as R
import ref64_analytic_lights as AL
import ref64_glass as RG
import ref64_glossy as G
import ref64_noise as N

PBR = 7
MARK = np.float32(2.0 ** -20)
PERTURBATIONS = ("lobe_draw_not_rescaled", "metal_f0_004", "roughness_from_r", "light_step_from_factors")
LOG_KEYS = ("vertices", "metal_choices", "plastic_choices", "below", "smooth_vertices", "light_evaluations", "lit", "image_map_hits",
            "noise_map_hits", "checker_map_hits", "image_base_hits", "noise_base_hits")


def new_log():
    return dict.fromkeys(LOG_KEYS, 0)


# --------------------------------------------------------------------------------------------------------------- the model
def byte(x, T):
    """floor(clip(x, 0, 1) 255 + 0.5), as integers held in T"""
    return np.floor(np.clip(x, 0, 1).astype(T) * T(255) + T(0.5)).astype(T)


def params(c, Gc, Bc, rf, mf, T):
    """(c8 [N][3], r8 [N], m8 [N]) of base colours c and map channels Gc, Bc under the factors rf, mf (fp32 values)"""
    rf, mf = np.float32(rf).astype(T), np.float32(mf).astype(T)
    return byte(c, T), byte(rf * Gc, T), byte(mf * Bc, T)


def unit(x8, T):
    """the float of a byte: x8 / 255 in fp32"""
    return (np.asarray(x8).astype(np.float32) / np.float32(255)).astype(T)


def choose(m8, ul, T, perturb=()):
    """(metal [N], ul' [N]) from the first draw"""
    m = unit(m8, T)
    metal = ul < m
    with np.errstate(all="ignore"):
        ulp = np.where(metal, ul, (ul - m) / (1 - m)).astype(T)
    if "lobe_draw_not_rescaled" in perturb:
        ulp = ul
    return metal, ulp


def alpha_of(r, T):
    """max(r r, 1e-3) in fp32, of an fp32 r"""
    r = np.asarray(r).astype(np.float32)
    return np.maximum(r * r, np.float32(1e-3)).astype(T)


# ------------------------------------------------------------------------------------------------- presenting it to ref64
def is_pbr_scene(S):
    return bool((S.mats["type"] == PBR).any())


def _r8_range(S, sc, mat, map_tex):
    """(lowest, highest) r8 the material can show"""
    rf = np.float32(S.mats["fuzz"][mat])
    if map_tex < 0:
        g = np.array([1.0])
    else:
        t = S.texs[map_tex]
        if t["type"] == R.IMAGE:
            g = np.unique(S.images[map_tex][:, :, 1]).astype(np.float64) / 255
        elif t["type"] == N.NOISE:
            g = np.linspace(min(t["c0"][1], t["c1"][1]), max(t["c0"][1], t["c1"][1]), 1025)
        else:
            g = np.array([t["c0"][1], t["c1"][1]] if t["type"] == R.CHECKER else [t["c0"][1]], np.float64)
    r8 = byte(np.float64(rf) * g, np.float64)
    return int(r8.min()), int(r8.max())


def present(S, sc):
    """a copy of the RefScene with every rough_glass (ref64_glass.present) and every pbr material shown as a plastic (see the
    module's docstring); sc: the product scene, for the maps"""
    P = RG.present(S)
    if not is_pbr_scene(S):
        return P
    P = copy.copy(P)
    P.mats, first = P.mats.copy(), len(P.texs)
    pbr = np.flatnonzero(S.mats["type"] == PBR)
    extra = np.zeros(len(pbr), P.texs.dtype)
    extra["type"] = R.SOLID
    P.texs = np.concatenate([P.texs, extra])
    P.pbr, P.pbr_slots, P.pbr_materials = {}, [], pbr
    thr8 = int(np.ceil(G.GLOSSY_MIN_ROUGHNESS * 255))  # r8 / 255 >= 0.05 iff r8 >= 13
    for j, m in enumerate(pbr):
        mp = sc.pbr_map(int(m))
        d = dict(material=int(m), base=int(S.mats["texture"][m]), map=-1 if mp is None else int(mp), mf=np.float32(S.mats["albedo"][m][0]),
                 rf=np.float32(S.mats["fuzz"][m]), slot=j)
        lo, hi = _r8_range(S, sc, m, d["map"])
        if (lo >= thr8) != (hi >= thr8):
            raise ValueError(f"material {m}: r8 runs from {lo} to {hi}, across the light-sample threshold ({thr8}): ref64.trace takes that "
                             "decision per material (see the module's docstring)")
        d["takes_light"] = lo >= thr8
        P.pbr[first + j] = d
        P.pbr_slots.append(d)
        P.mats["fuzz"][m] = np.float32(lo if d["takes_light"] else hi) / np.float32(255)
    P.mats["type"][pbr] = G.PLASTIC
    P.mats["texture"][pbr] = first + np.arange(len(pbr))
    P.mats["ir"][pbr] = -S.mats["ir"][pbr] * MARK
    return P


def _key(n, ud):
    a = np.ascontiguousarray(np.concatenate([n, ud], axis=1))
    return [row.tobytes() for row in a]


@contextlib.contextmanager
def installed(S, perturb=(), log=None, sc=None, lights_report=None):
    """ref64's r0_of, texture_value, glossy_sample and glossy_eval with the pbr material of the present()ed scene S, for the length
    of the block; inside ref64_analytic_lights, ref64_glass (quads; with sc, bumps) and ref64_noise (the noise textures of sc)"""
    slots = getattr(S, "pbr_slots", [])
    kinds = {}
    if sc is not None:
        kinds = {ti: int(t["type"]) for ti, t in enumerate(sc.textures())}
    chosen = {}

    def count(key, n):
        if log is not None:
            log[key] += int(n)

    with contextlib.ExitStack() as stack:
        stack.enter_context(AL.installed((), None, lights_report))
        stack.enter_context(RG.installed((), None, sc))
        if sc is not None:
            stack.enter_context(N.installed(sc))
        orig = {k: getattr(R, k) for k in ("r0_of", "texture_value", "glossy_sample", "glossy_eval")}

        def r0_of(ior):
            ior = np.asarray(ior, np.float32)
            mark = (ior < 0) & (ior > -1)
            with np.errstate(all="ignore"):
                return np.where(mark, -G.r0_of(np.where(mark, -ior / MARK, np.float32(1.5))), orig["r0_of"](np.where(mark, np.float32(1.5), ior))).astype(np.float32)

        def texture_value(S_, tex, p, T, o=None, d=None, t=None, idx=None, mov=None, time=None, perturb_=()):
            tex = np.asarray(tex)
            info = getattr(S_, "pbr", {})
            g = np.isin(tex, list(info))
            if not g.any():
                return orig["texture_value"](S_, tex, p, T, o, d, t, idx, mov, time, perturb_)
            out, texel = np.zeros_like(p), np.full(len(p), R.NONE, np.int64)
            if (~g).any():
                r = ~g
                sub = lambda x: None if x is None else x[r]
                out[r], texel[r] = orig["texture_value"](S_, tex[r], p[r], T, sub(o), sub(d), sub(t), sub(idx), sub(mov), sub(time), perturb_)
            for ti in np.unique(tex[g]):
                m, e = tex == ti, info[int(ti)]
                sub = lambda x: None if x is None else x[m]
                k = int(m.sum())
                at = lambda which: orig["texture_value"](S_, np.full(k, which, np.int64), p[m], T, sub(o), sub(d), sub(t), sub(idx), sub(mov), sub(time), perturb_)
                base, texel[m] = at(e["base"])
                mp = at(e["map"])[0] if e["map"] >= 0 else np.ones((k, 3), T)
                c8, r8, m8 = params(base, mp[:, 0] if "roughness_from_r" in perturb else mp[:, 1], mp[:, 2], e["rf"], e["mf"], T)
                out[m] = np.stack([c8[:, 0] + 256 * r8, c8[:, 1] + 256 * m8, c8[:, 2] + 256 * T(e["slot"])], axis=1).astype(T)
                for key, which in (("map", e["map"]), ("base", e["base"])):
                    kind = {R.IMAGE: "image", N.NOISE: "noise", R.CHECKER: "checker"}.get(kinds.get(which, -1))
                    if kind and f"{kind}_{key}_hits" in LOG_KEYS:
                        count(f"{kind}_{key}_hits", k)
            return out, texel

        def decode(rho, T):
            hi = np.floor(rho / 256)
            c8 = rho - 256 * hi
            return unit(c8, T), hi[:, 0], hi[:, 1], hi[:, 2].astype(np.int64)

        def as_chosen(metal, c, r0, T):
            f0 = np.where(metal[:, None], np.full_like(c, T(0.04)) if "metal_f0_004" in perturb else c, r0)
            return ~metal, f0.astype(T)

        def glossy_sample(n, ud, alpha, plastic, f0, rho, ul, u1, u2, T, perturb_=()):
            g = plastic & (f0[:, 0] < 0)
            chosen.clear()
            if not g.any():
                return orig["glossy_sample"](n, ud, alpha, plastic, f0, rho, ul, u1, u2, T, perturb_)
            N_ = len(n)
            outs = [np.zeros((N_, 3), T), np.zeros((N_, 3), T), np.zeros(N_, T), np.zeros(N_, bool), np.zeros(N_, bool), np.zeros(N_, bool)]
            r = ~g
            if r.any():
                for dst, src in zip(outs, orig["glossy_sample"](n[r], ud[r], alpha[r], plastic[r], f0[r], rho[r], ul[r], u1[r], u2[r], T, perturb_)):
                    dst[r] = src
            c, r8, m8, slot = decode(rho[g], T)
            rough = unit(r8, T)
            a = alpha_of(rough, T)
            metal, ulp = choose(m8, ul[g], T, perturb)
            pl, fx = as_chosen(metal, c, -f0[g], T)
            res = list(orig["glossy_sample"](n[g], ud[g], a, pl, fx, c, ulp, u1[g], u2[g], T, perturb_))
            res[5] = res[5] | metal  # (signed EV_COAT: ref64.trace sees a plastic row)
            for dst, src in zip(outs, res):
                dst[g] = src
            below = res[3]
            takes = np.array([slots[s]["takes_light"] for s in slot], bool)
            if "roughness_from_r" not in perturb and ((rough >= T(G.GLOSSY_MIN_ROUGHNESS)) != takes).any():
                raise ArithmeticError("a pbr hit's roughness lies on the other side of the light-sample threshold than its material was presented")
            for k, key in enumerate(_key(n[g], ud[g])):
                chosen[key] = (bool(metal[k]), a[k], int(slot[k]))
            count("vertices", g.sum()), count("below", below.sum())
            count("metal_choices", (metal & ~below).sum()), count("plastic_choices", (~metal & ~below).sum())
            count("smooth_vertices", (~takes & ~below).sum())
            return tuple(outs)

        def glossy_eval(n, ud, alpha, plastic, f0, rho, wl, T):
            g = plastic & (f0[:, 0] < 0)
            if not g.any():
                return orig["glossy_eval"](n, ud, alpha, plastic, f0, rho, wl, T)
            N_ = len(n)
            fcos, pdf = np.zeros((N_, 3), T), np.zeros(N_, T)
            r = ~g
            if r.any():
                fcos[r], pdf[r] = orig["glossy_eval"](n[r], ud[r], alpha[r], plastic[r], f0[r], rho[r], wl[r], T)
            c = decode(rho[g], T)[0]
            kept = [chosen[key] for key in _key(n[g], ud[g])]
            metal, a = np.array([k[0] for k in kept], bool), np.array([k[1] for k in kept], T)
            if "light_step_from_factors" in perturb:
                a = np.array([alpha_of(np.float32(slots[k[2]]["rf"]).astype(T), T) for k in kept], T)
            pl, fx = as_chosen(metal, c, -f0[g], T)
            fcos[g], pdf[g] = orig["glossy_eval"](n[g], ud[g], a, pl, fx, c, wl[g], T)
            count("light_evaluations", g.sum()), count("lit", (fcos[g] > 0).any(axis=1).sum())
            return fcos, pdf

        new = dict(r0_of=r0_of, texture_value=texture_value, glossy_sample=glossy_sample, glossy_eval=glossy_eval)
        for k, f in new.items():
            setattr(R, k, f)
        try:
            yield
        finally:
            for k, f in orig.items():
                setattr(R, k, f)


def _rest(perturb):
    return tuple(x for x in perturb if x not in PERTURBATIONS)


def _prepared(S, sc):
    if len(S.lights) and not hasattr(S, "analytic"):
        AL.attach(S, sc)
    return present(S, sc)


def trace(S, words, sc, perturb=(), log=None, **kw):
    """ref64.trace on the RefScene S of the product scene sc, with the pbr material installed"""
    P = _prepared(S, sc)
    with installed(P, perturb, log, sc, {} if kw.get("dtype") == np.float32 else None):
        return R.trace(P, words, perturb=_rest(perturb), **kw)


def reference(S, words, sc, shutter=None):
    """ref64.reference's four results; the tally holds ref64.tally's counts and, as pbr_*, the log of the fp64 run"""
    P, log = _prepared(S, sc), new_log()
    with installed(P, (), log, sc):
        rgb, sig64, draws = R.trace(P, words, shutter=shutter)
    with installed(P, (), None, sc, {}):  # (the fp32 run's radiance is discarded: its signatures say which samples are stable)
        _, sig32, _ = R.trace(P, words, dtype=np.float32, shutter=shutter)
    return rgb, R.same_signature(sig64, sig32), draws, dict(R.tally(sig64, P), **{"pbr_" + k: v for k, v in log.items()})
