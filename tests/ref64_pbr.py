"""The metallic-roughness material for ref64.py, in NumPy at a floating type of the caller's choice.

Test infrastructure only, written from the definition of the material (include/rtmi.h, rt_scene_add_pbr), not from
csrc/rt_pbr.h: plain operations, no fused ones.  At a hit, with the base colour c and the map's channels G, B (1 without a map):
    byte(x) = floor(clip(x, 0, 1) 255 + 0.5);  c8 = byte(c),  r8 = byte(rf G),  m8 = byte(mf B)
    c = c8 / 255,  r = r8 / 255,  m = m8 / 255,  alpha = max(r r, 1e-3): these four are fp32 values BY DEFINITION (one fp32
    division, one fp32 product), formed at float32 whatever the caller's type, as ref64_glossy.alpha_of forms the packer's alpha
    draws ul, u1, u2 (plastic's order);  ul < m: a rough metal, F0 = c;  else a plastic, body c, r0 of the coat's index,
    lobe draw ul' = (ul - m) / (1 - m).  Everything else is that material's rule (ref64_glossy), for the scatter step and for the
    light sample, which both see the lobe the vertex chose.

This file holds the model alone and imports nothing of ref64.  ref64.trace()'s glossy block states the vertex: the base texture's
and the map's values at the hit, params(), choose() from ul, the chosen material's row for ref64_glossy.glossy_sample and -- kept
in the loop's per-vertex arrays -- for glossy_eval at the light sample, which the vertex takes iff ITS r >= 0.05: the decision
is the hit's, so a map may carry one material across the threshold.  A metal choice is signed EV_COAT, a plastic one EV_COAT /
EV_BODY as its own lobe draw says.  trace()'s log counts what the signatures do not keep, under LOG_KEYS.

Deliberate mistakes (names in `perturb`, as ref64.trace takes them; the last three are the loop's own):
  lobe_draw_not_rescaled   a plastic choice uses ul as it is
  metal_f0_004             a metal choice has F0 = 0.04 in place of the base colour
  roughness_from_r         the map's R channel scales the roughness
  light_step_from_factors  the light sample's alpha and r come from the factors rf, not from the hit
"""
import numpy as np

PBR = 7
PERTURBATIONS = ("lobe_draw_not_rescaled", "metal_f0_004", "roughness_from_r", "light_step_from_factors")
LOG_KEYS = tuple("pbr_" + k for k in ("vertices", "metal_choices", "plastic_choices", "below", "smooth_vertices", "light_evaluations", "lit",
                                      "image_map_hits", "noise_map_hits", "checker_map_hits", "image_base_hits", "noise_base_hits"))


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
