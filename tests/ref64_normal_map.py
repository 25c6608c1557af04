"""Tangent-space normal maps for ref64.py: the tangent frame of every primitive type and the rule that replaces the
shading normal, in NumPy at a floating type of the caller's choice.

Test infrastructure only, written from the model's text (include/rtmi.h) and from the PARAMETRISATION each primitive
has in ref64.hit_uv, not from csrc/rt_tangent.h; plain operations, no fused ones:
    decoding   x = max((r8 - 128) / 127, -1), y from g8, z from b8;  r8 == g8 == 128 or z <= 0: the vertex keeps n
    raw (T, B) = (dp/du, dp/dv) up to positive factors
      sphere     o the outward unit normal: T = (o_z, 0, -o_x), B = o x T
      rectangle  the unit vectors of the axes behind u and v, signed by the extents
      cylinder   M^-1 (-y_o, x_o, 0) and M^-1 e_z sign(zmax - zmin), M the linear part of the world-to-object matrix (inverted
                 with numpy.linalg.inv: nothing here assumes a rotation)
      triangle   hit_uv pairs (u1, v1) with the weight that is 1 at corner 3, (u2, v2) with corner 2, (u3, v3) with corner 1:
                 E1 = V2 - V3, E2 = V1 - V3, du1 = u2 - u1, du2 = u3 - u1 (dv alike), det = du1 dv2 - du2 dv1,
                 T = (dv2 E1 - dv1 E2) / det, B = (du1 E2 - du2 E1) / det;  det = 0: not finite
      quad       the record's edges u and v
    frame      T' = unit(T - (T.n) n),  B' = unit(B - (B.n) n - (B.T') T');  B' zero or not finite: cross(sigma n, T');
               T' zero or not finite: the vertex keeps n
    normal     b = sigma s (x T' + y B') + z n,  n' = b / |b|;  n' replaces n iff finite, n'.g > 0 and n'.(-unit(d)) > 0

This file holds the model alone and imports nothing of ref64: ref64.hit_record finds each hit's material and its map (RefScene
read them from Scene.normal_map), reads the texel at ref64.hit_uv's (u, v), calls decode(), raw_tangents() and normal() and counts
what the signature does not keep into trace()'s log.

Deliberate mistakes (names in `perturb`, as ref64.trace takes them; nm_off is hit_record's own):
  nm_off               no perturbation
  nm_swap_tb           T and B swapped
  nm_back_unsigned     sigma = 1 on back hits
  nm_not_about_n       the frame projected about the geometric normal g, not re-orthogonalised about a smooth triangle's n
  nm_2c_minus_1        glTF's decoding 2 c / 255 - 1
"""
import numpy as np

from ref64_base import SPHERE, XY_RECT, XZ_RECT, YZ_RECT, CYLINDER, TRIANGLE, _affine, _cross, _dot, _rect_axes
from ref64_base import _unit as _unit_rows

PERTURBATIONS = ("nm_off", "nm_swap_tb", "nm_back_unsigned", "nm_not_about_n", "nm_2c_minus_1")


def decode(rgb8, T, perturb=()):
    """(xyz [n][3] at T, active [n]: the texel tilts the normal) of the byte triples rgb8 [n][3]"""
    c = np.asarray(rgb8).astype(np.int64)
    if "nm_2c_minus_1" in perturb:
        xyz = (T(2) * c.astype(T) / T(255) - T(1)).astype(T)
    else:
        xyz = np.maximum((c - 128).astype(T) / T(127), T(-1)).astype(T)
    active = ~((c[:, 0] == 128) & (c[:, 1] == 128)) & (xyz[:, 2] > 0)
    return xyz, active


def _unit(a):
    with np.errstate(all="ignore"):
        l2 = _dot(a, a)
        u = a / np.sqrt(l2)[:, None]
    return u, np.isfinite(l2) & (l2 > 0) & np.isfinite(u).all(axis=1)


def raw_tangents(pr, p, T):
    """(T [n][3], B [n][3]) of the primitive record pr at the surface points p [n][3]"""
    ty, f = int(pr["type"]), pr["f"].astype(T)
    n = len(p)
    Tt, Bt = np.zeros((n, 3), T), np.zeros((n, 3), T)
    with np.errstate(all="ignore"):
        if ty == SPHERE:
            o = (p - f[:3]) / f[3]
            Tt = np.stack([o[:, 2], np.zeros(n, T), -o[:, 0]], axis=1)
            Bt = _cross(o, Tt)
        elif ty in (XY_RECT, XZ_RECT, YZ_RECT):
            _, aa, ba = _rect_axes(ty)
            Tt[:, aa] = T(-1) if f[1] - f[0] < 0 else T(1)
            Bt[:, ba] = T(-1) if f[3] - f[2] < 0 else T(1)
        elif ty == CYLINDER:
            M, tr = _affine(pr["m_inv"], T)
            inv = np.linalg.inv(M.astype(np.float64)).astype(T)
            op = p @ M.T + tr
            Tt = np.stack([-op[:, 1], op[:, 0], np.zeros(n, T)], axis=1) @ inv.T
            Bt = np.tile((inv @ np.array([0, 0, 1], T)) * (T(-1) if f[2] - f[1] < 0 else T(1)), (n, 1))
        elif ty == TRIANGLE:
            m, c = pr["m"].astype(T), pr["m_inv"].astype(T)
            v1, v2, v3 = m[0:3], m[3:6], m[6:9]
            uv1, uv2, uv3 = c[0:2], c[2:4], c[4:6]
            e1, e2 = v2 - v3, v1 - v3
            du1, dv1 = uv2 - uv1
            du2, dv2 = uv3 - uv1
            det = du1 * dv2 - du2 * dv1
            Tt = np.tile((dv2 * e1 - dv1 * e2) / det, (n, 1))
            Bt = np.tile((du1 * e2 - du2 * e1) / det, (n, 1))
        else:
            m = pr["m"].astype(T)  # a quad: its edges
            u, v = m[3:6], m[6:9]
            Tt, Bt = np.tile(u, (n, 1)), np.tile(v, (n, 1))
    return Tt.astype(T), Bt.astype(T)


def frame(n, front, Tr, Br, T, perturb=(), g=None):
    """(T' [n][3], B' [n][3], usable [n]) about the face-turned shading normal n"""
    if "nm_swap_tb" in perturb:
        Tr, Br = Br, Tr
    a = g if "nm_not_about_n" in perturb and g is not None else n
    with np.errstate(all="ignore"):
        Tp, okT = _unit(Tr - _dot(Tr, a)[:, None] * a)
        Bq = Br - _dot(Br, a)[:, None] * a
        Bp, okB = _unit(Bq - _dot(Bq, Tp)[:, None] * Tp)
        sigma = np.where(front, T(1), T(-1))
        Bp = np.where(okB[:, None], Bp, _cross(sigma[:, None] * n, Tp))
    return Tp.astype(T), Bp.astype(T), okT


def normal(n, g, d, front, s, Tr, Br, xyz, active, T, perturb=(), parts=None):
    """(n' where the rule accepts it, else n; replaced [n] bool).  s: the scale, one or one per vertex.
    parts: a dict that receives "usable" [n], whether the frame could be built (no pole, det != 0)"""
    s = np.asarray(s, np.float32).astype(T)
    sigma = np.ones(len(n), T) if "nm_back_unsigned" in perturb else np.where(front, T(1), T(-1))
    Tp, Bp, usable = frame(n, front, Tr, Br, T, perturb, g)
    with np.errstate(all="ignore"):
        b = (sigma * s)[:, None] * (xyz[:, 0:1] * Tp + xyz[:, 1:2] * Bp) + xyz[:, 2:3] * n
        nb = b / np.sqrt(_dot(b, b))[:, None]
        ok = active & usable & np.isfinite(nb).all(axis=1) & (_dot(nb, g) > 0) & (_dot(nb, -_unit_rows(d)) > 0)
    if parts is not None:
        parts["usable"] = usable
    return np.where(ok[:, None], nb, n).astype(T), ok
