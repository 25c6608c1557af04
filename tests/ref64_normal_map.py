"""Tangent-space normal maps for ref64.py: the tangent frame of every primitive type and the rule that replaces the
shading normal, in NumPy at a floating type of the caller's choice.

Test infrastructure only, written from the model's text (include/rtmi.h) and from the PARAMETRISATION each primitive
has in ref64.hit_uv and ref64_quads, not from csrc/rt_tangent.h; plain operations, no fused ones:
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

ref64.py is not edited.  installed(sc) replaces ref64.hit_record for the length of a block, in the manner of ref64_bump.installed:
the wrapper calls the function it replaced (ref64_quads' wrapper when quads are installed: install THIS one inside it), once more
with flat=True for g, finds each hit's material and its map (sc.normal_map(material)), reads the texel at ref64.hit_uv's (u, v)
and applies the rule.  Movers do not go through hit_record in ref64.trace: a mapped mover is refused by the product.

Deliberate mistakes (names in `perturb`):
  nm_off               no perturbation
  nm_swap_tb           T and B swapped
  nm_back_unsigned     sigma = 1 on back hits
  nm_not_about_n       the frame projected about the geometric normal g, not re-orthogonalised about a smooth triangle's n
  nm_2c_minus_1        glTF's decoding 2 c / 255 - 1
"""
import contextlib

import numpy as np

import ref64 as R
import ref64_pbr as RP
import ref64_quads as Q

PERTURBATIONS = ("nm_off", "nm_swap_tb", "nm_back_unsigned", "nm_not_about_n", "nm_2c_minus_1")
ROUGH_GLASS, PBR = 6, 7


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
        l2 = R._dot(a, a)
        u = a / np.sqrt(l2)[:, None]
    return u, np.isfinite(l2) & (l2 > 0) & np.isfinite(u).all(axis=1)


def raw_tangents(pr, p, T):
    """(T [n][3], B [n][3]) of the primitive record pr at the surface points p [n][3]"""
    ty, f = int(pr["type"]), pr["f"].astype(T)
    n = len(p)
    Tt, Bt = np.zeros((n, 3), T), np.zeros((n, 3), T)
    with np.errstate(all="ignore"):
        if ty == R.SPHERE:
            o = (p - f[:3]) / f[3]
            Tt = np.stack([o[:, 2], np.zeros(n, T), -o[:, 0]], axis=1)
            Bt = R._cross(o, Tt)
        elif ty in (R.XY_RECT, R.XZ_RECT, R.YZ_RECT):
            _, aa, ba = R._rect_axes(ty)
            Tt[:, aa] = T(-1) if f[1] - f[0] < 0 else T(1)
            Bt[:, ba] = T(-1) if f[3] - f[2] < 0 else T(1)
        elif ty == R.CYLINDER:
            M, tr = R._affine(pr["m_inv"], T)
            inv = np.linalg.inv(M.astype(np.float64)).astype(T)
            op = p @ M.T + tr
            Tt = np.stack([-op[:, 1], op[:, 0], np.zeros(n, T)], axis=1) @ inv.T
            Bt = np.tile((inv @ np.array([0, 0, 1], T)) * (T(-1) if f[2] - f[1] < 0 else T(1)), (n, 1))
        elif ty == R.TRIANGLE:
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
            _, u, v, _, _, _ = Q.record(pr, T)
            Tt, Bt = np.tile(u, (n, 1)), np.tile(v, (n, 1))
    return Tt.astype(T), Bt.astype(T)


def frame(n, front, Tr, Br, T, perturb=(), g=None):
    """(T' [n][3], B' [n][3], usable [n]) about the face-turned shading normal n"""
    if "nm_swap_tb" in perturb:
        Tr, Br = Br, Tr
    a = g if "nm_not_about_n" in perturb and g is not None else n
    with np.errstate(all="ignore"):
        Tp, okT = _unit(Tr - R._dot(Tr, a)[:, None] * a)
        Bq = Br - R._dot(Br, a)[:, None] * a
        Bp, okB = _unit(Bq - R._dot(Bq, Tp)[:, None] * Tp)
        sigma = np.where(front, T(1), T(-1))
        Bp = np.where(okB[:, None], Bp, R._cross(sigma[:, None] * n, Tp))
    return Tp.astype(T), Bp.astype(T), okT


def normal(n, g, d, front, s, Tr, Br, xyz, active, T, perturb=(), parts=None):
    """(n' where the rule accepts it, else n; replaced [n] bool).  s: the scale, one or one per vertex.
    parts: a dict that receives "usable" [n], whether the frame could be built (no pole, det != 0)"""
    s = np.asarray(s, np.float32).astype(T)
    sigma = np.ones(len(n), T) if "nm_back_unsigned" in perturb else np.where(front, T(1), T(-1))
    Tp, Bp, usable = frame(n, front, Tr, Br, T, perturb, g)
    with np.errstate(all="ignore"):
        b = (sigma * s)[:, None] * (xyz[:, 0:1] * Tp + xyz[:, 1:2] * Bp) + xyz[:, 2:3] * n
        nb = b / np.sqrt(R._dot(b, b))[:, None]
        ok = active & usable & np.isfinite(nb).all(axis=1) & (R._dot(nb, g) > 0) & (R._dot(nb, -R._unit(d)) > 0)
    if parts is not None:
        parts["usable"] = usable
    return np.where(ok[:, None], nb, n).astype(T), ok


def new_log():
    """what installed() counts: mapped vertices in all, on back faces, those whose texel tilts, and those where one of the two
    GUARDS kept n: the texel tilts and the frame was built (a pole or det == 0, where no frame can be, is not counted)"""
    return dict(mapped=0, back=0, tilting=0, kept=0)


@contextlib.contextmanager
def installed(sc, perturb=(), log=None):
    """ref64.hit_record with the normal maps of the product scene sc, for the length of the block"""
    original = R.hit_record
    maps = {}
    for m in range(len(sc.materials())):
        b = sc.normal_map(m)
        if b is not None:
            maps[m] = (int(b[0]), np.float32(b[1]))

    def hit_record(S, o, d, t, idx, T, flat=False):
        p, n, front = original(S, o, d, t, idx, T, flat)
        mat = S.prims["material"][idx]
        which = np.isin(mat, list(maps))
        if flat or not which.any() or "nm_off" in perturb:
            return p, n, front
        _, g, _ = original(S, o, d, t, idx, T, True)
        u, v = R.hit_uv(S, o, d, t, idx, T)
        n = n.copy()
        for i in np.unique(idx[which]):
            sel = which & (idx == i)
            tex, s = maps[int(S.prims["material"][i])]
            img = S.images[tex]
            row, col = R.image_texel(img, u[sel], v[sel], T)
            xyz, active = decode(img[row, col], T, perturb)
            Tr, Br = raw_tangents(S.prims[i], p[sel], T)
            parts = {}
            n[sel], ok = normal(n[sel], g[sel], d[sel], front[sel], s, Tr, Br, xyz, active, T, perturb, parts)
            if log is not None:
                log["mapped"] += int(sel.sum())
                log["back"] += int((~front[sel]).sum())
                log["tilting"] += int(active.sum())
                log["kept"] += int((active & parts["usable"] & ~ok).sum())
        return p, n, front
    R.hit_record = hit_record
    try:
        yield
    finally:
        R.hit_record = original


def _rest(perturb):
    return tuple(x for x in perturb if x not in PERTURBATIONS)


def trace(sc, S, words, perturb=(), log=None, **kw):
    """ref64.trace on the RefScene S of the product scene sc: inside ref64_pbr's stack (analytic lights, rough glass, quads,
    bumps, noise, pbr) with the maps installed innermost, so that a quad's hits reach them too"""
    P = RP._prepared(S, sc)
    with RP.installed(P, (), None, sc, {} if kw.get("dtype") == np.float32 else None):
        with installed(sc, perturb, log):
            return R.trace(P, words, perturb=_rest(perturb), **kw)


def reference(sc, S, words, shutter=None):
    """ref64.reference's four results: the fp64 radiance, which samples keep their signature at fp32, the draws, the tally"""
    rgb, sig64, draws = trace(sc, S, words, shutter=shutter)
    _, sig32, _ = trace(sc, S, words, dtype=np.float32, shutter=shutter)  # (its radiance is discarded: its signatures say which samples are stable)
    return rgb, R.same_signature(sig64, sig32), draws, R.tally(sig64, RP._prepared(S, sc))


def tally(sig, S, sc, log=None):
    """What a normal-map case is there for.  From the reference's signatures: the surface vertices whose material carries a map,
    by material type, and the share of samples with at least one.  From the wrapper's log: the mapped vertices on back faces,
    those whose texel tilts and those where a guard kept n."""
    v = sig[:, R.SAMPLE_COLUMNS:].reshape(len(sig), -1, R.VERTEX_COLUMNS)
    event, prim = v[:, :, R.C_EVENT], v[:, :, R.C_PRIM]
    surface = (event != R.NONE) & (event != R.EV_MISS) & (event != R.EV_MEDIUM) & (prim >= 0)
    if len(S.movers):
        surface &= ~(v[:, :, R.C_MOVER] >= 0)
    mat = np.where(surface, S.prims["material"][np.clip(prim, 0, len(S.prims) - 1)], -1)
    mats = sc.materials()
    mapped = np.isin(mat, [m for m in range(len(mats)) if sc.normal_map(m) is not None])
    mtype = np.where(mapped, np.asarray(mats["type"])[np.clip(mat, 0, len(mats) - 1)], -1)
    ptype = np.where(mapped, S.prims["type"][np.clip(prim, 0, len(S.prims) - 1)], -1)
    out = dict(nm_vertices=int(mapped.sum()), nm_share=float(mapped.any(axis=1).mean()))
    for name, kind in (("lambertian", R.LAMBERTIAN), ("metal", R.METAL), ("dielectric", R.DIELECTRIC), ("rough_metal", R.ROUGH_METAL),
                       ("plastic", R.PLASTIC), ("rough_glass", ROUGH_GLASS), ("pbr", PBR)):
        out["nm_" + name] = int((mtype == kind).sum())
    for name, kinds in (("sphere", (R.SPHERE,)), ("rect", (R.XY_RECT, R.XZ_RECT, R.YZ_RECT)), ("cylinder", (R.CYLINDER,)),
                        ("triangle", (R.TRIANGLE,)), ("quad", (Q.QUAD,))):
        out["nm_on_" + name] = int(np.isin(ptype, kinds).sum())
    out["nm_light_samples"] = int((mapped & (v[:, :, R.C_LIGHT] != R.NONE)).sum())
    if log is not None:
        out["nm_back"], out["nm_tilting"], out["nm_kept"] = log["back"], log["tilting"], log["kept"]
    return out
