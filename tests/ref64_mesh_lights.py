"""The triangle light sample of DESIGN 7n (mesh lights) for ref64.py, in NumPy at a floating type of the caller's choice.

Test infrastructure only, written from the definition: a point uniform by area on the triangle (v1, v2, v3) from two uniforms,
    s = sqrt(u1),  b1 = 1 - s,  b2 = u2 s,  y = v1 + b1 e1 + b2 e2,   e1 = v2 - v1,  e2 = v3 - v1,
the vector ld = y - p from the vertex, and the light strategy's solid-angle density of that direction,
    p_l = selection / area x |ld|^2 / |n . ld / |ld||,
with n the triangle's GEOMETRIC unit normal (the primitive record's m[9..11]), whatever vertex normals it carries: an emitter
hit keeps the geometric normal, and ref64.light_pdf_of_hit states the same density from the hit's side.  The edges
are the fp32 differences of the fp32 vertices, which is what the light record holds; everything after that runs at dtype T with
plain (unfused) operations.  Emission: the light's colour, a checker's by the parity of the point p + ld, as for every light.

ref64.py is not edited: its sample_light reads the `f` words of a rectangle and would take a triangle for one.  installed()
puts a wrapper in its place while a trace runs -- the wrapper handles shape TRIANGLE itself and passes every other shape to the
function it replaced -- and takes it out again.  trace() and reference() are ref64's, called inside installed().

Deliberate mistakes (names in `perturb`, as ref64.trace takes them):
  tri_no_sqrt        the barycentrics taken without the square root (s = u1): points crowd towards v2
  tri_vertex_normal  the density stated with the triangle's first vertex normal in place of the geometric one (a triangle
                     without vertex normals: its geometric normal tilted by 0.5 about e1, so the name never does nothing)
"""
import contextlib

import numpy as np

import ref64 as R

PERTURBATIONS = ("tri_no_sqrt", "tri_vertex_normal")


def triangle_record(pr):
    """(v1, e1, e2, n) as the light record holds them: fp32, the edges fp32 differences of the fp32 vertices"""
    m = pr["m"].astype(np.float32)
    return m[0:3], m[3:6] - m[0:3], m[6:9] - m[0:3], m[9:12]


def triangle_area(pr):
    """|e1 x e2| / 2 in fp64 from the stored vertices"""
    m = pr["m"].astype(np.float64)
    return 0.5 * float(np.linalg.norm(np.cross(m[3:6] - m[0:3], m[6:9] - m[0:3])))


def sample_triangle(S, li, p, u1, u2, T, perturb=()):
    """ref64.sample_light's contract for a triangle light: (ld, p_l, emitted radiance, texel = NONE)"""
    L = S.lights[li]
    pr = S.prims[L["prim"]]
    v1, e1, e2, n = (a.astype(T) for a in triangle_record(pr))
    if "tri_vertex_normal" in perturb:
        n1 = R.prim_normals(pr)[0].astype(T)
        if not np.any(n1 != 0):
            t = e1 / np.sqrt((e1 * e1).sum())
            n1 = (np.cos(T(0.5)) * n + np.sin(T(0.5)) * np.cross(t, n)).astype(T)
        n = n1
    s = u1 if "tri_no_sqrt" in perturb else np.sqrt(u1)
    b1, b2 = 1 - s, u2 * s
    y = v1 + b1[:, None] * e1 + b2[:, None] * e2
    ld = (y - p).astype(T)
    d2 = R._dot(ld, ld)
    with np.errstate(all="ignore"):
        cos_l = np.abs(R._dot(n[None, :], ld)) / np.sqrt(d2)
        pl = T(L["probability"]) / T(L["area"]) * d2 / cos_l
    odd = R.checker_odd(p + ld, T)
    rad = np.where(odd[:, None], L["emission_odd"].astype(T), L["emission"].astype(T))
    return ld, pl.astype(T), rad, np.full(len(p), R.NONE, np.int64)


@contextlib.contextmanager
def installed():
    """ref64.sample_light with triangle lights, for the length of the block"""
    original = R.sample_light

    def sample_light(S, li, p, u1, u2, T, perturb=()):
        if S.lights[li]["shape"] == R.TRIANGLE:
            return sample_triangle(S, li, p, u1, u2, T, perturb)
        return original(S, li, p, u1, u2, T, perturb)
    R.sample_light = sample_light
    try:
        yield
    finally:
        R.sample_light = original


def trace(S, words, **kw):
    with installed():
        return R.trace(S, words, **kw)


def reference(S, words, shutter=None):
    with installed():
        return R.reference(S, words, shutter)


def tally(sig, S):
    """What a mesh-light case is there for, from the reference's signatures: light samples that picked a triangle light, those
    whose shadow ray was stopped (and those that reached the light), and BSDF hits on a triangle light weighted by MIS (the
    vertex before took a light sample and the light strategy could have produced the direction: the weight is below 1)"""
    v = sig[:, R.SAMPLE_COLUMNS:].reshape(len(sig), -1, R.VERTEX_COLUMNS)
    event, light, shadow, how, prim = (v[:, :, c] for c in (R.C_EVENT, R.C_LIGHT, R.C_SHADOW, R.C_HIT_WEIGHT, R.C_PRIM))
    tri_light = S.lights["shape"] == R.TRIANGLE
    picked = (light >= 0) & tri_light[np.clip(light, 0, len(tri_light) - 1)]
    is_tri_light = np.zeros(len(S.prims), bool)
    is_tri_light[S.lights["prim"][tri_light]] = True
    on = (event == R.EV_EMIT) & (prim >= 0) & is_tri_light[np.clip(prim, 0, len(S.prims) - 1)]
    return dict(triangle_picks=int(picked.sum()), other_picks=int(((light >= 0) & ~picked).sum()),
                triangle_shadow_stopped=int((picked & (shadow == R.SHADOW_OCCLUDED)).sum()),
                triangle_shadow_clear=int((picked & (shadow == R.SHADOW_CLEAR)).sum()),
                triangle_mis_hits=int((on & (how == R.HIT_MIS)).sum()),
                triangle_full_weight_hits=int((on & (how == R.HIT_UNSAMPLED)).sum()))
