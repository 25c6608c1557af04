"""Bump mapping for ref64.py: the analytic gradient of the noise textures' scalar and the rule that tilts the shading
normal, in NumPy at a floating type of the caller's choice.

Test infrastructure only, written from the model's text (include/rtmi.h), not from csrc/rt_noise.h, on top of
ref64_noise's lattice_hash, grad and fade:
    n(q, s) = sum_abc Wa(tx) Wb(ty) Wc(tz) g_abc(t),  g_abc(t) = G_abc . (t - (a, b, c)),  W0 = 1 - w, W1 = w,  t = q - floor(q)
    dn/dx   = sum_abc Wa Wb Wc G_abc.x + w'(tx) sum_bc Wb(ty) Wc(tz) (g_1bc - g_0bc),  w'(t) = 30 t^2 (t - 1)^2; same for y, z
              (G_abc is what grad() selects: grad is linear, so G = (grad(h, 1, 0, 0), grad(h, 0, 1, 0), grad(h, 0, 0, 1)));
              a coordinate outside (-2^30, 2^30) or a NaN: that component is 0
    grad S  = f sum_o grad_q n(2^o f p, seed + o),  grad A = f sum_o sgn(n_o) grad_q n_o, sgn(0) = 0
    fbm: 0.5 grad S where 0 < 0.5 + 0.5 S < 1, else 0;  turbulence: grad A where A < 1, else 0
    marble: 0.5 cos(f p[axis] + D A) (f e_axis + D grad A)
    the bump: n the face-turned shading normal, g the face-turned geometric one, sigma = +1 front / -1 back, G = grad s(p):
              Gt = G - (G . n) n,  b = n - sigma k Gt,  n' = b / |b|;  n' replaces n iff finite, n' . g > 0, n' . (-unit(d)) > 0

This file holds the model alone and imports nothing of ref64: ref64.hit_record finds each hit's material and its bump (RefScene
read them from Scene.bump), calls gradient_of() and bump() and counts what the signature does not keep into trace()'s log.

Deliberate mistakes (names in `perturb`, as ref64.trace takes them; bump_off is hit_record's own):
  bump_off                     no perturbation
  bump_full_gradient           G in place of Gt
  bump_back_unsigned           sigma = 1 on back hits
  bump_cubic_fade_derivative   w' = 6 t (1 - t)
"""
import numpy as np

import ref64_noise as N
from ref64_base import _dot, _unit

PERTURBATIONS = ("bump_off", "bump_full_gradient", "bump_back_unsigned", "bump_cubic_fade_derivative")
LIMIT = 2.0 ** 30


def fade_derivative(t, T, perturb=()):
    if "bump_cubic_fade_derivative" in perturb:
        return T(6) * t * (T(1) - t)
    return T(30) * t * t * (t - T(1)) * (t - T(1))


def noise_gradient(q, seed, T, perturb=()):
    """(n [n], grad_q n [n][3]) of the points q [n][3] at dtype T"""
    q = np.asarray(q, T)
    with np.errstate(invalid="ignore"):
        free = (q > T(-LIMIT)) & (q < T(LIMIT))  # (a NaN fails both)
        q = np.where(np.isnan(q), T(0), np.clip(q, T(-LIMIT), T(LIMIT))).astype(T)
    fl = np.floor(q)
    c = fl.astype(np.int64)
    t = (q - fl).astype(T)
    w = N.fade(t, T).astype(T)
    dw = fade_derivative(t, T, perturb).astype(T)
    W = (T(1) - w, w)
    one, zero = np.ones(len(q), T), np.zeros(len(q), T)
    n = np.zeros(len(q), T)
    dn = np.zeros((len(q), 3), T)
    g = {}
    for a in (0, 1):
        for b in (0, 1):
            for cc in (0, 1):
                h = N.lattice_hash(c[:, 0] + a, c[:, 1] + b, c[:, 2] + cc, seed)
                g[a, b, cc] = N.grad(h, t[:, 0] - T(a), t[:, 1] - T(b), t[:, 2] - T(cc)).astype(T)
                G = np.stack([N.grad(h, one, zero, zero), N.grad(h, zero, one, zero), N.grad(h, zero, zero, one)], axis=1).astype(T)
                weight = (W[a][:, 0] * W[b][:, 1] * W[cc][:, 2]).astype(T)
                n = (n + weight * g[a, b, cc]).astype(T)
                dn = (dn + weight[:, None] * G).astype(T)
    for j in (0, 1):
        for k in (0, 1):
            dn[:, 0] += dw[:, 0] * W[j][:, 1] * W[k][:, 2] * (g[1, j, k] - g[0, j, k])
            dn[:, 1] += dw[:, 1] * W[j][:, 0] * W[k][:, 2] * (g[j, 1, k] - g[j, 0, k])
            dn[:, 2] += dw[:, 2] * W[j][:, 0] * W[k][:, 1] * (g[j, k, 1] - g[j, k, 0])
    return n, np.where(free, dn, T(0)).astype(T)


def value_gradient(p, style, scale, octaves, seed, axis, distortion, T, perturb=()):
    """grad s [n][3] with respect to the world point, of the texture's scalar at the points p [n][3]; scale, seed and distortion:
    one each or one per point"""
    p = np.asarray(p, T)
    scale, distortion = np.asarray(scale, np.float32).astype(T), np.asarray(distortion, np.float32).astype(T)
    q = (scale[..., None] * p).astype(T)
    total = np.zeros(len(p), T)
    gsum = np.zeros((len(p), 3), T)
    amp = T(1)
    for o in range(int(octaves)):
        n, dn = noise_gradient(q, (np.asarray(seed, np.int64) + o) & 0xFFFFFFFF, T, perturb)
        total = (total + amp * (n if style == N.FBM else np.abs(n))).astype(T)
        gsum = (gsum + (dn if style == N.FBM else np.sign(n)[:, None] * dn)).astype(T)
        amp = T(amp * T(0.5))
        q = (q * T(2)).astype(T)
    gsum = (scale[..., None] * gsum).astype(T)
    if style == N.FBM:
        v = T(0.5) + T(0.5) * total
        return np.where(((v > 0) & (v < 1))[:, None], T(0.5) * gsum, T(0)).astype(T)
    if style == N.TURBULENCE:
        return np.where((total < 1)[:, None], gsum, T(0)).astype(T)
    e = np.zeros((len(p), 3), T)
    e[:, int(axis)] = scale
    with np.errstate(invalid="ignore"):
        c = T(0.5) * np.cos(scale * p[:, int(axis)] + distortion * total)
        return (c[:, None] * (e + distortion[..., None] * gsum)).astype(T)


def gradient_of(p, par, T, perturb=()):
    """grad s of the noise texture with the parameters par (the dict of Scene.noise())"""
    return value_gradient(p, N.STYLES[par["style"]], np.float32(par["scale"]), par["octaves"], par["seed"], N.AXES[par["axis"]],
                          np.float32(par["distortion"]), T, perturb)


def bump(n, g, d, front, k, G, T, perturb=()):
    """(n' where the rule accepts it, else n; accepted [n] bool).  k: the strength, one or one per vertex"""
    k = np.asarray(k, np.float32).astype(T)
    sigma = np.ones(len(n), T) if "bump_back_unsigned" in perturb else np.where(front, T(1), T(-1))
    Gt = G if "bump_full_gradient" in perturb else G - _dot(G, n)[:, None] * n
    with np.errstate(all="ignore"):
        b = n - (sigma * k)[:, None] * Gt
        nb = b / np.sqrt(_dot(b, b))[:, None]
        ok = np.isfinite(nb).all(axis=1) & (_dot(nb, g) > 0) & (_dot(nb, -_unit(d)) > 0)
    return np.where(ok[:, None], nb, n).astype(T), ok
