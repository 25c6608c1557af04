"""The noise textures of DESIGN 7o (fBm, turbulence, marble over hashed-lattice gradient noise) for ref64.py, in NumPy at a
floating type of the caller's choice.

Test infrastructure only, written from the model's text (include/rtmi.h), not from csrc/rt_noise.h:
    hash(i, j, k; s)  mod 2^32:  h = s ^ i 0x8DA6B343 ^ j 0xD8163841 ^ k 0xCB1AB31F;  h ^= h >> 16;  h *= 0x85EBCA6B;
                                 h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16
    grad(h, x, y, z)  g = h >> 28:  u = g < 8 ? x : y;  v = g < 4 ? y : (g in (12, 14) ? x : z);  (g & 1 ? -u : u) + (g & 2 ? -v : v)
    n(q, s)           q clamped to +-2^30 (NaN -> 0), c = floor(q), t = q - c, the eight corners' gradients at t - corner, faded by
                      w(t) = t^3 (t (6 t - 15) + 10) and interpolated along x, then y, then z as a + w (b - a)
    S = sum_o 2^-o n(2^o f p, seed + o),  A = the same over |n|
    fbm: clamp(0.5 + 0.5 S, 0, 1)   turbulence: min(1, A)   marble: 0.5 + 0.5 sin(f p[axis] + D A)   colour: c0 + s (c1 - c0)
Everything runs at dtype T with plain (unfused) operations; the lattice coordinates and the hash are integers at any T.

This file holds the model alone and imports nothing of ref64: ref64.texture_value calls colour() for a texture of type NOISE, with
the parameters RefScene read from Scene.noise(texture), and ref64.tally() counts the noise vertices.

Deliberate mistakes (names in `perturb`, as ref64.trace takes them):
  noise_cubic_fade   the fade 3 t^2 - 2 t^3 in place of the quintic
  noise_same_seed    every octave on the texture's seed (no + o)
  noise_wrong_axis   marble's phase along the next axis (x -> y -> z -> x); fbm and turbulence: the octaves' amplitudes not
                     halved, so that the name never does nothing
"""
import numpy as np

NOISE = 3
FBM, TURBULENCE, MARBLE = range(3)
STYLES = {"fbm": FBM, "turbulence": TURBULENCE, "marble": MARBLE}
AXES = {"x": 0, "y": 1, "z": 2}
PERTURBATIONS = ("noise_cubic_fade", "noise_same_seed", "noise_wrong_axis")
KX, KY, KZ = np.uint32(0x8DA6B343), np.uint32(0xD8163841), np.uint32(0xCB1AB31F)


def lattice_hash(i, j, k, seed):
    """uint32 hash of int lattice coordinates (arrays or scalars, any integer type: taken mod 2^32) and a uint32 seed"""
    u = lambda a: (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = u(seed) ^ (u(i) * KX) ^ (u(j) * KY) ^ (u(k) * KZ)
        h = h ^ (h >> np.uint32(16))
        h = h * np.uint32(0x85EBCA6B)
        h = h ^ (h >> np.uint32(13))
        h = h * np.uint32(0xC2B2AE35)
        h = h ^ (h >> np.uint32(16))
    return h


def grad(h, x, y, z):
    g = h >> np.uint32(28)
    u = np.where(g < 8, x, y)
    v = np.where(g < 4, y, np.where((g == 12) | (g == 14), x, z))
    return np.where(g & 1, -u, u) + np.where(g & 2, -v, v)


def fade(t, T, perturb=()):
    if "noise_cubic_fade" in perturb:
        return t * t * (T(3) - T(2) * t)
    return t * t * t * (t * (t * T(6) - T(15)) + T(10))


def noise(q, seed, T, perturb=()):
    """n(q, seed) of the points q [n][3] at dtype T"""
    q = np.asarray(q, T)
    with np.errstate(invalid="ignore"):
        q = np.where(np.isnan(q), T(0), np.clip(q, T(-2.0 ** 30), T(2.0 ** 30))).astype(T)
    fl = np.floor(q)
    c = fl.astype(np.int64)
    t = (q - fl).astype(T)
    w = fade(t, T, perturb).astype(T)
    corner = {}
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                h = lattice_hash(c[:, 0] + dx, c[:, 1] + dy, c[:, 2] + dz, seed)
                corner[dx, dy, dz] = grad(h, t[:, 0] - T(dx), t[:, 1] - T(dy), t[:, 2] - T(dz)).astype(T)
    lerp = lambda a, b, w: (a + w * (b - a)).astype(T)
    x = {(dy, dz): lerp(corner[0, dy, dz], corner[1, dy, dz], w[:, 0]) for dy in (0, 1) for dz in (0, 1)}
    y = {dz: lerp(x[0, dz], x[1, dz], w[:, 1]) for dz in (0, 1)}
    return lerp(y[0], y[1], w[:, 2])


def value(p, style, scale, octaves, seed, axis, distortion, T, perturb=()):
    """the texture's scalar s in [0, 1] at the points p [n][3]; scale, seed and distortion: one each or one per point"""
    p = np.asarray(p, T)
    scale, distortion = np.asarray(scale, np.float32).astype(T), np.asarray(distortion, np.float32).astype(T)
    q = (scale[..., None] * p).astype(T)
    total = np.zeros(len(p), T)
    amp = T(1)
    for o in range(int(octaves)):
        n = noise(q, (np.asarray(seed, np.int64) + (0 if "noise_same_seed" in perturb else o)) & 0xFFFFFFFF, T, perturb)
        total = (total + amp * (n if style == FBM else np.abs(n))).astype(T)
        if not ("noise_wrong_axis" in perturb and style != MARBLE):
            amp = T(amp * T(0.5))
        q = (q * T(2)).astype(T)
    if style == FBM:
        return np.clip(T(0.5) + T(0.5) * total, T(0), T(1)).astype(T)
    if style == TURBULENCE:
        return np.minimum(T(1), total).astype(T)
    a = (int(axis) + 1) % 3 if "noise_wrong_axis" in perturb else int(axis)
    return (T(0.5) + T(0.5) * np.sin(scale * p[:, a] + distortion * total)).astype(T)


def colour(p, c0, c1, par, T, perturb=()):
    """c0 + s (c1 - c0) per channel; par: the dict of Scene.noise()"""
    s = value(p, STYLES[par["style"]], np.float32(par["scale"]), par["octaves"], par["seed"], AXES[par["axis"]], np.float32(par["distortion"]),
              T, perturb)
    c0, c1 = np.asarray(c0, np.float32).astype(T), np.asarray(c1, np.float32).astype(T)
    return (c0[None, :] + s[:, None] * (c1 - c0)[None, :]).astype(T)
