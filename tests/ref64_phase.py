"""The Henyey-Greenstein phase function of anisotropic media for ref64.trace(): the distribution function, its
inverse, the density, the frame and a vertex's direction, in NumPy at a floating type of the caller's choice.  Test
infrastructure only.  A model file: it holds no loop and imports nothing of ref64.py (ref64_base.py holds what they share);
ref64.trace()'s medium vertex block calls hg_direction() where the stored g is not 0 and ref64.phase_density() calls
hg_density() for a light sample.

From the definitions (include/rtmi.h): a vertex in a medium with g != 0 takes no attempt of the rejection loop but two
uniforms u1, u2.  The polar angle t about the unit direction of travel w has the distribution function
    F(cos t) = (1 - g^2) / (2 g) (1 / sqrt(1 + g^2 - 2 g cos t) - 1 / (1 + g)),
inverted in closed form at u1; the azimuth is 2 pi u2, measured in the frame of Duff et al. 2017 about w (the frame the product's
documents name: the azimuth of a sample means nothing without it).  Angles through libm's arccos / sin / cos, no fused operation.

Deliberate mistakes (names of ref64.trace()'s `perturb`), for the tests that show the comparison can fail:
    "phase_isotropic"       g ignored: every medium vertex runs the rejection loop
    "phase_backward"        g negated
    "phase_swapped_draws"   u2 drives the polar angle, u1 the azimuth
"""
import numpy as np

PERTURBATIONS = ("phase_isotropic", "phase_backward", "phase_swapped_draws")


def stored_g(sc):
    """the asymmetries a product scene holds, in list order"""
    return np.array([sc.medium_phase(i) for i in range(len(sc.media()))], np.float32)


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
