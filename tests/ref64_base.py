"""What ref64.py and its model files (ref64_*.py) share: the three vector helpers, the primitive type codes and the two record
accessors that more than one of them reads.  It imports nothing of them, so a model file can take these without importing ref64."""
import numpy as np

SPHERE, XY_RECT, XZ_RECT, YZ_RECT, CYLINDER, TRIANGLE, QUAD = range(7)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _unit(a):
    return a / np.sqrt(_dot(a, a))[:, None]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _rect_axes(ptype):
    # (plane axis, first in-plane axis, second in-plane axis): xy_rect z = k, xz_rect y = k, yz_rect x = k
    return {XY_RECT: (2, 0, 1), XZ_RECT: (1, 0, 2), YZ_RECT: (0, 1, 2)}[int(ptype)]


def _affine(m, T):
    m = np.asarray(m, T).reshape(3, 4)
    return m[:, :3], m[:, 3]
