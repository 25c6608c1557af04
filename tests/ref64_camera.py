"""The fp64 statement of the camera projections: orthographic, panoramic and fisheye, built around ref64.trace()
without editing it.

trace()'s camera block reads S.cam through broadcasting expressions,
    o = origin + off,   d = lower_left + s horizontal + t vertical - origin - off,   off = lens_radius (lx u + ly v),
so a view of the scene whose `origin` and `lower_left` are PER-SAMPLE arrays -- the sample's pinhole origin o and its focus
point o + D -- with zero `horizontal` and `vertical` makes trace() start every sample on (o + off, D - off): the lens rule of
every projection.  view() computes o and D from the sample's first two words (the jitter, as trace() draws it) and returns that
view; samples of a fisheye outside the image circle get a ray like any other and their radiance is zeroed afterwards (trace()
and reference() below), which is what "no path" means for the frame.  The order and count of the draws do not depend on the
projection, so the lens draws and everything after them stay trace()'s.

The model (include/rtmi.h, rt_scene_set_projection), with u, v, w the camera frame, f = -w, a the aspect ratio, fd the focus
distance, all from Scene.get_camera()'s fp32 record and evaluated in fp64 (T) from there:
    orthographic  o = lookfrom + (s - 1/2) h a u + (t - 1/2) h v,  D = fd f
    panoramic     phi = (s - 1/2) hfov, psi = (t - 1/2) vfov,  D = fd (cos psi (cos phi f + sin phi u) + sin psi v),  o = lookfrom
    fisheye       (px, py) = ((2s - 1) max(a, 1), (2t - 1) max(1 / a, 1)), r = |(px, py)|, theta = r fov / 2,
                  D = fd (cos theta f + (sin theta / r)(px u + py v)),  o = lookfrom;  r > 1: no path

PERTURBATIONS, the deliberate mistakes (names in `perturb`, beside ref64.trace's own, which pass through):
    pano_mirrored            sin(phi) negated: the panorama as seen from outside
    pano_t_from_top          psi = (1/2 - t) vfov: the rows counted from the top
    fisheye_equisolid        theta = 2 asin(r sin(fov / 4)): the equisolid mapping with the same rim
    fisheye_circle_on_width  the image circle inscribed in the LONGER side: (px, py) = ((2s - 1) min(a, 1), (2t - 1) min(1 / a, 1))
    lens_keeps_direction     the lens ray (o + off, D): the direction not reduced by the offset, so nothing is in focus
    ortho_fixed_origin       every orthographic ray starts at lookfrom
"""
import copy

import numpy as np

import ref64 as R

PERTURBATIONS = ("pano_mirrored", "pano_t_from_top", "fisheye_equisolid", "fisheye_circle_on_width", "lens_keeps_direction",
                 "ortho_fixed_origin")
PERSPECTIVE, ORTHOGRAPHIC, PANORAMIC, FISHEYE = "perspective", "orthographic", "panoramic", "fisheye"


class Frame:
    """the camera frame and the projection of a product Scene, as fp64 values of its fp32 record"""

    def __init__(self, sc):
        cam = sc.get_camera()
        f64 = lambda k: np.array(getattr(cam, k)[:], np.float32).astype(np.float64)
        self.lookfrom, self.u, self.v, self.f = f64("origin"), f64("u"), f64("v"), -f64("w")
        self.fd, self.aspect, self.lens_radius = float(cam.focus_dist), float(cam.aspect), float(cam.lens_radius)
        self.kind, self.params = sc.projection


def pinhole(F, s, t, perturb=(), T=np.float64):
    """(o [N][3], D [N][3], seen [N]) of the projection F at the film points (s, t); perspective is not stated here"""
    s, t = np.asarray(s, T), np.asarray(t, T)
    u, v, f, lookfrom = (x.astype(T) for x in (F.u, F.v, F.f, F.lookfrom))
    a, fd, half = T(F.aspect), T(F.fd), T(0.5)
    o = np.broadcast_to(lookfrom, s.shape + (3,)).copy()
    seen = np.ones(s.shape, bool)
    if F.kind == ORTHOGRAPHIC:
        h = T(F.params[0])
        if "ortho_fixed_origin" not in perturb:
            o = lookfrom + ((s - half) * h * a)[..., None] * u + ((t - half) * h)[..., None] * v
        D = np.broadcast_to(fd * f, s.shape + (3,)).copy()
    elif F.kind == PANORAMIC:
        hfov, vfov = (T(np.deg2rad(x)) for x in F.params)
        phi = (s - half) * hfov
        psi = ((half - t) if "pano_t_from_top" in perturb else (t - half)) * vfov
        sp = -np.sin(phi) if "pano_mirrored" in perturb else np.sin(phi)
        D = fd * (np.cos(psi)[..., None] * (np.cos(phi)[..., None] * f + sp[..., None] * u) + np.sin(psi)[..., None] * v)
    elif F.kind == FISHEYE:
        fov = T(np.deg2rad(F.params[0]))
        mx, my = max(a, T(1)), max(T(1) / a, T(1))
        if "fisheye_circle_on_width" in perturb:
            mx, my = (T(1), T(1) / a) if a >= 1 else (a, T(1))
        px, py = (2 * s - 1) * mx, (2 * t - 1) * my
        r = np.sqrt(px * px + py * py)
        seen = r <= 1
        theta = 2 * np.arcsin(np.minimum(r, 1) * np.sin(fov / 4)) if "fisheye_equisolid" in perturb else r * fov / 2
        k = np.where(r > 0, np.sin(theta) / np.where(r > 0, r, 1), 0)
        D = fd * (np.cos(theta)[..., None] * f + (k * px)[..., None] * u + (k * py)[..., None] * v)
    else:
        raise ValueError(f"no projection {F.kind!r} here")
    return o, D, seen


def film_points(S, words, T=np.float64, first_pixel=0):
    """(s, t) of every sample, from its first two draws, as trace() forms them"""
    D = R._Draws(words, T)
    everyone = np.arange(len(words))
    pix = (first_pixel + everyone) % (S.width * S.height)
    s = ((pix % S.width).astype(T) + D.next(everyone)) / T(S.width - 1)
    t = ((pix // S.width).astype(T) + D.next(everyone)) / T(S.height - 1)
    return s, t, D


def view(S, F, words, perturb=(), T=np.float64):
    """(the view of RefScene S that makes trace() start sample k of `words` on projection F's ray, seen [N])"""
    s, t, D = film_points(S, words, T)
    o, Dv, seen = pinhole(F, s, t, perturb, T)
    focus = o + Dv
    if "lens_keeps_direction" in perturb and S.flags & 2:
        # trace() subtracts off from the direction: hand it a focus point that has it added (the same draws, from a cursor of our own)
        lens = T(S.lens_radius) * D.reject(np.arange(len(words)), 2, T)
        focus = focus + lens[:, :1] * S.cam["u"].astype(T) + lens[:, 1:2] * S.cam["v"].astype(T)
    V = copy.copy(S)
    zero = np.zeros(3, np.float64)
    V.cam = dict(S.cam, origin=o, lower_left=focus, horizontal=zero, vertical=zero)
    return V, seen


def trace(S, F, words, dtype=np.float64, perturb=(), shutter=None, probe=None, log=None):
    """ref64.trace() through projection F: (rgb, signature, draws); a fisheye sample outside the circle is zero and its
    signature empty (every column NONE, the draw count among them: no sample with a path has that row)"""
    V, seen = view(S, F, words, perturb, dtype)
    rgb, sig, draws = R.trace(V, words, dtype=dtype, perturb=tuple(p for p in perturb if p not in PERTURBATIONS), shutter=shutter,
                              probe=probe, log=log)
    rgb = np.where(seen[:, None], rgb, 0)
    return rgb, np.where(seen[:, None], sig, R.NONE), draws


def reference(S, F, words, shutter=None):
    """ref64.reference() through projection F: the fp64 radiance, the samples whose fp32 run took the same branches (the side
    of r = 1 among them), the draws, and the tally with the camera's own figures (tally["camera"], film_tally)"""
    log = R.new_log()
    rgb, sig64, draws = trace(S, F, words, shutter=shutter, log=log)
    _, sig32, _ = trace(S, F, words, dtype=np.float32, shutter=shutter)
    tally = R.tally(sig64, S, log)
    tally["camera"] = film_tally(S, F, words)
    return rgb, R.same_signature(sig64, sig32), draws, tally


def film_tally(S, F, words):
    """where the samples fall on the film: what camera_scenes.check_contents reads"""
    s, t, _ = film_points(S, words)
    out = dict(samples=len(words))
    if F.kind == FISHEYE:
        a = F.aspect
        r = np.hypot((2 * s - 1) * max(a, 1.0), (2 * t - 1) * max(1.0 / a, 1.0))
        out.update(inside=int((r <= 1).sum()), outside=int((r > 1).sum()), centre=int((r < 0.05).sum()))
    if F.kind == PANORAMIC:
        phi, psi = np.rad2deg((s - 0.5) * np.deg2rad(F.params[0])), np.rad2deg((t - 0.5) * np.deg2rad(F.params[1]))
        out.update(north=int((psi > 88).sum()), south=int((psi < -88).sum()), seam_left=int((phi < -178).sum()), seam_right=int((phi > 178).sum()))
    return out
