"""Camera projections (orthographic, panoramic and fisheye cameras) without a GPU:
  1. the interface -- Python, C (through it), JSON -- with every refusal and the round trip; the projection survives the other
     camera setters;
  2. a perspective scene is untouched: every shipped scene packs the bytes of the commit before the feature
     (tests/golden/camera_parent_tables.json, tools/make_camera_golden.py), a scene without the key is written as before, and
     a projection set and taken back packs the same bytes again;
  3. rt_camera_ray against closed forms;
  4. rt_camera_ray against the fp64 statement (ref64_camera.pinhole + the lens rule) on 10^5 random (s, t, lx, ly) per
     projection, within a bound derived from the fp32 operation sequence of csrc/rt_camera.h;
  5. the cases of camera_scenes.py hold the contents they are there for, and each deliberate mistake of ref64_camera changes
     the reference's samples on its case.
test_gpu_camera.py holds the kernels to that reference."""
import hashlib
import json
import os

import numpy as np
import pytest

import camera_scenes as CS
import nee_scenes as NS
import ref64 as R
import ref64_camera as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
RT_ERR_ARG, RT_ERR_SCENE = 1, 4
E = 2.0 ** -24  # the unit roundoff of fp32: one operation's relative error, and half an ulp of a value in [1, 2)


@pytest.fixture(scope="module")
def rtmi():
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


def small(rtmi, blur=False, aperture=0.0):
    """a 160 x 90 frame whose focus distance (9.96) exceeds every other length of the camera: |lookfrom|, h a, the lens radius"""
    sc = rtmi.Scene.new(160, 90, 1, 4)
    sc.set_background((0.1, 0.1, 0.1), sky_gradient=False, defocus_blur=blur)
    sc.camera((1.0, 2.0, 3.0), (-3.0, 0.5, -6.0), (0.1, 1.0, 0.0), 35.0, 0.0, aperture, 0.0)
    sc.sphere((0, 0, 0), 1.0, sc.lambertian((0.5, 0.5, 0.5)))
    return sc


PROJECTIONS = (("orthographic", (3.0,)), ("panoramic", (360.0, 180.0)), ("panoramic", (200.0, 90.0)), ("fisheye", (180.0,)),
               ("fisheye", (360.0,)))


# ------------------------------------------------------------------------------------------------------------ 1. the interface
def test_set_get_and_the_defaults(rtmi):
    sc = small(rtmi)
    assert sc.projection == ("perspective", ())
    for kind, params in PROJECTIONS:
        sc.set_projection(kind, *params)
        assert sc.projection == (kind, params)
    sc.set_projection("panoramic")
    assert sc.projection == ("panoramic", (360.0, 180.0))
    sc.set_projection("fisheye")
    assert sc.projection == ("fisheye", (180.0,))
    sc.set_projection(1, 2.5)  # (by number)
    assert sc.projection == ("orthographic", (2.5,))
    # the other camera setters keep it
    sc.camera((0, 1, 5), (0, 1, 0), (0, 1, 0), 40.0)
    sc.override(64, 36, 2, 3)
    assert sc.projection == ("orthographic", (2.5,)) and sc.clone().projection == ("orthographic", (2.5,))
    sc.set_projection("perspective")
    assert sc.projection == ("perspective", ())


@pytest.mark.parametrize("kind,params", [
    ("orthographic", ()), ("orthographic", (0.0,)), ("orthographic", (-1.0,)), ("orthographic", (float("nan"),)),
    ("orthographic", (float("inf"),)), ("orthographic", (1e-50,)),
    ("panoramic", (0.0, 90.0)), ("panoramic", (361.0, 90.0)), ("panoramic", (360.0, 0.0)), ("panoramic", (360.0, 180.5)),
    ("panoramic", (float("nan"), 90.0)), ("panoramic", (90.0, float("inf"))), ("panoramic", (-90.0, 90.0)),
    ("fisheye", (0.0,)), ("fisheye", (360.5,)), ("fisheye", (float("nan"),)), ("fisheye", (-180.0,)),
    (4, (1.0,)), (-1, ())])
def test_bad_parameters_are_refused_and_change_nothing(rtmi, kind, params):
    sc = small(rtmi)
    sc.set_projection("fisheye", 200.0)
    with pytest.raises(rtmi.RtmiError) as e:
        sc.set_projection(kind, *params)
    assert e.value.status == RT_ERR_ARG, str(e.value)
    assert sc.projection == ("fisheye", (200.0,))


def test_json_round_trips_every_projection(rtmi):
    sc = small(rtmi)
    plain = sc.to_json()
    assert "projection" not in plain  # (a scene without the key is written as before)
    for kind, params in PROJECTIONS:
        sc.set_projection(kind, *params)
        text = sc.to_json()
        assert json.loads(text)["camera"]["projection"]["type"] == kind
        back = rtmi.Scene.parse(text)
        assert back.projection == (kind, params) and back.to_json() == text
        assert back.table_image().tobytes() == sc.table_image().tobytes()
    sc.set_projection("perspective")
    assert sc.to_json() == plain and rtmi.Scene.parse(plain).projection == ("perspective", ())
    # the defaults of the file format
    doc = json.loads(plain)
    for given, want in (({"type": "panoramic"}, ("panoramic", (360.0, 180.0))), ({"type": "panoramic", "vfov": 90}, ("panoramic", (360.0, 90.0))),
                        ({"type": "fisheye"}, ("fisheye", (180.0,))), ({"type": "perspective"}, ("perspective", ())),
                        ({"type": "orthographic", "height": 4}, ("orthographic", (4.0,)))):
        doc["camera"]["projection"] = given
        assert rtmi.Scene.parse(json.dumps(doc)).projection == want


@pytest.mark.parametrize("projection", [
    "fisheye", 3, {}, {"type": 3}, {"type": "cubemap"}, {"type": "orthographic"}, {"type": "orthographic", "height": 0},
    {"type": "orthographic", "height": "4"}, {"type": "orthographic", "height": 4, "fov": 90}, {"type": "perspective", "height": 4},
    {"type": "panoramic", "hfov": 400}, {"type": "panoramic", "vfov": 181}, {"type": "panoramic", "fov": 90},
    {"type": "fisheye", "fov": 0}, {"type": "fisheye", "fov": 361}, {"type": "fisheye", "hfov": 180}, {"type": "fisheye", "fov": 180, "lens": 1}])
def test_json_refuses_bad_projections(rtmi, projection):
    doc = json.loads(small(rtmi).to_json())
    doc["camera"]["projection"] = projection
    with pytest.raises(rtmi.RtmiError) as e:
        rtmi.Scene.parse(json.dumps(doc))
    assert e.value.status == RT_ERR_SCENE, str(e.value)


# ------------------------------------------------------------------------------------------------------------ 2. perspective stays
def shipped():
    with open(os.path.join(ROOT, "tests", "golden", "camera_parent_tables.json")) as fh:
        return json.load(fh)


def test_the_golden_file_lists_every_scene_the_parent_shipped():
    assert len(shipped()) == 16 and "three_sphere.json" in shipped()


@pytest.mark.parametrize("scene_file", sorted(shipped()))
def test_shipped_perspective_scenes_pack_the_parents_bytes(rtmi, scene_file):
    want = shipped()[scene_file]
    sc = rtmi.Scene.load(os.path.join(PKG, "scenes", scene_file))
    assert sc.projection == ("perspective", ())
    info = sc.table_info()
    assert {k: int(getattr(info, k)) for k in want["info"]} == want["info"]
    assert hashlib.sha256(sc.table_image().tobytes()).hexdigest() == want["sha256"]
    # a projection set and taken back: the same bytes again; while set, the camera records alone may differ in a general layout
    sc.set_projection("fisheye", 180.0)
    assert hashlib.sha256(sc.table_image().tobytes()).hexdigest() != want["sha256"]
    sc.set_projection("perspective")
    assert hashlib.sha256(sc.table_image().tobytes()).hexdigest() == want["sha256"]


def test_a_projection_puts_a_sphere_only_scene_on_a_general_layout(rtmi):
    """the compact layouts' burst slab is the perspective camera's: a non-perspective scene gets the wide tables"""
    sc = small(rtmi)
    assert sc.table_info().kernel_variant in (2, 6)
    sc.set_projection("panoramic")
    assert sc.table_info().kernel_variant in (16, 36, 44)


# ------------------------------------------------------------------------------------------------------------ 3. closed forms
def frame_of(sc):
    F = RC.Frame(sc)
    return F, F.lookfrom, F.u, F.v, F.f, F.fd


def unit(d):
    d = np.asarray(d, np.float64)
    return d / np.linalg.norm(d)


def test_the_centre_looks_along_f_in_every_projection(rtmi):
    sc = small(rtmi)
    for kind, params in PROJECTIONS + (("perspective", ()),):
        sc.set_projection(kind, *params)
        F, lookfrom, u, v, f, fd = frame_of(sc)
        o, d, ok = sc.camera_ray(0.5, 0.5)
        assert ok and np.abs(o - lookfrom).max() <= 4 * E * 4 and np.abs(d / fd - f).max() <= 8 * E, (kind, o, d)


def test_orthographic_rays_are_parallel_and_span_the_film(rtmi):
    sc = small(rtmi)
    sc.set_projection("orthographic", 3.0)
    F, lookfrom, u, v, f, fd = frame_of(sc)
    rays = {(s, t): sc.camera_ray(s, t) for s in (0.0, 0.3, 1.0) for t in (0.0, 0.8, 1.0)}
    for (s, t), (o, d, ok) in rays.items():
        assert ok and d.tobytes() == rays[(0.0, 0.0)][1].tobytes()  # (one direction)
        want = lookfrom + (s - 0.5) * 3.0 * F.aspect * u + (t - 0.5) * 3.0 * v
        assert np.abs(o - want).max() <= 16 * E * 9.0, (s, t, o, want)
    across, up = rays[(1.0, 0.0)][0] - rays[(0.0, 0.0)][0], rays[(0.0, 1.0)][0] - rays[(0.0, 0.0)][0]
    assert abs(np.linalg.norm(across) - 3.0 * F.aspect) <= 1e-5 and abs(np.linalg.norm(up) - 3.0) <= 1e-5
    assert abs(np.dot(unit(across), u) - 1) <= 1e-6 and abs(np.dot(unit(up), v) - 1) <= 1e-6


def test_panoramic_edges_look_backwards_and_at_the_poles(rtmi):
    sc = small(rtmi)
    sc.set_projection("panoramic")
    F, lookfrom, u, v, f, fd = frame_of(sc)
    for s in (0.0, 1.0):
        o, d, ok = sc.camera_ray(s, 0.5)
        assert ok and np.abs(d / fd + f).max() <= 1e-6, (s, d)
    assert np.abs(sc.camera_ray(0.5, 0.0)[1] / fd + v).max() <= 1e-6   # t = 0: straight down
    assert np.abs(sc.camera_ray(0.5, 1.0)[1] / fd - v).max() <= 1e-6   # t = 1: straight up
    assert np.abs(sc.camera_ray(0.75, 0.5)[1] / fd - u).max() <= 1e-6  # increasing s turns right


def test_fisheye_rim_is_perpendicular_and_outside_is_invalid(rtmi):
    sc = small(rtmi)
    sc.set_projection("fisheye", 180.0)
    F, lookfrom, u, v, f, fd = frame_of(sc)
    a = F.aspect  # 16 / 9: the circle spans the frame's height, t = 0 and t = 1 lie on it (r = 1)
    for t, side in ((0.0, -1.0), (1.0, 1.0)):
        o, d, ok = sc.camera_ray(0.5, t)
        assert ok and abs(np.dot(d / fd, f)) <= 1e-6 and np.abs(d / fd - side * v).max() <= 1e-6, (t, d)
    o, d, ok = sc.camera_ray(0.5 + 0.5 / a, 0.5)  # r = 1 along the width
    assert ok and np.abs(d / fd - u).max() <= 1e-6
    for s, t in ((0.5 + 0.51 / a, 0.5), (0.0, 0.5), (1.0, 1.0), (0.9, 0.1)):
        o, d, ok = sc.camera_ray(s, t)
        assert not ok and not o.any() and not d.any()
        assert not rtmi.ray_valid((o, d))  # (what --pick reports as the invalid-ray case)


def test_every_lens_ray_of_a_sample_passes_through_the_focus_point(rtmi):
    sc = small(rtmi, blur=True, aperture=0.5)
    rng = np.random.default_rng(11)
    for kind, params in PROJECTIONS + (("perspective", ()),):
        sc.set_projection(kind, *params)
        fd = RC.Frame(sc).fd
        for s, t in ((0.5, 0.5), (0.45, 0.3), (0.6, 0.9)):
            o0, d0, ok = sc.camera_ray(s, t)
            assert ok
            for lx, ly in rng.uniform(-0.7, 0.7, (6, 2)):
                o, d, ok = sc.camera_ray(s, t, lx, ly)
                assert ok and np.abs(o - o0).max() > 1e-3  # (the lens acts)
                assert np.abs((o.astype(np.float64) + d) - (o0.astype(np.float64) + d0)).max() <= 8 * E * fd, (kind, s, t)
    sc.set_background((0.1, 0.1, 0.1), sky_gradient=False, defocus_blur=False)  # without the flag the lens sample does nothing, as in a render
    assert sc.camera_ray(0.4, 0.4, 0.5, 0.5)[0].tobytes() == sc.camera_ray(0.4, 0.4)[0].tobytes()


# ------------------------------------------------------------------------------------------------------------ 4. against fp64
# The bound, from the operation sequence of csrc/rt_camera.h (e = 2^-24: the relative error of one fp32 operation; a value
# below 1 has ulp <= e, so "sincosf at 2 ulp" is <= 4 e absolute on a sine or cosine).  Both sides start from the same fp32 s, t,
# lx, ly and the same fp32 frame (u, v, f, lookfrom, fd: Scene.get_camera's record is what the packer rounds), so only the
# records derived in fp64 and rounded once differ from the reference's own values: by one e each.  Errors are stated per
# component of the unit direction d^ (|components of u, v, f| <= 1), the result is then scaled by fd; scale = max(fd, every
# other length of the camera), which in small() is fd = |D|.
#   lens      off = fma(u, lr lx, v (lr ly)): 4 e lr;  D - off and o + off: one rounding each, e scale           -> 6 e, both
#   ortho     o = fma(t, ver, fma(s, hor, ll)): ll, hor, ver rounded once (3 e), a and u as fp32 in the reference (2 e), s and
#             t up to 1.04 (x 1.04), two fma roundings (2 e): 8 e;  D = fd f rounded once against fd x f: 3 e       -> 14 e, 9 e
#   pano      phi = (s - 1/2) hfov: subtraction, product, hfov rounded once: 3 e |phi| <= 3 e x 3.4 = 10.2 e; sin, cos of it:
#             + 4 e = 14.2 e;  psi likewise: 3 e x 1.7 + 4 e = 9.1 e;  kf = cos psi cos phi and ku: 14.2 + 9.1 + 1 = 24.3 e,
#             kv: 9.1 e;  d^ = fma(kv, v, fma(ku, u, kf f)): 24.3 + 24.3 + 9.1 + 3 roundings of values <= 1.8 (5.4 e) = 63.1 e;
#             x fd: + 1 e                                                                                           -> 6 e, 71 e
#   fisheye   px = fma(2, s, -1) mx, mx rounded once: 3 e relative, py likewise;  r^2 = fma(px, px, py py): 8 e relative, r:
#             5 e relative;  theta = r (fov / 2), fov / 2 rounded once: 7 e relative, theta <= pi (fov 360): 22 e;  sin, cos:
#             + 4 e = 26 e;  k px = (sin / r) px with |px / r| <= 1: 26 + (5 + 3 + 2) e = 36 e, k py likewise;  d^: 26 + 36 + 36
#             + 5.4 = 103.4 e;  x fd: + 1 e                                                                         -> 6 e, 111 e
# A sample within 1e-6 of r = 1 may fall on either side in fp32 (r carries 5 e): left out of the comparison, never more than a few.
BOUNDS = {"orthographic": (14, 9), "panoramic": (6, 71), "fisheye": (6, 111)}  # (origin, direction) in units of e x scale


def camera_rays(rtmi, sc, st, lens):
    """rt_camera_ray on n film points through one record (the C call itself: 10^5 calls of Scene.camera_ray would take a minute)"""
    import ctypes
    ray, ok = np.zeros(1, dtype=rtmi.RAY_DTYPE), ctypes.c_int(0)
    p, call, h = ray.ctypes.data_as(ctypes.c_void_p), rtmi._lib.rt_camera_ray, sc._h
    o, d, valid = np.zeros((len(st), 3)), np.zeros((len(st), 3)), np.zeros(len(st), bool)
    for k, (s, t, lx, ly) in enumerate(np.concatenate([st, lens], axis=1).tolist()):
        assert call(h, s, t, lx, ly, p, ctypes.byref(ok)) == 0
        o[k], d[k], valid[k] = ray["origin"][0], ray["dir"][0], ok.value
    return o, d, valid


# (the widest angles of each model, where the bound is attained, with the lens on: the pinhole ray is the lens sample (0, 0))
@pytest.mark.parametrize("kind,params,blur", [("orthographic", (3.0,), True), ("panoramic", (360.0, 180.0), True), ("fisheye", (360.0,), True),
                                              ("fisheye", (180.0,), False)])
def test_camera_ray_agrees_with_the_fp64_statement(rtmi, kind, params, blur):
    sc = small(rtmi, blur=blur, aperture=0.5)
    sc.set_projection(kind, *params)
    F = RC.Frame(sc)
    scale = max(F.fd, np.abs(F.lookfrom).max() + (params[0] * F.aspect if kind == "orthographic" else 0.0) + F.lens_radius)
    assert scale == F.fd
    rng = np.random.default_rng(2024)
    n = 100000
    st = rng.uniform(0.0, 1.0 + 1.0 / 89.0, (n, 2)).astype(np.float32)  # (the jitter reaches past 1: (H - 1 + xi) / (H - 1))
    lens = rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32)
    o64, D64, seen = RC.pinhole(F, st[:, 0].astype(np.float64), st[:, 1].astype(np.float64))
    off = F.lens_radius * (lens[:, :1].astype(np.float64) * F.u + lens[:, 1:].astype(np.float64) * F.v) if blur else 0.0
    want_o, want_d = o64 + off, D64 - off
    got_o, got_d, got_ok = camera_rays(rtmi, sc, st, lens)
    sure = np.ones(n, bool)
    if kind == "fisheye":
        a = F.aspect
        r = np.hypot((2 * st[:, 0].astype(np.float64) - 1) * max(a, 1.0), (2 * st[:, 1].astype(np.float64) - 1) * max(1.0 / a, 1.0))
        sure = np.abs(r - 1) > 1e-6
        assert (~sure).sum() <= 5 and seen.sum() > 20000 and (~seen).sum() > 20000
    assert (got_ok == seen)[sure].all()
    m = sure & seen
    err_o, err_d = np.abs(got_o - want_o)[m].max() / (E * scale), np.abs(got_d - want_d)[m].max() / (E * scale)
    print(f"\n{kind} {params} {'lens' if blur else 'pinhole'}: max error of the origin {err_o:.1f} e, of the direction {err_d:.1f} e "
          f"(bounds {BOUNDS[kind][0]} e, {BOUNDS[kind][1]} e; e = 2^-24 |D|)")
    assert err_o <= BOUNDS[kind][0] and err_d <= BOUNDS[kind][1], (err_o, err_d)
    assert not got_o[~seen & sure].any() and not got_d[~seen & sure].any()


# ------------------------------------------------------------------------------------------------------------ 5. the cases
@pytest.fixture(scope="module")
def words(rtmi):
    made = {}

    def of(name):
        seed = CS.seed_of(name)
        if seed not in made:
            made[seed] = R.uniforms(rtmi, seed, NS.REF_W, NS.REF_H, 0, NS.REF_K, NS.REF_DRAWS)
        return made[seed]
    return of


@pytest.mark.parametrize("name", list(CS.CASES))
def test_the_cases_hold_their_contents(rtmi, words, name):
    """from where the samples fall on the film alone (ref64_camera.film_tally): the reference is not traced for this"""
    sc = CS.scene(rtmi, name)
    S, F = R.RefScene(sc), RC.Frame(sc)
    tally = {"camera": RC.film_tally(S, F, words(name))}
    print("\n   ", name, tally["camera"])
    CS.check_contents(name, tally)
    assert CS.plain_twin(rtmi, name).projection == ("perspective", ()) and sc.projection[0] != "perspective"


@pytest.mark.parametrize("name,mistake", CS.MISTAKES)
def test_a_mistake_changes_the_references_samples(rtmi, words, name, mistake):
    """ref64_camera under each deliberate mistake differs from itself without it on the case's samples: the mistake can show"""
    assert mistake in RC.PERTURBATIONS
    sc = CS.scene(rtmi, name)
    S, F, w = R.RefScene(sc), RC.Frame(sc), words(name)[: 4 * NS.REF_W * NS.REF_H]
    good, _, _ = RC.trace(S, F, w)
    bad, _, _ = RC.trace(S, F, w, perturb=(mistake,))
    share = R.judge(bad, good, np.ones(len(good), bool))["share"]
    print(f"\n{name}, {mistake}: {100 * share:.1f} % of the samples stay within the per-sample tolerance")
    assert share < 0.9, share


def test_a_perspective_view_is_ref64s_own(rtmi, words):
    """the view mechanism itself: handing trace() the perspective camera's rays per sample gives ref64.trace's samples"""
    sc = CS.plain_twin(rtmi, "cam_ortho_blur")
    sc.set_background((0.0, 0.0, 0.0), sky_gradient=True, defocus_blur=True)
    S, w = R.RefScene(sc), words("cam_ortho_blur")[: NS.REF_W * NS.REF_H]
    s, t, _ = RC.film_points(S, w)
    cam = {k: v.astype(np.float64) for k, v in S.cam.items()}
    import copy
    V = copy.copy(S)
    V.cam = dict(S.cam, origin=np.broadcast_to(cam["origin"], (len(w), 3)).copy(),
                 lower_left=cam["lower_left"] + s[:, None] * cam["horizontal"] + t[:, None] * cam["vertical"],
                 horizontal=np.zeros(3), vertical=np.zeros(3))
    a, b = R.trace(S, w)[0], R.trace(V, w)[0]
    assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(a).max())
