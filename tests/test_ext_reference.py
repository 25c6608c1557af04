"""Triangles, the hit record's (u, v) and image textures in the fp64 statement (ref64.py), checked on its own, no GPU:

  1. whole paths of the plain twin of every case of ext_scenes.py against the fp32 checker (gate G2, as
     test_nee_reference.test_plain_path_against_the_checker runs it): the first check of the checker's triangles, (u, v) and image
     lookup on whole paths against an independent statement;
  2. how often the new cases sit on a branch (fp32 against fp64 signatures, at most 1 %), and that each contains what it is named for;
  3. that the per-sample comparison of the GPU test notices a transposed image lookup and the natural pairing of a triangle's
     area weights;
  4. closed forms of hit_uv and of the image lookup at fp64."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import ext_scenes as XS
import nee_scenes as NS
import ref64 as R
import rtcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64


@pytest.fixture(scope="module")
def rtmi():
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    """name -> (uniforms, shutter times or None), computed once per seed"""
    made = {}

    def of(name):
        key = (XS.seed_of(name), XS.family(name) == XS.MOTION)
        if key not in made:
            made[key] = XS.inputs(rtmi, name)
        return made[key]
    return of


# ---- 1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", XS.DISTINCT_TWINS)
def test_plain_twin_against_the_checker(rtmi, inputs, name):
    """gate G2 as DESIGN 2 states it: at least 97 % of the samples within 1e-4; and the draws consumed"""
    K = 4  # 5184 samples per scene
    sc = XS.plain_twin(rtmi, name)
    seed = XS.seed_of(name)
    w = inputs(name)[0][:K * NS.REF_W * NS.REF_H]
    S = R.RefScene(sc, nee=False)
    assert len(S.lights) == 0 and len(S.media) == 0 and len(S.movers) == 0 and S.env is None
    ref, stable, draws, tally = R.reference(S, w)
    floor = NS.REQUIRED_EVENTS * K // NS.REF_K  # 1 % of these samples, as nee_scenes.REQUIRED_EVENTS is of a case's
    assert tally["image_vertices"] >= floor and tally["triangle_vertices"] >= floor, tally
    osc, lib = rtcheck.OracleScene(sc), rtcheck.oracle_lib()
    got, odraws = np.zeros((len(w), 3)), np.zeros(len(w), np.int64)
    out = (C.c_float * 3)()
    for i in range(len(w)):
        pix, cnt = i % (NS.REF_W * NS.REF_H), rtcheck._RtoCounts()
        lib.rto_sample(C.byref(osc.c), seed, pix % NS.REF_W, pix // NS.REF_W, i // (NS.REF_W * NS.REF_H), out, C.byref(cnt))
        got[i], odraws[i] = out[:], cnt.rng_draws
    err = np.abs(got - ref).max(axis=1)
    share = (err < 1e-4).mean()
    agree = stable & (err < 1e-4)
    print(f"\n{name}: checker within 1e-4 of the reference on {100 * share:.2f} % of {len(w)} samples, median error {np.median(err):.2e}; "
          f"draw counts equal on {100 * (draws == odraws).mean():.2f} %; image vertices {tally['image_vertices']}, "
          f"triangle vertices {tally['triangle_vertices']}")
    assert share >= 0.97, share
    assert np.array_equal(draws[agree], odraws[agree])


# ---- 2 -----------------------------------------------------------------------------------------------------------------------
def test_branch_flip_rate_of_every_case(rtmi, inputs):
    """test_nee_reference.test_branch_flip_rate_of_every_scene's cap on the new cases, and their contents"""
    print()
    for name in XS.CASES:
        words, shutter = inputs(name)
        _, stable, draws, tally = R.reference(R.RefScene(XS.scene(rtmi, name)), words, shutter)
        flips = 1 - stable.mean()
        print(f"{name:40s} flips {100 * flips:.3f} %   draws <= {draws.max()}   " + ", ".join(f"{k} {tally[k]}" for k in R.EXT_KEYS if tally[k]))
        XS.check_contents(name, tally, len(words))
        assert draws.max() <= NS.REF_DRAWS
        assert flips <= 0.01, (name, flips)


def test_every_shipped_scene_is_in_scope(rtmi):
    scenes = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes")
    for f in sorted(os.listdir(scenes)):
        sc = rtmi.Scene.load(os.path.join(scenes, f))
        R.RefScene(sc, nee=False)


# ---- 3 -----------------------------------------------------------------------------------------------------------------------
def _verdict(rtmi, inputs, perturb=()):
    """the GPU test's (a) and (c) with the fp32 run of the CORRECT reference standing in for the kernel (test_nee_reference._verdict)"""
    S = R.RefScene(XS.scene(rtmi, XS.RECEIVERS))
    words, _ = inputs(XS.RECEIVERS)
    kernel_like, sig32, _ = R.trace(S, words, dtype=np.float32)
    ref, sig64, _ = R.trace(S, words, perturb=perturb)
    return R.judge(kernel_like, ref, R.same_signature(sig64, sig32))


def test_the_comparison_passes_the_correct_lookup(rtmi, inputs):
    j = _verdict(rtmi, inputs)
    assert j["share"] >= 0.97 and j["bias_ok"], j


@pytest.mark.parametrize("what", ["uv_transposed", "tri_natural_pairing"])
def test_the_comparison_notices_a_wrong_lookup(rtmi, inputs, what):
    j = _verdict(rtmi, inputs, perturb=(what,))
    caught = [k for k, bad in (("(a) agreement", j["share"] < 0.97), ("(c) paired bias", not j["bias_ok"])) if bad]
    print(f"\n{what} on {XS.RECEIVERS}: within {100 * j['share']:.2f} %, bias z {np.round(j['z'], 1)} -> caught by {caught}")
    assert caught, j


# ---- 4 -----------------------------------------------------------------------------------------------------------------------
def _one_of_each(rtmi):
    sc = rtmi.Scene.new(16, 9, 1, 2)
    m = sc.lambertian((0.5, 0.5, 0.5))
    sc.sphere((1.0, 2.0, 3.0), 2.0, m)                                                                   # 0
    sc.xy_rect(-1.0, 3.0, 2.0, 4.0, 0.5, m)                                                              # 1
    sc.xz_rect(-1.0, 3.0, 2.0, 4.0, 0.5, m)                                                              # 2
    sc.yz_rect(-1.0, 3.0, 2.0, 4.0, 0.5, m)                                                              # 3
    sc.cylinder(0.5, -1.0, 3.0, m, translate=(10.0, 0.0, 0.0))                                           # 4 (axis: world z through x = 10)
    sc.triangle((20, 0, 0), (24, 0, 0), (20, 4, 0), m, (0.125, 0.25), (0.875, 0.375), (0.375, 0.75))      # 5 (exact in fp32)
    sc.add_moving_sphere((30.0, 0.0, 0.0), (34.0, 2.0, 0.0), 1.0, m)
    return R.RefScene(sc)


def _uv(S, o, d, t, idx, mov=None, time=None):
    o, d = np.atleast_2d(np.asarray(o, F64)), np.atleast_2d(np.asarray(d, F64))
    n = len(o)
    u, v = R.hit_uv(S, o, d, np.full(n, t, F64), np.full(n, idx), F64, None if mov is None else np.full(n, mov),
                    None if time is None else np.full(n, time, F64))
    return float(u[0]), float(v[0])


def test_hit_uv_closed_forms(rtmi):
    """fp64 evaluations of exact inputs: 1e-12 absolute"""
    S = _one_of_each(rtmi)
    near = lambda got, want: np.allclose(got, want, rtol=0, atol=1e-12)
    c = np.array([1.0, 2.0, 3.0])
    # sphere: rays from the centre, t = radius / |d|.  u = (atan2(-z, x) + pi) / 2 pi, v = acos(-y) / pi
    for n, want in (((1, 0, 0), (0.5, 0.5)), ((0, 0, 1), (0.25, 0.5)), ((0, 0, -1), (0.75, 0.5)), ((0, 1, 0), (0.5, 1.0)), ((0, -1, 0), (0.5, 0.0))):
        assert near(_uv(S, c, n, 2.0, 0), want), n
    # the seam lies at -x: u = 1 just on the -z side of it... (atan2(-z, x): z > 0 gives -pi, u = 0; z < 0 gives +pi, u = 1)
    eps = 1e-9
    lo, hi = _uv(S, c, (-1, 0, eps), 2.0, 0)[0], _uv(S, c, (-1, 0, -eps), 2.0, 0)[0]
    assert lo < 1e-9 and hi > 1 - 1e-9, (lo, hi)
    # a mover: the same about c(s) = (32, 1, 0) at s = 0.5
    assert near(_uv(S, (32, 1, 0), (0, 0, 1), 1.0, -1, mov=0, time=0.5), (0.25, 0.5))
    assert near(_uv(S, (32, 1, 0), (1, 0, 0), 1.0, -1, mov=0, time=0.5), (0.5, 0.5))
    # the rectangles in their constructor order: (x, y), (x, z), (y, z) over [-1, 3] x [2, 4]
    for idx, o, d in ((1, (0, 2.5, 0), (0, 0, 1)), (2, (0, 0, 2.5), (0, 1, 0)), (3, (0, 0, 2.5), (1, 0, 0))):
        assert near(_uv(S, o, d, 0.5, idx), (0.25, 0.25)), idx
    assert near(_uv(S, (3, 4, 0), (0, 0, 1), 0.5, 1), (1.0, 1.0))  # the inclusive far edge
    assert near(_uv(S, (-1, 2, 0), (0, 0, 1), 0.5, 1), (0.0, 0.0))
    # the tube: u = (atan2(y, x) + 2 pi) / 4 pi in object space, v along the axis
    for n, u in (((1, 0, 0), 0.5), ((0, 1, 0), 0.625), ((-1, 0, 0), 0.75), ((0, -1, 0), 0.375)):
        assert near(_uv(S, (10, 0, 1.0), n, 0.5, 4), (u, 0.5)), n
    # the triangle: at a corner one sub-triangle is the whole.  The reference pairs w1 = |(r - v1) x (r - v2)| / ... with u1: at
    # r = v3 that is u1, at v2 it is u2 (through w2), at v1 it is u3 (through w3); at the centroid the three weights are 1/3
    tri = lambda x, y: _uv(S, (x, y, 5.0), (0, 0, -1), 5.0, 5)
    assert near(tri(20, 4), (0.125, 0.25)) and near(tri(24, 0), (0.875, 0.375)) and near(tri(20, 0), (0.375, 0.75))
    assert near(tri(20 + 4 / 3, 4 / 3), (1.375 / 3, 1.375 / 3))
    assert near(tri(22, 0), (0.625, 0.5625))  # midway between v1 and v2: w1 = 0, w2 = w3 = 1/2


def test_image_lookup(rtmi):
    """texel[int(frac(u) rows)][int(frac(v) cols)]: u indexes rows; a rectangle's inclusive far edge reads row 0"""
    img = np.arange(3 * 4 * 3, dtype=np.uint8).reshape(3, 4, 3)
    at = lambda u, v, perturb=(): tuple(int(x[0]) for x in R.image_texel(img, np.array([u], F64), np.array([v], F64), F64, perturb))
    assert at(0.0, 0.0) == (0, 0) and at(0.99, 0.99) == (2, 3) and at(0.34, 0.0) == (1, 0) and at(0.0, 0.26) == (0, 1)
    assert at(1.0, 1.0) == (0, 0) and at(-0.01, 2.26) == (2, 1)
    assert at(0.99, 0.0, ("uv_transposed",)) == (0, 3)
    # through a scene: the far corner of a textured rectangle, and the value / 255
    sc = rtmi.Scene.new(16, 9, 1, 2)
    sc.xy_rect(0.0, 3.0, 0.0, 4.0, 1.0, sc.lambertian(sc.image_texture(img)))
    S = R.RefScene(sc)
    o = np.array([[3.0, 4.0, 0.0], [2.9, 3.9, 0.0], [1.2, 0.5, 0.0]])
    d = np.tile([0.0, 0.0, 1.0], (3, 1))
    p = o + d
    val, texel = R.texture_value(S, np.array([int(S.mats["texture"][0])] * 3), p, F64, o, d, np.ones(3), np.zeros(3, np.int64))
    assert texel.tolist() == [0, 2 * 4 + 3, 1 * 4 + 0]
    assert np.allclose(val, img.reshape(-1, 3)[texel] / 255.0, rtol=0, atol=1e-15)
