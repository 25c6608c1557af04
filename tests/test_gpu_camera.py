"""Camera projections (orthographic, panoramic and fisheye cameras) on the GPU, against the fp64 statement of
ref64_camera.py (ref64.trace() started on each sample's own ray), sample by sample on the same draws: criteria (a) - (d) of
test_gpu_nee_reference.py with per_sample's thresholds, on the eight cases of camera_scenes.py -- every projection, with and
without the lens, in the plain, light-sampling, media, environment, motion and nested-grid kernels.  The (b) baseline is the
plain kernel on the case's twin -- the perspective projection, light sampling off, environment, media and movers cleared --
against the twin's reference (ref64.trace as it is).  Each case asserts its contents from the reference's tally alone
(camera_scenes.check_contents).

(d): the reference's draws stay within REF_DRAWS, and a reference with a deliberate mistake -- the panorama mirrored or counted
from the top, the equisolid fisheye, the image circle on the frame's width, a lens that keeps the direction, an orthographic
camera with one origin -- is far from 97 % against the kernel.  These tests fail without the feature.

Known answers that do not rest on the fp64 statement: inside a large sphere the first-hit normal of a panoramic and of a
fisheye camera is -d^ of rt_camera_ray at the sample's jitter; the depth of an orthographic camera facing a wall is the wall's
distance at every pixel; a fisheye's pixels outside the image circle are zero in the frame and in all three feature passes.

Then what every feature keeps: the same bytes in every layout, through a sample split, from the product library and through
the tiles entry point; the refusals; the command line on the shipped scene, --pick included.

Of these cases only cam_ortho_nested has a grid: the camera instances' grid walk -- from orthographic origins spread over a
plane, along panoramic directions through the poles -- is held to their linear scan in tests/test_gpu_walk_families.py
(DESIGN 7x).

Every case prints one row of figures (pytest -s)."""
import json
import os
import subprocess

import numpy as np
import pytest

import camera_scenes as CS
import nee_scenes as NS
import per_sample as PS
import ref64 as R
import ref64_camera as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def inputs(rtmi):
    return PS.input_cache(rtmi, CS)


@pytest.fixture(scope="module")
def cases(rtmi, inputs):
    """name -> (scene, RefScene, kernel samples, (ref, stable, draws, tally)): rendered and traced once, shared by the tests.
    per_sample.case_cache with the reference of ref64_camera in place of ref64's: a projection is no part of a RefScene"""
    made = {}

    def of(name):
        if name not in made:
            words, shutter = inputs(name)
            sc = CS.scene(rtmi, name)
            st = rtmi.Stats()
            sc.render(rtmi.Opts(seed=CS.seed_of(name), sample_count=1), st)
            layouts = (PS.NESTED_LAYOUT,) if name in CS.NESTED else PS.GENERAL_LAYOUTS
            assert st.kernel_variant & ~CS.FAMILIES in layouts and st.kernel_variant & CS.FAMILIES == CS.family(name), st.kernel_variant
            got = PS.kernel_samples(rtmi, sc, CS.seed_of(name), NS.REF_K, CS.FAMILIES, CS.family(name))
            S, F, ref = CS.reference(rtmi, name, words, shutter, sc)
            made[name] = (sc, S, got, ref, F)
        return made[name][:4]
    of.frame = lambda name: (of(name), made[name][4])[1]
    return of


@pytest.mark.parametrize("name", list(CS.CASES))
def test_kernel_against_fp64(rtmi, inputs, cases, name):
    print("\n    " + ", ".join(f"{k} {v}" for k, v in cases(name)[3][3]["camera"].items()))
    PS.check_kernel_against_fp64(rtmi, CS, inputs, cases, name)


@pytest.mark.parametrize("name,mistake", CS.MISTAKES)
def test_a_mistake_fails_the_agreement(inputs, cases, name, mistake):
    """per_sample.check_a_mistake_fails_the_agreement with ref64_camera.trace making the mistake"""
    words, shutter = inputs(name)
    sc, S, got, (ref, stable, _, _) = cases(name)
    wrong, _, _ = RC.trace(S, cases.frame(name), words, shutter=shutter, perturb=(mistake,))
    good, bad = R.judge(got, ref, stable), R.judge(got, wrong, stable)
    print(f"\n{name}, {mistake}: within tolerance {100 * good['share']:.2f} % -> {100 * bad['share']:.2f} %")
    PS.assert_perturbation_noticed(good, bad)


def test_layouts_a_sample_split_and_the_product_library_give_the_same_bytes(rtmi, tmp_path):
    """... and the perspective twin's frame differs"""
    PS.check_same_bytes(rtmi, CS, ("cam_ortho_blur", "cam_pano_nee", "cam_fisheye_env"), tmp_path, twin=lambda name: CS.twin(rtmi, name))


@pytest.mark.parametrize("name", ["cam_fisheye_blur_nee", "cam_pano_fog"])
def test_the_tiles_entry_point_gives_renders_bytes(rtmi, name):
    sc, st = CS.scene(rtmi, name), rtmi.Stats()
    sc.override(spp=NS.REF_K)
    o = rtmi.Opts(seed=CS.seed_of(name))
    ref = sc.render(o, st)
    assert st.kernel_variant & CS.FAMILIES == CS.family(name)
    assert np.array_equal(sc.render_tiles([0], o, st), ref)
    assert np.array_equal(sc.render_tiles([0], rtmi.Opts(seed=CS.seed_of(name), tile_rows=8), st), ref)


# ------------------------------------------------------------------------------------------------------------ known answers
def film_of_sample_zero(rtmi, sc, seed):
    """(s, t) [H x W] of sample 0 of every pixel as the kernels form them: ((float)x + xi) * (1 / (W - 1)) in fp32"""
    w, h = sc.width, sc.height
    words = R.uniforms(rtmi, seed, w, h, 0, 1, 2)
    xi = (words >> 8).astype(np.float32) * np.float32(2.0 ** -24)
    pix = np.arange(w * h)
    s = ((pix % w).astype(np.float32) + xi[:, 0]) * (np.float32(1) / np.float32(w - 1))
    t = ((pix // w).astype(np.float32) + xi[:, 1]) * (np.float32(1) / np.float32(h - 1))
    return s, t


def inside_a_sphere(rtmi, kind, *params):
    sc = rtmi.Scene.new(NS.REF_W, NS.REF_H, 1, 3)
    sc.set_background((0.2, 0.3, 0.4), sky_gradient=False, defocus_blur=False)
    sc.camera((1.0, 2.0, -1.0), (0.0, 2.5, -4.0), (0, 1, 0), 50.0)
    sc.sphere((1.0, 2.0, -1.0), 50.0, sc.lambertian((0.5, 0.6, 0.7)))
    sc.set_projection(kind, *params)
    return sc


@pytest.mark.parametrize("kind,params", [("panoramic", ()), ("fisheye", (220.0,))])
def test_the_normal_inside_a_large_sphere_is_minus_the_cameras_direction(rtmi, kind, params):
    """the camera at the centre of a sphere of radius 50: the first hit's normal, turned against the ray, is -d^; the depth is
    50 / |D|; to the 1e-5 test_gpu_features.py holds normals to.  A fisheye's pixels outside the circle are zeros"""
    sc = inside_a_sphere(rtmi, kind, *params)
    o = rtmi.Opts(seed=NS.REF_SEED, sample_first=0, sample_count=1)
    normal = sc.render_feature(rtmi.FEATURE_NORMAL, o).reshape(-1, 3).astype(np.float64)
    depth = sc.render_feature(rtmi.FEATURE_DEPTH, o).reshape(-1, 3).astype(np.float64)
    s, t = film_of_sample_zero(rtmi, sc, NS.REF_SEED)
    rays = [sc.camera_ray(float(a), float(b)) for a, b in zip(s, t)]
    seen = np.array([r[2] for r in rays])
    d = np.array([r[1] for r in rays], np.float64)
    fd = RC.Frame(sc).fd
    unit = d[seen] / np.linalg.norm(d[seen], axis=1)[:, None]
    worst_n, worst_t = np.abs(normal[seen] + unit).max(), np.abs(depth[seen, 0] * fd - 50.0).max()
    print(f"\n{kind}: {seen.sum()} of {len(seen)} samples see; worst |n + d^| {worst_n:.2e}, worst |t fd - 50| {worst_t:.2e}")
    assert seen.sum() >= (len(seen) if kind == "panoramic" else 400)
    assert worst_n < 1e-5 and worst_t < 1e-5 * 50.0 and (depth[seen, 1] == 1).all()
    assert not normal[~seen].any() and not depth[~seen].any()


def test_orthographic_depth_of_a_facing_wall_is_its_distance(rtmi):
    """a wall quad 7 units in front of an orthographic camera with focus distance 1 (|D| = 1: the hit record's t is the
    distance): 7 at every pixel, in every general layout"""
    sc = rtmi.Scene.new(NS.REF_W, NS.REF_H, 1, 3)
    sc.set_background((0.2, 0.3, 0.4), sky_gradient=False, defocus_blur=False)
    sc.camera((0.5, 1.0, 4.0), (0.5, 1.0, 0.0), (0, 1, 0), 50.0, 0.0, 0.0, 1.0)
    sc.quad((-9.5, -9.0, -3.0), (20.0, 0.0, 0.0), (0.0, 20.0, 0.0), sc.lambertian((0.5, 0.6, 0.7)))
    sc.sphere((0.0, 1.0, -6.0), 1.0, sc.lambertian((0.5, 0.5, 0.5)))  # (behind the wall)
    sc.set_projection("orthographic", 6.0)
    for variant in PS.GENERAL_LAYOUTS:
        depth = sc.render_feature(rtmi.FEATURE_DEPTH, rtmi.Opts(seed=NS.REF_SEED, sample_first=0, sample_count=1, variant=variant)).astype(np.float64)
        assert (depth[..., 1] == 1).all() and np.abs(depth[..., 0] - 7.0).max() < 1e-5 * 7.0, (variant, np.abs(depth[..., 0] - 7.0).max())
    normal = sc.render_feature(rtmi.FEATURE_NORMAL, rtmi.Opts(seed=NS.REF_SEED, sample_first=0, sample_count=1))
    assert np.abs(normal - np.array([0.0, 0.0, 1.0])).max() < 1e-5


def test_fisheye_pixels_outside_the_circle_are_zero_everywhere(rtmi):
    """cam_fisheye_env, bright everywhere (an environment map): sample 0 of a pixel outside the circle adds zeros to the frame
    and to all three feature passes, and counts as a sample -- a 13-sample frame is the sum of thirteen one-sample frames"""
    name = "cam_fisheye_env"
    sc, seed = CS.scene(rtmi, name), CS.seed_of(name)
    s, t = film_of_sample_zero(rtmi, sc, seed)
    a = RC.Frame(sc).aspect
    r = np.hypot((2 * s.astype(np.float64) - 1) * max(a, 1.0), (2 * t.astype(np.float64) - 1) * max(1.0 / a, 1.0))
    out, inside = r > 1 + 1e-6, r < 1 - 1e-6
    assert out.sum() > 600 and inside.sum() > 400
    o = rtmi.Opts(seed=seed, sample_first=0, sample_count=1)
    frame = sc.render(o).reshape(-1, 3)
    assert not frame[out].any() and (frame[inside].max(axis=1) > 0).mean() > 0.5  # (a path that ends inside the room is black too)
    for f in (rtmi.FEATURE_ALBEDO, rtmi.FEATURE_NORMAL, rtmi.FEATURE_DEPTH):
        got = sc.render_feature(f, o).reshape(-1, 3)
        assert not got[out].any(), f
    assert (sc.render_feature(rtmi.FEATURE_ALBEDO, o).reshape(-1, 3)[inside].max(axis=1) > 0).mean() > 0.9
    whole = sc.render(rtmi.Opts(seed=seed, sample_first=0, sample_count=3)).astype(np.float64)
    parts = sum(sc.render(rtmi.Opts(seed=seed, sample_first=k, sample_count=1)).astype(np.float64) for k in range(3))
    assert np.abs(whole - parts).max() <= 1e-5 * max(1.0, np.abs(whole).max())


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(rtmi):
    # the compact layouts' burst slab is the perspective camera's
    PS.check_compact_layouts_refuse(rtmi, lambda: CS.scene(rtmi, "cam_ortho"))
    for variant in (2, 6):
        assert "compact" in PS.refused(rtmi, lambda: CS.scene(rtmi, "cam_ortho").render(rtmi.Opts(variant=variant)))
    # the counting kernels carry no projection
    assert "counting" in PS.refused(rtmi, lambda: CS.scene(rtmi, "cam_ortho").count(rtmi.Opts(sample_count=1)))
    # a mask together with a projection: those kernels are not built
    import alpha_scenes as AS
    sc = AS.scene(rtmi, "al_sky")
    sc.render(rtmi.Opts(sample_count=1))
    sc.set_projection("panoramic")
    assert "alpha mask" in PS.refused(rtmi, lambda: sc.render(rtmi.Opts(sample_count=1)))
    assert "alpha mask" in PS.refused(rtmi, lambda: sc.render_feature(rtmi.FEATURE_DEPTH, rtmi.Opts(sample_count=1)))
    sc.set_projection("perspective")
    sc.render(rtmi.Opts(sample_count=1))


# ------------------------------------------------------------------------------------------------------------ the command line
@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_the_cli_renders_the_shipped_scene(rtmi, tmp_path, nee):
    PS.check_cli(rtmi, tmp_path, "camera_views.json", nee, CS.NEE, loaded=lambda sc: sc.projection == ("panoramic", (360.0, 180.0)))


@pytest.mark.parametrize("flag,want", [("orthographic:5", ("orthographic", (5.0,))), ("panoramic", ("panoramic", (360.0, 180.0))),
                                       ("fisheye:200", ("fisheye", (200.0,))), ("perspective", ("perspective", ()))])
def test_pick_follows_the_scenes_camera(rtmi, flag, want):
    """rtmi --projection ... --pick through the centre pixel of a 66 x 36 frame ((32 + 0.5) / 65 = (35 - 18 + 0.5) / 35 = 1 / 2)
    reports the primitive Scene.trace reports for Scene.camera_ray(0.5, 0.5)"""
    scene = os.path.join(PS.PKG, "scenes", "camera_views.json")
    p = subprocess.run([os.path.join(PS.PKG, "rtmi"), "-f", scene, "-w", "66", "-h", "36", "--projection", flag, "--pick", "32,18"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    sc = rtmi.Scene.load(scene)
    sc.override(66, 36)
    sc.set_projection(want[0], *want[1])
    s = np.float32(32.5) * (np.float32(1) / np.float32(65))
    t = np.float32(17.5) * (np.float32(1) / np.float32(35))
    o, d, ok = sc.camera_ray(float(s), float(t))
    hit = sc.trace([o], [d])
    assert ok and hit["prim"][0] >= 0
    assert json.loads(p.stdout.strip().splitlines()[-1])["prim"] == int(hit["prim"][0]), (p.stdout, hit)


def test_pick_outside_the_fisheye_circle_is_the_invalid_ray_case(rtmi):
    scene = os.path.join(PS.PKG, "scenes", "camera_views.json")
    p = subprocess.run([os.path.join(PS.PKG, "rtmi"), "-f", scene, "-w", "66", "-h", "36", "--projection", "fisheye", "--pick", "1,18"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "not a valid ray" in p.stderr, (p.returncode, p.stderr[-500:])
