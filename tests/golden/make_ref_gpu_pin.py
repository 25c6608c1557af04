"""Writes tests/golden/refgpu_records_<scene>.npz and refgpu_paths.npz: what the COMPILED gpu-version of the reference
(oracle/_ref/libref_gpu.so: its own hittable_list::hit, ray_color, camera, materials and textures behind oracle/shim/) returns on
this project's scenes.  Run where the reference checkout exists, after `make -C oracle`:

    python tests/golden/make_ref_gpu_pin.py

The fixtures hold data only: the scenes as this project's normalised JSON, the seed and SHA-256 of the rays (refgpu_pin.py makes
them again), sample ids by construction (refgpu_pin.sample_ids), the reference's outputs in fp32, and the reference's distance
from the fp64 statement (ref64.closest_hit / hit_record / hit_uv / trace) on the same inputs -- its own fp32 noise, measured without
any code under test, which the tests add to the bounds the project already holds against fp64.

One file per record scene: a scene's records (about 1500 hits of ten fp32 numbers) take 50 - 70 KB, and no fixture may be larger
than the largest file already here (about 100 KB).

Conditions checked here and recorded: the reference against fp64 sets aside at most 5 % of a record scene's rays and disagrees on
hit / miss or winner on none of the rest; on "ties" a same-t pair sets no ray aside for its winner (at least 95 % of those rays are decided); every emitter type
ends at least 1 % of a path scene's samples; at least 30 % of the samples have two or more dielectric events; "depth 3" cuts at
least 1 % of the samples that the full-depth scene finishes on a light."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402
import ref64 as R  # noqa: E402
import refgpu_pin as P  # noqa: E402
import rtcheck  # noqa: E402

rtmi = load_package()


# ---------------------------------------------------------------------------------------------------------- record scenes
def _frame():
    sc = rtmi.Scene.new(P.W, P.H, 1, 50)
    sc.set_background((0.1, 0.1, 0.1), sky_gradient=False, defocus_blur=False)
    sc.camera((0, 1, 8), (0, 0, 0), (0, 1, 0), 40.0)
    return sc, sc.lambertian((0.5, 0.5, 0.5)), sc.metal((0.8, 0.8, 0.8), 0.2), sc.dielectric(1.5), sc.diffuse_light((4, 4, 4))


def zoo():
    """a sphere and a negative-radius shell; one rect per axis; tubes untransformed, rotated, translated, rotated then translated"""
    sc, lam, met, glass, light = _frame()
    sc.sphere((-2.0, 0.3, 0.4), 0.8, lam)
    sc.sphere((-2.0, 0.3, 0.4), -0.6, glass)
    sc.xy_rect(-1.3, 1.5, -1.1, 1.4, -1.6, met)
    sc.xz_rect(-0.4, 2.1, -1.3, 1.2, -1.1, lam)
    sc.yz_rect(-1.2, 1.3, -1.4, 1.1, 2.6, light)
    sc.cylinder(0.5, -0.7, 0.6, lam)
    sc.cylinder(0.3, -1.3, 1.4, met, rotate=((1, 2, 3), 37.0))
    sc.cylinder(0.35, -0.6, 0.6, glass, translate=(1.5, 1.2, -0.5))
    sc.cylinder(0.45, -0.8, 0.5, light, rotate=((0, 1, 0.3), -120.0), translate=(-0.5, -1.4, 1.2))
    return sc


def inside():
    """spheres and tubes the rays start in: both roots, the open ends' clipping, the wall seen from inside"""
    sc, lam, met, glass, light = _frame()
    sc.sphere((0.0, 0.0, 0.0), 1.0, glass)
    sc.sphere((0.0, 0.0, 0.0), -0.5, glass)
    sc.sphere((2.2, 0.2, -0.3), 0.7, lam)
    sc.cylinder(0.6, -1.0, 0.8, met, translate=(-2.0, 0.0, 0.0))
    sc.cylinder(0.5, -0.9, 1.1, lam, rotate=((1, 2, 3), 37.0), translate=(0.3, 1.9, 0.2))
    sc.cylinder(0.25, -1.5, 1.5, light, rotate=((1, 0, 0), 80.0), translate=(0.4, -1.8, -0.2))
    return sc


def ties():
    """two identical rects with different materials; two rects overlapping in one plane; two identical spheres; two rects that share
    an edge"""
    sc, lam, met, glass, light = _frame()
    sc.xy_rect(-1.0, 0.0, -0.5, 0.5, 0.0, lam)
    sc.xy_rect(-1.0, 0.0, -0.5, 0.5, 0.0, met)
    sc.xz_rect(0.2, 1.2, -0.6, 0.4, -0.3, lam)
    sc.xz_rect(0.7, 1.7, -0.1, 0.9, -0.3, light)
    sc.sphere((0.5, 1.2, 0.3), 0.45, glass)
    sc.sphere((0.5, 1.2, 0.3), 0.45, lam)
    sc.yz_rect(-0.5, 0.25, -0.4, 0.6, -1.4, met)
    sc.yz_rect(0.25, 1.0, -0.4, 0.6, -1.4, lam)
    return sc


# ------------------------------------------------------------------------------------------------------------ path scenes
def glass_and_lights(max_depth=50):
    sc = rtmi.Scene.new(P.W, P.H, P.SPP, max_depth)
    sc.set_background((0.25, 0.45, 0.75), sky_gradient=False, defocus_blur=False)
    sc.camera((0.0, 1.3, 5.5), (0.0, 0.7, 0.0), (0, 1, 0), 42.0)
    glass = sc.dielectric(1.5)
    sc.sphere((-1.5, 0.75, 0.2), 0.75, glass)
    sc.sphere((0.1, 0.8, -0.3), 0.8, glass)
    sc.sphere((0.1, 0.8, -0.3), -0.65, glass)                                          # hollow
    sc.cylinder(0.45, -0.9, 0.9, glass, rotate=((1, 0, 0.3), 70.0), translate=(1.7, 0.85, 0.4))
    sc.xz_rect(-3.0, 3.0, -2.0, 3.0, -0.05, glass)                                      # two panes for a floor
    sc.xz_rect(-3.5, 3.5, -2.5, 3.5, -0.3, glass)
    sc.xy_rect(-2.2, 2.2, 0.1, 2.4, -2.2, sc.diffuse_light((4.0, 3.5, 3.0)))
    sc.cylinder(0.3, -1.6, 1.6, sc.diffuse_light((1.0, 2.0, 4.0)), rotate=((0, 1, 0), 90.0), translate=(0.0, 2.5, 0.8))
    return sc


def checker_furnace():
    sc = rtmi.Scene.new(P.W, P.H, P.SPP, 50)
    sc.set_background((0, 0, 0), sky_gradient=False, defocus_blur=False)
    sc.camera((0.3, 0.9, 3.4), (0.0, 0.4, 0.0), (0, 1, 0), 50.0)
    glass = sc.dielectric(1.5)
    sc.sphere((0.0, 0.0, 0.0), 9.0, sc.diffuse_light(sc.checker_texture((0.9, 0.8, 0.2), (0.1, 0.2, 0.9))))
    sc.xz_rect(-2.5, 2.5, -2.5, 2.5, -1.03, sc.diffuse_light(sc.checker_texture((2.0, 0.5, 0.5), (0.5, 2.0, 0.5))))
    sc.xy_rect(-1.7, 1.7, -0.6, 1.9, -2.07, sc.diffuse_light(sc.checker_texture((0.3, 0.3, 3.0), (3.0, 3.0, 0.3))))
    sc.yz_rect(-0.8, 1.6, -1.5, 1.5, -2.31, sc.diffuse_light(sc.checker_texture((1.5, 1.5, 1.5), (0.2, 0.2, 0.2))))
    sc.sphere((-0.9, 0.45, 0.4), 0.95, glass)
    sc.sphere((1.0, 0.3, 0.2), 0.85, glass)
    sc.sphere((1.0, 0.3, 0.2), -0.7, glass)
    sc.cylinder(0.45, -1.2, 1.2, glass, rotate=((0.2, 1, 0), 60.0), translate=(0.1, 1.6, -0.3))
    return sc


RECORD = {"zoo": zoo, "inside": inside, "ties": ties}
PATH = {"glass and lights": glass_and_lights, "checker furnace": checker_furnace, "depth 3": lambda: glass_and_lights(3)}
QUANTITIES = ("t", "p", "normal", "uv")


def record_fixture(name):
    sc = rtmi.Scene.parse(RECORD[name]().to_json())  # what a test will load: the tables of the normalised JSON
    text = sc.to_json()
    prims = sc.prims()
    o, d = P.make_record_rays(name, prims)
    ref = P.reference_records(rtcheck.RefGpuScene(sc), prims, o, d)
    f64 = P.fp64_records(R.RefScene(sc), o, d)
    judged, quirk, tie = P.decided(prims, o, d)
    finite = np.isfinite(ref["t"]) | (ref["index"] < 0)
    print(f"{name}: {len(o)} rays, {int((ref['index'] >= 0).sum())} hits, set aside {1 - judged.mean():.4f} (quirk classes "
          f"{quirk.mean():.4f}), reference records not finite {int((~finite).sum())} (decided among them {int((~finite & judged).sum())})")
    assert 1 - judged.mean() <= P.CAP, name
    fig, wrong = P.measure(prims, ref, f64, judged)
    assert wrong == 0, (name, "reference and fp64 disagree on", wrong, "decided rays")
    assert np.array_equal(ref["front"][judged], f64["front"][judged]), name
    if name == "ties":
        # a same-t pair sets no ray aside for its winner (the rule has no such clause); what is set aside there is near an edge,
        # t_min or another primitive
        print(f"    rays whose winner has a same-t partner: {int((tie >= 0).sum())}, decided among them {judged[tie >= 0].mean():.4f}")
        assert (tie >= 0).sum() >= 300 and judged[tie >= 0].mean() >= 0.95
        assert np.array_equal(ref["index"][tie >= 0] > tie[tie >= 0], np.ones(int((tie >= 0).sum()), bool)), "the later entry wins"
    for q in QUANTITIES:
        print(f"    reference vs fp64, {q}: max {fig[q][0]:.3g} median {fig[q][1]:.3g}")
    hit = ref["index"] >= 0
    out = dict(scene=np.array(text), rays_sha256=np.array(P.digest(o, d)), ray_seed=np.int64(P.RAY_SEED), n_rays=np.int64(len(o)),
               margin=np.float64(P.MARGIN), index=ref["index"].astype(np.int8), front=np.packbits(ref["front"][hit].astype(bool)),
               decided=np.packbits(judged), set_aside=np.float64(1 - judged.mean()), quirk=np.float64(quirk.mean()),
               ref_fp64_disagreements=np.int64(wrong), ref_fp64_dev=np.array([fig[q] for q in QUANTITIES], np.float64))
    for q in ("t", "p", "normal", "u", "v"):
        out[q] = ref[q][hit].astype(np.float32)
    path = os.path.join(HERE, f"refgpu_records_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"    {os.path.getsize(path)} bytes")


def path_fixture(name, z, full=None):
    sc = rtmi.Scene.parse(PATH[name]().to_json())
    text = sc.to_json()
    rs = rtcheck.RefGpuScene(sc)
    ids = P.sample_ids()
    n = len(ids)
    rgb, draws, cnt = np.zeros((n, 3), np.float32), np.zeros(n, np.int32), np.zeros((n, 3), np.int32)
    for i, (x, y, s) in enumerate(ids):
        rgb[i], draws[i], cnt[i] = rs.sample(P.SEED, int(x), int(y), int(s))
    assert draws.max() <= P.DRAWS
    prims, mats = sc.prims(), sc.materials()
    events, ended_by, cut = cnt[:, 0], cnt[:, 1], cnt[:, 2] != 0
    lights = [i for i, p in enumerate(prims) if int(mats[p["material"]]["type"]) == 3]
    shares = {i: float((ended_by == i).mean()) for i in lights}
    two = float((events >= 2).mean())
    print(f"{name}: ends on a light " + ", ".join(f"[{i}: type {int(prims[i]['type'])}] {100 * v:.1f} %" for i, v in shares.items())
          + f"; two or more dielectric events {100 * two:.1f} %; cut at depth {100 * cut.mean():.1f} %; most draws {draws.max()}")
    assert min(shares.values()) >= 0.01 and two >= 0.30, name
    words = R.uniforms(rtmi, P.SEED, P.W, P.H, 0, P.SPP, P.DRAWS)  # ordered (s, y, x), as ids
    rgb64, _, draws64 = R.trace(R.RefScene(sc), words)
    share, median = P.path_figures(rgb, rgb64)
    print(f"    reference vs fp64: within 1e-4 {100 * share:.3f} %, median {median:.3g}")
    k = P.key(name)
    if full is not None:  # "depth 3": what the full-depth scene finished on a light and this one cut
        lost = float((cut & (full["ended_by"] >= 0)).mean())
        print(f"    cut here, on a light at full depth: {100 * lost:.1f} %")
        assert lost >= 0.01
        z[f"{k}/cut_lit_share"] = np.float64(lost)
    z.update({f"{k}/scene": np.array(text), f"{k}/rgb": rgb, f"{k}/draws": draws.astype(np.uint8), f"{k}/events": events.astype(np.uint8),
              f"{k}/ended_by": ended_by.astype(np.int8), f"{k}/cut": np.packbits(cut), f"{k}/two_event_share": np.float64(two),
              f"{k}/light_shares": np.array(sorted(shares.items()), np.float64), f"{k}/ref_fp64_share": np.float64(share),
              f"{k}/ref_fp64_median": np.float64(median)})
    return dict(ended_by=ended_by)


def checker_fixture(z):
    pts = P.checker_points()
    odd = rtcheck.ref_gpu_checker(pts)
    clear = P.checker_clear(pts)
    assert np.array_equal(odd[clear], R.checker_odd(pts.astype(np.float64), np.float64)[clear])
    print(f"checker: {len(pts)} points, {100 * (1 - clear.mean()):.2f} % within the margin, odd {100 * odd.mean():.1f} %")
    z.update({"checker/points_sha256": np.array(P.digest(pts, pts[:0])), "checker/odd": np.packbits(odd)})


if __name__ == "__main__":
    for name in P.RECORD_SCENES:
        record_fixture(name)
    z = {"seed": np.int64(P.SEED), "width": np.int64(P.W), "height": np.int64(P.H), "spp": np.int64(P.SPP)}
    full = path_fixture("glass and lights", z)
    path_fixture("checker furnace", z)
    path_fixture("depth 3", z, full)
    checker_fixture(z)
    path = os.path.join(HERE, "refgpu_paths.npz")
    np.savez_compressed(path, **z)
    print(f"refgpu_paths.npz: {os.path.getsize(path)} bytes")
