"""Light sampling in participating media (rt_scene_set_media_light_sampling) on the host, no GPU needed: the switch
through every interface, what it packs, the host evaluation of a shadow ray's transmittance against fp64, the premises of the
fp64 statement (ref64.trace) and of the GPU scenes of test_gpu_media_nee.py, and the white furnace's sensitivity to
the statement's deliberate mistakes."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import media_nee_scenes as MN
import media_scenes as MS
import nee_scenes as NS
import per_sample as PS
import phase_scenes as PH
import ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
RTMI = os.path.join(PKG, "rtmi")
RT_ERR_ARG = 1


# ---- the switch ------------------------------------------------------------------------------------------------------------------
def test_switch_in_c(rtmi):
    lib = C.CDLL(os.path.join(PKG, "librtmi.so"))
    for name in ("rt_scene_set_media_light_sampling", "rt_scene_get_media_light_sampling", "rt_media_transmittance"):
        assert hasattr(lib, name), name
    lib.rt_scene_new.restype = C.c_void_p
    lib.rt_scene_free.argtypes = [C.c_void_p]
    lib.rt_scene_set_media_light_sampling.argtypes = [C.c_void_p, C.c_int]
    lib.rt_scene_get_media_light_sampling.argtypes = [C.c_void_p]
    lib.rt_abi_version.restype = C.c_int
    assert lib.rt_abi_version() == 3
    assert lib.rt_scene_set_media_light_sampling(None, 1) == RT_ERR_ARG and lib.rt_scene_get_media_light_sampling(None) == -RT_ERR_ARG
    s = lib.rt_scene_new(16, 9, 1, 4)
    assert lib.rt_scene_get_media_light_sampling(s) == 0  # (off by default)
    assert lib.rt_scene_set_media_light_sampling(s, 7) == 0 and lib.rt_scene_get_media_light_sampling(s) == 1  # (any nonzero value)
    assert lib.rt_scene_set_media_light_sampling(s, 0) == 0 and lib.rt_scene_get_media_light_sampling(s) == 0
    lib.rt_scene_free(s)


def test_switch_in_python_json_clone_and_version(rtmi, tmp_path):
    sc = MN.thin_fog(rtmi)
    assert sc.media_light_sampling is False and "media_light_sampling" not in json.loads(sc.to_json())
    off_text = sc.to_json()
    v0 = sc.table_info()  # (packs)
    before = sc.table_image().copy()
    sc.set_media_light_sampling(True)
    assert sc.media_light_sampling is True
    doc = json.loads(sc.to_json())
    assert doc["media_light_sampling"] is True
    path = tmp_path / "scene.json"
    path.write_text(sc.to_json())
    again = rtmi.Scene.load(str(path))
    assert again.media_light_sampling is True and again.to_json() == sc.to_json()
    assert sc.clone().media_light_sampling is True
    # alone the switch is inert: the tables are the bytes they were (and it bumps the version: the image is packed again)
    assert np.array_equal(sc.table_image().view(np.uint32), before.view(np.uint32)) and sc.table_info().kernel_variant == v0.kernel_variant
    assert not sc.table_info().kernel_variant & 256
    sc.set_media_light_sampling(False)
    assert sc.to_json() == off_text  # (written only when on: a round trip gives the text it gave)


def test_a_clone_keeps_its_own_switch(rtmi):
    sc = MN.thin_fog(rtmi)
    a = sc.clone()
    a.set_media_light_sampling(True)
    assert a.media_light_sampling and not sc.media_light_sampling


CPP = r'''
#include <cstdio>
#include "rtmi.hpp"
int main() {
    rtmi::scene s(16, 9, 1, 4);
    s.add(rtmi::xz_rect(-1, 1, -2, 2, 0.5f, rtmi::lambertian(rtmi::color(0.5f, 0.5f, 0.5f))));
    if (s.media_light_sampling()) return 1;
    s.set_media_light_sampling(true);
    if (!s.media_light_sampling()) return 2;
    fputs(s.to_json().c_str(), stdout);
    s.set_media_light_sampling(false);
    return s.media_light_sampling() ? 3 : 0;
}
'''


def test_switch_in_cpp(rtmi, tmp_path):
    src, exe = tmp_path / "t.cpp", tmp_path / "t"
    src.write_text(CPP)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", PKG, "-lrtmi", f"-Wl,-rpath,{PKG}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert json.loads(r.stdout)["media_light_sampling"] is True


def test_switch_in_the_cli(scenes_dir, tmp_path):
    """--nee-media is --nee plus the switch: the dumped scene carries both keys (what follows the dump needs a GPU and may fail
    without one)"""
    fog = os.path.join(scenes_dir, "fog_room.json")
    for flags, want in ((["--nee-media"], (True, True)), (["--nee"], (True, None)), ([], (None, None))):
        out = tmp_path / "scene.json"
        p = subprocess.run([RTMI, "-f", fog, "-w", "16", "-h", "9", "-spp", "1", *flags, "--dump-json", str(out),
                            "-o", str(tmp_path / "x.ppm"), "--no-png"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
        assert p.returncode != 2, p.stderr
        doc = json.loads(out.read_text())
        assert (doc.get("light_sampling"), doc.get("media_light_sampling")) == want, (flags, doc.get("light_sampling"), doc.get("media_light_sampling"))
    p = subprocess.run([RTMI, "--nee-media=1"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 2 and "--nee-media" in p.stderr


def test_the_showcase_carries_the_switch(rtmi, scenes_dir):
    sc = rtmi.Scene.load(os.path.join(scenes_dir, "fog_beams.json"))
    assert sc.media_light_sampling and len(sc.media()) == 1 and len(sc.analytic_lights()) == 2
    sc.set_light_sampling(True)
    assert len(sc.lights()) == 3 and sc.table_info().kernel_variant & (256 | 2048) == 256 | 2048
    halo = open(os.path.join(scenes_dir, "fog_halo.json")).read()
    assert "media_light_sampling" not in halo


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def test_tables_switch_off_is_the_media_image_and_on_adds_the_light_tables(rtmi):
    """off: the image and kernel_variant of the scene as the parent packs it (the switch is read by no packer stage); on, with
    light sampling: the media image's words in front -- every part up to the light tables -- with 7a's light records and alias
    table found by content behind them, and layout | 2048 | 256"""
    sc = MN.thin_fog(rtmi, 0.7)
    plain_img, plain_info = sc.table_image().copy(), sc.table_info()
    assert plain_info.kernel_variant & 2048 and not plain_info.kernel_variant & 256
    sc.set_media_light_sampling(True)
    assert np.array_equal(sc.table_image().view(np.uint32), plain_img.view(np.uint32))
    sc.set_light_sampling(True)
    on_img, on_info = sc.table_image().copy(), sc.table_info()
    assert on_info.kernel_variant & (2048 | 256) == 2048 | 256 and on_info.kernel_variant & 255 in (16, 36, 44)
    lights = sc.lights()
    assert len(lights) == 1
    thr, alias = R.find_alias_table(on_img, lights)  # (raises unless the records stand there exactly once)
    assert len(thr) == 1 and alias[0] == 0
    # what light sampling adds to the media image is what it adds to the same room without media (7a's tables, nothing else) ...
    bare = MS.room(rtmi)
    n0 = bare.table_image().size
    bare.set_light_sampling(True)
    assert on_img.size - plain_img.size == bare.table_image().size - n0 > 0
    # ... and the media tail stands behind it as it stood: the last RT_MEDIUM_STRIDE float4 per medium, {box, albedo, density, g}
    tail = 12 * len(sc.media())
    assert np.array_equal(on_img.reshape(-1)[-tail:].view(np.uint32), plain_img.reshape(-1)[-tail:].view(np.uint32))
    assert on_img.reshape(-1)[-tail + 7] == np.float32(0.08) and on_img.reshape(-1)[-1] == np.float32(0.7)
    # the same scene with the switch off packs the same image (the switch changes routing, not tables)
    sc.set_media_light_sampling(False)
    assert np.array_equal(sc.table_image().view(np.uint32), on_img.view(np.uint32))


# ---- rt_media_transmittance against fp64 ----------------------------------------------------------------------------------------
def _fp64_tau(media, o, d, t_max):
    """the optical depth from the definitions, in fp64, on the fp32 inputs"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    tau, n_stays = 0.0, 0
    for m in media:
        a, b, ok = R.medium_interval(m, o[None, :], d[None, :], np.array([t_max], np.float64), np.float64)
        if ok[0] and m["density"] > 0:
            tau += float(m["density"]) * float(b[0] - a[0]) * float(np.sqrt(d @ d))
            n_stays += 1
    return tau, n_stays


# The tolerance, from the operation count.  With u = 2^-24: per stay, a and b each carry the interval formula's error --
# the box: one division, one subtraction, one product each, <= 3 u relative to max(|a|, |b|) <= 1, so <= 6 u on b - a (absolute, in
# units of t <= 1); the sphere: measured by tests/test_media.py at <= 1e-5 |t| for well-conditioned rays, which we take as 84 u
# -- then the subtraction (u), sigma * s (u), |d| from three products and a root (2.5 u) and the fma (u): tau's ABSOLUTE error is
# at most sum over stays of sigma |d| (2 x 84 u + 5.5 u (b - a)) <= n sigma_max |d| 174 u.  exp(-tau): expf's 1 ulp (u) plus
# the propagated d tau (|dT| = T d tau <= d tau), plus the final rounding.  So |T - T64| <= 174 u n sigma_max |d| + 2 u.
def _bound(n_stays, sigma_max, length):
    u = 2.0 ** -24
    return 174 * u * n_stays * sigma_max * length + 2 * u


@pytest.mark.parametrize("case", ["one medium", "two overlapping media", "no media"])
def test_transmittance_against_fp64(rtmi, case):
    sc = rtmi.Scene.new(16, 9, 1, 4)
    sc.sphere((0, -100, 0), 1.0, sc.lambertian((0.5, 0.5, 0.5)))
    if case != "no media":
        sc.add_medium_box((-2.5, 0.2, -1.0), (0.5, 2.2, 2.5), 0.6, (0.9, 0.5, 0.5))
    if case == "two overlapping media":
        sc.add_medium_sphere((0.3, 1.4, 1.2), 1.0, 1.5, (0.4, 0.6, 0.9))
    media = sc.media()
    rng = np.random.default_rng(11)
    worst, worst_bound, crossing, missing = 0.0, 0.0, 0, 0
    for _ in range(4000):
        o = rng.uniform(-4, 4, 3).astype(np.float32)
        y = rng.uniform(-4, 4, 3).astype(np.float32)
        d = (y - o).astype(np.float32)
        T = sc.media_transmittance(o, d, 0.999)
        tau, n = _fp64_tau(media, o, d, np.float64(np.float32(0.999)))
        if n == 0:
            missing += 1
            if T != 1.0:  # (a stay that fp32 sees and fp64 does not, or the other way, is a grazing ray: its tau is within the bound of 0)
                assert abs(T - 1.0) <= _bound(1, 1.5, float(np.linalg.norm(d)))
            continue
        crossing += 1
        err, bound = abs(T - np.exp(-tau)), _bound(n, float(media["density"].max()), float(np.linalg.norm(d.astype(np.float64))))
        if err / bound > worst / max(worst_bound, 1e-300):
            worst, worst_bound = err, bound
        assert err <= bound, (o, d, T, np.exp(-tau), err, bound)
    print(f"\n{case}: {crossing} rays with a stay, {missing} without; worst |T - T64| {worst:.3e} at a bound of {worst_bound:.3e}")
    if case == "no media":
        assert crossing == 0
    else:
        assert crossing >= 1000 and missing >= 200


def test_a_ray_that_misses_every_medium_gives_exactly_one(rtmi):
    sc = MS.ref_cases()["two overlapping media"](rtmi)
    for o, d in (((0, 5, 0), (1, 0.1, 0)), ((5, 5, 5), (1, 1, 1)), ((0, 1, 8), (0, 0, 1))):
        assert sc.media_transmittance(o, d, 0.999) == 1.0
    assert rtmi.Scene.new(16, 9, 1, 4).media_transmittance((0, 0, 0), (1, 0, 0)) == 1.0
    assert sc.media_transmittance((-2, 1, 0), (2, 0, 0), 0.999) < 1.0  # (and one that stays in the box does not)


# ---- the fp64 statement's premises --------------------------------------------------------------------------------------------
W, H, K = 24, 14, 4


@pytest.fixture(scope="module")
def words(rtmi):
    return R.uniforms(rtmi, MN.REF_SEED, W, H, 0, K, NS.REF_DRAWS)


def _small(sc):
    sc.override(width=W, height=H)
    return sc


@pytest.mark.parametrize("name", list(MS.ref_cases()))
def test_with_no_lights_it_is_ref64_of_the_media_scene(rtmi, golden_dir, name):
    """... as ref64.trace stated it before light sampling in media joined its loop: held to golden/ref64_media_pin.npz"""
    S, _, _, tally = PS.check_media_pin(rtmi, golden_dir, "media/" + name, MS.ref_cases()[name](rtmi))
    assert len(S.lights) == 0 and tally["medium_light_samples"] == tally["surface_light_samples"] == 0


@pytest.mark.parametrize("key", ["phase/" + n for n in PH.ref_cases()] + ["media_nee/" + n for n in MN.ref_cases()])
def test_the_anisotropic_and_the_light_sampling_cases_trace_as_pinned(rtmi, golden_dir, key):
    """what ref64_phase.trace and ref64_media_nee.trace returned on their cases while they were tracers of their own"""
    group, name = key.split("/")
    _, _, _, tally = PS.check_media_pin(rtmi, golden_dir, key, PH.scene(rtmi, name) if group == "phase" else MN.scene(rtmi, name))
    assert tally["anisotropic_events"] > 0 if group == "phase" else tally["medium_light_samples"] > 0


@pytest.mark.parametrize("name", list(MS.ref_cases()))
def test_with_every_sigma_zero_it_is_ref64_with_light_sampling(rtmi, words, name):
    """the case's media at density 0 take no draw and attenuate nothing: ref64.reference() of the room with light sampling"""
    rr = 0.8 if name == "russian roulette" else 0.0
    sc, plain = _small(MS.room(rtmi, rr=rr)), _small(MS.room(rtmi, rr=rr))
    for m in MS.ref_cases()[name](rtmi).media():
        if m["shape"] == 0:
            sc.add_medium_sphere(m["f"][:3], m["f"][3], 0.0, m["albedo"])
        else:
            sc.add_medium_box(m["f"][:3], m["f"][3:], 0.0, m["albedo"])
    sc.set_light_sampling(True), plain.set_light_sampling(True)
    got, _, draws = R.trace(R.RefScene(sc), words)
    ref, _, rdraws, _ = R.reference(R.RefScene(plain), words)
    assert np.abs(got - ref).max() <= 1e-12 and np.array_equal(draws, rdraws)


def test_ref64_itself_still_refuses_the_combination(rtmi, words):
    """a light sample in a scene with media traces; what DESIGN defines no order for still raises: a shadow ray past a mover, and
    one towards the environment light in a scene with media"""
    sc = MN.switch_on(_small(MN.thin_fog(rtmi)))
    rgb, sig, _ = R.trace(R.RefScene(sc), words)
    assert rgb.any() and R.tally(sig)["medium_light_samples"] > 0
    env = sc.clone()
    env.set_environment(np.ones((4, 8, 3), np.float32))
    assert R.RefScene(env).lights[-1]["shape"] == R.ENVIRONMENT
    with pytest.raises(NotImplementedError, match="environment"):
        R.trace(R.RefScene(env), words)
    for mover in (sc.clone(), _small(MS.room(rtmi))):  # (with media and without)
        mover.add_moving_sphere((0, 1, 0), (0.2, 1, 0), 0.3, mover.lambertian((0.5, 0.5, 0.5)))
        mover.set_light_sampling(True)
        with pytest.raises(NotImplementedError, match="mover"):
            R.trace(R.RefScene(mover), words, shutter=np.full(len(words), 0.5))


def test_every_mistake_changes_the_statement(rtmi, words):
    """each perturbation moves the radiance of many samples on the scene that is to show it (media_nee_scenes.MISTAKES)"""
    for mistake, name in MN.MISTAKES.items():
        sc = _small(MN.scene(rtmi, name))
        S = R.RefScene(sc)
        good, _, _ = R.trace(S, words)
        bad, _, _ = R.trace(S, words, perturb=(mistake,))
        moved = (np.abs(good - bad) > 1e-4 * np.maximum(1.0, np.abs(good))).any(axis=1).mean()
        print(f"\n{mistake} on {name}: {100 * moved:.1f} % of the samples move")
        assert moved > 0.03, (mistake, moved)


# ---- premises of the GPU scenes ------------------------------------------------------------------------------------------------
def test_buried_medium_premise(rtmi):
    sc = MS.mixed_scene(rtmi)
    MS.bury_medium_mixed(sc)
    MS.check_buried_mixed(rtmi, sc)


@pytest.fixture(scope="module")
def furnace_words(rtmi):
    return R.uniforms(rtmi, MN.REF_SEED, 64, 36, 0, 2, 2048)


FURNACE_KEYS = ("medium_events", "anisotropic_events", "medium_light_samples", "surface_light_samples", "medium_samples_clear", "clear_through_media",
                "occluded_through_media", "medium_then_emitter", "medium_then_emitter_mis")


@pytest.mark.parametrize("g", MN.FURNACE_G)
def test_white_furnace_premises_and_sensitivity(rtmi, furnace_words, g):
    """the box is closed; at the GPU test's depth the fp64 statement ends NO path of these samples by depth and reads no draw
    past the request; every sample's expectation is 1, so the mean is 1 within 5 of its own standard errors -- and with
    the transmittance left out, an isotropic pdf_b at g != 0, or the continuation at full weight it is not"""
    sc = MN.switch_on(MN.furnace(rtmi, g))
    MN.check_furnace_closed(sc)
    S, log = R.RefScene(sc), R.new_log()
    rgb, sig, draws = R.trace(S, furnace_words, log=log)
    assert log["ended_by_depth"] == 0 and draws.max() <= furnace_words.shape[1]
    t = {k: R.tally(sig)[k] for k in FURNACE_KEYS}
    assert t["medium_light_samples"] > 1000 and t["clear_through_media"] > 1000 and t["medium_then_emitter_mis"] > 100, t
    v = rgb[:, 0]
    assert np.array_equal(rgb[:, 0], rgb[:, 1]) and np.array_equal(rgb[:, 0], rgb[:, 2])
    se = v.std() / np.sqrt(len(v))
    print(f"\ng = {g}: mean {v.mean():.5f}, standard error {se:.5f}, {t}")
    assert abs(v.mean() - 1) <= 5 * se
    for mistake in ("no_transmittance", "medium_full_weight") + (("isotropic_pdf",) if g != 0 else ()):
        bad, _, _ = R.trace(S, furnace_words, perturb=(mistake,))
        b = bad[:, 0]
        bse = b.std() / np.sqrt(len(b))
        print(f"    {mistake}: mean {b.mean():.5f}, standard error {bse:.5f}")
        assert abs(b.mean() - 1) > 5 * bse, (mistake, b.mean(), bse)
