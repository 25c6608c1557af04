"""-m gpu: ray queries on the device (rt_trace_hip).  The kernel's walk, in every layout, beside the fp32 restatement
(bit for bit) and beside ref64 in fp64, on the arbitrary rays of tests/trace_cases.py: rays that start inside a cluster, graze
a nested cell or run parallel to an axis are here by construction, not by what a camera happens to see."""
import json
import os
import subprocess

import numpy as np
import pytest

import ref64 as R
import trace_cases as TC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTMI = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "rtmi")
_runs = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def raw(records):
    return np.ascontiguousarray(records).view(np.uint8).reshape(len(records), -1)


def run(rtmi, name, variant=0):
    """the full batch of a scene in one layout: once per process"""
    key = (name, variant)
    if key not in _runs:
        sc, o, d, t_max = TC.case(name)
        st = rtmi.Stats()
        _runs[key] = (sc.trace(o, d, t_max, opts=rtmi.Opts(variant=variant), stats=st), st.kernel_variant)
    return _runs[key]


def _check_against_restatement(rtmi, sc, o, d, h, p32, t32, u32, v32):
    hit = p32 >= 0
    assert np.array_equal(h["prim"], p32), int((h["prim"] != p32).sum())
    assert np.array_equal(bits(h["t"]), bits(t32))
    assert np.array_equal(bits(h["u"])[hit], bits(u32)[hit]) and np.array_equal(bits(h["v"])[hit], bits(v32)[hit])
    assert np.array_equal(h["material"][hit], sc.prims()["material"][p32[hit]])
    # a miss is a miss: t = +inf, prim -1, every other word 0
    miss = raw(h[~hit]).view(np.uint32)
    assert (h["t"][~hit] == np.inf).all() and (miss[:, 2:] == 0).all()
    assert set(np.unique(h["front"][hit]).tolist()) <= {0, 1}


def _check_record_against_fp64(S, o, d, h):
    """point, normal and front of the hits against ref64.hit_record in fp64 AT THE KERNEL'S OWN t"""
    hit = h["prim"] >= 0
    o64, d64 = o[hit].astype(np.float64), d[hit].astype(np.float64)
    p, n, front = R.hit_record(S, o64, d64, h["t"][hit].astype(np.float64), h["prim"][hit].astype(np.int64), np.float64)
    dp = np.sqrt(((h["point"][hit] - p) ** 2).sum(axis=1)) / np.maximum(1.0, np.sqrt((p * p).sum(axis=1)))
    dn = np.abs(h["normal"][hit] - n).max(axis=1)
    print("point", dp.max(), "normal", dn.max())
    assert dp.max() <= 1e-5
    assert dn.max() <= 2e-5
    clear = np.abs((d64 * n).sum(axis=1)) / np.sqrt((d64 * d64).sum(axis=1)) > 1e-4
    assert clear.mean() > 0.99 and np.array_equal(h["front"][hit][clear] != 0, front[clear])
    assert 0 < (h["front"][hit] != 0).mean() < 1 or len(set(h["prim"][hit].tolist())) < 3


@pytest.mark.parametrize("name", ["mixed", "rtiow"])
def test_the_restatement_bit_for_bit(rtmi, rtcheck, name):
    """1. prim, t and (u, v) of every ray equal rtcheck.oracle_hit_uv as bits at layout 0; material is the primitive's;
    point, normal and front against fp64 at the kernel's own t."""
    sc, o, d, t_max = TC.case(name)
    h, kv = run(rtmi, name)
    assert kv & rtmi.TRACE_LAYOUT and (kv & ~rtmi.TRACE_LAYOUT) in (16, 24, 36, 44)
    _check_against_restatement(rtmi, sc, o, d, h, *TC.restatement(name))
    _check_record_against_fp64(TC.ref_scene(name), o, d, h)


def test_the_restatement_bit_for_bit_where_the_ground_wins(rtmi, rtcheck):
    """1, beyond the issue's cases: scene (c) under the plain recipe (the box of all primitives, the ground sphere of radius
    1000 included), where the two references part (tests/trace_cases.py) but the kernel and the restatement must not"""
    sc, o, d, p32, t32, u32, v32 = TC.rtiow_plain_recipe()
    assert (p32 >= 0).mean() > 0.3
    _check_against_restatement(rtmi, sc, o, d, sc.trace(o, d), p32, t32, u32, v32)


@pytest.mark.parametrize("name", TC.SCENES)
def test_the_independent_fp64_statement(rtmi, name):
    """2. the same primitive as ref64.closest_hit for at least 99 % of the rays; where they agree, t within 2e-5 relative"""
    h, _ = run(rtmi, name)
    p64, t64 = TC.fp64(name)
    same = h["prim"] == p64
    both = same & (p64 >= 0)
    rel = TC.rel_t(h["t"][both], t64[both])
    print(name, "same primitive", same.mean(), "hits", int(both.sum()), "max rel t", rel.max())
    assert same.mean() >= 0.99
    assert rel.max() <= 2e-5
    assert both.sum() > 500


def test_layouts_give_the_same_bytes(rtmi):
    """3. 16 / 24 / 36 / 44 (and 0) on (a), 52 against 16 (and 24, 0) on (b), 0 against 16 (and 24) on (c)"""
    for name, layouts, default in (("mixed", (16, 24, 36, 44), None), ("clump", (52, 16, 24), 52), ("rtiow", (16, 24), 16)):
        base, kv = run(rtmi, name)
        if default is not None:
            assert kv == default | rtmi.TRACE_LAYOUT
        assert (base["prim"] >= 0).sum() > 500
        for v in layouts:
            h, kv = run(rtmi, name, v)
            assert kv == v | rtmi.TRACE_LAYOUT
            assert np.array_equal(raw(h), raw(base)), (name, v, int((raw(h) != raw(base)).any(axis=1).sum()))
    # a layout the scene's tables do not have is refused, not approximated
    sc = TC.case("rtiow")[0]
    for v in (36, 44, 52):
        with pytest.raises(rtmi.RtmiError):
            sc.trace([(0, 1, 5)], [(0, 0, -1)], opts=rtmi.Opts(variant=v))
    for v in (36, 44):
        with pytest.raises(rtmi.RtmiError):
            TC.case("clump")[0].trace([(0, 1, 5)], [(0, 0, -1)], opts=rtmi.Opts(variant=v))


def test_batch_independence(rtmi):
    """4. the first n rays of (a)'s batch give the first n records of the full batch, for n around the wave and the work item;
    and a second run of the full batch gives the same bytes"""
    sc, o, d, t_max = TC.case("mixed")
    full, _ = run(rtmi, "mixed")
    item = rtmi.TRACE_ITEM
    for n in sorted({1, 63, 64, 65, item - 1, item, item + 1, 3 * item + 7}):
        for variant in (0, 36):
            h = sc.trace(o[:n], d[:n], opts=rtmi.Opts(variant=variant))
            assert np.array_equal(raw(h), raw(full[:n])), (n, variant)
    assert np.array_equal(raw(sc.trace(o, d)), raw(full))
    # the batch a ray arrives in: the same rays in reverse order
    assert np.array_equal(raw(sc.trace(o[::-1], d[::-1])[::-1]), raw(full))


def test_t_max(rtmi, rtcheck):
    """5. t_max = the reported t still hits, with the same record; nextafter(t, 0) misses; 0.5 t misses, 2 t hits; below 0.001
    misses.  The expectation is the restatement's: a hit iff its t <= t_max."""
    sc, o, d, _ = TC.case("mixed")
    p32, t32, _, _ = TC.restatement("mixed")
    full, _ = run(rtmi, "mixed")
    hit = p32 >= 0
    oh, dh, th = o[hit], d[hit], t32[hit]
    for variant in (0, 36):
        opts = rtmi.Opts(variant=variant)
        assert np.array_equal(raw(sc.trace(oh, dh, th, opts=opts)), raw(full[hit]))
        assert np.array_equal(raw(sc.trace(oh, dh, np.float32(2.0) * th, opts=opts)), raw(full[hit]))
        for cut in (np.nextafter(th, np.float32(0.0)), np.float32(0.5) * th):
            h = sc.trace(oh, dh, cut, opts=opts)
            assert (h["prim"] == -1).all() and (h["t"] == np.inf).all() and (raw(h).view(np.uint32)[:, 2:] == 0).all()
        for below in (0.00099, 0.0, -1.0, -np.inf):
            assert (sc.trace(o, d, below, opts=opts)["prim"] == -1).all()
        # any far end: the restatement's hit iff its t <= t_max
        t_any = (np.float32(1.0) + np.random.default_rng(9).uniform(-0.5, 0.5, len(o)).astype(np.float32)) * np.where(hit, t32, 1.0).astype(np.float32)
        h = sc.trace(o, d, t_any, opts=opts)
        want = hit & (t32 <= t_any)
        assert np.array_equal(h["prim"] >= 0, want) and np.array_equal(raw(h[want]), raw(full[want])) and 0.2 < want[hit].mean() < 0.8


def test_occlusion(rtmi, rtcheck):
    """6. occlusion equals prim >= 0 of the closest-hit run on the same rays and t_max, boundary cases of 5 included, on all
    five layouts"""
    for name, layouts in (("mixed", (0, 16, 24, 36, 44)), ("clump", (52, 16)), ("rtiow", (0, 24))):
        sc, o, d, t_max = TC.case(name)
        full, _ = run(rtmi, name)
        hit = full["prim"] >= 0
        th = full["t"][hit]
        n_hit = int(hit.sum())
        oo = np.concatenate([o] + [o[hit]] * 4)
        dd = np.concatenate([d] + [d[hit]] * 4)
        tt = np.concatenate([t_max, th, np.nextafter(th, np.float32(0.0)), np.float32(0.5) * th, np.minimum(np.float32(2.0) * th, t_max[hit])])
        want = np.concatenate([hit, np.ones(n_hit, bool), np.zeros(2 * n_hit, bool), np.ones(n_hit, bool)])
        for variant in layouts:
            opts = rtmi.Opts(variant=variant)
            st = rtmi.Stats()
            occ = sc.trace(oo, dd, tt, occluded=True, opts=opts, stats=st)
            assert occ.dtype == bool and occ.shape == (len(oo),) and st.launches == 1 and st.kernel_variant & rtmi.TRACE_LAYOUT
            closest = sc.trace(oo, dd, tt, opts=opts)
            assert np.array_equal(occ, closest["prim"] >= 0), (name, variant)
            assert np.array_equal(occ, want), (name, variant, int((occ != want).sum()))


def test_invalid_rays(rtmi):
    """7. the guard table's invalid rays at positions 0, 63, 64 and in the middle of a batch of valid ones: RT_HIT_INVALID (0 in
    occlusion mode), and every valid neighbour returns the bytes of a run without them.  The host evaluation of the guard is
    checked first: a ray it lets through would enter the walk."""
    invalid = TC.check_guard(rtmi)
    sc, o, d, _ = TC.case("mixed")
    n_valid = 300
    full, _ = run(rtmi, "mixed")
    where = [0, 63, 64] + list(range(150, 150 + len(invalid) - 3))
    n = n_valid + len(invalid)
    is_bad = np.zeros(n, bool)
    is_bad[where] = True
    rays = np.zeros(n, rtmi.RAY_DTYPE)
    with np.errstate(over="ignore"):
        bad = np.concatenate([rtmi.pack_rays([r[1]], [r[2]], r[3]) for r in invalid])
    rays[is_bad] = bad
    rays[~is_bad] = rtmi.pack_rays(o[:n_valid], d[:n_valid])
    for variant in (0, 16, 24, 36, 44):
        opts = rtmi.Opts(variant=variant)
        h = sc.trace(rays["origin"], rays["dir"], rays["t_max"], opts=opts)
        assert (h["prim"][is_bad] == rtmi.HIT_INVALID).all() and (h["t"][is_bad] == np.inf).all()
        assert (raw(h[is_bad]).view(np.uint32)[:, 2:] == 0).all()
        assert np.array_equal(raw(h[~is_bad]), raw(full[:n_valid])), variant
        occ = sc.trace(rays["origin"], rays["dir"], rays["t_max"], occluded=True, opts=opts)
        assert not occ[is_bad].any() and np.array_equal(occ[~is_bad], full["prim"][:n_valid] >= 0)
    # a batch of nothing but invalid rays
    h = sc.trace(bad["origin"], bad["dir"], bad["t_max"])
    assert (h["prim"] == rtmi.HIT_INVALID).all()
    # the nested walk and the compact scene's scan
    for name in ("clump", "rtiow"):
        sc2, o2, d2, t2 = TC.case(name)
        full2, _ = run(rtmi, name)
        r2 = np.zeros(n, rtmi.RAY_DTYPE)
        r2[is_bad] = bad
        r2[~is_bad] = rtmi.pack_rays(o2[:n_valid], d2[:n_valid], t2[:n_valid])
        h = sc2.trace(r2["origin"], r2["dir"], r2["t_max"])
        assert (h["prim"][is_bad] == rtmi.HIT_INVALID).all() and np.array_equal(raw(h[~is_bad]), raw(full2[:n_valid])), name


def test_device_entry_on_a_torch_stream(rtmi):
    """8. torch tensors for rays and hits on a non-default stream: after a stream synchronise the bytes of the host entry; the
    words `reserved` occupies are ignored"""
    import torch
    sc, o, d, t_max = TC.case("mixed")
    full, _ = run(rtmi, "mixed")
    rays = rtmi.pack_rays(o, d, t_max)
    words = rays.view(np.float32).reshape(-1, 8).copy()
    words[:, 7] = np.float32(np.nan)
    words[::3, 7] = np.float32(-1e30)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d_rays = torch.from_numpy(words).to(dev, non_blocking=False)
        d_hits = torch.full((len(rays), 12), -7.0, dtype=torch.float32, device=dev)
        d_occ = torch.full((len(rays),), 9, dtype=torch.uint8, device=dev)
        assert torch.cuda.current_stream().cuda_stream == stream.cuda_stream != 0
        sc.trace_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        sc.trace_device(d_rays.data_ptr(), len(rays), d_occ.data_ptr(), occluded=True, stream=torch.cuda.current_stream().cuda_stream)
    stream.synchronize()
    got = d_hits.cpu().numpy().view(rtmi.HIT_DTYPE).reshape(-1)
    assert np.array_equal(raw(got), raw(full))
    assert np.array_equal(d_occ.cpu().numpy() != 0, full["prim"] >= 0)
    # with stats the call returns when the work is done, and says what ran
    st = rtmi.Stats()
    d_hits.fill_(0.0)
    torch.cuda.synchronize()
    sc.trace_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), stream=stream.cuda_stream, stats=st)
    assert st.launches == 1 and st.kernel_ms > 0 and st.kernel_variant & rtmi.TRACE_LAYOUT
    assert np.array_equal(raw(d_hits.cpu().numpy().view(rtmi.HIT_DTYPE).reshape(-1)), raw(full))


def test_what_a_query_ignores(rtmi):
    """9. scene (a) with a fog box, an environment map and light sampling added returns the bytes of scene (a); so does a
    change of frame size, camera, max_depth and Russian roulette"""
    import nee_scenes as NS
    sc, o, d, t_max = TC.case("mixed")
    full, _ = run(rtmi, "mixed")
    other = TC.mixed(rtmi)
    other.add_medium_box((-12, -1, -12), (12, 8, 12), 0.3, (0.9, 0.9, 0.9))
    env, scale, rotate = NS._sun_map()
    other.set_environment(env, scale, rotate)
    other.set_light_sampling(True)
    other.set_russian_roulette(0.8)
    other.override(width=17, height=9, spp=3, max_depth=2)
    other.camera((3.0, 1.0, -2.0), (0.0, 0.5, 0.0), (0, 1, 0), 70.0, aperture=0.2)
    for variant in (0, 36, 16):
        assert np.array_equal(raw(other.trace(o, d, opts=rtmi.Opts(variant=variant))), raw(full)), variant
    assert np.array_equal(other.trace(o, d, occluded=True), full["prim"] >= 0)


def _pixel_ray(sc, x, y):
    """the ray through the centre of pixel (x from the left, y from the top) in fp32, up to the rounding of its three fmas"""
    cam, info = sc.get_camera(), sc.info
    u = (np.float32(x) + np.float32(0.5)) * (np.float32(1.0) / np.float32(info.width - 1))
    v = (np.float32(info.height - 1 - y) + np.float32(0.5)) * (np.float32(1.0) / np.float32(info.height - 1))
    org = np.array(cam.origin[:], np.float64)
    dirn = np.array(cam.lower_left[:], np.float64) + float(u) * np.array(cam.horizontal[:], np.float64) + float(v) * np.array(cam.vertical[:], np.float64) - org
    return org, dirn


def test_cli_pick_and_focus_at(rtmi, tmp_path):
    """10. rtmi -f <scene (a) as JSON> --pick X,Y for a hit and a miss prints the record Scene.trace gives for the same ray;
    --focus-at on the hit pixel makes --dump-json show focus_dist = t |dir| to fp32 rounding"""
    sc = TC.mixed(rtmi)
    scene_file = str(tmp_path / "mixed.json")
    with open(scene_file, "w") as f:
        f.write(sc.to_json())
    w, h = sc.width, sc.height

    def pick(x, y):
        p = subprocess.run([RTMI, "-f", scene_file, "--pick", "%d,%d" % (x, y)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert p.returncode == 0, p.stderr
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 1, p.stdout
        return json.loads(lines[0])

    # a pixel that looks at the floor just below the frame's centre, and the top-left corner, which looks over everything
    hit_px, miss_px = (w // 2, h - 3), (0, 0)
    got = pick(*hit_px)
    assert set(got) >= {"prim", "type", "material", "t", "distance", "point", "normal"} and got["prim"] >= 0
    org, dirn = _pixel_ray(sc, *hit_px)
    assert np.allclose(got["origin"], org, rtol=0, atol=1e-6) and np.allclose(got["dir"], dirn, rtol=0, atol=1e-5)
    rec = sc.trace([got["origin"]], [got["dir"]])[0]
    assert rec["prim"] == got["prim"] and rec["material"] == got["material"] and rec["front"] == got["front"]
    assert np.float32(got["t"]) == rec["t"] and np.array_equal(np.float32(got["point"]), rec["point"])
    assert np.array_equal(np.float32(got["normal"]), rec["normal"]) and np.array_equal(np.float32(got["uv"]), [rec["u"], rec["v"]])
    assert got["type"] == ["sphere", "xy_rect", "xz_rect", "yz_rect", "cylinder", "triangle"][int(sc.prims()[rec["prim"]]["type"])]
    length = np.sqrt((np.float64(got["dir"]) ** 2).sum())
    assert abs(got["distance"] - float(rec["t"]) * length) <= 1e-6 * got["distance"]
    assert pick(*miss_px) == {"prim": -1}
    o2, d2 = _pixel_ray(sc, *miss_px)
    assert sc.trace([o2], [d2])[0]["prim"] == -1

    dump = str(tmp_path / "focused.json")
    p = subprocess.run([RTMI, "-f", scene_file, "--focus-at", "%d,%d" % hit_px, "--dump-json", dump, "-w", str(w), "-h", str(h), "-spp", "1",
                        "-o", str(tmp_path / "f.ppm"), "--no-png"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr
    focus = json.load(open(dump))["camera"]["focus_dist"]
    assert abs(focus - got["distance"]) <= 2e-7 * got["distance"], (focus, got["distance"])
    p = subprocess.run([RTMI, "-f", scene_file, "--focus-at", "%d,%d" % miss_px, "-o", str(tmp_path / "g.ppm"), "--no-png"],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert p.returncode != 0 and "meets nothing" in p.stderr
