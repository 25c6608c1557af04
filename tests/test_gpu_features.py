"""First-hit feature passes (rt_render_hip_feature) on the GPU.

  * albedo: bit for bit the CPU checker's render of an EMISSIVE CLONE of the scene -- same camera, flags, background and
    primitives, every material a diffuse_light on the same texture (metal: a solid of its albedo, dielectric: solid white),
    roulette and light sampling off: the checker adds emitted x 1 at the first hit and stops, and returns the background on a
    miss (oracle/rt_oracle.c)
  * depth at spp 1: the first record of the checker's trace of that sample (t or miss), through the checker's 2^-24 quantisation
  * normal at spp 1: an fp64 derivation from the traced camera ray and the primitive its hit point lies on, to the 1e-5 that
    tests/test_primitives_fuzz.py uses for hit points; and it faces the ray
  * exact invariance under sample splits, row shards, spp_chunk and the layout"""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from test_nested_grid import dense_room
from test_textures_triangles import _showcase

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
SCENES = os.path.join(PKG, "scenes")
GOLDEN_SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
SEED = 2023
ALBEDO, NORMAL, DEPTH = 0, 1, 2


def emissive_clone(rtmi, sc):
    """S': every material a diffuse_light on the same texture; built from the scene's own description (public Python API)."""
    j = json.loads(sc.to_json())
    texs = j["texture"]["data"]
    mats = []
    for m in j["material"]["data"]:
        if m["type"] in ("lambertian", "diffuse_light"):
            mats.append({"type": "diffuse_light", "texture": m["texture"]})
        else:
            texs.append({"type": "solid_color", "color": m["albedo"] if m["type"] == "metal" else [1, 1, 1]})
            mats.append({"type": "diffuse_light", "texture": len(texs) - 1})
    j["material"]["data"] = mats
    for key in ("russian_roulette", "light_sampling", "nested_grid"):
        j.pop(key, None)
    clone = rtmi.Scene.parse(json.dumps(j))
    assert np.array_equal(clone.prims().view(np.uint8), sc.prims().view(np.uint8))
    a, b = clone.get_camera(), sc.get_camera()
    assert bytes(a) == bytes(b) and clone.info.flags == sc.info.flags and list(clone.info.background) == list(sc.info.background)
    # a metal's albedo arrived in its solid texture unchanged
    for m_old, m_new in zip(sc.materials(), clone.materials()):
        if m_old["type"] == 1:
            assert np.array_equal(clone.textures()[m_new["texture"]]["c0"], m_old["albedo"])
    return clone


def rtiow(rtmi, w=64, h=36):
    return rtmi.Scene.rtiow(7, w, h, 4, 20)


def mixed(rtmi, w=64, h=36):
    sc = rtmi.Scene.load(os.path.join(SCENES, "mixed_emissive.json"))
    sc.override(w, h, 4)
    return sc


def sample_scene(rtmi, w=64, h=36):
    sc = rtmi.Scene.load(os.path.join(GOLDEN_SCENES, "sample_scene.json"))
    sc.override(w, h, 4)
    return sc


def _albedo_equals_clone(rtmi, rtcheck, sc, rows=None):
    clone = rtcheck.OracleScene(emissive_clone(rtmi, sc))
    for first, count in ((0, 1), (0, 3), (2, 3)):
        got = sc.render_feature(ALBEDO, rtmi.Opts(seed=SEED, sample_first=first, sample_count=count))
        for y0, y1 in ([(0, sc.height)] if rows is None else [(y, y + 1) for y in rows]):
            ref, _ = rtcheck.oracle_render(clone, seed=SEED, rows=(y0, y1), sample_first=first, sample_count=count)
            bad = (got[y0:y1] != ref[y0:y1]).any(axis=2).sum()
            assert bad == 0, f"samples [{first}, +{count}) rows {y0}..{y1}: {bad} pixels differ from the emissive clone"
    return got


@pytest.mark.parametrize("make", [rtiow, mixed, sample_scene], ids=["rtiow", "mixed_emissive", "sample_scene"])
def test_albedo_is_the_emissive_clone(rtmi, rtcheck, make):
    sc = make(rtmi)
    img = _albedo_equals_clone(rtmi, rtcheck, sc)
    assert img.std() > 0


def test_albedo_with_roulette_and_light_sampling_on(rtmi, rtcheck):
    sc = mixed(rtmi)
    plain = sc.render_feature(ALBEDO, rtmi.Opts(seed=SEED))
    sc.set_russian_roulette(0.8)
    sc.set_light_sampling(True)
    assert np.array_equal(sc.render_feature(ALBEDO, rtmi.Opts(seed=SEED)), plain)
    _albedo_equals_clone(rtmi, rtcheck, sc)


def test_albedo_of_textured_triangles(rtmi, rtcheck, tmp_path):
    _albedo_equals_clone(rtmi, rtcheck, _showcase(rtmi, tmp_path))


def test_albedo_of_the_nested_dense_room(rtmi, rtcheck):
    sc = dense_room(rtmi, w=160, h=90, spp=2)
    sc.set_nested_grid(True)
    assert sc.nested_info().cells > 0
    st = rtmi.Stats()
    img = sc.render_feature(ALBEDO, rtmi.Opts(seed=SEED, sample_count=3), st)
    assert st.kernel_variant == (52 | 512)
    _albedo_equals_clone(rtmi, rtcheck, sc, rows=(5, 47, 70))
    for f in (ALBEDO, NORMAL, DEPTH):  # ... and the nested walk finds what the linear scan finds
        walk = sc.render_feature(f, rtmi.Opts(seed=SEED, sample_count=3))
        scan = sc.render_feature(f, rtmi.Opts(seed=SEED, sample_count=3, variant=24))
        assert np.array_equal(walk, scan), f
    assert np.array_equal(img, sc.render_feature(ALBEDO, rtmi.Opts(seed=SEED, sample_count=3, variant=52)))


def _quantize(v):
    """the checker's sample -> fixed point -> fp32 of one value (oracle/rt_oracle.c: clamp to +-65536, 2^-24 steps)"""
    v = np.clip(np.asarray(v, np.float32), -65536.0, 65536.0)
    return (np.rint(v.astype(np.float64) * 16777216.0) * (1.0 / 16777216.0)).astype(np.float32)


def _traces(rtcheck, sc, seed):
    """first query of sample 0 of every pixel: (H, W, 8) rows of (origin, direction, t or -1, hit)"""
    osc = rtcheck.OracleScene(sc)
    out = np.zeros((sc.height, sc.width, 8), np.float32)
    for y in range(sc.height):
        for x in range(sc.width):
            _, rec = rtcheck.oracle_trace_sample(osc, seed, x, y, 0, max_queries=4)
            out[y, x] = rec[0]
    return out


@pytest.mark.parametrize("make", [sample_scene, mixed], ids=["sample_scene", "mixed_emissive"])
def test_depth_is_the_first_trace_record(rtmi, rtcheck, make):
    sc = make(rtmi)
    got = sc.render_feature(DEPTH, rtmi.Opts(seed=SEED, sample_count=1))
    tr = _traces(rtcheck, sc, SEED)
    hit = tr[..., 7] != 0
    assert hit.any()
    want = np.zeros_like(got)
    want[..., 0] = np.where(hit, _quantize(tr[..., 6]), 0.0)
    want[..., 1] = hit
    assert np.array_equal(got, want), f"{(got != want).any(axis=2).sum()} pixels differ"


def zoo(rtmi, w=64, h=36):
    """one of each primitive (a sphere, the three rects, a rotated cylinder, a triangle) in front of a sky"""
    sc = rtmi.Scene.new(w, h, 1, 4)
    sc.set_background((0.5, 0.7, 1.0), sky_gradient=True, defocus_blur=True)
    sc.camera((5, 4, 9), (0, 1, 0), (0, 1, 0), 40.0, 0.0, 0.05, 0.0)
    grey = sc.lambertian((0.6, 0.6, 0.6))
    sc.xz_rect(-6, 6, -6, 6, 0.0, grey)
    sc.xy_rect(-4, 4, 0, 4, -4.0, sc.metal((0.8, 0.8, 0.8), 0.1))
    sc.yz_rect(0, 3, -4, 4, -4.0, grey)
    sc.sphere((0, 1, 0), 1.0, sc.dielectric(1.5))
    sc.sphere((2.5, 0.6, 1.5), -0.6, grey)
    sc.cylinder(0.5, -1.0, 1.0, grey, rotate=((1, 0.3, 0), 70.0), translate=(-2.5, 1.2, 1.0))
    sc.triangle((1, 0.2, 3), (3.5, 0.3, 3.5), (2, 2.0, 2.5), grey)
    return sc


def _fp64_normal(prims, o, d, t):
    """the normal at o + t d of the primitive that point lies on, turned against d; (normal, residual of the surface equation)"""
    P = o + t * d
    best = (np.inf, None)
    for p in prims:
        f, m, mi = p["f"].astype(np.float64), p["m"].astype(np.float64), p["m_inv"].astype(np.float64)
        typ = int(p["type"])
        if typ == 0:
            c, r = f[:3], f[3]
            res, n = abs(np.linalg.norm(P - c) - abs(r)), (P - c) / r
        elif typ in (1, 2, 3):
            ka, (ia, ib) = {1: (2, (0, 1)), 2: (1, (0, 2)), 3: (0, (1, 2))}[typ]
            inside = f[0] - 1e-6 <= P[ia] <= f[1] + 1e-6 and f[2] - 1e-6 <= P[ib] <= f[3] + 1e-6
            res = abs(P[ka] - f[4]) if inside else np.inf
            n = np.zeros(3)
            n[ka] = 1.0
        elif typ == 4:
            M, Mi = m.reshape(3, 4), mi.reshape(3, 4)
            q = Mi[:, :3] @ P + Mi[:, 3]
            rad = np.hypot(q[0], q[1])
            res = abs(rad - abs(f[0])) if f[1] - 1e-6 <= q[2] <= f[2] + 1e-6 else np.inf
            n = M[:, :3] @ np.array([q[0] / rad, q[1] / rad, 0.0])
        else:
            v1, v2, v3 = m[0:3], m[3:6], m[6:9]
            n = np.cross(v2 - v1, v3 - v1)
            n /= np.linalg.norm(n)
            a = np.array([np.dot(np.cross(v2 - v1, P - v1), n), np.dot(np.cross(v3 - v2, P - v2), n), np.dot(np.cross(v1 - v3, P - v3), n)])
            res = abs(np.dot(P - v1, n)) if (a >= -1e-6).all() else np.inf
        if res < best[0]:
            best = (res, n)
    res, n = best
    return (n if np.dot(n, d) < 0 else -n), res


@pytest.mark.parametrize("make", [zoo, sample_scene], ids=["zoo", "sample_scene"])
def test_normal_against_fp64(rtmi, rtcheck, make):
    sc = make(rtmi)
    got = sc.render_feature(NORMAL, rtmi.Opts(seed=SEED, sample_count=1)).astype(np.float64)
    tr = _traces(rtcheck, sc, SEED).astype(np.float64)
    prims = sc.prims()
    worst, hits, kinds = 0.0, 0, set()
    for y in range(sc.height):
        for x in range(sc.width):
            o, d, t, hit = tr[y, x, 0:3], tr[y, x, 3:6], tr[y, x, 6], tr[y, x, 7]
            if not hit:
                assert not got[y, x].any()
                continue
            n, res = _fp64_normal(prims, o, d, t)
            assert res < 1e-4 * max(1.0, t * np.linalg.norm(d)), (x, y, res)
            worst = max(worst, np.abs(got[y, x] - n).max())
            assert np.dot(got[y, x], d) <= 0.0, (x, y)
            hits += 1
    print(f"normal: {hits} hits, worst |difference| {worst:.3g}")
    assert hits > 100 and worst < 1e-5


def test_sample_splits_shards_and_chunks(rtmi):
    for make in (rtiow, mixed):
        sc = make(rtmi, 100, 60)
        for f in (ALBEDO, NORMAL, DEPTH):
            full = sc.render_feature(f, rtmi.Opts(seed=SEED, sample_count=3))
            # A one-sample frame holds the sample's fixed-point value exactly (a 2^-24 grid value of an fp32 number has at most
            # 24 significant bits), so the fp64 sum of three of them is the exact pixel sum, and its fp32 rounding is the
            # conversion the library applies to the sum of the whole range.
            parts = [sc.render_feature(f, rtmi.Opts(seed=SEED, sample_first=k, sample_count=1)).astype(np.float64) for k in range(3)]
            assert np.array_equal((parts[0] + parts[1] + parts[2]).astype(np.float32), full), f
            assert np.array_equal(sc.render_feature(f, rtmi.Opts(seed=SEED, sample_count=3, spp_chunk=1)), full), f
            out = np.zeros_like(full)
            for r in range(2):
                o = rtmi.Opts(seed=SEED, sample_count=3, tile_first=r, tile_stride=2)
                out[sc.shard_global_rows(o)] = sc.render_feature(f, o)
            assert np.array_equal(out, full), f


def test_every_layout_gives_the_same_bytes(rtmi):
    # RTIOW has compact tables: its own layout (0, 2 or 6: the scan in LDS) and the scans 16 / 24
    sc = rtiow(rtmi)
    for f in (ALBEDO, NORMAL, DEPTH):
        st = rtmi.Stats()
        want = sc.render_feature(f, rtmi.Opts(seed=SEED), st)
        assert st.kernel_variant == (16 | 512)
        for v in (2, 16, 24):
            assert np.array_equal(sc.render_feature(f, rtmi.Opts(seed=SEED, variant=v)), want), (f, v)
    sc = mixed(rtmi)
    for f in (ALBEDO, NORMAL, DEPTH):
        want = sc.render_feature(f, rtmi.Opts(seed=SEED))
        for v in (16, 24, 36, 44):
            assert np.array_equal(sc.render_feature(f, rtmi.Opts(seed=SEED, variant=v)), want), (f, v)
    with pytest.raises(rtmi.RtmiError) as e:
        sc.render_feature(ALBEDO, rtmi.Opts(seed=SEED, variant=64))
    assert e.value.status == 1


def test_a_large_sphere_only_scene_has_no_limit(rtmi):
    """70 000 spheres: wide tables in global memory (layout 44); the feature pass must not answer RT_ERR_LIMIT"""
    rng = np.random.default_rng(3)
    sc = rtmi.Scene.new(64, 36, 1, 4)
    sc.set_background((0.5, 0.7, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((0, 30, 60), (0, 0, 0), (0, 1, 0), 40.0)
    m = sc.lambertian((0.5, 0.4, 0.3))
    for c in rng.uniform(-40, 40, (70000, 3)):
        sc.sphere((float(c[0]), float(c[1]) * 0.1, float(c[2])), 0.2, m)
    st = rtmi.Stats()
    cov = sc.render_feature(DEPTH, rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant & 512 and cov[..., 1].sum() > 0
    assert np.array_equal(cov, sc.render_feature(DEPTH, rtmi.Opts(seed=SEED, variant=24)))


_PRODUCT = textwrap.dedent("""
    import os, sys
    import numpy as np
    sys.path.insert(0, %r)
    from __graft_entry__ import load_package
    rtmi = load_package()
    assert not rtmi.has_ablations()
    sc = rtmi.Scene.load(os.path.join(%r, "mixed_emissive.json")); sc.override(64, 36, 8)
    o = rtmi.Opts(seed=%d)
    img = sc.render(o)
    f = [sc.render_feature(k, o) for k in range(3)]
    np.savez(sys.argv[1], img=img, a=f[0], n=f[1], d=f[2], den=rtmi.denoise(img, 8, f[0], f[1], f[2], 8, iterations=3),
             rt=rtmi.Scene.rtiow(7, 64, 36, 2, 8).render_feature(1, o))
""") % (ROOT, SCENES, SEED)


def test_product_library_gives_the_same_bytes(rtmi, tmp_path):
    out = str(tmp_path / "prod.npz")
    env = dict(os.environ, RTMI_LIB=os.path.join(PKG, "librtmi_product.so"))
    p = subprocess.run([sys.executable, "-c", _PRODUCT, out], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    got = np.load(out)
    sc = mixed(rtmi)
    sc.override(64, 36, 8)
    o = rtmi.Opts(seed=SEED)
    img = sc.render(o)
    f = [sc.render_feature(k, o) for k in range(3)]
    assert np.array_equal(got["img"], img)
    for key, want in zip("and", f):
        assert np.array_equal(got[key], want), key
    assert np.array_equal(got["den"], rtmi.denoise(img, 8, f[0], f[1], f[2], 8, iterations=3))
    assert np.array_equal(got["rt"], rtmi.Scene.rtiow(7, 64, 36, 2, 8).render_feature(1, o))
