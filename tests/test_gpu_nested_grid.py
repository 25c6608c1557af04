"""-m gpu: the nested grid (rt_scene_set_nested_grid) on the device.  Kernel variant 52 walks the sub-grid of a nested cell while
the ray is inside it; its image must equal the reference's linear scan (rt_opts.variant 16 / 24) on the whole frame and the
CPU checker (oracle/) on sampled rows, bit for bit, through every entry point that goes through render_impl."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from test_nested_grid import clump, dense_room

pytestmark = pytest.mark.gpu
SEED = 2023
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "librtmi_product.so")
RT_ERR_ARG = 1


def _rows_equal_checker(rtcheck, sc, img, seed, rows):
    osc = rtcheck.OracleScene(sc)
    for y in rows:
        ref, _ = rtcheck.oracle_render(osc, seed=seed, rows=(y, y + 1))
        assert np.array_equal(img[y], ref[y]), f"row {y} differs from the CPU checker"


def _nested(sc):
    sc.set_nested_grid(True)
    assert sc.nested_info().cells > 0
    return sc


def _equals_scan(rtmi, rtcheck, sc, scan_variant, rows):
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant == 52
    flat = sc.render(rtmi.Opts(seed=SEED, variant=scan_variant))
    assert np.array_equal(img, flat), f"{(img != flat).any(axis=2).sum()} pixels differ from the linear scan"
    assert np.array_equal(img, sc.render(rtmi.Opts(seed=SEED, variant=52)))
    _rows_equal_checker(rtcheck, sc, img, SEED, rows)
    return img


def test_dense_room_equals_the_linear_scan(rtmi, rtcheck):
    """51 200 triangles inside one unit square of a 20-unit room at 160 x 90 x 2, depth 8"""
    sc = _nested(dense_room(rtmi, w=160, h=90, spp=2))
    img = _equals_scan(rtmi, rtcheck, sc, 24, (5, 47, 70))
    assert img.max() > 0


def test_sphere_clump_equals_the_linear_scan(rtmi, rtcheck):
    sc = _nested(clump(rtmi, w=160, h=90, spp=2, depth=8))
    assert sc.table_info().np <= 100
    _equals_scan(rtmi, rtcheck, sc, 16, (3, 40, 66))


def test_textured_dense_room_equals_the_linear_scan(rtmi, rtcheck):
    """the EXT instance on both of its features: triangles, and an image texture on a third of them"""
    sc = _nested(dense_room(rtmi, w=160, h=90, spp=2, tex=True))
    _equals_scan(rtmi, rtcheck, sc, 24, (6, 45, 71))


def test_work_per_query(rtmi):
    """Primitives a query examines, switch off against on, on one row tile of the dense room.  rt_stats.prim_tests is by
    definition the REFERENCE's count (queries x primitives, the same for every kernel), so the figure is put together from the
    counters of what the kernel did: list entries tested per lane (lane_clusters), the always-tested prefixes of the four
    tables once per query, and everything the cells list for the rare lane that scans it (query_maxpop).  Off, every query
    examines at least the 46 270 demoted triangles; on, a few leaf lists of a few dozen entries: at most 1/50."""
    sc = dense_room(rtmi, w=160, h=90, spp=2)
    opts = rtmi.Opts(seed=SEED, tile_rows=8, tile_first=6, tile_stride=100000)

    def per_query(want_mode):
        t = sc.table_info()
        c = sc.count(opts)
        assert c.cull_mode == want_mode and c.queries > 0
        always = t.np + t.nr_a + t.nc_a + t.nt_a
        listed = (t.ns - t.np) + (t.nr - t.nr_a) + (t.nc - t.nc_a) + (t.nt - t.nt_a)
        return (c.lane_clusters + c.query_maxpop * listed) / c.queries + always, c

    off, c_off = per_query(7)
    assert off >= 46270
    _nested(sc)
    on, c_on = per_query(8)
    assert c_on.kernel_variant == 52 and c_on.queries == c_off.queries and c_on.hits == c_off.hits
    print(f"primitives examined per query: off {off:.1f}, on {on:.1f} (cell steps per query on: {c_on.lane_cands / c_on.queries:.1f})")
    assert on <= off / 50


def test_accumulate_shards_and_adaptive(rtmi):
    sc = _nested(dense_room(rtmi, w=96, h=56, spp=4))
    full = sc.render(rtmi.Opts(seed=SEED))
    # two half-sample accumulate calls equal one render
    acc, _ = sc.accumulate(None, rtmi.Opts(seed=SEED, sample_first=0, sample_count=2), want_image=False)
    acc, img = sc.accumulate(acc, rtmi.Opts(seed=SEED, sample_first=2, sample_count=2))
    assert np.array_equal(img, full)
    # two row shards scattered equal the frame; spp_chunk is scheduling only
    out = np.zeros_like(full)
    for first in (0, 1):
        o = rtmi.Opts(seed=SEED, tile_rows=8, tile_first=first, tile_stride=2, spp_chunk=1)
        sc.scatter_rows(o, sc.render(o), out)
    assert np.array_equal(out, full)
    # adaptive: every tile equals the plain render at its count
    img_a, spp_map, st = sc.render_adaptive(0.05, min_spp=2, max_spp=4, opts=rtmi.Opts(seed=SEED))
    plain = {n: sc.render(rtmi.Opts(seed=SEED, sample_count=int(n))) for n in np.unique(spp_map)}
    for n, ref in plain.items():
        mask = spp_map == n
        assert np.array_equal(img_a[mask], ref[mask])


def test_error_paths(rtmi):
    rtiow = rtmi.Scene.rtiow(7, 64, 36, 2, 8)
    with pytest.raises(rtmi.RtmiError) as e:
        rtiow.render(rtmi.Opts(variant=52))
    assert e.value.status == RT_ERR_ARG and "nested" in str(e.value)
    sc = _nested(dense_room(rtmi, w=64, h=36, spp=1))
    with pytest.raises(rtmi.RtmiError) as e:
        sc.render(rtmi.Opts(variant=44))
    assert e.value.status == RT_ERR_ARG and "nested" in str(e.value)
    sc.xz_rect(-1, 1, -1, 1, 6.0, sc.diffuse_light((4, 4, 4)))
    sc.set_light_sampling(True)
    assert sc.nested_info().cells > 0
    with pytest.raises(rtmi.RtmiError) as e:
        sc.render(rtmi.Opts())
    assert e.value.status == RT_ERR_ARG and "light sampling" in str(e.value)
    sc.set_light_sampling(False)
    sc.render(rtmi.Opts())


_SCRIPT = textwrap.dedent("""
    import os, sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
    from __graft_entry__ import load_package
    rtmi = load_package()
    from test_nested_grid import dense_room
    sc = dense_room(rtmi, w=96, h=56, spp=2)
    sc.set_nested_grid(True)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=5), st)
    assert st.kernel_variant == 52, st.kernel_variant
    np.save(sys.argv[1], img)
    print("rendered", int(rtmi.has_ablations()))
""") % (ROOT, ROOT)


def test_product_library_renders_the_dense_room(tmp_path):
    outs = []
    for lib, abl in ((None, "1"), (PRODUCT, "0")):
        env = dict(os.environ)
        if lib:
            env["RTMI_LIB"] = lib
        out = str(tmp_path / ("img%s.npy" % abl))
        p = subprocess.run([sys.executable, "-c", _SCRIPT, out], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0 and ("rendered " + abl) in p.stdout, p.stdout + p.stderr
        outs.append(np.load(out))
    assert np.array_equal(outs[0], outs[1])
