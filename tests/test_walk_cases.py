"""The premises of tests/test_gpu_walk_families.py, and the host coverage checks on scenes with quads (no GPU).

The GPU test compares every layout of every kernel group with the group's linear scan on the scenes of walk_cases.py.  That
says something about the grid walk only where a grid exists, lists most of the scene and decides what the camera sees -- and
a layout may be held to "no refusal" only where the tables are known to fit.  Each of these is asserted here on every generated
case; a case that fails one is a broken test.  The figures a case prints (pytest -s) are DESIGN 7x's.

Coverage: test_tables.check_coverage and test_nested_grid.check_nested_coverage -- every cell (leaf) a primitive's exact box
touches lists it, or it is in the always-tested part of its table -- with quads among the primitives (Scene.quad_counts says
how many lead their table as always-tested), flat on every shape and nested on the clumps and on quad_scenes.nested."""
import numpy as np
import pytest

import quad_scenes as QS
import ref64 as R
import walk_cases as W
from test_nested_grid import Leaves, check_nested_coverage
from test_tables import check_coverage

IDS = ["%s-%d-%s" % c for c in W.CASES]
MIN_LISTED_SHARE = 0.5   # of the primitives that are no spheres are listed in the cells
MIN_LISTED_HITS = 0.30   # of the camera rays that hit anything have a listed primitive as their closest hit (fp64)


@pytest.mark.parametrize("family,seed,shape", W.CASES, ids=IDS)
def test_the_grid_exists_and_matters(rtmi, family, seed, shape):
    g, sc = W.GROUPS[family], W.scene(rtmi, seed, family, shape)
    t, P, listed = sc.table_info(), sc.prims(), W.listed_prims(sc)
    assert 150 <= len(P) <= 900, len(P)
    assert 40 <= sc.width <= 96 and 24 <= sc.height <= 56 and 1 <= sc.spp <= 3 and 2 <= sc.max_depth <= 8
    assert t.grid_cells > 0 and t.ncl > 0
    others = [i for i in range(len(P)) if int(P["type"][i]) != 0]
    share = sum(1 for i in others if i in listed) / len(others)
    assert share >= MIN_LISTED_SHARE, share
    # the always-tested prefixes are not empty (the wall, the long thin cylinder and quad), and every kind is listed too
    nq, nq_a = sc.quad_counts()
    assert t.nr_a >= 1 and t.nc_a >= 1 and nq_a >= 1
    assert t.nr > t.nr_a and t.nc > t.nc_a and t.nt > t.nt_a and nq > nq_a and t.ns > t.np
    # what the camera sees is decided by the lists: the closest hit in fp64 of the rays through the pixel centres
    o, d = W.camera_rays(sc)
    _, idx = R.closest_hit(R.RefScene(sc), o, d, np.inf, np.float64)
    hit = idx >= 0
    assert hit.sum() >= 200, hit.sum()
    by_list = float(np.isin(idx[hit], sorted(listed)).mean())
    ni = sc.nested_info()
    print(f"\n{family:15s} {seed} {shape:6s} {sc.width:2d} x {sc.height:2d} x {sc.spp} depth {sc.max_depth} | {len(P):3d} primitives, {t.grid_cells:4d} cells, "
          f"{ni.cells} nested | listed {100 * share:3.0f} % | tables {t.hot_bytes_grid:6d} bytes | closest hit listed {100 * by_list:3.0f} %")
    assert by_list >= MIN_LISTED_HITS, by_list


@pytest.mark.parametrize("family,seed,shape", W.CASES, ids=IDS)
def test_every_layout_will_accept_it(rtmi, family, seed, shape):
    g, sc = W.GROUPS[family], W.scene(rtmi, seed, family, shape)
    t, ni = sc.table_info(), sc.nested_info()
    # layout 36 stages the grid tables in LDS beside four wave accumulators and, with masks, the alpha state (render_host.hip)
    assert t.hot_bytes_grid + W.LDS_BESIDE_TABLES <= W.LDS_BYTES, t.hot_bytes_grid
    assert t.kernel_variant & W.FAMILIES == g.bits & ~(W.FEATURE | W.TRACE)  # (a pass and a query are calls, not scenes)
    assert t.kernel_variant & ~W.FAMILIES in ((52,) if g.nested else (36, 44))
    assert (t.grid_wide == 2) == g.nested and (ni.cells > 0) == g.nested
    if g.nested:  # some nested cell's leaves list a quad, and some a triangle
        L = Leaves(sc)
        nq, _ = sc.quad_counts()
        tri0 = t.ns + t.nr + t.nc
        kinds = set()
        for c in np.flatnonzero(L.nested):
            _, _, n, first = L.grids[1 + int(L.words[c, 0])]
            for leaf in range(first, first + int(n.prod())):
                for gid in L.entries(leaf)[1]:
                    kinds.add("triangle" if tri0 <= gid < tri0 + t.nt else "quad" if tri0 + t.nt <= gid < tri0 + t.nt + nq else "other")
        assert {"triangle", "quad"} <= kinds, kinds


@pytest.mark.parametrize("family,seed,shape", W.CASES, ids=IDS)
def test_the_dress_is_the_groups(rtmi, family, seed, shape):
    """the same primitives under every group of a seed; what the group adds is there"""
    g, sc = W.GROUPS[family], W.scene(rtmi, seed, family, shape)
    plain = W.scene(rtmi, seed, "plain", shape)
    assert sc.prims()["type"].tobytes() == plain.prims()["type"].tobytes()
    for field in ("f", "m", "m_inv"):
        assert sc.prims()[field].tobytes() == plain.prims()[field].tobytes(), field
    assert sorted(set(int(x) for x in sc.prims()["type"])) == list(range(7))
    mats = sc.materials()
    assert {0, 1, 2, 4, 5, 6} <= set(int(x) for x in mats["type"][sc.prims()["material"]]), "a material kind is on no primitive"
    assert {0, 1, 2} <= {int(sc.textures()[m["texture"]]["type"]) for m in mats if int(m["type"]) == 0}  # solid, checker, image
    lit = {int(p["type"]) for p in sc.prims() if int(mats["type"][p["material"]]) == 3}
    assert {0, 4, 5, 6} <= lit and lit & {1, 2, 3}, lit  # an emitter on a sphere, a rectangle, a cylinder, a triangle and a quad
    masked = [m for m in range(len(mats)) if sc.alpha(m) is not None]
    assert (len(masked) >= 5) == g.alpha
    movers = sc.moving_spheres()
    assert len(movers) == (3 if g.motion else 0) and not any(int(m["material"]) in masked for m in movers)
    assert len(sc.media()) == (2 if g.media else 0)
    assert (sc.environment is not None) == g.env
    assert sc.light_sampling == g.nee and sc.mesh_lights == g.nee and len(sc.analytic_lights()) == (3 if g.nee else 0)
    assert sc.projection[0] == (g.camera or "perspective") and sc.nested_grid == g.nested
    if g.camera == "orthographic":  # exactly along -z from every pixel
        for s, u in ((0.0, 0.0), (0.37, 0.81), (1.0, 1.0)):
            _, d, ok = sc.camera_ray(s, u)
            assert ok and d[0] == 0.0 and d[1] == 0.0 and d[2] < 0.0, d
    if g.nee:  # with mesh lights, every kind is among the sampled emitters
        assert {0, 4, 5, 6} <= {int(x) for x in sc.lights()["shape"]}
    if g.trace:
        o, d, t_max = W.rays(sc, seed)
        assert len(o) == W.N_RAYS and np.isfinite(t_max).sum() == (W.N_RAYS + 1) // 2
        assert all(rtmi.ray_valid(r) for r in rtmi.pack_rays(o, d, t_max)[::97])
    # the twin, where the group has one, is the scene without what the group shows
    tw = W.twin_family(family)
    assert (tw is not None) == bool(g.alpha or g.camera or g.media or g.motion)
    assert set(W.layouts(family)) <= {0, 24, 36, 44, 52} and (52 in W.layouts(family)) == g.nested


def test_every_projection_serves_two_groups_and_the_built_in_edges_occur():
    cams = [g.camera for g in W.GROUPS.values() if g.camera]
    assert all(cams.count(p) >= 2 for p in ("orthographic", "panoramic", "fisheye"))
    seeds = [s for _, s, _ in W.CASES]
    assert len(set(seeds)) == len(seeds)
    inside = [(s % 3 == 0 and not W.GROUPS[f].passes and not W.GROUPS[f].camera) or W.GROUPS[f].camera == "panoramic" for f, s, _ in W.CASES]
    for share, lo, hi in (([(s // 2) % 2 == 0 for s in seeds], 0.4, 0.6), (inside, 0.25, 0.4),
                          ([s % 5 != 0 for s in seeds], 0.7, 0.9), ([s % 4 == 1 for s in seeds], 0.2, 0.3)):
        assert lo <= np.mean(share) <= hi, np.mean(share)  # the far mirror, the camera inside, the ground, roulette


@pytest.mark.parametrize("seed,shape", [(s, shape) for _, s, shape in W.CASES[::5]] + [(117, "clump"), (133, "clump")])
def test_flat_tables_cover_every_primitive_quads_among_them(rtmi, seed, shape):
    sc = W.scene(rtmi, seed, "plain", shape)
    T = check_coverage(sc)
    nq, nq_a = sc.quad_counts()
    assert T.t.grid_wide == 1 and T.t.grid_cells > 0 and nq - nq_a >= 20  # (listed quads: checked cell by cell)


@pytest.mark.parametrize("seed", [s for f, s, _ in W.CASES if W.GROUPS[f].nested])
def test_nested_tables_cover_every_primitive_quads_among_them(rtmi, seed):
    sc = W.scene(rtmi, seed, "nested", "clump")
    checked, L = check_nested_coverage(sc)
    nq, nq_a = sc.quad_counts()
    assert L.ni.cells > 0 and nq - nq_a >= 20 and checked >= len(W.listed_prims(sc))


def test_the_quad_suites_nested_clump_is_covered(rtmi):
    """quad_scenes.nested: 288 quads of 48 turned boxes in nested cells; and the same scene's flat tables"""
    sc = QS.nested(rtmi)
    checked, L = check_nested_coverage(sc)
    nq, nq_a = sc.quad_counts()
    assert (nq, L.ni.cells > 0) == (288, True) and checked >= nq - nq_a > 0
    sc.set_nested_grid(False)
    check_coverage(sc)
    assert sc.quad_counts()[0] == 288


def test_where_the_feature_suites_have_a_grid(rtmi):
    """The census behind this file (pytest -s prints it): grid_cells of every case of the feature suites' scene
    modules.  Asserted: what the docstrings of test_gpu_{alpha,camera,media,motion}.py say of their own cases -- whoever gives
    one of them a grid changes that sentence too."""
    import importlib

    import media_scenes as MS
    import motion_scenes as MO
    cells = {}
    for mod in ("alpha", "analytic_light", "bump", "camera", "glass", "glossy", "mesh_light", "noise", "normal_map", "pbr", "quad", "ext"):
        M = importlib.import_module(mod + "_scenes")
        cells[mod] = {name: M.scene(rtmi, name).table_info().grid_cells for name in M.CASES}
        print(f"\n{mod:15s}", ", ".join(f"{n}: {c}" for n, c in cells[mod].items()), end="")
    for mod, made in (("media_scenes", MS.ref_cases()), ("motion_scenes", dict(MO.ref_cases(), two_movers=MO.two_movers))):
        cells[mod] = {name: build(rtmi).table_info().grid_cells for name, build in made.items()}
        print(f"\n{mod:15s}", ", ".join(f"{n}: {c}" for n, c in cells[mod].items()), end="")
    total = sum(len(v) for v in cells.values())
    print(f"\n{sum(1 for v in cells.values() for c in v.values() if c > 0)} of {total} cases have a grid")
    assert not any(cells["alpha"].values()) and not any(cells["media_scenes"].values()) and not any(cells["motion_scenes"].values())
    assert [n for n, c in cells["camera"].items() if c > 0] == ["cam_ortho_nested"]
    fog = [n for v in cells.values() for n, c in v.items() if n.endswith("_fog") and c > 0]
    motion = [n for v in cells.values() for n, c in v.items() if n.endswith("_motion") and c > 0]
    assert fog == ["quad_fog"] and motion == ["quad_motion"]


def test_quad_counts_interface(rtmi):
    """the additive entry point: counts of a scene with and without quads, null arguments, the ABI version it leaves alone"""
    import ctypes as C
    sc = rtmi.Scene.new(16, 9, 1, 2)
    sc.camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0)
    m = sc.lambertian((0.5, 0.5, 0.5))
    sc.sphere((0, 0, 0), 1.0, m)
    assert sc.quad_counts() == (0, 0)
    sc.box((-1, -1, -1), (1, 1, 1), m)
    assert sc.quad_counts() == (6, 6)  # a small scene: nothing is listed
    lib, a, b = rtmi._lib, C.c_int32(), C.c_int32()
    assert lib.rt_scene_quad_counts(None, C.byref(a), C.byref(b)) == 1 and lib.rt_scene_quad_counts(sc._h, None, C.byref(b)) == 1
    assert lib.rt_scene_quad_counts(sc._h, C.byref(a), None) == 1
    assert rtmi.abi_version() == 3 and "rt_scene_quad_counts" in rtmi.C_SYMBOLS
