"""-m gpu: the control flow that the headline kernel's scalar and branch diet rewrote -- rt_sqrtf's voted guard behind its root
(the fast sequence runs first, a wave with an odd lane replaces the result), `resolve` as straight-line code (the winner by
selects, the tie rule behind a vote of the wave), the odd list's second entry read as the table holds it, and the walk's
thresholds on a scalar popcount -- each held to something other than itself: every frame to the reference's linear scan
(variant 16) byte for byte through the default kernel (and the 3-D walk, variant 6, where the scene has the compact tables),
two rows of every frame to the CPU checker, ray queries to the checker's own closest hit, the counting build to the
checker's counts.  Frames of at most 96 x 54 at 8 spp: every case is a few launches of well under a second.

The tie construction is test_gpu_headline_votes.py's: two spheres with the same centre and radius and different materials
always land in the same part of the table (the prefix is cut by |r|), their roots tie on every ray, and the later list entry
wins -- so the frame changes with the pair's order, and each order equals the scan and the checker."""
import numpy as np
import pytest

from test_tables import Tables

pytestmark = pytest.mark.gpu
SEED = 2023
CAM = (0.0, 2.0, 14.0)


def _mixed(sc, rng):
    return [sc.lambertian(rng.uniform(0.2, 0.9, 3)) for _ in range(4)] + [sc.metal((0.8, 0.8, 0.8), 0.1), sc.dielectric(1.5)]


def _field(rtmi, w=96, h=54, spp=3, depth=8, lookat=(0.0, 0.5, 0.0), tall=True):
    """A ground sphere, a 6 x 6 sheet of small spheres on it and (tall) one sphere taller than the layer: spheres only, so the
    compact tables and a grid one cell high -- variant 0 is the x-z walk (2), and the 3-D walk (6) reads the same tables."""
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera(CAM, lookat, (0, 1, 0), 40.0)
    rng = np.random.default_rng(5)
    mats = _mixed(sc, rng)
    sc.sphere((0.0, -1000.0, 0.0), 1000.0, mats[0])
    for i in range(6):
        for j in range(6):
            r = float(rng.uniform(0.15, 0.25))
            sc.sphere((1.1 * (i - 2.5) + float(rng.uniform(-0.2, 0.2)), r, 1.1 * (j - 2.5) + float(rng.uniform(-0.2, 0.2))), r,
                      mats[(6 * i + j) % len(mats)])
    if tall:
        sc.sphere((0.4, 1.0, -0.3), 1.0, mats[-1])
    return sc, mats


def _held(rtmi, rtcheck, sc, expect=None):
    """Variant 0 (and 6 on compact tables) equal the linear scan byte for byte; the frame's last two rows equal the CPU
    checker.  Returns the scan's frame."""
    scan = sc.render(rtmi.Opts(seed=SEED, variant=16))
    assert scan.any()
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED), st)
    if expect is not None:
        assert st.kernel_variant == expect
    assert np.array_equal(img, scan), f"variant 0 (kernel {st.kernel_variant}): {(img != scan).any(axis=2).sum()} pixels differ from the linear scan"
    if st.kernel_variant in (2, 6):
        other = sc.render(rtmi.Opts(seed=SEED, variant=6))
        assert np.array_equal(other, scan), f"variant 6: {(other != scan).any(axis=2).sum()} pixels differ from the linear scan"
    y0, y1 = sc.height - 2, sc.height
    ref, _ = rtcheck.oracle_render(sc, seed=SEED, rows=(y0, y1))
    assert ref[y0:y1].any()
    assert np.array_equal(img[y0:y1], ref[y0:y1]), f"rows {y0} and {y1 - 1} differ from the CPU checker"
    return scan


# ---- 1. the tie vote: taken by some lanes of a wave and not by others, and by none

@pytest.mark.parametrize("small,kernel", [(0.3, 2), (0.45, 6)], ids=["sheet_walk", "3d_walk"])
def test_ties_in_a_cell_and_in_the_prefix_beside_plain_hits(rtmi, rtcheck, small, kernel):
    """A coincident pair among the small spheres (one cell's list holds both; of radius 0.3 the grid stays one cell high and
    variant 0 is the headline instance, of radius 0.45 it grows to three layers and the 3-D walk) and a coincident pair of
    radius 2.5 in the always-tested prefix, in one frame with the sheet, the ground and the sky.  At this camera the small
    pair is four to six pixels across and the big one under thirty: the 8 x 8 tiles that show them hold lanes whose winner
    ties, lanes with a plain hit on the ground or a neighbour, and lanes that hit nothing -- the vote is taken with the tie
    rule's lanes a part of the wave.  The frame changes with the pairs' order, and each order equals the scan and the
    checker."""
    frames = []
    for order in ((0, 4), (4, 0)):
        sc, mats = _field(rtmi)
        for m in order:
            sc.sphere((0.3, small, 2.6), small, mats[m])
        for m in order:
            sc.sphere((-2.0, 2.5, -4.5), 2.5, mats[1 if m == 0 else m])
        frames.append(_held(rtmi, rtcheck, sc, expect=kernel))
    assert not np.array_equal(frames[0], frames[1]), "the pairs' order changed nothing: no tie was resolved"
    # each pair on its own changes the frame too (the two votes are separate sites: the pair pass and the prefix)
    for centre, r, pair in (((0.3, small, 2.6), small, (0, 4)), ((-2.0, 2.5, -4.5), 2.5, (1, 4))):
        one = []
        for order in (pair, pair[::-1]):
            sc, mats = _field(rtmi)
            for m in order:
                sc.sphere(centre, r, mats[m])
            one.append(sc.render(rtmi.Opts(seed=SEED)))
            assert np.array_equal(one[-1], sc.render(rtmi.Opts(seed=SEED, variant=16)))
        assert not np.array_equal(one[0], one[1]), f"the pair of radius {r} never tied"


def test_no_lane_ever_ties(rtmi, rtcheck):
    """The same field without a coincident pair: spheres of distinct random centres and radii, so no two roots of a ray are
    equal and the tie rule's block is never entered."""
    sc, _ = _field(rtmi)
    _held(rtmi, rtcheck, sc, expect=2)


# ---- 2. second candidates: both entries of a pair pass, records 1, 2 and 3 of the prefix, lists of length 1, 2 and 3

BIG = (((-2.0, 2.5, -4.5), 2.5), ((-1.2, 2.3, -4.3), 2.3), ((-1.6, 2.1, -3.8), 2.1))
COMMON = (-1.6, 2.3, -4.2)  # inside all three


def _overlaps(rtmi, w=96, h=54, spp=4, depth=12):
    """A ground sphere; on it singles, overlapping pairs and overlapping triples of radius 0.2 a few cells apart (glass, fuzzy
    metal, matte), so that cells list one, two and three spheres -- a lane whose ray crosses a pair's or a triple's common
    part gets both entries of a pair pass as candidates, its neighbours one or none, and a list of length 1 or 3 reads its
    last pair pass's second entry from past its end; and three overlapping big spheres, which with the ground make a prefix
    of exactly four records: the camera looks at a point inside all three, so the rays about the frame's centre are
    candidates for records 1, 2 and 3 at once, the rays further out for two, one or none."""
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((0.0, 2.5, 9.0), COMMON, (0, 1, 0), 50.0)
    mats = [sc.dielectric(1.5), sc.metal((0.8, 0.7, 0.6), 0.1), sc.lambertian((0.6, 0.3, 0.2))]
    sc.sphere((0.0, -1000.0, 0.0), 1000.0, sc.lambertian((0.5, 0.5, 0.5)))
    r, n = 0.2, 0
    for i in range(-3, 4):
        for j in range(-3, 4):
            x, z = 1.3 * i, 1.3 * j
            for a in range(1 + (i + j) % 3):
                sc.sphere((x + 0.05 * np.cos(2.1 * a), r, z + 0.05 * np.sin(2.1 * a)), r, mats[(n + a) % 3])
            n += 1
    for k, (c, rad) in enumerate(BIG):
        sc.sphere(c, rad, mats[k])
    return sc


def test_second_candidates_in_pair_passes_and_in_the_prefix(rtmi, rtcheck):
    sc = _overlaps(rtmi)
    t = Tables(sc)
    assert not t.t.grid_wide and t.t.grid_cells > 0
    # the prefix: the ground and the three big spheres, nothing else
    assert t.t.np == 4
    assert sorted(float(x) for x in t.img[:4, 3]) == sorted(float(np.float32(r) * np.float32(r)) for r in (2.1, 2.3, 2.5, 1000.0))
    for c, rad in BIG:
        assert np.linalg.norm(np.subtract(COMMON, c)) < 0.8 * rad  # the camera's central rays cross all three
    # lists of length 1, 2 and 3 (odd ones end their last pair pass on the entry behind them)
    assert {1, 2, 3} <= set(int(x) for x in t.n_near), sorted(set(int(x) for x in t.n_near))
    # a list of two or three whose spheres overlap: both entries of a pair pass are candidates on rays through the common part
    overlapping = 0
    for c in np.flatnonzero(t.n_near >= 2):
        s = t.near(c)
        a, b = t.img[s[0]], t.img[s[1]]
        overlapping += int(np.linalg.norm(a[:3] - b[:3]) < 0.5 * (np.sqrt(a[3]) + np.sqrt(b[3])))
    assert overlapping > 0
    _held(rtmi, rtcheck, sc, expect=2)


# ---- 3. the root's slow path entered by a wave with one odd lane

def _tangent_batch(lanes=(0, 17, 63)):
    """Three waves of 64 rays along +x over the sheet of _field from x = -4.25, at heights and depths that meet its spheres,
    the ground or nothing.  In wave w the ray of lane lanes[w] is replaced by one exactly tangent to a sphere about (0, 0.25,
    w - 1) of radius 0.25 (r^2 = 0.0625): origin (-4, 0.5, w - 1), direction (1, 0, 0), so oc = (-4, 0.25, 0),
    cc = fma(16, ...(0.0625 - 0.0625)) = 16, hb = -4, |d|^2 = 1 and disc = fma(hb, hb, -16) = 0 exactly in fp32: below 2^-96,
    the whole wave takes sqrtf().  Its root is (4 - 0) x 1 = 4."""
    rng = np.random.default_rng(11)
    n = 64 * len(lanes)
    o = np.stack([np.full(n, -4.25), rng.uniform(0.02, 0.6, n), rng.uniform(-3.2, 3.2, n)], axis=1).astype(np.float32)
    d = np.stack([np.ones(n), rng.uniform(-0.05, 0.02, n), rng.uniform(-0.1, 0.1, n)], axis=1).astype(np.float32)
    at = []
    for w, lane in enumerate(lanes):
        k = 64 * w + lane
        o[k], d[k] = (-4.0, 0.5, float(w - 1)), (1.0, 0.0, 0.0)
        at.append(k)
    return o, d, at


def _tangent_scene(rtmi, wide):
    sc, mats = _field(rtmi, tall=False)
    first = len(sc.prims())
    for w in range(3):
        sc.sphere((0.0, 0.25, float(w - 1)), 0.25, mats[w])
    if wide:  # other primitives: the wide tables, whose walk (layout 36) the query kernel takes
        sc.xy_rect(-1.0, 1.5, 0.1, 1.0, -3.0, mats[4])
        sc.cylinder(0.3, -0.5, 0.5, mats[1], rotate=((1.0, 0.0, 0.0), 35.0), translate=(2.0, 0.6, 1.0))
    return sc, first


@pytest.mark.parametrize("wide", [False, True], ids=["scan_layouts", "wide_walk"])
def test_a_tangent_ray_among_63_ordinary_ones(rtmi, rtcheck, wide):
    """disc == 0 in one lane of a wave: the slow path's sqrtf() replaces the fast root of every lane.  (Through the ray-query
    entry point: a camera's rays leave one point through jittered pixels, and no pixel's ray can be held to an exact tangent.
    The query kernel and the linear scan take rt_sqrtf<true> and resolve from render_body.h as the render kernels do; the
    function itself, with one odd lane in a wave, is swept over all bit patterns by test_gpu_headline_roots.py.)  The records of all 192
    rays equal the linear scan's bytes in every layout the scene has, t and the primitive of every ray equal the CPU
    checker's closest hit (its own sqrtf) as bits, and the tangent rays hit their sphere at exactly 4."""
    sc, first = _tangent_scene(rtmi, wide)
    o, d, at = _tangent_batch()
    scan = sc.trace(o, d, opts=rtmi.Opts(variant=16))
    for variant in ((0, 36, 44) if wide else (0, 24)):
        st = rtmi.Stats()
        h = sc.trace(o, d, opts=rtmi.Opts(variant=variant), stats=st)
        if variant == 0:
            assert st.kernel_variant == (36 if wide else 16) | rtmi.TRACE_LAYOUT
        assert np.array_equal(h.view(np.uint8), scan.view(np.uint8)), f"layout {variant}: {(h != scan).sum()} records differ from the linear scan"
    osc = rtcheck.OracleScene(sc)
    hits = 0
    for k in range(len(o)):
        hit, _, t, prim = rtcheck.oracle_hit_uv(osc, o[k], d[k])
        if hit:
            hits += 1
            assert scan["prim"][k] == prim and np.float32(t).view(np.uint32) == scan["t"][k:k + 1].view(np.uint32)[0], k
        else:
            assert scan["prim"][k] == -1, k
    assert 64 < hits, "too few ordinary hits beside the tangent rays"
    assert (scan["prim"] == -1).any(), "every lane hit something"
    for w, k in enumerate(at):
        assert scan["prim"][k] == first + w and scan["t"][k] == np.float32(4.0), (k, scan[k])


# ---- 4. the walk's three thresholds, all fed by mask_count

def _counts_held(rtmi, rtcheck, sc, sheet):
    """The counting build (the 3-D walk, kernel 6, also on a sheet) reports resumed walks; its image equals the scan's; its
    counters equal the counting run asked for variant 16 and the CPU checker's own counts (samples, queries, hits, misses,
    scatter events, draws: none of them depends on how candidates are found)."""
    st, cimg = sc.count(rtmi.Opts(seed=SEED), want_image=True)
    assert st.kernel_variant == 6 and st.cull_mode == 5 and st.grid_sheet == sheet
    print("walk_resumed", st.walk_resumed, "queries", st.queries, "lane_groups", st.lane_groups)
    assert st.walk_resumed > 0, "no walk was cut short and resumed"
    scan = sc.render(rtmi.Opts(seed=SEED, variant=16))
    assert np.array_equal(cimg, scan)
    st16 = sc.count(rtmi.Opts(seed=SEED, variant=16))
    for k in ("samples", "queries", "hits", "misses"):
        assert getattr(st, k) == getattr(st16, k), k
    _, want = rtcheck.oracle_render(sc, seed=SEED, want_counts=True)
    got = st.as_dict()
    for k, v in want.items():
        assert got[k] == v, k
    assert got["samples"] == sc.width * sc.height * sc.spp and got["hits"] + got["misses"] == got["queries"]


def test_rtiow_walks_cut_short_and_resumed_on_the_sheet(rtmi, rtcheck):
    """Scene.rtiow(7) at 96 x 54, 8 spp, depth 50 from a camera low over the sheet: grazing rays cross many cells, so waves
    run step passes while some lanes still test (RT_STEP_AT) and leave stragglers for the next iteration (RT_WALK_TAIL,
    RT_WALK_WAITING).  The x-z walk (2) and the 3-D walk (6) equal the scan."""
    sc = rtmi.Scene.rtiow(7, 96, 54, 8, 50)
    sc.camera((13.0, 0.9, 3.0), (0.0, 0.3, 0.0), (0, 1, 0), 25.0)
    _held(rtmi, rtcheck, sc, expect=2)
    _counts_held(rtmi, rtcheck, sc, sheet=1)


def test_volume_walks_cut_short_and_resumed_in_3d(rtmi, rtcheck):
    """400 spheres in a volume seen from its edge, 64 x 40 at 8 spp: variant 0 is the 3-D walk."""
    sc = rtmi.Scene.new(64, 40, 8, 24)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((0.0, 0.5, 7.0), (0.0, 0.0, 0.0), (0, 1, 0), 60.0)
    rng = np.random.default_rng(29)
    mats = _mixed(sc, rng)
    for i in range(400):
        sc.sphere(rng.uniform(-4.0, 4.0, 3), float(rng.uniform(0.05, 0.25)), mats[i % len(mats)])
    assert sc.table_info().grid_n[1] > 1
    _held(rtmi, rtcheck, sc, expect=6)
    _counts_held(rtmi, rtcheck, sc, sheet=0)


# ---- 5. the instances that take the shared code with other template arguments

def _cloud_with_others(rtmi, w=64, h=36, spp=4, depth=12):
    """200 random spheres in a volume with a rectangle and a cylinder among them: the wide tables, whose cells list the two
    behind their spheres (WIDE / OTHERS: kernel 36)."""
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((0.0, 2.0, 14.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0)
    rng = np.random.default_rng(23)
    mats = _mixed(sc, rng)
    for i in range(200):
        sc.sphere(rng.uniform(-3.0, 3.0, 3), float(rng.uniform(0.05, 0.25)), mats[i % len(mats)])
    sc.xy_rect(-1.0, 1.5, -0.5, 1.0, -1.0, mats[4])
    sc.cylinder(0.4, -1.0, 1.0, mats[1], rotate=((1.0, 0.0, 0.0), 35.0), translate=(1.0, 0.5, 1.0))
    return sc


def test_wide_tables_with_a_cylinder_and_a_rectangle_in_the_cells(rtmi, rtcheck):
    sc = _cloud_with_others(rtmi)
    t = Tables(sc)
    assert t.t.grid_wide == 1 and (t.n_other > 0).any(), "no cell lists the rectangle or the cylinder"
    _held(rtmi, rtcheck, sc, expect=36)


def test_closest_hit_queries_through_the_wide_walk(rtmi):
    """1031 rays (sixteen whole waves and a ragged one) from around and inside the same cloud, half aimed into it: the query
    kernel's walk (layout 36, and 44: the same tables from global memory) gives the linear scan's records byte for byte."""
    sc = _cloud_with_others(rtmi)
    rng = np.random.default_rng(31)
    n = 1031
    o = rng.uniform(-4.5, 4.5, (n, 3))
    d = np.where((np.arange(n) % 2 == 0)[:, None], rng.uniform(-3.0, 3.0, (n, 3)) - o, rng.normal(0.0, 1.0, (n, 3)))
    o, d = o.astype(np.float32), d.astype(np.float32)
    scan = sc.trace(o, d, opts=rtmi.Opts(variant=16))
    hit = scan["prim"] >= 0
    assert 200 < hit.sum() < n - 200
    kinds = set(int(x) for x in sc.prims()["type"][scan["prim"][hit]])
    assert len(kinds) == 3, f"the rays met {kinds}: not spheres, the rectangle and the cylinder"
    for variant in (0, 36, 44):
        st = rtmi.Stats()
        h = sc.trace(o, d, opts=rtmi.Opts(variant=variant), stats=st)
        assert st.kernel_variant == (variant or 36) | rtmi.TRACE_LAYOUT
        assert np.array_equal(h.view(np.uint8), scan.view(np.uint8)), f"layout {variant}: {(h != scan).sum()} records differ from the linear scan"
