"""-m gpu: the sphere-only compact-table instances (variants 2 and 6), whose bursts trace their 64 camera rays (render_body.h):
the first closest-hit query of every path runs in the burst, a path that ends there (the sky, an emitter, the roulette) is
settled there, and a lane that pops the slot of a scattering hit rebuilds the hit record and goes straight to its scatter
step.  Every frame is held to the reference's linear scan (variant 16) byte for byte on the whole frame and to the CPU
checker on two rows; each scene asserts that variant 0 resolves to 2, so that the instance under test is the one that runs.
The frames are at most 24 x 16 pixels (24 x 40 for the shard, and 32 x 24 for the tile list, whose passes need tiles that stop
at different sample counts: the frame of test_gpu_headline_bursts.py's case), so a case is a few launches of milliseconds; the scan and the
checker's rows of a configuration are computed once and shared by the two variants.

What the cases reach: batches in which every slot is dead (a view of the sky: re-pops over dead slots, several bursts inside
one refill, the last batch of an item ending the loop), batches in which every slot is live (a view straight down), off-image,
dead and live slots in one batch (17 x 9), each material as the first vertex (matte, fuzzy metal, glass from outside and from
inside, a checker ground), an emitter that ends the path in the burst, the roulette's first draw in the burst with and without
a lens, paths that end at or right after the popped vertex (depth 1 and 2), ties at the first hit in a cell's list and in the
prefix, first walks across the whole sheet (the burst's walk is never cut short), and the hand-out cases of
test_gpu_headline_bursts.py once more: a shard's rows, a tile list, fewer items than waves."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 2023
VIEW = ((0.0, 2.0, 9.0), (0.0, 0.4, 0.0))       # the sheet from the front: sky above the horizon, spheres and ground below
SKY = ((0.0, 2.0, 9.0), (0.0, 12.0, 19.0))      # up and away from the scene: every camera ray leaves it
DOWN = ((0.0, 7.0, 0.0), (0.0, 0.0, 0.0))       # straight down at the sheet: every camera ray hits the ground or a sphere
ALONG = ((-11.0, 0.22, 0.05), (11.0, 0.2, 0.0))  # low over the sheet, along its long side: first walks of many cells


def _scene(rtmi, w, h, spp, depth=8, view=VIEW, aperture=0.0, defocus=False, rr=0.0, ground=None, extra=None, nx=5, nz=5, sky=True):
    """A ground sphere and an nx x nz sheet of small spheres on it (matte, metal, glass), plus what `extra(sc, mats)` adds:
    spheres only and one cell high, so the compact tables -- variant 0 is the x-z walk (2), and the 3-D walk (6) reads the
    same tables."""
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.7, 0.8, 1.0) if sky else (0.3, 0.4, 0.5), sky_gradient=sky, defocus_blur=defocus)
    vup = (0, 0, -1) if view is DOWN else (0, 1, 0)
    sc.camera(view[0], view[1], vup, 40.0, aperture=aperture, focus_dist=9.0 if aperture > 0.0 else 0.0)
    rng = np.random.default_rng(5)
    mats = [sc.lambertian(rng.uniform(0.2, 0.9, 3)) for _ in range(3)] + [sc.metal((0.8, 0.8, 0.8), 0.1), sc.dielectric(1.5)]
    sc.sphere((0.0, -1000.0, 0.0), 1000.0, mats[0] if ground is None else ground(sc))
    for i in range(nx):
        for j in range(nz):
            r = float(rng.uniform(0.2, 0.3))
            sc.sphere((1.2 * (i - (nx - 1) / 2) + float(rng.uniform(-0.2, 0.2)), r, 1.2 * (j - (nz - 1) / 2) + float(rng.uniform(-0.2, 0.2))), r,
                      mats[(nz * i + j) % len(mats)])
    if extra is not None:
        extra(sc, mats)
    if rr > 0.0:
        sc.set_russian_roulette(rr)
    info = sc.table_info()
    assert not info.grid_wide and info.grid_cells > 0 and info.kernel_variant == 2
    return sc


def _first_queries(rtcheck, sc, sample=0):
    """The checker's first closest-hit query of one sample of every pixel: (hits, misses, paths that made no query)."""
    hits = misses = none = 0
    for y in range(sc.height):
        for x in range(sc.width):
            _, q = rtcheck.oracle_trace_sample(sc, SEED, x, y, sample, max_queries=1)
            if len(q) == 0:
                none += 1
            elif q[0][7] != 0.0:
                hits += 1
            else:
                misses += 1
    return hits, misses, none


_refs = {}


def _reference(rtmi, rtcheck, key, sc, lit=True, **opts):
    """The linear scan's frame and the CPU checker's first two rows of the frame (of a shard: of its first two local rows),
    once per configuration.  lit: those two rows are not all black."""
    if key not in _refs:
        scan = sc.render(rtmi.Opts(seed=SEED, variant=16, **opts))
        assert scan.any()
        o = rtmi.Opts(seed=SEED, **opts)
        rows = [int(g) for g in sc.shard_global_rows(o)[:2]]
        chk = np.stack([rtcheck.oracle_render(sc, seed=SEED, rows=(g, g + 1))[0][g] for g in rows])
        assert chk.any() or not lit
        _refs[key] = (scan, chk)
    return _refs[key]


def _held(rtmi, rtcheck, key, sc, variant, lit=True, **opts):
    scan, chk = _reference(rtmi, rtcheck, key, sc, lit=lit, **opts)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED, variant=variant, **opts), st)
    assert st.kernel_variant == variant
    assert img.shape == scan.shape
    assert np.array_equal(img, scan), f"variant {variant}: {(img != scan).any(axis=2).sum()} pixels differ from the linear scan"
    assert np.array_equal(img[:2], chk), f"variant {variant}: the first two rows differ from the CPU checker"
    return img


# ---- every slot dead, every slot live, and all three kinds in one batch

@pytest.mark.parametrize("variant", [2, 6])
@pytest.mark.parametrize("spp,chunk", [(1, 0), (3, 0), (3, 1), (65, 0), (65, 1)], ids=["spp1", "spp3", "spp3_chunk1", "spp65", "spp65_chunk1"])
def test_only_misses(rtmi, rtcheck, spp, chunk, variant):
    """The camera looks at the sky: every path ends in its burst, every slot is dead.  A lane that wants a path pops dead slots
    through the whole batch, the loop runs burst after burst inside one refill, and the last batch of an item ends it with
    the lanes still unserved."""
    sc = _scene(rtmi, 24, 16, spp, view=SKY)
    if ("sky", "first") not in _refs:
        _refs[("sky", "first")] = _first_queries(rtcheck, _scene(rtmi, 24, 16, 1, view=SKY))
    assert _refs[("sky", "first")] == (0, 24 * 16, 0)
    _held(rtmi, rtcheck, ("sky", spp, chunk), sc, variant, spp_chunk=chunk)


@pytest.mark.parametrize("variant", [2, 6])
@pytest.mark.parametrize("spp,chunk", [(1, 0), (65, 1)], ids=["spp1", "spp65_chunk1"])
def test_only_scattering_hits(rtmi, rtcheck, spp, chunk, variant):
    """The camera looks straight down at the ground: every slot holds a hit point, every pop rebuilds a hit record."""
    sc = _scene(rtmi, 24, 16, spp, view=DOWN)
    if ("down", "first") not in _refs:
        _refs[("down", "first")] = _first_queries(rtcheck, _scene(rtmi, 24, 16, 1, view=DOWN))
    assert _refs[("down", "first")] == (24 * 16, 0, 0)
    _held(rtmi, rtcheck, ("down", spp, chunk), sc, variant, spp_chunk=chunk)


@pytest.mark.parametrize("variant", [2, 6])
@pytest.mark.parametrize("spp,chunk", [(1, 0), (3, 1), (65, 0)], ids=["spp1", "spp3_chunk1", "spp65"])
def test_off_image_dead_and_live_slots_in_one_batch(rtmi, rtcheck, spp, chunk, variant):
    """17 x 9, sky above the horizon: ragged tiles, so every batch holds off-image slots beside those of paths that ended in the
    burst and those that go on."""
    sc = _scene(rtmi, 17, 9, spp)
    if ("mixed", "first") not in _refs:
        _refs[("mixed", "first")] = _first_queries(rtcheck, _scene(rtmi, 17, 9, 1))
    hits, misses, none = _refs[("mixed", "first")]
    assert hits > 0 and misses > 0 and none == 0
    _held(rtmi, rtcheck, ("mixed", spp, chunk), sc, variant, spp_chunk=chunk)


# ---- each material as the first vertex

def _ball(material):
    """a sphere of radius 1.1 in front of the camera, filling the middle of the view (and, above four times the median radius, a
    member of the always-tested prefix)"""
    return lambda sc, mats: sc.sphere((0.0, 1.1, 5.5), 1.1, material(sc, mats))


FIRST_VERTEX = {
    "matte": dict(extra=_ball(lambda sc, mats: mats[1])),
    "fuzzy_metal": dict(extra=_ball(lambda sc, mats: sc.metal((0.9, 0.7, 0.5), 0.4))),
    "glass_outside": dict(extra=_ball(lambda sc, mats: sc.dielectric(1.5))),
    # the camera stands at the centre of a glass sphere: front == false at every first hit
    "glass_inside": dict(extra=lambda sc, mats: sc.sphere((0.0, 2.0, 9.0), 1.2, sc.dielectric(1.5))),
    "checker_ground": dict(ground=lambda sc: sc.lambertian(sc.checker_texture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))),
}


@pytest.mark.parametrize("variant", [2, 6])
@pytest.mark.parametrize("what", list(FIRST_VERTEX))
def test_each_material_as_the_first_vertex(rtmi, rtcheck, what, variant):
    sc = _scene(rtmi, 24, 16, 5, **FIRST_VERTEX[what])
    img = _held(rtmi, rtcheck, ("vertex", what), sc, variant)
    if what != "matte":  # (the matte ball is the scene every other case changes one thing of)
        plain = _reference(rtmi, rtcheck, ("vertex", "matte"), _scene(rtmi, 24, 16, 5, **FIRST_VERTEX["matte"]))[0]
        assert not np.array_equal(img, plain), "the material changed nothing"


def test_inside_the_glass_sphere_every_first_hit_is_a_back_face(rtmi, rtcheck):
    """The checker's first query of every pixel hits at t |d| = 1.2, the sphere's radius: the camera ray leaves the glass."""
    sc = _scene(rtmi, 24, 16, 1, **FIRST_VERTEX["glass_inside"])
    for x, y in ((0, 0), (23, 15), (12, 8)):
        _, q = rtcheck.oracle_trace_sample(sc, SEED, x, y, 0, max_queries=1)
        assert q[0][7] != 0.0 and abs(q[0][6] * float(np.linalg.norm(q[0][3:6])) - 1.2) < 1e-3


@pytest.mark.parametrize("variant", [2, 6])
@pytest.mark.parametrize("sky", [True, False], ids=["sky", "constant_background"])
def test_an_emitter_ends_the_path_in_the_burst(rtmi, rtcheck, sky, variant):
    """An emissive sphere fills the middle of the view: those paths add their emission in the burst; under the constant
    background the burst's miss takes the other branch as well."""
    lamp = _ball(lambda sc, mats: sc.diffuse_light((4.0, 3.0, 2.0)))
    sc = _scene(rtmi, 24, 16, 5, extra=lamp, sky=sky)
    img = _held(rtmi, rtcheck, ("lamp", sky), sc, variant)
    assert img.max() >= 4.0 * 5, "no pixel looked into the emitter with all of its samples"


# ---- the roulette's first draw in the burst

@pytest.mark.parametrize("variant", [2, 6])
@pytest.mark.parametrize("defocus", [False, True], ids=["pinhole", "lens"])
def test_russian_roulette_draws_in_the_burst(rtmi, rtcheck, variant, defocus):
    """rr = 0.8: a starting path's draw follows the lens loop in the burst, a killed path leaves a dead slot and adds nothing,
    and a survivor's slot holds the state after the draw.  Checked on the scene first: the roulette kills paths whose camera
    ray would have reached the sky (the order of draw and add matters for them), and paths that would have hit."""
    kw = dict(depth=12, aperture=0.3 if defocus else 0.0, defocus=defocus)
    sc = _scene(rtmi, 17, 9, 6, rr=0.8, **kw)
    key = ("roulette", defocus)
    if (key, "first") not in _refs:
        free = _scene(rtmi, 17, 9, 6, **kw)
        killed_sky = killed_hit = 0
        for y in range(9):
            for x in range(17):
                _, q = rtcheck.oracle_trace_sample(sc, SEED, x, y, 0, max_queries=1)
                if len(q) == 0:  # no query: the roulette ended the path at its start
                    _, f = rtcheck.oracle_trace_sample(free, SEED, x, y, 0, max_queries=1)
                    killed_sky += f[0][7] == 0.0
                    killed_hit += f[0][7] != 0.0
        _refs[(key, "first")] = (killed_sky, killed_hit)
    killed_sky, killed_hit = _refs[(key, "first")]
    assert killed_sky > 0 and killed_hit > 0
    _held(rtmi, rtcheck, key, sc, variant)


# ---- paths that end at or right after the popped vertex

@pytest.mark.parametrize("variant", [2, 6])
@pytest.mark.parametrize("depth", [1, 2])
def test_short_paths(rtmi, rtcheck, depth, variant):
    """max_depth 1: the popped vertex's scatter step uses up the depth, only the burst's own additions are left in the frame;
    max_depth 2: one ray after it."""
    sc = _scene(rtmi, 24, 16, 5, depth=depth)
    # (the frame's first two rows see the ground: at depth 1 they are black, and the sky's rows carry the frame)
    _held(rtmi, rtcheck, ("depth", depth), sc, variant, lit=depth > 1)


# ---- ties at the first hit: of two coincident spheres the later list entry wins

@pytest.mark.parametrize("variant", [2, 6])
@pytest.mark.parametrize("where", ["cell", "prefix"])
def test_ties_at_the_first_hit(rtmi, rtcheck, where, variant):
    """Two spheres with the same centre and radius and different materials, seen by camera rays: small ones (one cell's list
    holds both) or of radius 1.1 (both in the prefix).  The frame differs from that of the pair in the other order."""
    frames = []
    for order in ((1, 4), (4, 1)):
        def pair(sc, mats, order=order):
            for m in order:
                if where == "cell":
                    sc.sphere((0.3, 0.3, 4.5), 0.3, mats[m])
                else:
                    sc.sphere((0.0, 1.1, 5.5), 1.1, mats[m])
        sc = _scene(rtmi, 24, 16, 5, extra=pair)
        frames.append(_held(rtmi, rtcheck, ("tie", where, order), sc, variant))
    assert not np.array_equal(frames[0], frames[1]), "the pair's order changed nothing: no tie was resolved"


# ---- long first walks

@pytest.mark.parametrize("variant", [2, 6])
def test_first_walks_along_the_sheet(rtmi, rtcheck, variant):
    """A camera low over a sheet of 16 x 3 spheres, looking along it: camera rays cross many cells before they hit or leave.
    The main loop would cut such a walk short and go on in the next iteration; the burst's walk runs to its end."""
    sc = _scene(rtmi, 24, 16, 5, view=ALONG, nx=16, nz=3)
    assert sc.table_info().grid_cells >= 16
    _held(rtmi, rtcheck, ("along",), sc, variant)


# ---- the hand-out cases of the bursts' file, on the view with dead and live slots

@pytest.mark.parametrize("variant", [2, 6])
@pytest.mark.parametrize("rotate", [0, 2])
def test_a_shard_of_row_tiles(rtmi, rtcheck, variant, rotate):
    """Shard 2 of 3 over row tiles of 4 rows (tile_first = tile_stride - 1 = 2; tile_rotate 0 and 2): the home row that shares
    its register with the winner's id goes through the shard's deal."""
    sc = _scene(rtmi, 24, 40, 3)
    _held(rtmi, rtcheck, ("shard", rotate), sc, variant, tile_rows=4, tile_first=2, tile_stride=3, tile_rotate=rotate)


@pytest.mark.parametrize("variant", [2, 6])
def test_an_adaptive_tile_list(rtmi, rtcheck, variant):
    """Adaptive sampling renders its later passes from a tile list: the sums and the sample counts equal the linear scan's,
    and two rows equal the checker's sums of each pixel's own sample count."""
    sc = _scene(rtmi, 32, 24, 32)
    key = ("adaptive",)
    if key not in _refs:
        # the first threshold of a falling ladder at which the scan's tiles stop at two or more different counts: the later
        # passes then render a list that holds a part of the frame's tiles
        for thr in (0.5, 0.3, 0.2, 0.12, 0.08, 0.05, 0.03):
            img, spp, st = sc.render_adaptive(thr, min_spp=4, opts=rtmi.Opts(seed=SEED, variant=16))
            if st.passes > 1 and len(np.unique(spp)) > 1:
                break
        assert st.passes > 1 and len(np.unique(spp)) > 1, "one pass, or one sample count: no partial tile list was rendered"
        _refs[("adaptive", "threshold")] = thr
        chk = np.zeros((2,) + img.shape[1:], dtype=np.float32)
        for n in np.unique(spp[:2]):
            ref, _ = rtcheck.oracle_render(sc, seed=SEED, rows=(0, 2), sample_count=int(n))
            chk[spp[:2] == n] = ref[:2][spp[:2] == n]
        _refs[key] = (img, spp, chk)
    scan, scan_spp, chk = _refs[key]
    img, spp, _ = sc.render_adaptive(_refs[("adaptive", "threshold")], min_spp=4, opts=rtmi.Opts(seed=SEED, variant=variant))
    assert np.array_equal(spp, scan_spp)
    assert np.array_equal(img, scan)
    assert np.array_equal(img[:2], chk)


@pytest.mark.parametrize("variant", [2, 6])
@pytest.mark.parametrize("spp", [1, 2])
def test_fewer_items_than_a_workgroup_has_waves(rtmi, rtcheck, variant, spp):
    """9 x 5 pixels: two tiles, so two or four items for the fifteen waves of the one workgroup -- the others find the queue
    empty at their first fetch and leave."""
    sc = _scene(rtmi, 9, 5, spp)
    _held(rtmi, rtcheck, ("tiny", spp), sc, variant, spp_chunk=1)


@pytest.mark.parametrize("variant", [2, 6])
def test_two_renders_are_equal(rtmi, variant):
    sc = _scene(rtmi, 17, 9, 65, rr=0.8, depth=12)
    a = sc.render(rtmi.Opts(seed=SEED, variant=variant))
    b = sc.render(rtmi.Opts(seed=SEED, variant=variant))
    assert a.any() and np.array_equal(a, b)
