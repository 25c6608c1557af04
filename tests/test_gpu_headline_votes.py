"""-m gpu: the paths that the headline kernel's second instruction diet touches -- the wave votes kept as lane masks (the
query's entry, the walk's entry, the scan from beyond the lists, the refill's start mask and the loop's exit), the walk state
and the rejection loop's sample left unset for the lanes that never read them, the tile accumulator's 32-bit LDS address, the
tie rule's 32-bit record offset and the off-image mark in a pool pixel's row -- each held to the reference's linear scan (variant 16) byte for byte through the
default kernel (and the 3-D walk, variant 6, where the scene has the compact tables), and two rows of each frame to the CPU
checker.  Small frames: every case is a few launches of well under a second."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 2023
CAM = (0.0, 2.0, 14.0)


def _mixed(sc, rng):
    return [sc.lambertian(rng.uniform(0.2, 0.9, 3)) for _ in range(4)] + [sc.metal((0.8, 0.8, 0.8), 0.1), sc.dielectric(1.5)]


def _glass_and_lamps(sc, rng):
    return [sc.dielectric(1.5), sc.diffuse_light((4.0, 3.0, 2.0)), sc.dielectric(1.3), sc.diffuse_light((1.0, 2.0, 5.0))]


def _field(rtmi, w, h, spp, depth, materials=_mixed, sky=True, background=(0.7, 0.8, 1.0), defocus=False, lookfrom=CAM,
           lookat=(-3.1, 1.0, 0.0), ground=None):
    """A ground sphere, a 6 x 6 sheet of small spheres on it and one sphere taller than the layer: spheres only, so the
    compact tables and a grid one cell high -- variant 0 is the x-z walk (2), and the 3-D walk (6) reads the same tables.
    Returns the scene and its materials."""
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background(background, sky_gradient=sky, defocus_blur=defocus)
    sc.camera(lookfrom, lookat, (0, 1, 0), 40.0, aperture=0.3 if defocus else 0.0, focus_dist=12.0 if defocus else 0.0)
    rng = np.random.default_rng(5)
    mats = materials(sc, rng)
    sc.sphere((0.0, -1000.0, 0.0), 1000.0, mats[0] if ground is None else ground(sc))
    for i in range(6):
        for j in range(6):
            r = float(rng.uniform(0.15, 0.25))
            sc.sphere((1.1 * (i - 2.5) + float(rng.uniform(-0.2, 0.2)), r, 1.1 * (j - 2.5) + float(rng.uniform(-0.2, 0.2))), r,
                      mats[(6 * i + j) % len(mats)])
    sc.sphere((0.4, 1.0, -0.3), 1.0, mats[-1])  # taller than the layer of cells
    return sc, mats


def _held(rtmi, rtcheck, sc, rows=None, **kw):
    """Variant 0 (and 6 on compact tables) equal the linear scan byte for byte; rows [y0, y1) equal the CPU checker."""
    scan = sc.render(rtmi.Opts(seed=SEED, variant=16, **kw))
    assert scan.any()
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED, **kw), st)
    assert np.array_equal(img, scan), f"variant 0 (kernel {st.kernel_variant}): {(img != scan).any(axis=2).sum()} pixels differ from the linear scan"
    if st.kernel_variant in (2, 6):
        other = sc.render(rtmi.Opts(seed=SEED, variant=6, **kw))
        assert np.array_equal(other, scan), f"variant 6: {(other != scan).any(axis=2).sum()} pixels differ from the linear scan"
    y0, y1 = rows if rows is not None else (sc.height - 2, sc.height)
    ref, _ = rtcheck.oracle_render(sc, seed=SEED, rows=(y0, y1), spp_chunk=kw.get("spp_chunk", 0))
    assert np.array_equal(img[y0:y1], ref[y0:y1]), f"rows {y0} .. {y1 - 1} differ from the CPU checker"
    return scan, st


# ---- votes with empty and nearly empty waves

def test_one_ragged_tile_most_waves_never_get_an_item(rtmi, rtcheck):
    """5 x 3 at 1 spp: one work item whose pool is mostly off-image (49 of 64 pixels carry the off-image row); every other
    wave of the launch finds the queue dry and leaves through the exit that the start mask and the idle mask now decide."""
    sc, _ = _field(rtmi, 5, 3, 1, 8)
    _held(rtmi, rtcheck, sc, rows=(1, 3))


def test_items_of_one_sample_retire_with_orphans_alive(rtmi, rtcheck):
    """9 x 9 at 3 spp in chunks of one sample: four ragged tiles, twelve items of at most 64 paths each, so items retire while
    paths are alive (orphans) and idle lanes wait for the orphan bound."""
    sc, _ = _field(rtmi, 9, 9, 3, 8)
    _held(rtmi, rtcheck, sc, spp_chunk=1)


# ---- a rejection loop nobody enters, one only disk lanes enter, one both kinds share

def test_no_lane_draws_a_sphere_or_disk_sample(rtmi, rtcheck):
    """Dielectric and emissive spheres under a constant background, no defocus blur: no lane ever enters the rejection loop,
    and the scatter step and the camera ray read nothing of its (unset) sample."""
    sc, _ = _field(rtmi, 96, 54, 3, 8, materials=_glass_and_lamps, sky=False, background=(0.3, 0.4, 0.5))
    _held(rtmi, rtcheck, sc)


def test_only_starting_lanes_enter_the_rejection_loop(rtmi, rtcheck):
    """The same scene through a lens: only lanes that start a path sample (a disk: two draws, z = 0)."""
    sc, _ = _field(rtmi, 96, 54, 3, 8, materials=_glass_and_lamps, sky=False, background=(0.3, 0.4, 0.5), defocus=True)
    blur_off, _ = _field(rtmi, 96, 54, 3, 8, materials=_glass_and_lamps, sky=False, background=(0.3, 0.4, 0.5))
    scan, _ = _held(rtmi, rtcheck, sc)
    assert not np.array_equal(scan, blur_off.render(rtmi.Opts(seed=SEED, variant=16))), "the lens changed nothing"


def test_sphere_and_disk_lanes_share_one_loop(rtmi, rtcheck):
    """Lambertian and metal spheres through a lens: scattering lanes (three draws) and starting lanes (two) in one loop."""
    sc, _ = _field(rtmi, 96, 54, 3, 8, defocus=True)
    _held(rtmi, rtcheck, sc)


# ---- walk state of lanes that never enter the grid

def test_primary_rays_miss_the_grid_and_bounces_enter_it(rtmi, rtcheck):
    """The camera above the sheet, looking up at a fuzz-free mirror of radius 1000 whose lowest point hangs 30 units above the
    ground: no primary ray meets the grid's bounds (the lanes' walk state stays unset), and what the mirror sends back
    enters the grid from the far tier of the cells' lists."""
    sc, _ = _field(rtmi, 96, 54, 3, 8, lookfrom=(0.0, 6.0, 0.5), lookat=(0.0, 30.0, 0.0))
    sc.sphere((0.0, 1030.0, 0.0), 1000.0, sc.metal((0.95, 0.95, 0.95), 0.0))
    st = sc.count(rtmi.Opts(seed=SEED))
    assert st.lane_groups > 0, "no lane entered the grid"
    assert st.queries > st.lane_groups + st.query_maxpop, "every query reached the grid"
    _held(rtmi, rtcheck, sc)


def test_far_tier_and_beyond_mirrors(rtmi, rtcheck):
    """Two fuzz-free mirrors of radius 1000 that touch points about 40 and about 90 units from the sheet and face so that the
    camera's ray to each point goes on to the sheet's centre: queries come back from the far tier and from beyond the lists'
    reach (the scan whose lanes are now a lane mask), next to the near tier's."""
    sc, _ = _field(rtmi, 96, 54, 4, 8)
    cam = np.array(CAM)
    mirror = sc.metal((0.95, 0.95, 0.95), 0.0)
    for reach, towards in ((40.0, (-0.9, 0.25, -0.6)), (90.0, (0.35, 0.25, -1.0))):
        p = reach * np.array(towards) / np.linalg.norm(towards)
        n = (cam - p) / np.linalg.norm(cam - p) - p / np.linalg.norm(p)  # bisects the directions to the camera and to the sheet
        c = p - 1000.0 * n / np.linalg.norm(n)
        sc.sphere(tuple(float(x) for x in c), 1000.0, mirror)
    st = sc.count(rtmi.Opts(seed=SEED))
    assert st.group_maxpop > 0, "no lane walked the far tier"
    assert st.query_maxpop > 0, "no lane scanned from beyond the lists' reach"
    assert st.lane_groups > st.group_maxpop, "no lane walked the near tier"
    _held(rtmi, rtcheck, sc)


# ---- the tile accumulator's address

def test_one_full_tile_all_192_sums(rtmi, rtcheck):
    """An 8 x 8 frame at 16 spp under a bright constant background: every one of the tile's 192 sums is non-zero."""
    sc, _ = _field(rtmi, 8, 8, 16, 8, sky=False, background=(3.0, 2.0, 1.5))
    scan, _ = _held(rtmi, rtcheck, sc)
    assert (scan > 0).all()


def test_one_full_tile_radiance_above_128(rtmi, rtcheck):
    """The same tile with emitters of radiance 300 among the spheres and as the tall sphere in the frame's middle: samples at
    and above 128 take the wide fixed-point conversion, and the sums keep their 24-byte stride."""
    lamps = lambda sc, rng: [sc.lambertian(rng.uniform(0.2, 0.9, 3)), sc.diffuse_light((300.0, 200.0, 150.0))]
    sc, _ = _field(rtmi, 8, 8, 16, 8, materials=lamps, sky=False, background=(3.0, 2.0, 1.5), lookat=(0.4, 1.0, -0.3))
    scan, _ = _held(rtmi, rtcheck, sc)
    assert (scan > 0).all()
    assert scan.max() > 300.0, "no sample looked into an emitter"


# ---- the tie rule: of two coincident spheres the later list entry wins

def test_coincident_small_spheres_in_one_cell(rtmi, rtcheck):
    """Two spheres with the same centre and radius and different materials among the small ones (one cell's list holds
    both).  The frame differs from that of the pair in the other order, and each equals the scan and the checker."""
    frames = []
    for order in ((0, 4), (4, 0)):
        sc, mats = _field(rtmi, 96, 54, 3, 8, lookat=(0.0, 0.5, 0.0))
        for m in order:
            sc.sphere((0.3, 0.45, 2.6), 0.45, mats[m])
        frames.append(_held(rtmi, rtcheck, sc)[0])
    assert not np.array_equal(frames[0], frames[1]), "the pair's order changed nothing: no tie was resolved"


def test_coincident_big_spheres_in_the_prefix(rtmi, rtcheck):
    """Two coincident spheres of radius 2.5 (above four times the median radius: both in the always-tested prefix)."""
    frames = []
    for order in ((1, 4), (4, 1)):
        sc, mats = _field(rtmi, 96, 54, 3, 8, lookat=(0.0, 0.5, 0.0))
        for m in order:
            sc.sphere((-2.0, 2.5, -4.5), 2.5, mats[m])
        frames.append(_held(rtmi, rtcheck, sc)[0])
    assert not np.array_equal(frames[0], frames[1]), "the pair's order changed nothing: no tie was resolved"


def test_a_prefix_sphere_and_a_cell_sphere_with_equal_roots(rtmi, rtcheck):
    """The prefix holds the spheres above four times the median radius, so two spheres with the SAME radius are never split
    between the prefix and a cell.  The nearest thing that can be built: a hollow-glass pair, radius 1.0 (the tall sphere, in
    the prefix) and -1.0 about the same centre -- |r| decides the part, so both land in the prefix as well, and their roots
    tie on every ray; plus a coincident pair in a cell under it.  Ties between the two parts would need equal roots from
    unequal spheres, which fp32 does not give on purpose."""
    frames = []
    for order in ((2, 4), (4, 2)):
        sc, mats = _field(rtmi, 96, 54, 3, 8, lookat=(0.0, 0.5, 0.0))
        sc.sphere((0.4, 1.0, -0.3), -1.0, mats[order[0]])  # coincides with the tall sphere, which comes first in the list
        for m in order:
            sc.sphere((0.4, 0.2, 1.2), 0.2, mats[m])
        frames.append(_held(rtmi, rtcheck, sc)[0])
    assert not np.array_equal(frames[0], frames[1]), "the pair's order changed nothing: no tie was resolved"
