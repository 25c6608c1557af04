"""-m gpu: the sphere-only compact-table instances (variants 2 and 6) in their workgroups of 15 waves, whose paths start from
a per-wave slab of 64 prepared camera rays (render_body.h, the burst).  Every frame is held to the reference's linear scan
(variant 16) byte for byte on the whole frame and to the CPU checker on two rows.  The frames are at most 24 x 16 pixels, so a
case is a few launches of milliseconds; the scan and the checker's rows of a configuration are computed once and shared by
the two variants.

What the cases reach: one batch per item (spp 1), items of several batches and a last item shorter than the others (spp 3 and
65, in chunks of 1 and the default), ragged tiles whose every batch holds off-image slots (17 x 9), the lens disk's own
rejection loop with a real lens and with radius 0, the roulette draw that follows a pop from the stored generator state,
a shard's rows, a tile list, and a launch of fewer items than a workgroup has waves."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 2023
SIZES = {"24x16": (24, 16), "17x9": (17, 9)}


def _sheet(rtmi, w, h, spp, depth=8, aperture=0.0, defocus=False, rr=0.0):
    """A ground sphere and a 5 x 5 sheet of small spheres on it (matte, metal, glass): spheres only and one cell high, so the
    compact tables -- variant 0 is the x-z walk (2), and the 3-D walk (6) reads the same tables."""
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=defocus)
    sc.camera((0.0, 2.0, 9.0), (0.0, 0.4, 0.0), (0, 1, 0), 40.0, aperture=aperture, focus_dist=9.0 if aperture > 0.0 else 0.0)
    rng = np.random.default_rng(5)
    mats = [sc.lambertian(rng.uniform(0.2, 0.9, 3)) for _ in range(3)] + [sc.metal((0.8, 0.8, 0.8), 0.1), sc.dielectric(1.5)]
    sc.sphere((0.0, -1000.0, 0.0), 1000.0, mats[0])
    for i in range(5):
        for j in range(5):
            r = float(rng.uniform(0.2, 0.3))
            sc.sphere((1.2 * (i - 2) + float(rng.uniform(-0.2, 0.2)), r, 1.2 * (j - 2) + float(rng.uniform(-0.2, 0.2))), r,
                      mats[(5 * i + j) % len(mats)])
    if rr > 0.0:
        sc.set_russian_roulette(rr)
    info = sc.table_info()
    assert not info.grid_wide and info.grid_cells > 0 and info.kernel_variant == 2
    return sc


_refs = {}


def _reference(rtmi, rtcheck, key, sc, **opts):
    """The linear scan's frame and the CPU checker's first two rows of the frame (of a shard: of its first two local rows),
    once per configuration."""
    if key not in _refs:
        scan = sc.render(rtmi.Opts(seed=SEED, variant=16, **opts))
        assert scan.any()
        o = rtmi.Opts(seed=SEED, **opts)
        rows = [int(g) for g in sc.shard_global_rows(o)[:2]]
        chk = np.stack([rtcheck.oracle_render(sc, seed=SEED, rows=(g, g + 1))[0][g] for g in rows])
        assert chk.any()
        _refs[key] = (scan, chk)
    return _refs[key]


def _held(rtmi, rtcheck, key, sc, variant, **opts):
    scan, chk = _reference(rtmi, rtcheck, key, sc, **opts)
    st = rtmi.Stats()
    img = sc.render(rtmi.Opts(seed=SEED, variant=variant, **opts), st)
    assert st.kernel_variant == variant
    assert img.shape == scan.shape
    assert np.array_equal(img, scan), f"variant {variant}: {(img != scan).any(axis=2).sum()} pixels differ from the linear scan"
    assert np.array_equal(img[:2], chk), f"variant {variant}: the first two rows differ from the CPU checker"


@pytest.mark.parametrize("variant", [2, 6])
@pytest.mark.parametrize("spp,chunk", [(1, 0), (3, 0), (3, 1), (65, 0), (65, 1)], ids=["spp1", "spp3", "spp3_chunk1", "spp65", "spp65_chunk1"])
@pytest.mark.parametrize("size", list(SIZES))
def test_batches_per_item_and_ragged_tiles(rtmi, rtcheck, size, spp, chunk, variant):
    w, h = SIZES[size]
    sc = _sheet(rtmi, w, h, spp)
    _held(rtmi, rtcheck, ("plain", size, spp, chunk), sc, variant, spp_chunk=chunk)


def test_variant_0_is_the_instance_under_test(rtmi):
    """rt_stats.kernel_variant: the default kernel of this file's scene is the headline instance, and asking for 6 runs 6."""
    sc = _sheet(rtmi, 24, 16, 3)
    st = rtmi.Stats()
    sc.render(rtmi.Opts(seed=SEED), st)
    assert st.kernel_variant == 2
    sc.render(rtmi.Opts(seed=SEED, variant=6), st)
    assert st.kernel_variant == 6


@pytest.mark.parametrize("variant", [2, 6])
@pytest.mark.parametrize("aperture", [0.3, 0.0], ids=["lens", "radius0"])
@pytest.mark.parametrize("size", list(SIZES))
def test_defocus_blur_draws_its_disk_in_the_burst(rtmi, rtcheck, size, aperture, variant):
    """RT_FLAG_DEFOCUS_BLUR on: every sample draws its lens point (two draws per attempt) between the jitter and the first
    bounce, with a lens of radius 0 as well -- the draws are spent and the offset is zero."""
    w, h = SIZES[size]
    sc = _sheet(rtmi, w, h, 5, aperture=aperture, defocus=True)
    assert (sc.get_camera().lens_radius > 0.0) == (aperture > 0.0)
    _held(rtmi, rtcheck, ("defocus", size, aperture), sc, variant)


@pytest.mark.parametrize("variant", [2, 6])
@pytest.mark.parametrize("defocus", [False, True], ids=["pinhole", "lens"])
def test_russian_roulette_draws_after_the_pop(rtmi, rtcheck, variant, defocus):
    """The roulette draw of a started lane is the next draw of the generator state the slot holds."""
    sc = _sheet(rtmi, 17, 9, 6, depth=12, aperture=0.3 if defocus else 0.0, defocus=defocus, rr=0.8)
    _held(rtmi, rtcheck, ("roulette", defocus), sc, variant)


@pytest.mark.parametrize("variant", [2, 6])
@pytest.mark.parametrize("rotate", [0, 2])
def test_a_shard_of_row_tiles(rtmi, rtcheck, variant, rotate):
    """Shard 2 of 3 over row tiles of 4 rows (tile_first = tile_stride - 1 = 2; tile_rotate 0 and 2): a lane's home row goes
    through the shard's deal, and tiles are ragged against the shard's rows."""
    sc = _sheet(rtmi, 24, 40, 3)
    _held(rtmi, rtcheck, ("shard", rotate), sc, variant, tile_rows=4, tile_first=2, tile_stride=3, tile_rotate=rotate)


@pytest.mark.parametrize("variant", [2, 6])
def test_an_adaptive_tile_list(rtmi, rtcheck, variant):
    """Adaptive sampling renders its later passes from a tile list: the sums and the sample counts equal the linear scan's,
    and two rows equal the checker's sums of each pixel's own sample count."""
    sc = _sheet(rtmi, 32, 24, 32)
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
    sc = _sheet(rtmi, 9, 5, spp)
    _held(rtmi, rtcheck, ("tiny", spp), sc, variant, spp_chunk=1)
