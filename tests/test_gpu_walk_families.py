"""-m gpu: the grid walk of EVERY kernel group against the group's own linear scan, byte for byte.

The candidate search is where a wrong image costs nothing to produce: a primitive missing from one cell, a walk that stops a
cell early at a shadow ray's far end or resumes wrongly behind an alpha hole is a silently wrong pixel.  The reference of a
candidate search is brute force -- layout 16, the linear scan of the same family, which each family's suite holds to fp64 per
sample -- and equality with it is exact and needs no tolerance.  The feature suites assert it on hand-built cases that mostly
have no grid; here the scenes are walk_cases.py's (a grid that lists most of the scene and decides what the camera sees, tables
that fit every layout: tests/test_walk_cases.py asserts those premises without a GPU), two seeds per group:

  plain, nee, env, env + nee, media, motion, feature (on the plain and on the env scene), nested;
  alpha masks x {plain, nested, feature, motion, nee, env + nee}; a projection x {plain, nested, feature, motion, nee, env,
  media}; ray queries on flat and on nested tables.

Every frame runs with a Stats that must report the group's family bits and the layout asked for; a refusal (RtmiError) fails
the test: the CPU test has shown that every layout fits.  Each group's scan is rendered once and shared."""
import time

import numpy as np
import pytest

import per_sample as PS
import walk_cases as W

pytestmark = pytest.mark.gpu
PASSES = (0, 1, 2)  # FEATURE_ALBEDO, FEATURE_NORMAL, FEATURE_DEPTH
SCAN = 16
IDS = ["%s-%d-%s" % c for c in W.CASES]
BY_LAYOUT = [(f, s, sh, layout) for f, s, sh in W.CASES for layout in W.layouts(f)]


@pytest.fixture(scope="module")
def rtmi():
    return PS.gpu_package()


@pytest.fixture(scope="module")
def frames(rtmi):
    """of(family, seed, shape, layout) -> the group's frames in that layout: [the frame], the three feature passes, or [the
    closest-hit records]; rendered once, the family bits and the layout checked on every launch"""
    scenes, made = {}, {}
    t0 = time.time()

    def scene(family, seed, shape):
        if (family, seed, shape) not in scenes:
            sc = W.scene(rtmi, seed, family, shape)
            scenes[family, seed, shape] = (sc, W.rays(sc, seed) if W.GROUPS[family].trace else None)
        return scenes[family, seed, shape]

    def of(family, seed, shape, layout):
        key = (family, seed, shape, layout)
        if key in made:
            return made[key]
        g = W.GROUPS[family]
        sc, rays = scene(family, seed, shape)
        want = layout or sc.table_info().kernel_variant & ~W.FAMILIES

        def ran(st):
            assert st.kernel_variant & W.FAMILIES == g.bits, (key, st.kernel_variant)
            assert st.kernel_variant & ~W.FAMILIES == want, (key, st.kernel_variant)

        out = []
        if g.trace:
            o, d, t_max = rays
            st = rtmi.Stats()
            rec = sc.trace(o, d, t_max, opts=rtmi.Opts(variant=layout), stats=st)
            ran(st)
            st = rtmi.Stats()
            occluded = sc.trace(o, d, t_max, occluded=True, opts=rtmi.Opts(variant=layout), stats=st)
            ran(st)
            assert np.array_equal(occluded, rec["prim"] >= 0), (key, int((occluded != (rec["prim"] >= 0)).sum()))
            out.append(rec)
        else:
            for feature in (PASSES if g.passes else (None,)):
                st = rtmi.Stats()
                opts = rtmi.Opts(seed=seed, variant=layout)
                out.append(sc.render(opts, st) if feature is None else sc.render_feature(feature, opts, st))
                ran(st)
        made[key] = out
        return out

    yield of
    print(f"\ntest_gpu_walk_families.py: {len(made)} frame sets of {len(scenes)} scenes in {time.time() - t0:.1f} s")


def same(a, b):
    """(equal byte for byte, what differs) of two frames or two arrays of hit records"""
    if a.dtype.names:  # records: per ray
        ra, rb = (np.ascontiguousarray(x).view(np.uint8).reshape(len(x), -1) for x in (a, b))
        diff = (ra != rb).any(axis=1)
        what = "rays"
    else:
        diff = (a.view(np.uint32) != b.view(np.uint32)).any(axis=-1)
        what = "pixels"
    if not diff.any():
        return True, ""
    first = tuple(int(i) for i in np.argwhere(diff)[0])
    at = first[0] if what == "rays" else first
    return False, f"{int(diff.sum())} of {diff.size} {what} differ, the first at {at}: {a[at]} against {b[at]}"


@pytest.mark.parametrize("family,seed,shape,layout", BY_LAYOUT, ids=["%s-%d-%s-%d" % c for c in BY_LAYOUT])
def test_layout_equals_the_scan(rtmi, frames, family, seed, shape, layout):
    if layout == 24 and W.GROUPS[family].bits == 0 and not rtmi.has_ablations():
        return  # (the plain scan over global tables is a measurement variant: the product library has none to compare)
    scan, got = frames(family, seed, shape, SCAN), frames(family, seed, shape, layout)
    assert len(scan) == len(got)
    for k, (a, b) in enumerate(zip(scan, got)):
        ok, what = same(a, b)
        assert ok, f"{family} seed {seed} {shape}, layout {layout} against the scan, frame {k}: {what}"


@pytest.mark.parametrize("family,seed,shape", W.CASES, ids=IDS)
def test_the_scan_shows_the_scene_and_the_groups_feature(rtmi, frames, family, seed, shape):
    g = W.GROUPS[family]
    scan = frames(family, seed, shape, SCAN)
    if g.trace:
        hit = scan[0]["prim"] >= 0
        assert 500 <= hit.sum() < len(hit), hit.sum()  # hits and misses
        return
    for a in scan:
        assert a.any() and np.isfinite(a).all()
    twin = W.twin_family(family)
    if twin is None:
        return
    # the feature is visible in the case: its frames differ from the same seed's plain scene, and from the scene that lacks
    # nothing but the feature (the twin group's scene: the same tables where only the camera or the masks differ)
    for other in {"feature" if g.passes else "plain", twin}:
        for k, (a, b) in enumerate(zip(scan, frames(other, seed, shape, SCAN))):
            assert not same(a, b)[0], f"{family} seed {seed} {shape}: frame {k} is that of {other!r}"
