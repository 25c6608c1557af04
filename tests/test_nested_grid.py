"""The nested grid (rt_scene_set_nested_grid), host side, no GPU: the tables csrc/pack.hip builds for a scene whose geometry
is clustered -- a detailed mesh standing in a room -- read back through rt_scene_table_info / rt_scene_nested_info /
rt_scene_table_image.  With the switch off the flat grid hands an overfull cell's members to the always-tested set; with it
on such a cell carries a sub-grid.  Checked here: what gets nested, how long the lists a walk can meet are (against the flat
packer on an evenly spread mesh), coverage of every leaf, that scenes with nothing to nest keep their bytes, termination,
and the interface.  The decoder of the nested format lives here (tests/test_tables.py reads the flat format only)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from test_tables import other_box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
RTMI = os.path.join(PKG, "rtmi")
RT_ERR_ARG = 1  # include/rtmi.h
NESTED_MARK = 1023  # a nested cell's header word 1 (include/rtmi.h, rt_nested_info)


def room(rtmi, n, side, spheres=200, room=20.0, seed=5, w=320, h=180, spp=4, depth=8, tex=False):
    """n x n height field of side `side` centred in a `room`-unit room: ground sphere, two walls, `spheres` small spheres.
    tex: the mesh's first material carries an image texture (the EXT builds' other feature)."""
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((8, 5, 9), (0, 0.5, 0), (0, 1, 0), 35.0)
    rng = np.random.default_rng(seed)
    m = [sc.lambertian((0.7, 0.3, 0.3)), sc.metal((0.8, 0.8, 0.8), 0.05), sc.lambertian((0.3, 0.6, 0.3))]
    if tex:
        px = (np.arange(16 * 16 * 3, dtype=np.uint32).reshape(16, 16, 3) * 37 % 251).astype(np.uint8)
        m[0] = sc.lambertian(sc.image_texture(px))
    step = side / n
    hgt = rng.uniform(0, 2.5 * step, size=(n + 1, n + 1))
    P = lambda i, j: (float(i * step - side / 2), float(0.2 + hgt[i, j]), float(j * step - side / 2))
    for i in range(n):
        for j in range(n):
            k = m[(i + 2 * j) % 3]
            sc.triangle(P(i, j), P(i + 1, j), P(i, j + 1), k)
            sc.triangle(P(i + 1, j), P(i + 1, j + 1), P(i, j + 1), k)
    sc.sphere((0, -1000, 0), 1000.0, m[2])
    sc.xy_rect(-room / 2, room / 2, 0, room / 2, -room / 2, m[0])
    sc.yz_rect(0, room / 2, -room / 2, room / 2, -room / 2, m[2])
    for k in range(spheres):
        c = rng.uniform(-room / 2, room / 2, 3)
        sc.sphere((float(c[0]), float(abs(c[1])) + 0.3, float(c[2])), float(rng.uniform(0.05, 0.15)), m[k % 3])
    return sc


def dense_room(rtmi, **kw):
    return room(rtmi, 160, 1.0, **kw)


def spread_room(rtmi, **kw):
    return room(rtmi, 160, 20.0, **kw)


def clump(rtmi, w=32, h=20, spp=2, depth=4):
    """100 spheres of radius 0.02 over [-4, 4]^3 and 1100 of radius 0.005 inside a cube of side 0.4 at (-1, 0.5, 1)"""
    sc = rtmi.Scene.new(w, h, spp, depth)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((0, 2, 14), (0, 0, 0), (0, 1, 0), 35.0)
    rng = np.random.default_rng(3)
    m = [sc.lambertian((0.7, 0.3, 0.3)), sc.metal((0.8, 0.8, 0.8), 0.05), sc.lambertian((0.3, 0.6, 0.3))]
    for k in range(100):
        c = rng.uniform(-4, 4, 3)
        sc.sphere((float(c[0]), float(c[1]), float(c[2])), 0.02, m[k % 3])
    for k in range(1100):
        c = np.array([-1.0, 0.5, 1.0]) + rng.uniform(-0.2, 0.2, 3)
        sc.sphere((float(c[0]), float(c[1]), float(c[2])), 0.005, m[k % 3])
    return sc


class Leaves:
    """Every list a walk can reach, decoded from table_image(): the plain cells of the top level and the sub-cells of the
    nested ones.  grids[0] is the top level; a nested cell's sub-grid is grids[1 + header word 0]."""

    def __init__(self, sc):
        self.t = t = sc.table_info()
        self.ni = ni = sc.nested_info()
        assert t.grid_wide in (1, 2) and (t.grid_wide == 2) == (ni.cells > 0)
        img = sc.table_image()
        self.img = img
        u32 = img.view(np.uint32).reshape(-1)
        top = int(np.prod(list(t.grid_n)))
        assert t.grid_cells == top
        n_headers = (ni.first_sub_cell + ni.sub_cells) if ni.cells else top
        self.words = u32[t.off_grid_cells * 4: t.off_grid_cells * 4 + 2 * n_headers].reshape(-1, 2).astype(np.int64)
        self.items = u32[t.off_grid_items * 4:].astype(np.int64)
        self.grids = [(np.array(list(t.grid_min), np.float64), np.array(list(t.grid_size), np.float64),
                       np.array(list(t.grid_n), np.int64), 0)]
        if ni.cells:
            assert ni.off_sub_cells * 4 == t.off_grid_cells * 4 + 2 * ni.first_sub_cell and ni.first_sub_cell >= top
            for i in range(ni.cells):
                r = img[ni.off_sub_grids + 4 * i: ni.off_sub_grids + 4 * i + 4]
                n = r[3, :3].view(np.int32).astype(np.int64)
                first = int(r[0, 3:4].view(np.int32)[0])
                assert np.allclose(r[1, :3] * r[2, :3], 1.0, rtol=1e-6) and (n >= 1).all() and (n <= ni.axis_cap).all()
                assert ni.first_sub_cell <= first and first + int(n.prod()) <= ni.first_sub_cell + ni.sub_cells
                self.grids.append((r[0, :3].astype(np.float64), r[2, :3].astype(np.float64), n, first))
        w1 = self.words[:, 1]
        self.nested = w1 == NESTED_MARK
        assert not self.nested[top:].any(), "one level of nesting: a sub-cell is never nested"
        assert int(self.nested.sum()) == ni.cells
        self.n_near, self.n_all, self.n_other = w1 & 1023, (w1 >> 10) & 1023, w1 >> 20
        plain = ~self.nested
        assert (self.n_near[plain] <= self.n_all[plain]).all()
        self.length = np.where(plain, self.n_all + self.n_other, 0)
        self.leaf = plain.copy()
        self.leaf[top:ni.first_sub_cell if ni.cells else top] = False  # (the padding header between the two levels)

    def cells_of_box(self, grid, lo, hi):
        gmin, gsize, n, first = self.grids[grid]
        i0 = np.clip(np.floor((np.asarray(lo, np.float64) - gmin) / gsize), 0, n - 1).astype(np.int64)
        i1 = np.clip(np.floor((np.asarray(hi, np.float64) - gmin) / gsize), 0, n - 1).astype(np.int64)
        nx, ny = int(n[0]), int(n[1])
        return [first + (iz * ny + iy) * nx + ix for iz in range(i0[2], i1[2] + 1) for iy in range(i0[1], i1[1] + 1)
                for ix in range(i0[0], i1[0] + 1)]

    def entries(self, c):
        """(near-tier sphere slots, other primitives' grouped ids) of the plain cell c"""
        f = int(self.words[c, 0])
        return self.items[f: f + self.n_near[c]], self.items[f + self.n_all[c]: f + self.n_all[c] + self.n_other[c]]

    def leaves_of_box(self, lo, hi):
        """the leaf cells a box touches: plain top-level cells, and inside a nested one the sub-cells the box touches (the
        sub-grid's bounds hold what its entries reach of the cell; indices are clamped to it, as the packer's and the walk's)"""
        out = []
        for c in self.cells_of_box(0, lo, hi):
            if not self.nested[c]:
                out.append(c)
            else:
                out.extend(self.cells_of_box(1 + int(self.words[c, 0]), lo, hi))
        return out

    def stats(self):
        occ = self.leaf & (self.length > 0)
        return float(self.length[occ].mean()), int(self.length[occ].max())


def test_dense_room_is_nested_instead_of_demoted(rtmi):
    """The flat grid hands 46 270 of the 51 200 triangles to the always-tested set; nested, none.  Fails without the feature."""
    sc = dense_room(rtmi)
    off = sc.table_info()
    assert off.nt == 51200 and off.nt_a > 0 and off.kernel_variant == 44 and sc.nested_info().cells == 0
    sc.set_nested_grid(True)
    on, ni = sc.table_info(), sc.nested_info()
    assert on.nt_a == 0 and on.kernel_variant == 52 and on.grid_wide == 2
    assert ni.cells > 0 and ni.sub_cells > 0 and ni.sub_items > 0 and ni.threshold == 64 and ni.axis_cap == 32
    assert list(on.grid_n) == [56, 29, 57]  # the top level is sized as the flat grid of the undemoted scene


def test_leaf_lists_are_as_short_as_an_even_mesh_gets(rtmi):
    """Mean over occupied leaves and longest leaf list of the nested dense room: each at most twice what the flat packer gives
    the evenly spread mesh (the factor allows for integer sub-grid dimensions, the per-axis cap and triangles cut by the outer
    cell's faces).  Measured: spread flat 17.8 / 32 (see DESIGN 7c for the dense room's)."""
    flat = spread_room(rtmi)
    assert flat.table_info().nt_a == 0
    mean_flat, longest_flat = Leaves(flat).stats()
    sc = dense_room(rtmi)
    sc.set_nested_grid(True)
    L = Leaves(sc)
    mean_on, longest_on = L.stats()
    print(f"spread room flat: mean {mean_flat:.2f} longest {longest_flat}; dense room nested: mean {mean_on:.2f} longest {longest_on}")
    assert longest_on == L.ni.longest
    assert mean_on <= 2 * mean_flat and longest_on <= 2 * longest_flat


def check_nested_coverage(sc):
    """every primitive that is not always-tested is listed by every leaf cell its own bounding box overlaps"""
    L = Leaves(sc)
    t, img, P = L.t, L.img, sc.prims()
    ns = t.ns
    slot_of, gid_of = {}, {}
    for slot in range(t.np, ns):
        if not np.isneginf(img[slot, 3]):
            slot_of[int(img[t.off_sph_cold + slot].view(np.uint32)[2])] = slot
    for j in range(t.nr_a, t.nr):
        gid_of[int(img[t.off_rect_cold + j].view(np.uint32)[1])] = ns + j
    for k in range(t.nc_a, t.nc):
        gid_of[int(img[t.off_cyl_cold + 4 * k + 3].view(np.uint32)[1])] = ns + t.nr + k
    for k in range(t.nt_a, t.nt):
        gid_of[int(img[t.off_tri_cold + 2 * k].view(np.uint32)[1])] = ns + t.nr + t.nc + k
    nq, nq_a = sc.quad_counts()  # (their records follow the triangles')
    for k in range(nq_a, nq):
        gid_of[int(img[t.off_tri_cold + 2 * (t.nt + k)].view(np.uint32)[1])] = ns + t.nr + t.nc + t.nt + k
    assert all((int(P["type"][prim]) == 6) == (g >= ns + t.nr + t.nc + t.nt) for prim, g in gid_of.items())
    cache = {}

    def entries(c):
        if c not in cache:
            a, b = L.entries(c)
            cache[c] = (set(a.tolist()), set(b.tolist()))
        return cache[c]

    checked = 0
    for prim in range(len(P)):
        if prim in slot_of:
            c3, r = P["f"][prim][:3].astype(np.float64), abs(float(P["f"][prim][3]))
            for c in L.leaves_of_box(c3 - r, c3 + r):
                assert slot_of[prim] in entries(c)[0], (prim, c)
                checked += 1
        elif prim in gid_of:
            lo, hi = other_box(P[prim])
            for c in L.leaves_of_box(lo, hi):
                assert gid_of[prim] in entries(c)[1], (prim, c)
                checked += 1
    return checked, L


def test_every_leaf_a_box_touches_lists_it(rtmi):
    sc = dense_room(rtmi)
    sc.set_nested_grid(True)
    checked, L = check_nested_coverage(sc)
    assert checked > 51200 and L.ni.cells > 0
    sc = clump(rtmi)
    sc.set_nested_grid(True)
    checked, L = check_nested_coverage(sc)
    assert checked >= 1200 - L.t.np and L.ni.cells > 0


def test_nothing_to_nest_changes_nothing(rtmi, golden_dir):
    scenes = [spread_room(rtmi), rtmi.Scene.rtiow(7, 96, 54, 3, 20), rtmi.Scene.load(os.path.join(golden_dir, "scenes", "sample_scene.json"))]
    for sc in scenes:
        v0, b0 = sc.table_info().kernel_variant, sc.table_image().tobytes()
        sc.set_nested_grid(True)
        assert sc.nested_grid and sc.nested_info().cells == 0
        assert sc.table_info().kernel_variant == v0 and sc.table_image().tobytes() == b0
    sc = dense_room(rtmi)
    b0 = sc.table_image().tobytes()
    sc.set_nested_grid(True)
    assert sc.table_image().tobytes() != b0
    sc.set_nested_grid(False)
    assert sc.table_image().tobytes() == b0 and sc.table_info().kernel_variant == 44


def test_copies_of_one_sphere_still_pack(rtmi):
    """1500 copies of one sphere overflow their sub-cell too: one level of nesting, then they are tested for every query"""
    sc = rtmi.Scene.new(32, 20, 2, 4)
    sc.camera((0, 2, 14), (0, 0, 0), (0, 1, 0), 35.0)
    m = sc.lambertian((0.5, 0.5, 0.5))
    for _ in range(1500):
        sc.sphere((0.5, 0.25, -0.5), 0.1, m)
    for k in range(40):
        sc.sphere((float(k % 7) - 3, float(k % 5) - 2, float(k % 3) - 1), 0.05, m)
    sc.set_nested_grid(True)
    assert sc.table_info().np >= 1500


def test_a_separable_clump_is_separated(rtmi):
    sc = clump(rtmi)
    off = sc.table_info()
    assert off.np == 1100 and list(off.grid_n) == [6, 6, 6]  # the flat packer tests the whole clump for every query
    sc.set_nested_grid(True)
    on = sc.table_info()
    assert on.np <= 100 and on.kernel_variant == 52 and sc.nested_info().cells > 0


def test_interface(rtmi, tmp_path, golden_dir):
    sample = os.path.join(golden_dir, "scenes", "sample_scene.json")
    sc = rtmi.Scene.load(sample)
    assert not sc.nested_grid and "nested_grid" not in json.loads(sc.to_json())
    sc.set_nested_grid()
    assert sc.nested_grid and json.loads(sc.to_json())["nested_grid"] is True
    assert rtmi.Scene.parse(sc.to_json()).nested_grid and sc.clone().nested_grid
    sc.set_nested_grid(False)
    assert not sc.nested_grid and "nested_grid" not in json.loads(sc.to_json())
    j = json.loads(sc.to_json())
    for bad in (1, "yes", None):
        j["nested_grid"] = bad
        with pytest.raises(rtmi.RtmiError):
            rtmi.Scene.parse(json.dumps(j))
    j["nested_grid"] = False
    assert not rtmi.Scene.parse(json.dumps(j)).nested_grid
    # NULL arguments
    lib = rtmi._lib
    assert lib.rt_scene_set_nested_grid(None, 1) == RT_ERR_ARG and lib.rt_scene_get_nested_grid(None) == -RT_ERR_ARG
    assert lib.rt_scene_nested_info(None, C.byref(rtmi.NestedInfo())) == RT_ERR_ARG
    assert lib.rt_scene_nested_info(sc._h, None) == RT_ERR_ARG
    # the ctypes mirror, and the ABI version the change leaves alone
    assert lib.rt_struct_size(10) == C.sizeof(rtmi.NestedInfo) and lib.rt_struct_size(11) == 0
    assert rtmi.abi_version() == 3
    for name in ("rt_scene_set_nested_grid", "rt_scene_get_nested_grid", "rt_scene_nested_info"):
        assert name in rtmi.C_SYMBOLS
    # the CLI: --nested-grid is a flag (the dumped scene carries the key); what follows needs a GPU and may fail without one
    out = tmp_path / "scene.json"
    p = subprocess.run([RTMI, "-f", sample, "-w", "16", "-h", "9", "-spp", "1", "--nested-grid",
                        "--dump-json", str(out), "-o", str(tmp_path / "x.ppm"), "--no-png"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode != 2, p.stderr
    assert json.loads(out.read_text())["nested_grid"] is True
    p = subprocess.run([RTMI, "--nested-grid=1"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 2
