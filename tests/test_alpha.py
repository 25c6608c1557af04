"""Alpha cutouts (an image's alpha channel opens holes in a surface) without a GPU:
  1. PNG alpha decoding: RGBA, grey + alpha and palette + tRNS files written here keep their alpha as a plane, an RGB file has none;
  2. the packed bytes: a scene that never touches the new calls, one whose images carry all-255 planes and one whose masks were
     set and removed pack to the same bytes; a plane lands in the texel words' top byte as 255 - a8; the mask records;
  3. the cutoff byte: 0.5 -> 128, 1 -> 255, 1e-9 -> 1; a texel of 127 is a hole against 128 and one of 128 is not;
  4. the interface -- Python, C, C++ (tests/alpha_host_driver.cpp), JSON -- with every refusal and the round trip;
  5. the fp64 statement (ref64.opaque_hit): all-opaque masks give ref64's own samples, all-transparent masks the samples of the
     scene without those primitives, the tally counts as stated, the 65th masked hit of a query is opaque, and every case of
     alpha_scenes.py holds the contents it is there for; two cases trace as pinned before the statement moved into ref64.py;
  6. a stand-alone program over the PNG reader and the packer with masked scenes under -fsanitize=address,undefined.
test_gpu_alpha.py holds the kernels to that reference."""
import ctypes
import hashlib
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import alpha_scenes as AS
import nee_scenes as NS
import ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-in-cuda_amd")
RT_ERR_ARG, RT_ERR_SCENE = 1, 4


# ------------------------------------------------------------------------------------------------------------ 1. PNG files
def write_png(path, ctype, rows, cols, raw, palette=None, trns=None, filters=None):
    """an 8-bit non-interlaced PNG of colour type `ctype` from raw[rows][cols * channels] bytes, each row with the filter
    type filters[row] (applied here)"""
    raw = np.asarray(raw, np.uint8).reshape(rows, -1)
    ch = raw.shape[1] // cols
    lines = b""
    for y in range(rows):
        f = 0 if filters is None else filters[y % len(filters)]
        cur, up = raw[y].astype(np.int64), (raw[y - 1].astype(np.int64) if y else np.zeros(raw.shape[1], np.int64))
        left = np.concatenate([np.zeros(ch, np.int64), cur[:-ch]])
        pred = {0: 0 * cur, 1: left, 2: up, 3: (left + up) // 2}[f]
        lines += bytes([f]) + ((cur - pred) % 256).astype(np.uint8).tobytes()

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, 8, ctype, 0, 0, 0))
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    if trns is not None:
        out += chunk(b"tRNS", np.asarray(trns, np.uint8).tobytes())
    out += chunk(b"IDAT", zlib.compress(lines, 6)) + chunk(b"IEND", b"")
    with open(path, "wb") as fh:
        fh.write(out)
    return str(path)


def png_files(d):
    """name -> (path, expected rgb [rows][cols][3], expected alpha [rows][cols] or None)"""
    rng = np.random.default_rng(4)
    out = {}
    rgba = rng.integers(0, 256, (5, 7, 4)).astype(np.uint8)
    rgba[0, 0, 3], rgba[0, 1, 3], rgba[0, 2, 3] = 127, 128, 0
    out["rgba"] = (write_png(d / "rgba.png", 6, 5, 7, rgba.reshape(5, -1), filters=(0, 1, 2, 3)), rgba[..., :3], rgba[..., 3])
    ga = rng.integers(0, 256, (3, 4, 2)).astype(np.uint8)
    out["grey_alpha"] = (write_png(d / "ga.png", 4, 3, 4, ga.reshape(3, -1), filters=(1, 2)), np.repeat(ga[..., :1], 3, axis=2), ga[..., 1])
    pal = rng.integers(0, 256, (6, 3)).astype(np.uint8)
    idx = rng.integers(0, 6, (4, 5)).astype(np.uint8)
    trns = np.array([0, 200, 127, 128], np.uint8)  # (shorter than the palette: the entries beyond it are opaque)
    out["palette_trns"] = (write_png(d / "pal.png", 3, 4, 5, idx, palette=pal, trns=trns), pal[idx],
                           np.concatenate([trns, [255, 255]]).astype(np.uint8)[idx])
    out["palette"] = (write_png(d / "pal_plain.png", 3, 4, 5, idx, palette=pal), pal[idx], None)
    rgb = rng.integers(0, 256, (4, 4, 3)).astype(np.uint8)
    out["rgb"] = (write_png(d / "rgb.png", 2, 4, 4, rgb.reshape(4, -1), filters=(3,)), rgb, None)
    grey = rng.integers(0, 256, (2, 3)).astype(np.uint8)
    out["grey"] = (write_png(d / "grey.png", 0, 2, 3, grey), np.repeat(grey[..., None], 3, axis=2), None)
    return out


def test_png_files_keep_their_alpha(rtmi, tmp_path):
    sc = rtmi.Scene.new(16, 9, 1, 2)
    for name, (path, rgb, alpha) in png_files(tmp_path).items():
        t = sc.image_texture(path)
        assert np.array_equal(sc.get_image(t), rgb), name
        got = sc.get_image_alpha(t)
        if alpha is None:
            assert got is None, name
        else:
            assert got is not None and got.dtype == np.uint8 and np.array_equal(got, alpha), name
    with pytest.raises(ValueError):
        sc.image_texture(str(tmp_path / "rgba.png"), alpha=np.zeros((5, 7), np.uint8))


# ------------------------------------------------------------------------------------------------------------ 2. packed bytes
def _five(rtmi, alpha=None, touch=False):
    """an image-textured scene on five shapes; alpha: the planes its two images get (None: the parent's call, without one);
    touch: masks set on every material and removed again"""
    sc = rtmi.Scene.new(32, 18, 1, 4)
    sc.camera((0, 1, 6), (0, 0.5, 0), (0, 1, 0), 40.0)
    px = [AS.colours(AS.PLANES["blocks8"]), AS.colours(AS.PLANES["bars"])]
    img = [sc.image_texture(p) if alpha is None else sc.image_texture(p, alpha=a) for p, a in zip(px, alpha or [None, None])]
    ids = [sc.lambertian(img[0]), sc.metal((0.8, 0.8, 0.8), 0.1), sc.dielectric(1.5), sc.rough_metal((0.9, 0.7, 0.4), 0.3), sc.plastic(img[1], 1.5, 0.3),
           sc.rough_glass(1.5, 0.2), sc.pbr(img[0], 0.5, 0.4), sc.diffuse_light((4.0, 4.0, 4.0))]
    sc.sphere((-3, 0.5, 0), 0.4, ids[0])
    sc.xy_rect(-2.5, -1.5, 0, 1, 0, ids[1])
    sc.cylinder(0.3, -0.5, 0.5, ids[2], translate=(-0.5, 0.5, 0))
    sc.quad((0.5, 0, 0), (1, 0, 0), (0, 1, 0), ids[3])
    sc.triangle((2, 0, 0), (3, 0, 0), (2, 1, 0), ids[4], (0, 0), (1, 0), (0, 1))
    for k, m in enumerate(ids[5:]):
        sc.sphere((k - 1.0, 2.0, 0.0), 0.4, m)
    if touch:
        for m in ids[:7]:
            sc.set_alpha(m, img[m % 2], 0.5)
        for m in ids[:7]:
            sc.set_alpha(m, -1)
    return sc, img, ids


def test_a_scene_without_masks_packs_to_the_bytes_it_packed_to(rtmi):
    plain = _five(rtmi)[0].table_image().tobytes()
    full = [np.full(AS.PLANES[k].shape, 255, np.uint8) for k in ("blocks8", "bars")]
    assert _five(rtmi, alpha=full)[0].table_image().tobytes() == plain          # (an all-255 plane equals no plane)
    assert _five(rtmi, alpha=full, touch=True)[0].table_image().tobytes() == plain  # (masks set and removed leave nothing)
    # a plane with holes changes the texel words' top bytes and nothing else while no mask is set
    holes = [AS.PLANES["blocks8"], AS.PLANES["bars"]]
    a = np.frombuffer(_five(rtmi, alpha=holes)[0].table_image().tobytes(), np.uint32)
    b = np.frombuffer(plain, np.uint32)
    assert a.size == b.size and ((a ^ b) & 0x00ffffff == 0).all()
    changed = np.flatnonzero(a != b)
    assert len(changed) == int((holes[0] != 255).sum() + (holes[1] != 255).sum())
    assert sorted(set((a[changed] >> 24).tolist())) == [255]  # (a8 = 0 -> 255 - 0)


def test_the_packed_mask_records(rtmi):
    """with a mask in the scene: one record per material straight behind the material table, {word offset of the mask's texels,
    rows, cols, c8}, zeros for a material without a mask; the material records (Scene.materials) do not change"""
    holes = [AS.PLANES["blocks8"], AS.PLANES["edge"]]
    sc, img, ids = _five(rtmi, alpha=[holes[0], np.resize(holes[1], AS.PLANES["bars"].shape)])
    before = sc.table_image().reshape(-1).copy()
    mats_before = sc.materials().tobytes()
    sc.set_alpha(ids[0], img[0], 0.5)
    sc.set_alpha(ids[4], img[1], 1.0)
    sc.set_alpha(ids[2], img[1], 1e-9)
    w = sc.table_image().reshape(-1)
    assert sc.materials().tobytes() == mats_before
    n = len(ids)
    assert w.size == before.size + 4 * n
    bits = w.view(np.int32)
    # the records: n rows of which three are set, found by content
    want = {ids[0]: (8, 8, 128), ids[4]: (4, 8, 255), ids[2]: (4, 8, 1)}
    found = [k for k in range(0, w.size - 4 * n + 4, 4)
             if all((tuple(bits[k + 4 * m + 1:k + 4 * m + 4]) == want[m]) if m in want else not bits[k + 4 * m:k + 4 * m + 4].any() for m in range(n))]
    assert len(found) == 1, found
    k = found[0]
    # the word offsets point at the images' texels: the top bytes there are 255 - a8
    for m, plane in ((ids[0], holes[0]), (ids[4], sc.get_image_alpha(img[1]))):
        at = int(bits[k + 4 * m])
        words = w.view(np.uint32)[at:at + plane.size]
        assert np.array_equal(words >> 24, 255 - plane.reshape(-1).astype(np.uint32))
        assert np.array_equal(words & 0xff, sc.get_image(img[0] if m == ids[0] else img[1]).reshape(-1, 3)[:, 0])
    # the records stand straight behind the material table; taken out, the image is the unmasked scene's but for the words that
    # hold offsets behind them: record offsets grow by the n rows, texel word offsets by 4 n words
    rest = np.concatenate([w[:k], w[k + 4 * n:]]).view(np.int32)
    moved = np.flatnonzero(rest != before.view(np.int32))
    assert 0 < len(moved) < 40 and set((rest[moved] - before.view(np.int32)[moved]).tolist()) <= {n, 4 * n}, moved
    # (the material table ends where the records begin: the last material's rows lie in front of them)
    assert list(w[k - 12 + 4:k - 12 + 7]) == [np.float32(4.0)] * 3  # (the diffuse_light's solid colour: its row c0)


# ------------------------------------------------------------------------------------------------------------ 3. the cutoff byte
def test_the_cutoff_byte(rtmi):
    assert R.cutoff_byte(0.5) == 128 and R.cutoff_byte(1.0) == 255 and R.cutoff_byte(1e-9) == 1
    assert R.cutoff_byte(np.float32(0.5)) == 128 and R.cutoff_byte(128 / 255) in (128, 129) and R.cutoff_byte(0.999) == 255
    # the packer's byte (csrc/rt_alpha.h) through the packed record, and the verdict through the reference's closest hit
    for cutoff, c8 in ((0.5, 128), (1.0, 255), (1e-9, 1), (0.25, 64), (0.7, 179)):
        sc = rtmi.Scene.new(8, 8, 1, 2)
        t = sc.image_texture(np.zeros((1, 2, 3), np.uint8), alpha=np.array([[c8 - 1, c8]], np.uint8))
        m = sc.lambertian((0.5, 0.5, 0.5))
        sc.set_alpha(m, t, cutoff)
        sc.xy_rect(-1, 1, -1, 1, 0.0, m)  # (u from x, v from y: the column from y)
        bits = sc.table_image().reshape(-1).view(np.int32)
        assert any(tuple(bits[k:k + 4][1:]) == (1, 2, c8) for k in range(0, bits.size, 4)), (cutoff, c8)
        S = R.RefScene(sc)
        assert S.alpha_masks[m][1] == c8
        o = np.array([[0.0, -0.5, 3.0], [0.0, 0.5, 3.0]])
        d = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0]])
        _, idx = R.opaque_hit(S, o, d, np.inf, np.float64)
        assert idx.tolist() == [-1, 0], (cutoff, idx)  # (a8 = c8 - 1 is a hole, a8 = c8 is not)


# ------------------------------------------------------------------------------------------------------------ 4. the interface
def test_python_sets_gets_removes_and_refuses(rtmi):
    holes = [AS.PLANES["blocks8"], AS.PLANES["bars"]]
    sc, img, ids = _five(rtmi, alpha=holes)
    assert rtmi.MATERIAL_DTYPE.itemsize == 28 == rtmi.struct_size(3) and rtmi.abi_version() == 3
    plain = sc.image_texture(AS.colours(AS.PLANES["two"]))
    solid = sc.solid_color((0.5, 0.5, 0.5))
    before = sc.materials().tobytes()
    assert all(sc.alpha(m) is None for m in ids)
    for k, m in enumerate(ids[:7]):
        sc.set_alpha(m, img[k % 2], 0.1 * (k + 1))
        assert sc.alpha(m) == (img[k % 2], float(np.float32(0.1 * (k + 1))))
    sc.set_alpha(ids[0], img[0])
    assert sc.alpha(ids[0]) == (img[0], 0.5)  # (the default cutoff)
    assert sc.materials().tobytes() == before  # (a side table: the material records do not change)
    assert sc.clone().alpha(ids[3]) == sc.alpha(ids[3])
    assert np.array_equal(sc.clone().get_image_alpha(img[1]), holes[1]) and sc.get_image_alpha(plain) is None
    rgba = np.concatenate([AS.colours(holes[0]), holes[0][..., None]], axis=2)
    four = sc.image_texture(rgba)  # (a (rows, cols, 4) array brings its own plane)
    assert np.array_equal(sc.get_image_alpha(four), holes[0]) and np.array_equal(sc.get_image(four), rgba[..., :3])
    nan, inf = float("nan"), float("inf")
    light = ids[7]
    for call in (lambda: sc.set_alpha(99, img[0], 0.5), lambda: sc.set_alpha(-1, img[0], 0.5), lambda: sc.set_alpha(light, img[0], 0.5),
                 lambda: sc.set_alpha(ids[0], solid, 0.5), lambda: sc.set_alpha(ids[0], plain, 0.5), lambda: sc.set_alpha(ids[0], 99, 0.5),
                 lambda: sc.set_alpha(ids[0], -2, 0.5), lambda: sc.set_alpha(ids[0], img[0], nan), lambda: sc.set_alpha(ids[0], img[0], inf),
                 lambda: sc.set_alpha(ids[0], img[0], 0.0), lambda: sc.set_alpha(ids[0], img[0], -0.5), lambda: sc.set_alpha(ids[0], img[0], 1.0001),
                 lambda: sc.alpha(99), lambda: sc.alpha(-1), lambda: sc.get_image_alpha(solid), lambda: sc.get_image_alpha(999)):
        with pytest.raises(rtmi.RtmiError) as e:
            call()
        assert e.value.status == RT_ERR_ARG, str(e.value)
    assert sc.alpha(ids[0]) == (img[0], 0.5)  # (a refused call changes nothing)
    sc.set_alpha(ids[0], -1)
    sc.set_alpha(light, -1)  # (removing what is not there: allowed)
    assert sc.alpha(ids[0]) is None and sc.alpha(ids[1]) is not None
    for name in ("rt_scene_add_image_texture_rgba", "rt_scene_get_image_alpha", "rt_scene_set_alpha", "rt_scene_get_alpha"):
        assert name in rtmi.C_SYMBOLS


def test_the_c_entry_points(rtmi):
    lib = ctypes.CDLL(rtmi.LIB_PATH)
    sc, img, ids = _five(rtmi, alpha=[AS.PLANES["blocks8"], AS.PLANES["bars"]])
    plain = sc.image_texture(AS.colours(AS.PLANES["two"]))
    i, f, p, vp = ctypes.c_int, ctypes.c_float, ctypes.POINTER, ctypes.c_void_p
    lib.rt_scene_set_alpha.argtypes, lib.rt_scene_set_alpha.restype = [vp, i, i, f], i
    lib.rt_scene_get_alpha.argtypes, lib.rt_scene_get_alpha.restype = [vp, i, p(i), p(f)], i
    lib.rt_scene_add_image_texture_rgba.argtypes, lib.rt_scene_add_image_texture_rgba.restype = [vp, i, i, vp], i
    lib.rt_scene_get_image_alpha.argtypes, lib.rt_scene_get_image_alpha.restype = [vp, i, p(i), p(i), vp, ctypes.c_size_t], i
    lib.rt_last_error.restype = ctypes.c_char_p
    s = sc._h
    t, k = i(5), f(5)
    assert lib.rt_scene_get_alpha(s, ids[2], ctypes.byref(t), ctypes.byref(k)) == 0 and (t.value, k.value) == (-1, 0.0)
    assert lib.rt_scene_set_alpha(s, ids[2], img[0], 0.25) == 0
    assert lib.rt_scene_get_alpha(s, ids[2], ctypes.byref(t), ctypes.byref(k)) == 0 and (t.value, k.value) == (img[0], 0.25)
    assert lib.rt_scene_get_alpha(s, ids[2], None, None) == 0
    for call in (lambda: lib.rt_scene_set_alpha(None, ids[2], img[0], 0.25), lambda: lib.rt_scene_set_alpha(s, len(ids), img[0], 0.25),
                 lambda: lib.rt_scene_set_alpha(s, ids[7], img[0], 0.25), lambda: lib.rt_scene_set_alpha(s, ids[1], plain, 0.25),
                 lambda: lib.rt_scene_set_alpha(s, ids[1], img[0], float("nan")), lambda: lib.rt_scene_set_alpha(s, ids[1], img[0], 0.0),
                 lambda: lib.rt_scene_get_alpha(None, 0, None, None), lambda: lib.rt_scene_get_alpha(s, len(ids), ctypes.byref(t), ctypes.byref(k))):
        assert call() == RT_ERR_ARG and lib.rt_last_error()
    assert lib.rt_scene_set_alpha(s, ids[2], -1, 0.0) == 0 and sc.alpha(ids[2]) is None
    px = np.arange(2 * 3 * 4, dtype=np.uint8)
    tex = lib.rt_scene_add_image_texture_rgba(s, 2, 3, px.ctypes.data_as(vp))
    assert tex >= 0 and np.array_equal(sc.get_image_alpha(tex), px.reshape(2, 3, 4)[..., 3]) and np.array_equal(sc.get_image(tex), px.reshape(2, 3, 4)[..., :3])
    rows, cols, small = i(), i(), np.zeros(5, np.uint8)
    assert lib.rt_scene_get_image_alpha(s, tex, ctypes.byref(rows), ctypes.byref(cols), None, 0) == 1 and (rows.value, cols.value) == (2, 3)
    assert lib.rt_scene_get_image_alpha(s, plain, None, None, None, 0) == 0
    for call in (lambda: lib.rt_scene_add_image_texture_rgba(s, 0, 3, px.ctypes.data_as(vp)), lambda: lib.rt_scene_add_image_texture_rgba(s, 2, 3, None),
                 lambda: lib.rt_scene_add_image_texture_rgba(None, 2, 3, px.ctypes.data_as(vp)),
                 lambda: lib.rt_scene_get_image_alpha(s, tex, None, None, small.ctypes.data_as(vp), small.nbytes),
                 lambda: lib.rt_scene_get_image_alpha(s, 999, None, None, None, 0)):
        assert call() == -RT_ERR_ARG and lib.rt_last_error()


def test_json_reads_writes_and_refuses(rtmi, tmp_path):
    holes = [AS.PLANES["blocks8"], AS.PLANES["bars"]]
    sc, img, ids = _five(rtmi, alpha=holes)
    path, _, file_alpha = png_files(tmp_path)["rgba"]
    from_file = sc.image_texture(path)
    for k, m in enumerate(ids[:7]):
        sc.set_alpha(m, [img[0], img[1], from_file][k % 3], 0.125 * (k + 1))
    text = sc.to_json()
    doc = json.loads(text)
    mats, texs = doc["material"]["data"], doc["texture"]["data"]
    assert [m.get("alpha") for m in mats] == [{"texture": [img[0], img[1], from_file][k % 3], "cutoff": 0.125 * (k + 1)} for k in range(7)] + [None]
    assert texs[img[0]]["alpha"] == holes[0].reshape(-1).tolist() and "alpha" not in texs[from_file] and texs[from_file]["file"] == path
    back = rtmi.Scene.parse(text)
    assert [back.alpha(m) for m in ids] == [sc.alpha(m) for m in ids]
    assert np.array_equal(back.get_image_alpha(img[1]), holes[1]) and np.array_equal(back.get_image_alpha(from_file), file_alpha)
    assert back.table_image().tobytes() == sc.table_image().tobytes()
    assert back.to_json() == text

    def with_material(i, x):
        d = json.loads(text)
        d["material"]["data"][i] = x
        return json.dumps(d)

    def with_texture(i, x):
        d = json.loads(text)
        d["texture"]["data"][i] = x
        return json.dumps(d)
    for i in range(7):
        rtmi.Scene.parse(with_material(i, mats[i]))
    al = {"texture": img[0], "cutoff": 0.5}
    bad = [(7, dict(mats[7], alpha=al))]  # a diffuse_light
    plain = len(texs)  # (an image without a plane, appended below)
    for i in range(7):
        bad += [(i, dict(mats[i], alpha=dict(al, scale=1))), (i, dict(mats[i], alpha={"cutoff": 0.5})), (i, dict(mats[i], alpha=dict(al, texture=99))),
                (i, dict(mats[i], alpha=dict(al, texture=-1))), (i, dict(mats[i], alpha=dict(al, texture=1.5))), (i, dict(mats[i], alpha=dict(al, cutoff="x"))),
                (i, dict(mats[i], alpha=dict(al, cutoff=0))), (i, dict(mats[i], alpha=dict(al, cutoff=1.5))), (i, dict(mats[i], alpha=[img[0], 0.5])),
                (i, dict(mats[i], alpha=3)), (i, dict(mats[i], alpha=dict(al, texture=plain)))]
    for k, (i, x) in enumerate(bad):
        d = json.loads(with_material(i, x))
        d["texture"]["data"].append({"type": "image", "rows": 1, "cols": 1, "data": [1, 2, 3]})
        with pytest.raises(rtmi.RtmiError) as e:
            rtmi.Scene.parse(json.dumps(d))
        assert e.value.status == RT_ERR_SCENE, (k, str(e.value))
        assert "material %d" % i in str(e.value), str(e.value)
    # the cutoff defaults to 0.5
    assert rtmi.Scene.parse(with_material(0, dict(mats[0], alpha={"texture": img[1]}))).alpha(0) == (img[1], 0.5)
    # an inline image's plane: rows * cols bytes, and only beside inline pixels
    t0 = texs[img[0]]
    for x in (dict(t0, alpha=t0["alpha"][:-1]), dict(t0, alpha=t0["alpha"] + [0]), dict(t0, alpha=[256] + t0["alpha"][1:]), dict(t0, alpha=[0.5] + t0["alpha"][1:]),
              dict(t0, alpha="x"), dict(texs[from_file], alpha=[0])):
        with pytest.raises(rtmi.RtmiError) as e:
            rtmi.Scene.parse(with_texture(img[0] if "file" not in x else from_file, x))
        assert e.value.status == RT_ERR_SCENE, str(e.value)
    # a mask whose image lost its plane is refused when the file is read
    d = json.loads(text)
    del d["texture"]["data"][img[0]]["alpha"]
    with pytest.raises(rtmi.RtmiError):
        rtmi.Scene.parse(json.dumps(d))


def _build(args, **kw):
    r = subprocess.run(args, capture_output=True, text=True, **kw)
    assert r.returncode == 0, r.stderr[-3000:]


def test_the_cpp_wrapper(rtmi, tmp_path):
    """include/rtmi.hpp through tests/alpha_host_driver.cpp: image_texture_rgba() and alpha_masked() carry the mask through the
    scene's build, the texture may be the material's own image, an emitter and an image without a plane are refused"""
    exe = str(tmp_path / "w")
    pkg = os.path.dirname(rtmi.LIB_PATH)
    _build(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "alpha_host_driver.cpp"), "-L", pkg, "-lrtmi",
            "-Wl,-rpath," + pkg])
    out = subprocess.run([exe, "wrapper"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    doc = json.loads(out.stdout)
    assert doc["material"]["data"][:3] == [{"type": "lambertian", "texture": 0, "alpha": {"texture": 0, "cutoff": 0.5}},
                                          {"type": "lambertian", "texture": 0},
                                          {"type": "metal", "albedo": [0.5, 0.5, 0.5], "fuzz": 0, "alpha": {"texture": 0, "cutoff": 0.25}}]
    assert doc["texture"]["data"][0]["alpha"] == [0, 255, 0, 255, 0, 255] and doc["texture"]["data"][0]["data"][:3] == [0, 200, 50]


# ------------------------------------------------------------------------------------------------------------ 5. the reference
@pytest.fixture(scope="module")
def words(rtmi):
    return R.uniforms(rtmi, NS.REF_SEED, NS.REF_W, NS.REF_H, 0, 2, NS.REF_DRAWS)


@pytest.mark.parametrize("name", ["al_sky", "al_lights"])
def test_opaque_masks_give_the_plain_references_samples(rtmi, words, name):
    sc = AS.scene(rtmi, name, masks="opaque")
    log = R.new_log()
    a, sa, da = R.trace(R.RefScene(sc), words, log=log)
    b, sb, db = R.trace(R.RefScene(AS.scene(rtmi, name, masks=False)), words)
    assert np.array_equal(a, b) and np.array_equal(sa, sb) and np.array_equal(da, db)
    assert log["alpha_masked_hits"] > 1000 and log["alpha_passes"] == 0 and log["alpha_opaque"] == log["alpha_masked_hits"] and log["alpha_max_passes"] == 0


@pytest.mark.parametrize("name", ["al_sky", "al_layers", "al_lights"])
def test_clear_masks_give_the_samples_of_the_scene_without_those_primitives(rtmi, words, name):
    """every primitive type is among the masked ones.  The rays restart at every hole, so the comparison is at rounding level
    (fp64: 1e-9) with the same draws consumed -- on every sample but those with a surface within t_min behind a hole, which the
    model skips and deleting does not (each sample that differs is shown to be one)"""
    clear, gone = AS.scene(rtmi, name, masks="clear"), AS.scene(rtmi, name, masks="deleted")
    types = {int(p["type"]) for p in clear.prims() if clear.alpha(int(p["material"])) is not None}
    if name == "al_sky":
        assert len(types) >= 4, types  # sphere, rectangle, cylinder, quad (al_layers adds the triangles)
    log = R.new_log()
    G = R.RefScene(gone)
    near = np.zeros(len(words), bool)  # samples one of whose holes has a surface of the remaining scene within t_min behind it

    def on_pass(samples, at, d):
        # a ray from t_min in FRONT of the hole, over 2 t_min: what it meets lies within t_min behind the hole (with a margin
        # of a thousandth of t_min for the two roundings)
        tm = R.T_MIN
        _, idx = R.closest_hit(G, at - tm * d, d, 2.001 * tm, np.float64)
        near[samples[idx >= 0]] = True
    a, _, da = R.trace(R.RefScene(clear), words, log=log, on_pass=on_pass)
    b, _, db = R.trace(G, words)
    same = np.abs(a - b).max(axis=1) <= 1e-9 * np.maximum(1.0, np.abs(b).max(axis=1))
    print(f"\n{name}: {(~same).sum()} of {len(same)} samples differ, {near.sum()} have a surface within t_min behind a hole")
    # the model's one difference from deleting: a surface within t_min behind a hole is skipped (the floor under a resting masked
    # sphere, met at a grazing angle).  Every sample that differs is such a sample; every other one agrees, draws included
    assert not (~same & ~near).any(), np.flatnonzero(~same & ~near)
    assert np.array_equal(da[same], db[same]) and (~same).sum() <= 3
    assert log["alpha_passes"] == log["alpha_masked_hits"] > 1000 and log["alpha_opaque"] == 0


def test_the_tally_and_the_cap(rtmi):
    """70 stacked all-transparent quads in front of a wall: the head-on query passes 64 and the 65th hit is opaque"""
    sc = AS.stack(rtmi)
    S = R.RefScene(sc)
    o, d = np.array([[0.0, 0.0, 10.0], [0.0, 0.0, 10.0], [30.0, 0.0, 10.0]]), np.array([[0.0, 0.0, -1.0], [0.0, 0.0, -20.0], [0.0, 0.0, -1.0]])
    log = R.new_log()
    t, idx = R.opaque_hit(S, o, d, np.inf, np.float64, log=log, samples=np.arange(3))
    quad65 = 1 + R.CAP  # (the wall is primitive 0, the quads follow)
    assert idx.tolist() == [quad65, quad65, -1]
    assert abs(t[0] - (10.0 - (4.0 - 0.1 * R.CAP))) < 1e-6 and abs(t[1] - t[0] / 20) < 1e-9  # (the total t, from the first origin; the quad's z is an fp32)
    assert log["alpha_masked_hits"] == 130 and log["alpha_passes"] == 128 and log["alpha_opaque"] == 2 and log["alpha_max_passes"] == R.CAP
    assert sorted(log["alpha_masked_samples"]) == [0, 1] and log["alpha_path_queries"] == 3 and log["alpha_shadow_queries"] == 0
    # a shadow query (an array of far ends) whose far end lies behind 3 quads passes them and is clear; one that ends on the
    # 66th hit is occluded by the 65th
    far = np.array([6.25, 20.0])
    t, idx = R.opaque_hit(S, o[:2], np.array([[0.0, 0.0, -1.0]] * 2), far, np.float64, log=log)
    assert idx.tolist() == [-1, quad65] and log["alpha_shadow_through"] == 2 and log["alpha_shadow_queries"] == 2
    # 64 quads: all passed, the wall is the winner; without masks: the first quad
    few = AS.stack(rtmi, n=R.CAP)
    assert R.opaque_hit(R.RefScene(few), o[:1], d[:1], np.inf, np.float64)[1].tolist() == [0]
    assert R.opaque_hit(R.RefScene(AS.stack(rtmi, masks=False)), o[:1], d[:1], np.inf, np.float64)[1].tolist() == [1]
    # the mistakes change the verdicts
    assert R.opaque_hit(S, o[:1], d[:1], np.inf, np.float64, perturb=("al_off",))[1].tolist() == [1]
    assert R.opaque_hit(S, o[:1], d[:1], np.inf, np.float64, perturb=("al_inverted",))[1].tolist() == [1]
    assert R.opaque_hit(S, o[:1], d[:1], far[1:], np.float64, perturb=("al_shadow_opaque",))[1].tolist() == [1]
    # the frame's centre pixel is the 65th quad's colour under the white background
    w = R.uniforms(rtmi, 5, 9, 9, 0, 1, 64)
    rgb, _, _ = R.trace(S, w)
    assert np.abs(rgb.reshape(9, 9, 3)[4, 4] - np.array(AS.stack_colour(R.CAP))).max() < 1e-6


def test_the_nested_clump_holds_its_contents(rtmi):
    """the nested case's conditions, from the reference's tally (its grid is the kernels' business: layout 52 against the flat
    walk is test_gpu_alpha.py's)"""
    tally = AS.nested_tally(rtmi)
    print("\n    " + ", ".join(f"{k} {v if isinstance(v, int) else round(v, 3)}" for k, v in tally.items() if k.startswith("alpha_")))
    AS.check_contents("al_nested", tally)


@pytest.mark.parametrize("name", list(AS.CASES))
def test_every_case_holds_its_contents(rtmi, name):
    """the conditions test_gpu_alpha.py asserts before it compares, checked here without a device"""
    words, shutter = AS.inputs(rtmi, name)
    rgb, stable, draws, tally = R.reference(R.RefScene(AS.scene(rtmi, name)), words, shutter)
    print("\n    " + ", ".join(f"{k} {v if isinstance(v, int) else round(v, 3)}" for k, v in tally.items() if k.startswith("alpha_")))
    AS.check_contents(name, tally)
    assert draws.max() <= NS.REF_DRAWS and np.isfinite(rgb).all() and 1 - stable.mean() <= 0.01


@pytest.mark.parametrize("name,mistake", AS.MISTAKES)
def test_a_mistake_changes_the_reference(rtmi, words, name, mistake):
    S = R.RefScene(AS.scene(rtmi, name))
    w = words[:NS.REF_W * NS.REF_H]
    good, _, _ = R.trace(S, w)
    wrong, _, _ = R.trace(S, w, perturb=(mistake,))
    moved = (np.abs(good - wrong).max(axis=1) > 1e-4).mean()
    print(f"\n{name}, {mistake}: {100 * moved:.1f} % of the samples move")
    assert moved > 0.03, (mistake, moved)


@pytest.mark.parametrize("name", ["al_layers", "al_lights"])
def test_the_alpha_cases_trace_as_pinned(rtmi, golden_dir, name):
    """golden/ref64_alpha_pin.npz holds what the reference returned on al_layers (several passes in one query) and al_lights
    (shadow rays through holes) while the alpha-aware query was a module of its own that stood in ref64.closest_hit's place for
    the length of a trace (golden/make_ref64_alpha_pin.py; the first sample of each pixel).  Compared as
    test_glass.py::test_the_extensions_trace_as_pinned compares: the draws, the signature, the seven counters and first_idx
    exact; the radiance at rtol 1e-9 -- the fp64 run's after rounding to float32, as it is stored; the fp32 run's by its bytes"""
    pin = np.load(os.path.join(golden_dir, "ref64_alpha_pin.npz"))
    cases = json.loads(str(pin["cases"]))
    at, rec = list(cases).index(name), cases[name]
    S, sha = R.RefScene(AS.scene(rtmi, name)), lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    words = AS.inputs(rtmi, name)[0][:NS.REF_W * NS.REF_H]
    for k, (tag, dtype) in enumerate((("64", np.float64), ("32", np.float32))):
        log, probe = R.new_log(), {}
        rgb, sig, draws = R.trace(S, words, dtype=dtype, log=log, probe=probe)
        assert np.array_equal(draws, pin["draws"][k][at]) and sha(sig) == rec["sig" + tag], (name, tag)
        assert {c: log["alpha_" + c] for c in R.ALPHA_COUNTERS} == rec["counters" + tag], (name, tag)
        assert sha(probe["first_idx"]) == rec["first_idx" + tag], (name, tag)
        if tag == "64":
            assert np.allclose(rgb.astype(np.float32), pin["rgb64"][at], rtol=1e-9, atol=1e-12), (name, tag)
        else:
            assert sha(rgb) == rec["rgb32"], (name, tag)


def test_the_tool_writes_the_shipped_scene(rtmi, scenes_dir):
    """tools/make_alpha_maps.py reproduces scenes/cutout_garden.json byte for byte; the file stays small, parses from its own
    text and carries the masks the README names"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_alpha_maps
    finally:
        sys.path.pop(0)
    with open(os.path.join(scenes_dir, "cutout_garden.json")) as f:
        text = f.read()
    assert make_alpha_maps.scene_text() == text
    assert len(text) < 96 * 1024
    sc = rtmi.Scene.parse(text)
    masked = [m for m in range(len(sc.materials())) if sc.alpha(m) is not None]
    assert len(masked) == 4 and all(0.2 < (sc.get_image_alpha(sc.alpha(m)[0]) >= R.cutoff_byte(sc.alpha(m)[1])).mean() < 0.8 for m in masked)


# ------------------------------------------------------------------------------------------------------------ 6. sanitizers
def test_the_reader_and_the_packer_are_sanitizer_clean(tmp_path):
    """tests/alpha_host_driver.cpp with -DALPHA_DRIVER_PACK: a stand-alone program (its own main) over the PNG reader, scene.cpp,
    capi.cpp and the packer compiled as plain C++ with -fsanitize=address,undefined, run as a child on the PNG files above"""
    csrc = os.path.join(PKG, "csrc")
    exe = str(tmp_path / "alpha_san")
    _build(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DALPHA_DRIVER_PACK",
            "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "alpha_host_driver.cpp"), os.path.join(csrc, "scene.cpp"),
            os.path.join(csrc, "capi.cpp"), "-x", "c++", os.path.join(csrc, "pack.hip"), "-o", exe])
    files = [v[0] for v in png_files(tmp_path).values()]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "pack"] + files, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print("\n" + r.stdout.strip())
    assert "alpha driver ok: 3 images with alpha" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr
