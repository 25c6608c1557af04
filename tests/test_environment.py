"""Environment maps without a GPU: the file readers, the scene interface, the lookup against a restatement through
the checker library's atan2 / acos, the sampling tables, the light list and the untouched tables of scenes without a map."""
import ctypes as C
import hashlib
import os
import struct
import zlib

import numpy as np
import pytest

PI32 = np.float32(3.1415927410125732421875)
TWO_PI32 = np.float32(6.283185482025146484375)


def small_scene(rtmi, env=None, scale=1.0, rotate=0.0):
    sc = rtmi.Scene.new(64, 36, 4, 4)
    sc.set_background((0.1, 0.2, 0.3), sky_gradient=False, defocus_blur=False)
    sc.camera((0, 1, 4), (0, 0.5, 0), (0, 1, 0), 50.0)
    sc.xz_rect(-5, 5, -5, 5, 0.0, sc.lambertian((0.5, 0.5, 0.5)))
    sc.sphere((0, 0.5, 0), 0.5, sc.lambertian((0.3, 0.5, 0.7)))
    if env is not None:
        sc.set_environment(env, scale, rotate)
    return sc


def random_map(rows=8, cols=16, seed=1, zeros=True):
    rng = np.random.default_rng(seed)
    env = (rng.random((rows, cols, 3)) * 4 + 0.01).astype(np.float32)
    if zeros:
        env[2, :] = 0
        env[5, 3] = 0
        env[rows - 1, cols - 1] = 0
    return env


# ---- readers -----------------------------------------------------------------------------------------------------------------
def rgbe_encode(img):
    """float RGB -> RGBE bytes (the reference encoder of the format: frexp of the largest channel)"""
    m = img.max(axis=2)
    mant, ex = np.frexp(m)
    sc = np.where(m < 1e-32, 0.0, mant * 256.0 / np.maximum(m, 1e-38))
    out = np.zeros(img.shape[:2] + (4,), np.uint8)
    out[..., :3] = (img * sc[..., None]).astype(np.uint8)
    out[..., 3] = np.where(m < 1e-32, 0, ex + 128).astype(np.uint8)
    return out


def rgbe_decode(q):
    f = np.where(q[..., 3] == 0, 0.0, np.ldexp(1.0, q[..., 3].astype(np.int32) - 136))
    return (q[..., :3].astype(np.float64) * f[..., None]).astype(np.float32)


def rle_scanline(row):
    """new-style run-length scanline of one row of RGBE pixels [W][4]"""
    w = row.shape[0]
    out = bytearray([2, 2, w >> 8, w & 255])
    for ch in range(4):
        v = row[:, ch]
        x = 0
        while x < w:
            run = 1
            while x + run < w and run < 127 and v[x + run] == v[x]:
                run += 1
            if run >= 3:
                out += bytes([128 + run, int(v[x])])
                x += run
            else:
                n = 1
                while x + n < w and n < 128 and not (x + n + 2 < w and v[x + n] == v[x + n + 1] == v[x + n + 2]):
                    n += 1
                out += bytes([n]) + bytes(int(b) for b in v[x:x + n])
                x += n
    return bytes(out)


def hdr_file(img, rle):
    q = rgbe_encode(img)
    head = b"#?RADIANCE\n# made by a test\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n-Y %d +X %d\n" % img.shape[:2]
    body = b"".join(rle_scanline(r) for r in q) if rle else q.tobytes()
    return head + body, rgbe_decode(q)


def pfm_file(img, little):
    flipped = img[::-1].astype("<f4" if little else ">f4")
    return b"PF\n%d %d\n%s\n" % (img.shape[1], img.shape[0], b"-1.0" if little else b"1.0") + flipped.tobytes()


def png_file(img8):
    h, w, _ = img8.shape
    raw = b"".join(b"\x00" + img8[y].tobytes() for y in range(h))
    chunk = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b"")


def hdr_image(rows=6, cols=24):
    rng = np.random.default_rng(5)
    img = (rng.random((rows, cols, 3)) * np.exp(rng.uniform(-6, 8, (rows, cols, 1)))).astype(np.float32)
    img[1, 4:14] = img[1, 4]  # (runs for the encoder)
    img[3, :] = 0
    return img


@pytest.mark.parametrize("rle", [False, True])
def test_hdr_reader(rtmi, tmp_path, rle):
    img = hdr_image()
    data, decoded = hdr_file(img, rle)
    p = tmp_path / "map.hdr"
    p.write_bytes(data)
    sc = small_scene(rtmi)
    sc.set_environment(file=str(p), scale=1.5, rotate=10.0)
    got, scale, rot = sc.environment
    assert (scale, rot) == (1.5, 10.0)
    assert np.array_equal(got, decoded)  # what the bytes say, exactly
    # ... and the image within RGBE's quantisation: 8-bit mantissas scaled by the largest channel
    assert np.all(np.abs(got - img) <= img.max(axis=2, keepdims=True) / 128.0)


@pytest.mark.parametrize("little", [False, True])
def test_pfm_reader(rtmi, tmp_path, little):
    img = hdr_image(5, 7)
    p = tmp_path / "map.pfm"
    p.write_bytes(pfm_file(img, little))
    sc = small_scene(rtmi)
    sc.set_environment(file=str(p))
    assert np.array_equal(sc.environment[0], img)


def test_ldr_readers(rtmi, tmp_path):
    rng = np.random.default_rng(2)
    img8 = rng.integers(0, 256, (4, 6, 3), dtype=np.uint8)
    (tmp_path / "m.png").write_bytes(png_file(img8))
    (tmp_path / "m.ppm").write_bytes(b"P6\n6 4\n255\n" + img8.tobytes())
    for name in ("m.png", "m.ppm"):
        sc = small_scene(rtmi)
        sc.set_environment(file=str(tmp_path / name))
        assert np.array_equal(sc.environment[0], img8.astype(np.float32) / np.float32(255.0)), name


def test_malformed_files_fail_cleanly(rtmi, tmp_path):
    img = hdr_image()
    flat, _ = hdr_file(img, False)
    rle, _ = hdr_file(img, True)
    pfm = pfm_file(img, True)
    bad = {
        "trunc_flat.hdr": (flat[:-5], 2), "trunc_rle.hdr": (rle[:-3], 2), "trunc.pfm": (pfm[:-4], 2),
        "orient.hdr": (flat.replace(b"-Y 6 +X 24", b"+Y 6 +X 24"), 4), "format.hdr": (flat.replace(b"32-bit_rle_rgbe", b"32-bit_rle_xyze"), 4),
        "nohead.hdr": (b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n", 4), "size.hdr": (flat.replace(b"-Y 6 +X 24", b"-Y 0 +X 24"), 4),
        "grey.pfm": (b"Pf\n2 2\n-1.0\n" + b"\0" * 16, 4), "scale.pfm": (b"PF\n2 2\n0\n" + b"\0" * 48, 4), "head.pfm": (b"PF\n2\n", 4),
        "neg.pfm": (pfm_file(-img, True), 4), "huge.pfm": (b"PF\n8192 8192\n-1.0\n", 6), "huge.hdr": (flat.replace(b"-Y 6 +X 24", b"-Y 65536 +X 65536"), 6),
    }
    sc = small_scene(rtmi)
    for name, (data, status) in bad.items():
        p = tmp_path / name
        p.write_bytes(data)
        with pytest.raises(rtmi.RtmiError) as e:
            sc.set_environment(file=str(p))
        assert e.value.status == status, (name, e.value.status, str(e.value))
        assert sc.environment is None
    with pytest.raises(rtmi.RtmiError) as e:
        sc.set_environment(file=str(tmp_path / "missing.hdr"))
    assert e.value.status == 2
    # a run that would write past its scanline
    q = bytearray(rle)
    at = q.index(b"\n\n") + 2 + len(b"-Y 6 +X 24\n") + 4
    q[at] = 128 + 127
    (tmp_path / "run.hdr").write_bytes(bytes(q))
    with pytest.raises(rtmi.RtmiError) as e:
        sc.set_environment(file=str(tmp_path / "run.hdr"))
    assert e.value.status in (2, 4)


# ---- scene interface ---------------------------------------------------------------------------------------------------------
def test_json_and_clone_round_trips(rtmi, tmp_path):
    env = random_map()
    sc = small_scene(rtmi, env, 2.5, 75.0)
    for other in (rtmi.Scene.parse(sc.to_json()), sc.clone()):
        got, scale, rot = other.environment
        assert np.array_equal(got, env) and (scale, rot) == (2.5, 75.0)
        assert np.array_equal(other.table_image(), sc.table_image())
    assert rtmi.Scene.parse(rtmi.Scene.parse(sc.to_json()).to_json()).to_json() == rtmi.Scene.parse(sc.to_json()).to_json()
    # a file-backed environment is written as its path
    (tmp_path / "sky.pfm").write_bytes(pfm_file(env, True))
    sc.set_environment(None)
    text = sc.to_json()
    assert '"environment"' not in text
    text = text.replace('"camera"', '"environment": {"file": "sky.pfm", "scale": 0.5, "rotate": -20}, "camera"', 1)
    (tmp_path / "scene.json").write_text(text)
    loaded = rtmi.Scene.load(str(tmp_path / "scene.json"))
    got, scale, rot = loaded.environment
    assert np.array_equal(got, env) and (scale, rot) == (0.5, -20.0)
    assert '"environment": {"file": "sky.pfm", "scale"' in loaded.to_json()
    # clearing
    loaded.set_environment(None)
    assert loaded.environment is None and np.array_equal(loaded.table_image(), small_scene(rtmi).table_image())


def test_limits_and_argument_errors(rtmi):
    sc = small_scene(rtmi)
    lib = C.CDLL(rtmi.LIB_PATH)
    lib.rt_scene_set_environment.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float]
    one = (C.c_float * 3)(1, 1, 1)
    assert lib.rt_scene_set_environment(sc._h, 1 << 13, (1 << 12) + 1, one, 1.0, 0.0) == 6  # beyond 2^25 texels: before any read
    assert lib.rt_scene_set_environment(sc._h, 1 << 20, 1 << 20, one, 1.0, 0.0) == 6
    assert lib.rt_scene_set_environment(sc._h, 1, 1, None, 1.0, 0.0) == 1
    assert lib.rt_scene_set_environment(sc._h, -1, 4, one, 1.0, 0.0) == 1
    assert lib.rt_scene_set_environment(None, 1, 1, one, 1.0, 0.0) == 1
    for scale, rot in ((-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("nan")), (1.0, float("inf"))):
        assert lib.rt_scene_set_environment(sc._h, 1, 1, one, scale, rot) == 1
    bad = (C.c_float * 3)(1, -0.5, 1)
    assert lib.rt_scene_set_environment(sc._h, 1, 1, bad, 1.0, 0.0) == 4
    bad = (C.c_float * 3)(1, float("nan"), 1)
    assert lib.rt_scene_set_environment(sc._h, 1, 1, bad, 1.0, 0.0) == 4
    assert sc.environment is None
    with pytest.raises(rtmi.RtmiError):
        sc.environment_eval((0, 1, 0))  # no environment
    sc.set_environment(random_map())
    with pytest.raises(rtmi.RtmiError):
        sc.environment_eval((0, 0, 0))
    with pytest.raises(rtmi.RtmiError):
        sc.environment_sample(1.0, 0.5)
    for text in ('{"rows": 2, "cols": 2, "data": [1, 2, 3]}', '{"rows": 0, "cols": 2, "data": []}', '{"file": 3}', '[1]',
                 '{"rows": 1, "cols": 1, "data": [1, -1, 1]}', '{"rows": 1, "cols": 1, "data": [1, 1, 1], "scale": -2}'):
        j = small_scene(rtmi).to_json().replace('"camera"', '"environment": %s, "camera"' % text, 1)
        with pytest.raises(rtmi.RtmiError) as e:
            rtmi.Scene.parse(j)
        assert e.value.status == 4, text


# ---- the lookup --------------------------------------------------------------------------------------------------------------
def checker_trig(rtcheck):
    lib = rtcheck.oracle_lib()
    lib.rto_atan2f.restype = C.c_float
    lib.rto_atan2f.argtypes = [C.c_float, C.c_float]
    lib.rto_acosf.restype = C.c_float
    lib.rto_acosf.argtypes = [C.c_float]
    return lib


def restated_texel(lib, d, rows, cols, rotate):
    """DESIGN 7e, one fp32 operation per step, through the checker library's atan2 / acos"""
    f = np.float32
    d = (np.asarray(d, np.float64) / np.linalg.norm(np.asarray(d, np.float64))).astype(np.float32)
    v = f(lib.rto_acosf(float(d[1]))) / PI32
    row = min(int(f(v * f(rows))), rows - 1)
    u = f(f(lib.rto_atan2f(float(-d[2]), float(d[0]))) + PI32) / TWO_PI32
    t = rotate / 360.0
    uoff = f(t - np.floor(t))
    uoff = uoff if uoff < 1 else f(0)
    u = f(u + uoff)
    u = f(u - np.floor(u))
    col = min(int(f(u * f(cols))), cols - 1)
    return row, col


@pytest.mark.parametrize("rows,cols,rotate,scale", [(8, 16, 0.0, 1.0), (7, 13, 33.3, 2.5), (16, 8, -100.0, 0.125), (1, 1, 0.0, 3.0), (3, 64, 725.0, 1.0)])
def test_eval_matches_the_restatement_on_every_direction(rtmi, rtcheck, rows, cols, rotate, scale):
    lib = checker_trig(rtcheck)
    env = random_map(rows, cols, seed=rows * 100 + cols, zeros=False)
    sc = small_scene(rtmi, env, scale, rotate)
    rng = np.random.default_rng(11)
    dirs = rng.normal(size=(3000, 3)) * np.exp(rng.uniform(-3, 3, (3000, 1)))
    dirs = np.concatenate([dirs, [[0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [-1, 0, 1e-9], [-1, 0, -1e-9]]])
    for d in dirs:
        rgb, _ = sc.environment_eval(d)
        row, col = restated_texel(lib, d, rows, cols, rotate)
        assert np.array_equal(rgb, np.float32(scale) * env[row, col]), (d, row, col)


def texel_centre(rows, cols, i, j):
    theta, phi = np.pi * (i + 0.5) / rows, 2 * np.pi * (j + 0.5) / cols - np.pi  # phi = atan2(-z, x)
    return np.array([np.sin(theta) * np.cos(phi), np.cos(theta), -np.sin(theta) * np.sin(phi)])


def test_rotation_by_whole_columns_is_a_roll(rtmi):
    rows, cols = 6, 12
    env = random_map(rows, cols, seed=3, zeros=False)
    for k in (1, 5, -2, 12 + 3):
        rot = small_scene(rtmi, env, 1.0, 360.0 * k / cols)
        rolled = small_scene(rtmi, np.roll(env, -k, axis=1))
        for i in range(rows):
            for j in range(cols):
                d = texel_centre(rows, cols, i, j)
                assert np.array_equal(rot.environment_eval(d)[0], rolled.environment_eval(d)[0]), (k, i, j)
                assert np.array_equal(rolled.environment_eval(d)[0], env[i, (j + k) % cols])


# ---- the tables --------------------------------------------------------------------------------------------------------------
def stored_tables(sc, rows, cols):
    """the fp32 tables as the packed image holds them, behind the texels (csrc/rt_env.h)"""
    img = sc.table_image().reshape(-1)
    env = sc.environment[0].reshape(-1)
    n = env.size
    starts = [k for k in range(0, img.size - n + 1, 4) if img[k] == env[0] and np.array_equal(img[k:k + n], env)]
    assert len(starts) == 1
    at = starts[0] + n
    marg = img[at:at + rows + 1]; at += rows + 1
    cond = img[at:at + rows * (cols + 1)].reshape(rows, cols + 1); at += rows * (cols + 1)
    band = img[at:at + rows]; at += rows
    ct = img[at:at + rows + 1]
    return marg, cond, band, ct


def test_tables_pdf_and_sampler(rtmi):
    rows, cols = 8, 16
    env = random_map(rows, cols)
    env[1, 2] = 400.0  # a sun
    sc = small_scene(rtmi, env, 2.0, 30.0)
    sc.set_light_sampling(True)
    marg, cond, band, ct = stored_tables(sc, rows, cols)
    lum = 0.2126 * env[..., 0].astype(np.float64) + 0.7152 * env[..., 1] + 0.0722 * env[..., 2]
    d_omega = (2 * np.pi / cols) * (np.cos(np.pi * np.arange(rows) / rows) - np.cos(np.pi * (np.arange(rows) + 1) / rows))
    assert np.allclose(band, d_omega, rtol=1e-6) and marg[0] == 0 and marg[rows] == 1
    assert np.all(np.diff(marg) >= 0) and np.all(np.diff(cond, axis=1) >= 0)
    w = lum * d_omega[:, None]
    assert np.allclose(np.diff(marg.astype(np.float64)), w.sum(1) / w.sum(), atol=2e-7)
    # the pdf of every texel, through eval at its centre: pmf from the stored tables over the band's solid angle; integrates to 1
    total = 0.0
    k = round(30.0 / 360.0 * cols * 3) // 3  # (30 degrees is not a whole number of columns: centres are looked up unrotated)
    plain = small_scene(rtmi, env, 2.0, 0.0)
    for i in range(rows):
        for j in range(cols):
            rgb, pdf = plain.environment_eval(texel_centre(rows, cols, i, j))
            assert np.array_equal(rgb, np.float32(2.0) * env[i, j])
            pmf = np.float32(marg[i + 1] - marg[i]) * np.float32(cond[i, j + 1] - cond[i, j])
            assert pdf == np.float32(pmf / band[i])
            assert (pdf == 0) == (lum[i, j] == 0)
            total += float(pdf) * d_omega[i]
    assert abs(total - 1.0) < 1e-5, total
    # the sampler on a stratified grid: the texel numpy's inverse CDF of the same tables predicts, eval's pdf, never a black texel
    n = 96
    for a in range(n):
        for b in range(n):
            u1, u2 = np.float32((a + 0.5) / n), np.float32((b + 0.37) / n)
            d, rgb, pdf = plain.environment_sample(u1, u2)
            i = int(np.searchsorted(marg, u1, side="right")) - 1
            j = int(np.searchsorted(cond[i], u2, side="right")) - 1
            assert np.array_equal(rgb, np.float32(2.0) * env[i, j]), (a, b, i, j)
            assert lum[i, j] > 0 and pdf > 0
            rgb2, pdf2 = plain.environment_eval(d)
            assert np.array_equal(rgb, rgb2) and pdf == pdf2
            assert abs(np.linalg.norm(d.astype(np.float64)) - 1) < 1e-5
    # ... and rotated: the sampled direction evaluates to the texel the tables chose
    for a in range(0, n, 5):
        for b in range(0, n, 5):
            u1, u2 = np.float32((a + 0.5) / n), np.float32((b + 0.37) / n)
            d, rgb, pdf = sc.environment_sample(u1, u2)
            i = int(np.searchsorted(marg, u1, side="right")) - 1
            j = int(np.searchsorted(cond[i], u2, side="right")) - 1
            assert np.array_equal(rgb, np.float32(2.0) * env[i, j]), (a, b, i, j)
    # the sun's share of the samples is its share of the weight
    hits = sum(np.array_equal(plain.environment_sample((a + 0.5) / n, (b + 0.5) / n)[1], np.float32(2.0) * env[1, 2]) for a in range(n) for b in range(n))
    assert abs(hits / n ** 2 - w[1, 2] / w.sum()) < 0.01


def test_lights_list_and_weight(rtmi, scenes_dir):
    sc = rtmi.Scene.load(os.path.join(scenes_dir, "mixed_emissive.json"))
    before = sc.lights().copy()
    assert len(before) == 3 and np.all(before["prim"] >= 0)
    env = random_map()
    sc.set_environment(env, 0.5, 40.0)
    after = sc.lights()
    assert len(after) == 4 and after[-1]["prim"] == -1 and after[-1]["shape"] == rtmi.LIGHT_ENVIRONMENT == 100
    assert after[-1]["area"] == np.float32(4 * np.pi)
    # the weight: r^2 x scale x sum(luminance x solid angle) beside area x luminance, r from the primitives' boxes
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for p in sc.prims():
        f = p["f"].astype(np.float64)
        if p["type"] == 0:
            box = (f[:3] - abs(f[3]), f[:3] + abs(f[3]))
        elif p["type"] in (1, 2, 3):
            ax = {1: (0, 1, 2), 2: (0, 2, 1), 3: (1, 2, 0)}[int(p["type"])]
            a, b = np.zeros(3), np.zeros(3)
            a[ax[0]], b[ax[0]], a[ax[1]], b[ax[1]], a[ax[2]], b[ax[2]] = f[0], f[1], f[2], f[3], f[4], f[4]
            box = (a, b)
        else:
            m = p["m"].astype(np.float64).reshape(3, 4)
            pts = np.array([m[:, :3] @ np.array([sx * abs(f[0]), sy * abs(f[0]), z]) + m[:, 3] for sx in (-1, 1) for sy in (-1, 1) for z in (f[1], f[2])])
            box = (pts.min(0), pts.max(0))
        lo, hi = np.minimum(lo, box[0]), np.maximum(hi, box[1])
    r = 0.5 * np.linalg.norm(hi - lo)
    lum = lambda c: 0.2126 * c[..., 0].astype(np.float64) + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]
    d_omega = (2 * np.pi / 16) * (np.cos(np.pi * np.arange(8) / 8) - np.cos(np.pi * (np.arange(8) + 1) / 8))
    w_env = r * r * 0.5 * (lum(env) * d_omega[:, None]).sum()
    w_area = before["area"].astype(np.float64) * 0.5 * (lum(before["emission"]) + lum(before["emission_odd"]))
    want = np.append(w_area, w_env) / (w_area.sum() + w_env)
    assert np.allclose(after["probability"], want, rtol=1e-5)
    assert np.allclose(after["emission"][-1], 0.5 * (env.astype(np.float64) * d_omega[:, None, None]).sum((0, 1)) / (4 * np.pi), rtol=1e-5)
    # an all-zero map, and a map at scale 0, are no light; the list is what it was
    for e, s in ((np.zeros((4, 8, 3), np.float32), 1.0), (env, 0.0)):
        sc.set_environment(e, s)
        assert np.array_equal(sc.lights(), before)
        assert sc.environment_sample(0.5, 0.5)[2] == 0 or s == 0.0
    sc.set_environment(None)
    assert np.array_equal(sc.lights(), before)


def test_table_info_reports_the_environment_kernels(rtmi, scenes_dir):
    sc = rtmi.Scene.rtiow(7, 96, 54, 4, 10)
    assert sc.table_info().kernel_variant == 2 and sc.table_info().grid_wide == 0
    hot = sc.table_info().hot_bytes_grid
    sc.set_environment(random_map())
    t = sc.table_info()
    assert t.grid_wide == 1 and t.kernel_variant & 1024 and (t.kernel_variant & 1023) in (36, 44)
    sc = rtmi.Scene.load(os.path.join(scenes_dir, "mixed_emissive.json"))
    hot = sc.table_info().hot_bytes_grid
    sc.set_environment(random_map())
    assert sc.table_info().kernel_variant == 16 | 1024 and sc.table_info().hot_bytes_grid == hot  # (never staged into LDS)
    sc.set_light_sampling(True)
    assert sc.table_info().kernel_variant == 16 | 1024 | 256


def test_scenes_without_an_environment_keep_their_tables(rtmi, scenes_dir):
    """sha256 of rt_scene_table_image, taken at the commit before environment maps existed"""
    h = lambda sc: hashlib.sha256(sc.table_image().tobytes()).hexdigest()
    a = rtmi.Scene.load(os.path.join(scenes_dir, "three_sphere.json"))
    b = rtmi.Scene.load(os.path.join(scenes_dir, "mixed_emissive.json"))
    b.set_light_sampling(True)
    c = rtmi.Scene.rtiow(7, 96, 54, 4, 10)
    assert h(a) == "65d9f693d8145364cab143a7c4275c2119516b42e1e892ee7c3ab8cf6af2d97a"
    assert h(b) == "063862a7e5224dbc5bc379afcedeb1a8cce28a7390a25956892041d7527593fd"
    assert h(c) == "ebe6f7e3d5c21fea1b38fc3a607e1aa12497cd96d9482ec648c9921b8735b978"
    # setting and clearing a map leaves nothing behind
    b.set_environment(random_map())
    assert h(b) != "063862a7e5224dbc5bc379afcedeb1a8cce28a7390a25956892041d7527593fd"
    b.set_environment(None)
    assert h(b) == "063862a7e5224dbc5bc379afcedeb1a8cce28a7390a25956892041d7527593fd"
