#!/usr/bin/env python3
"""Writes scenes/cutout_garden.json with its RGBA images, made with numpy alone.
usage: tools/make_alpha_maps.py [SCENE.json]      (default: ray-tracing-in-cuda_amd/scenes/cutout_garden.json)

An image is [rows][cols] texels whose ROW index runs along the hit record's u and whose COLUMN index along v (image_texel's
convention).  Its alpha plane is what a material's "alpha" mask reads: a texel whose alpha byte lies below ceil(255 x cutoff)
is a hole.  The shapes are drawn as coverage in [0, 1] over the unit square at the texel centres and stored as bytes, so a soft
edge moves with the material's cutoff.  The images are 32 x 32 texels and sit INLINE in the scene file ("rows", "cols", "data",
"alpha"): a shipped scene must parse again from its own JSON text, without a directory to resolve file names against
(tests/sanitize_driver.cpp), so it cannot name image files.  write_png() writes any of them as an 8-bit RGBA PNG (colour type 6,
written here with zlib) for use elsewhere -- the renderer reads such a file's alpha as the plane:
    python -c "import make_alpha_maps as m; m.write_png('leaf.png', *m.leaf(*m.grid(64)))" """
import json
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 32


def grid(n=None):
    n = n or N
    a = (np.arange(n) + 0.5) / n
    return np.meshgrid(a, a, indexing="ij")  # (u along rows, v along columns)


def _soft(d, w=0.04):
    """coverage of a shape from its signed distance d (negative inside)"""
    return np.clip(0.5 - d / w, 0.0, 1.0)


def _rgb(u, base, vary):
    c = np.clip(np.asarray(base)[None, None, :] + vary[..., None] * np.array([0.15, 0.2, 0.1]), 0.0, 1.0)
    return np.rint(255 * c).astype(np.uint8)


def leaf(u, v):
    """a pointed leaf along u with a midrib: two circular arcs; green, lighter towards the rib"""
    x, y = u - 0.5, v - 0.5
    r = 0.62
    d = np.maximum(np.hypot(x, y - (r - 0.27)), np.hypot(x, y + (r - 0.27))) - r
    rib = np.exp(-(y / 0.03) ** 2)
    return _rgb(u, (0.16, 0.42, 0.12), rib - 0.3 * np.abs(x)), _soft(d)


def fence(u, v, cells=6, wire=0.09):
    """chain link: two families of diagonal wires"""
    a, b = (u + v) * cells, (u - v) * cells
    d = np.minimum(np.abs(a - np.rint(a)), np.abs(b - np.rint(b))) / cells - wire / cells
    return _rgb(u, (0.55, 0.57, 0.6), 0.2 * np.sin(40 * u)), _soft(d, 0.01)


def perforated(u, v, count=5, hole=0.3):
    """round holes on a square lattice (twice as many along u: a sphere's u spans 360 degrees)"""
    a, b = u * 2 * count, v * count
    d = hole - np.hypot(a - np.floor(a) - 0.5, b - np.floor(b) - 0.5)
    return _rgb(u, (0.8, 0.62, 0.35), 0.0 * u), _soft(d, 0.05)


def decal(u, v):
    """a round stamp with a ragged edge: the radius wobbles with the angle"""
    x, y = u - 0.5, v - 0.5
    ang = np.arctan2(y, x)
    rad = 0.36 + 0.05 * np.sin(7 * ang) + 0.03 * np.sin(13 * ang + 1.0)
    ring = np.abs(np.hypot(x, y) - 0.22) < 0.05
    return _rgb(u, (0.7, 0.12, 0.1), np.where(ring, 1.0, 0.0)), _soft(np.hypot(x, y) - rad, 0.03)


def write_png(path, rgb, coverage):
    rows, cols, _ = rgb.shape
    rgba = np.concatenate([rgb, np.rint(255 * coverage).astype(np.uint8)[..., None]], axis=2)
    raw = b"".join(b"\x00" + rgba[r].tobytes() for r in range(rows))  # (filter 0 on every scanline)
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 9)) + chunk(b"IEND", b""))


IMAGES = {"leaf": leaf, "fence": fence, "perforated": perforated, "decal": decal}

# the scene: leaf cards on a stem, a chain-link fence quad in front of a small light (its lattice shadow falls on the floor
# with --nee), a perforated rough-metal sphere with a red marble inside, a pbr decal with a ragged edge lying on the floor
HEAD = {'output_file': 'cutout_garden.png', 'background': [0.03, 0.04, 0.06], 'sky_gradient': False, 'defocus_blur': False, 'max_depth': 12, 'samples_per_pixel': 64, 'width': 320, 'height': 180, 'camera': {'lookfrom': [0.4, 2.0, 7.0], 'lookat': [0, 0.9, 0], 'vup': [0, 1, 0], 'vfov': 34, 'aperture': 0}}
OBJECTS = [
    {'type': 'xz_rect', 'x0': -20, 'x1': 20, 'z0': -20, 'z1': 20, 'k': 0.0, 'material': 0},
    {'type': 'quad', 'q': [-6, 0, -3], 'u': [12, 0, 0], 'v': [0, 5, 0], 'material': 1},
    # the stem (a thin box) and five leaf cards on it
    {'type': 'box', 'min': [-0.04, 0, -0.04], 'max': [0.04, 2.0, 0.04], 'material': 2, 'translate': [-1.9, 0, 0.6]},
    {'type': 'quad', 'q': [-1.9, 0.5, 0.6], 'u': [0.9, 0.35, 0.2], 'v': [-0.15, 0.3, 0.5], 'material': 3},
    {'type': 'quad', 'q': [-1.9, 0.9, 0.6], 'u': [-0.9, 0.3, 0.25], 'v': [0.1, 0.3, -0.5], 'material': 3},
    {'type': 'quad', 'q': [-1.9, 1.3, 0.6], 'u': [0.8, 0.4, -0.3], 'v': [0.2, 0.25, 0.5], 'material': 3},
    {'type': 'quad', 'q': [-1.9, 1.6, 0.6], 'u': [-0.7, 0.45, -0.2], 'v': [-0.2, 0.2, -0.5], 'material': 3},
    {'type': 'quad', 'q': [-1.9, 1.95, 0.6], 'u': [0.1, 0.8, 0.1], 'v': [0.5, 0.0, -0.2], 'material': 3},
    # the fence, between the light and the floor in front of it
    {'type': 'quad', 'q': [-0.6, 0.0, -1.2], 'u': [3.6, 0, 0], 'v': [0, 2.4, 0], 'material': 4},
    {'type': 'xy_rect', 'x0': 0.7, 'x1': 1.5, 'y0': 2.6, 'y1': 3.2, 'k': -2.6, 'material': 7},
    # the perforated sphere and the marble inside it
    {'type': 'sphere', 'center': [1.4, 0.75, 1.4], 'radius': 0.75, 'material': 5},
    {'type': 'sphere', 'center': [1.4, 0.3, 1.4], 'radius': 0.28, 'material': 8},
    # the decal, lifted 0.01 over the floor
    {'type': 'xz_rect', 'x0': -1.0, 'x1': 0.4, 'z0': 1.6, 'z1': 3.0, 'k': 0.01, 'material': 6},
]
MATERIALS = [  # (a texture given as a string: the image of that name)
    {'type': 'lambertian', 'texture': 0},
    {'type': 'lambertian', 'texture': 1},
    {'type': 'lambertian', 'texture': 2},
    {'type': 'lambertian', 'texture': 'leaf', 'alpha': {'texture': 'leaf', 'cutoff': 0.5}},
    {'type': 'rough_metal', 'albedo': [0.6, 0.62, 0.65], 'roughness': 0.4, 'alpha': {'texture': 'fence', 'cutoff': 0.5}},
    {'type': 'rough_metal', 'albedo': [0.85, 0.65, 0.35], 'roughness': 0.3, 'alpha': {'texture': 'perforated', 'cutoff': 0.5}},
    {'type': 'pbr', 'texture': 'decal', 'metallic': 0.0, 'roughness': 0.4, 'alpha': {'texture': 'decal', 'cutoff': 0.35}},
    {'type': 'diffuse_light', 'texture': 3},
    {'type': 'lambertian', 'texture': 4},
]
TEXTURES = [
    {'type': 'solid_color', 'color': [0.45, 0.45, 0.42]},
    {'type': 'solid_color', 'color': [0.5, 0.48, 0.45]},
    {'type': 'solid_color', 'color': [0.3, 0.2, 0.1]},
    {'type': 'solid_color', 'color': [60, 54, 44]},
    {'type': 'solid_color', 'color': [0.8, 0.15, 0.15]},
    'leaf',
    'fence',
    'perforated',
    'decal',
]


def scene_text():
    u, v = grid()
    texs, where = [], {}
    for k, t in enumerate(TEXTURES):
        if isinstance(t, str):
            where[t] = k
            rgb, cov = IMAGES[t](u, v)
            t = {"type": "image", "rows": rgb.shape[0], "cols": rgb.shape[1], "data": [int(x) for x in rgb.reshape(-1)],
                 "alpha": [int(x) for x in np.rint(255 * cov).astype(np.uint8).reshape(-1)]}
        texs.append(json.dumps(t))
    mats = []
    for m in MATERIALS:
        m = json.loads(json.dumps(m))
        if isinstance(m.get("texture"), str):
            m["texture"] = where[m["texture"]]
        if "alpha" in m:
            m["alpha"]["texture"] = where[m["alpha"]["texture"]]
        mats.append(json.dumps(m))
    rows = lambda items: ",\n".join("    " + x for x in items)
    out = "{\n" + "".join("  %s: %s,\n" % (json.dumps(k), json.dumps(v)) for k, v in HEAD.items())
    out += '  "object": {"data": [\n' + rows(json.dumps(o) for o in OBJECTS) + "\n  ]},\n"
    out += '  "material": {"data": [\n' + rows(mats) + "\n  ]},\n"
    out += '  "texture": {"data": [\n' + rows(texs) + "\n  ]}\n}\n"
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "cutout_garden.json")
    with open(path, "w") as f:
        f.write(scene_text())
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
