#!/usr/bin/env python3
"""Writes scenes/normal_map_wall.json with its normal maps, derived from height functions with numpy alone.
usage: tools/make_normal_maps.py [SCENE.json]      (default: ray-tracing-in-cuda_amd/scenes/normal_map_wall.json)

A map is a [rows][cols] image whose ROW index runs along the hit record's u and whose COLUMN index along v (image_texel's
convention).  From a periodic height field h over the unit square, sampled at the texel centres, the slopes by central
differences h_u, h_v (in units of the square), the normal (-h_u, -h_v, 1) / |.|, and the bytes the renderer decodes with
x = (r8 - 128) / 127: r8 = 128 + round(127 x), so a flat texel is exactly (128, 128, 255) and leaves the normal alone.
The maps are 32 x 32 texels and sit INLINE in the scene file ("rows", "cols", "data"), about 13 KB of text each: a shipped
scene must parse again from its own JSON text, without a directory to resolve file names against (tests/sanitize_driver.cpp),
so it cannot name image files.  write_png() writes any of them as an 8-bit RGB PNG for use elsewhere:
    python -c "import make_normal_maps as m; m.write_png('bricks.png', m.normal_map(m.bricks(*m.grid(64))))" """
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


def bricks(u, v, across=4, along=4, mortar=0.12):
    """courses stacked along v, bricks laid along u (a wall quad whose u edge is horizontal), every other course shifted by half
    a brick; the mortar lies lower, with a soft edge"""
    u, v = v, u
    cu = u * across
    course = np.floor(cu)
    cv = v * along + 0.5 * (course % 2)
    du, dv = np.abs(cu - course - 0.5), np.abs(cv - np.floor(cv) - 0.5)
    edge = lambda d, half, w: np.clip((half - d) / w, 0.0, 1.0)
    return edge(du, 0.5, mortar * 2) * edge(dv, 0.5, mortar) * 0.05


def dimples(u, v, count=3, depth=0.035):
    """a golf ball's: smooth round pits on a square lattice (twice as many along u: a sphere's u spans 360 degrees)"""
    a, b = u * 2 * count, v * count
    r2 = (a - np.floor(a) - 0.5) ** 2 + (b - np.floor(b) - 0.5) ** 2
    return -depth * np.exp(-r2 / 0.045)


def rivets(u, v, count=2, height=0.03):
    """round heads near the corners of every plate, and a shallow seam between the plates"""
    a, b = u * count, v * count
    fa, fb = a - np.floor(a), b - np.floor(b)
    h = np.zeros_like(u)
    for ca in (0.18, 0.82):
        for cb in (0.18, 0.82):
            h += height * np.exp(-((fa - ca) ** 2 + (fb - cb) ** 2) / 0.006)
    seam = np.minimum(np.minimum(fa, 1 - fa), np.minimum(fb, 1 - fb))
    return h - 0.01 * np.exp(-(seam / 0.03) ** 2)


def ripples(u, v, height=0.012):
    """two crossing wave trains"""
    return height * (np.sin(2 * np.pi * (5 * u + 2 * v)) + 0.6 * np.sin(2 * np.pi * (3 * v - 4 * u) + 1.0))


def normal_map(h, strength=1.0):
    n = h.shape[0]
    hu = (np.roll(h, -1, 0) - np.roll(h, 1, 0)) * (n / 2.0)
    hv = (np.roll(h, -1, 1) - np.roll(h, 1, 1)) * (n / 2.0)
    nrm = np.stack([-strength * hu, -strength * hv, np.ones_like(h)], axis=-1)
    nrm /= np.sqrt((nrm * nrm).sum(axis=-1))[..., None]
    return np.clip(np.rint(128 + 127 * nrm), 0, 255).astype(np.uint8)


def write_png(path, rgb):
    rows, cols, _ = rgb.shape
    raw = b"".join(b"\x00" + rgb[r].tobytes() for r in range(rows))  # (filter 0 on every scanline)
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 9)) + chunk(b"IEND", b""))


MAPS = {"bricks": bricks, "dimples": dimples, "rivets": rivets, "ripples": ripples}

# the scene: a brick-relief wall quad and floor, a dimpled pbr ball, a riveted rough_metal box, a rippled dielectric sheet with a
# red marble under it, one small light (light sampling is left to --nee)
HEAD = {'output_file': 'normal_map_wall.png', 'background': [0.02, 0.025, 0.035], 'sky_gradient': False, 'defocus_blur': False, 'max_depth': 12, 'samples_per_pixel': 64, 'width': 320, 'height': 180, 'camera': {'lookfrom': [0.6, 2.2, 7.0], 'lookat': [0, 1.0, 0], 'vup': [0, 1, 0], 'vfov': 34, 'aperture': 0}}
OBJECTS = [
    {'type': 'xz_rect', 'x0': -20, 'x1': 20, 'z0': -20, 'z1': 20, 'k': 0.0, 'material': 0},
    {'type': 'xz_rect', 'x0': -4, 'x1': 4, 'z0': -2, 'z1': 4, 'k': 0.01, 'material': 1},
    {'type': 'quad', 'q': [-4, 0, -2], 'u': [8, 0, 0], 'v': [0, 3.2, 0], 'material': 2},
    {'type': 'sphere', 'center': [-1.7, 0.8, 0.8], 'radius': 0.8, 'material': 3},
    {'type': 'box', 'min': [-0.6, 0, -0.6], 'max': [0.6, 1.2, 0.6], 'material': 4, 'rotate': {'axis': [0, 1, 0], 'angle': 28}, 'translate': [1.7, 0.01, 0.6]},
    {'type': 'xz_rect', 'x0': -0.9, 'x1': 0.9, 'z0': 1.8, 'z1': 3.4, 'k': 0.35, 'material': 5},
    {'type': 'sphere', 'center': [0.2, 0.3, 2.6], 'radius': 0.12, 'material': 7},
    {'type': 'xz_rect', 'x0': -0.5, 'x1': 0.5, 'z0': 0.8, 'z1': 1.6, 'k': 4.2, 'material': 6},
]
MATERIALS = [
    {'type': 'lambertian', 'texture': 0},
    {'type': 'lambertian', 'texture': 1, 'normal_map': {'texture': 4, 'scale': 1}},
    {'type': 'lambertian', 'texture': 2, 'normal_map': {'texture': 4, 'scale': 1.5}},
    {'type': 'pbr', 'texture': 3, 'metallic': 0.0, 'roughness': 0.35, 'normal_map': {'texture': 5}},
    {'type': 'rough_metal', 'albedo': [0.85, 0.75, 0.55], 'roughness': 0.3, 'normal_map': {'texture': 6, 'scale': 1}},
    {'type': 'dielectric', 'index_of_refraction': 1.33, 'normal_map': {'texture': 7, 'scale': 1}},
    {'type': 'diffuse_light', 'texture': 8},
    {'type': 'lambertian', 'texture': 9},
]
TEXTURES = [  # (a string: the map of that name, inline)
    {'type': 'solid_color', 'color': [0.45, 0.45, 0.42]},
    {'type': 'solid_color', 'color': [0.55, 0.5, 0.45]},
    {'type': 'solid_color', 'color': [0.62, 0.3, 0.22]},
    {'type': 'solid_color', 'color': [0.9, 0.9, 0.85]},
    'bricks',
    'dimples',
    'rivets',
    'ripples',
    {'type': 'solid_color', 'color': [70, 62, 50]},
    {'type': 'solid_color', 'color': [0.8, 0.2, 0.2]},
]


def scene_text():
    u, v = grid()
    texs = []
    for t in TEXTURES:
        if isinstance(t, str):
            rgb = normal_map(MAPS[t](u, v))
            t = {"type": "image", "rows": rgb.shape[0], "cols": rgb.shape[1], "data": [int(x) for x in rgb.reshape(-1)]}
        texs.append(json.dumps(t))
    rows = lambda items: ",\n".join("    " + x for x in items)
    out = "{\n" + "".join("  %s: %s,\n" % (json.dumps(k), json.dumps(v)) for k, v in HEAD.items())
    out += '  "object": {"data": [\n' + rows(json.dumps(o) for o in OBJECTS) + "\n  ]},\n"
    out += '  "material": {"data": [\n' + rows(json.dumps(m) for m in MATERIALS) + "\n  ]},\n"
    out += '  "texture": {"data": [\n' + rows(texs) + "\n  ]}\n}\n"
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes", "normal_map_wall.json")
    with open(path, "w") as f:
        f.write(scene_text())
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
