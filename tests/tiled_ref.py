"""Tiled coding restated in numpy and struct, from the formulas of include/fri_hip.h ("tiled coding") and include/fri_emit.h (the `frit` container): the tile
grid, the split with edge replication, the merge, and a parser of the container that does not call the library. No GPU involved."""
import struct

import numpy as np

from tests.common import gen_image

MAGIC = b"frit"
HEADER = 32


def grid(w, h, tile_w, tile_h):
    """(nx, ny) = (ceil(W / tile_w), ceil(H / tile_h))"""
    return -(-w // tile_w), -(-h // tile_h)


def split_tiles(img, tile_w, tile_h):
    """image [H][W][C] -> tiles [ny nx][tile_h][tile_w][C]: tile(t, y, x, c) = image(min(j tile_h + y, H - 1), min(i tile_w + x, W - 1), c), t = j nx + i"""
    img = np.asarray(img, np.uint8)
    h, w, c = img.shape
    nx, ny = grid(w, h, tile_w, tile_h)
    out = np.empty((ny * nx, tile_h, tile_w, c), np.uint8)
    for j in range(ny):
        rows = np.minimum(j * tile_h + np.arange(tile_h), h - 1)
        for i in range(nx):
            cols = np.minimum(i * tile_w + np.arange(tile_w), w - 1)
            out[j * nx + i] = img[rows][:, cols]
    return out


def merge_tiles(tiles, w, h, fill=0):
    """tiles [ny nx][tile_h][tile_w][C] -> image [H][W][C]: the pixels with j tile_h + y < H and i tile_w + x < W (every image pixel exactly once)"""
    tiles = np.asarray(tiles, np.uint8)
    n, tile_h, tile_w, c = tiles.shape
    nx, ny = grid(w, h, tile_w, tile_h)
    assert n == nx * ny
    out = np.full((h, w, c), fill, np.uint8)
    for j in range(ny):
        for i in range(nx):
            y0, x0 = j * tile_h, i * tile_w
            hh, ww = min(tile_h, h - y0), min(tile_w, w - x0)
            out[y0:y0 + hh, x0:x0 + ww] = tiles[j * nx + i, :hh, :ww]
    return out


def parse_frit(data):
    """The container, field by field: dict(H, W, tile_h, tile_w, ny, nx, offsets, payloads). ValueError for anything the format forbids."""
    data = bytes(data)
    if len(data) < HEADER or data[:4] != MAGIC:
        raise ValueError("magic")
    version, h, w, tile_h, tile_w, ny, nx = struct.unpack_from("<7I", data, 4)
    if version != 1:
        raise ValueError("version")
    if not (h and w and tile_h and tile_w):
        raise ValueError("zero size")
    if (nx, ny) != grid(w, h, tile_w, tile_h):
        raise ValueError("grid")
    n = nx * ny
    if len(data) < HEADER + 8 * (n + 1):
        raise ValueError("table")
    offsets = struct.unpack_from(f"<{n + 1}Q", data, HEADER)
    if offsets[0] != HEADER + 8 * (n + 1) or offsets[n] != len(data):
        raise ValueError("ends of the table")
    if any(b <= a for a, b in zip(offsets, offsets[1:])):
        raise ValueError("offsets not strictly increasing")
    payloads = [data[a:b] for a, b in zip(offsets, offsets[1:])]
    for p in payloads:  # a complete frif file of a tile_h x tile_w image, the same metadata word everywhere
        if p[:4] != b"frif" or struct.unpack_from("<2I", p, 4) != (tile_h, tile_w) or p[12:16] != payloads[0][12:16] or p[-2:] != b"\xff\xdf":
            raise ValueError("payload")
    return dict(H=h, W=w, tile_h=tile_h, tile_w=tile_w, ny=ny, nx=nx, offsets=list(offsets), payloads=payloads)


def mixed_image(w, h, c, tile_w, seed=0):
    """smooth where x % tile_w < tile_w / 2 and noise elsewhere: every tile gets both, so that every tile fills all ten contexts"""
    smooth, noise = gen_image("smooth", w, h, c, seed), gen_image("noise", w, h, c, seed + 1)
    x = np.arange(w)
    return np.where(((x % tile_w) < tile_w / 2)[None, :, None], smooth, noise).astype(np.uint8)
