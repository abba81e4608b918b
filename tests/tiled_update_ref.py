"""Region update restated in numpy and struct from the formulas of include/fri_emit.h ("Region update"), independent of the library: the covered rectangle, the
region split as a literal per-pixel definition over the raster, and the splice of two `frit` files by their tables. No GPU involved."""
import struct

import numpy as np

from tests.tiled_ref import HEADER, parse_frit
from tests.tiled_region_ref import region_tiles


def region_cover(w, h, tile_w, tile_h, x, y, rw, rh):
    """(cx, cy, cw, ch): the image pixels the tiles touched by the region are made of; None for a region region_tiles refuses"""
    r = region_tiles(w, h, tile_w, tile_h, x, y, rw, rh)
    if r is None:
        return None
    i0, j0, ni, nj = r
    cx, cy = i0 * tile_w, j0 * tile_h
    return cx, cy, min((i0 + ni) * tile_w, w) - cx, min((j0 + nj) * tile_h, h) - cy


def split_region(img, tile_w, tile_h, x, y, rw, rh):
    """image [H][W][C] -> the sub-grid's tile raster [nj ni][tile_h][tile_w][C], pixel by pixel:
    sub(b ni + a, yy, xx, c) = image(min((j0 + b) tile_h + yy, H - 1), min((i0 + a) tile_w + xx, W - 1), c)"""
    img = np.asarray(img, np.uint8)
    h, w, c = img.shape
    i0, j0, ni, nj = region_tiles(w, h, tile_w, tile_h, x, y, rw, rh)
    out = np.empty((nj * ni, tile_h, tile_w, c), np.uint8)
    for b in range(nj):
        for a in range(ni):
            for yy in range(tile_h):
                gy = min((j0 + b) * tile_h + yy, h - 1)
                for xx in range(tile_w):
                    out[b * ni + a, yy, xx] = img[gy, min((i0 + a) * tile_w + xx, w - 1)]
    return out


def split_region_fast(img, tile_w, tile_h, x, y, rw, rh):
    """split_region with index arrays in the place of the two inner loops (the large shapes); tests/test_tiled_update_host.py holds it to split_region"""
    img = np.asarray(img, np.uint8)
    h, w, c = img.shape
    i0, j0, ni, nj = region_tiles(w, h, tile_w, tile_h, x, y, rw, rh)
    out = np.empty((nj * ni, tile_h, tile_w, c), np.uint8)
    for b in range(nj):
        rows = np.minimum((j0 + b) * tile_h + np.arange(tile_h), h - 1)
        for a in range(ni):
            cols = np.minimum((i0 + a) * tile_w + np.arange(tile_w), w - 1)
            out[b * ni + a] = img[rows][:, cols]
    return out


def sub_tiles(nx, i0, j0, ni, nj):
    """the file's tile index of every sub-tile, in the sub-grid's order"""
    return [(j0 + b) * nx + (i0 + a) for b in range(nj) for a in range(ni)]


def splice(file_a, file_b, x, y, rw, rh):
    """The `frit` file with file_b's payloads on the tiles the region touches and file_a's everywhere else, file_a's header, the table rebuilt"""
    fa, fb = parse_frit(file_a), parse_frit(file_b)
    assert all(fa[k] == fb[k] for k in ("H", "W", "tile_h", "tile_w", "ny", "nx"))
    i0, j0, ni, nj = region_tiles(fa["W"], fa["H"], fa["tile_w"], fa["tile_h"], x, y, rw, rh)
    touched = set(sub_tiles(fa["nx"], i0, j0, ni, nj))
    payloads = [fb["payloads"][t] if t in touched else fa["payloads"][t] for t in range(len(fa["payloads"]))]
    table, at = [], fa["offsets"][0]
    for p in payloads:
        table.append(at)
        at += len(p)
    return bytes(file_a[:HEADER]) + struct.pack(f"<{len(table) + 1}Q", *table, at) + b"".join(payloads)
