"""Tiled RGBA coding restated in numpy by composition of the existing restatements (include/fri_hip.h, "Tiled RGBA coding"): tests.alpha_ref.split_rgba then
tests.tiled_ref.split_tiles of the colour raster and of the alpha plane; merge_tiles of both then merge_rgba; the plane order; and the `frit` container assembled
from per-tile files with struct, without the library. No GPU involved."""
import struct

import numpy as np

from tests.alpha_ref import ALPHA_CLEAN, ALPHA_KEEP, merge_rgba, split_rgba
from tests.tiled_ref import HEADER, MAGIC, grid, merge_tiles, split_tiles


def plane_index(n, t, channel):
    """plane(t, c) = 3 t + c for c = 0, 1, 2; plane(t, A) = 3 n + t (channel 3)"""
    return 3 * t + channel if channel < 3 else 3 * n + t


def plane_order(per_tile):
    """per_tile: n quadruples (c0, c1, c2, A) of anything -> the 4 n items in plane order"""
    n = len(per_tile)
    out = [None] * (4 * n)
    for t, planes in enumerate(per_tile):
        for c in range(4):
            out[plane_index(n, t, c)] = planes[c]
    return out


def split_tiles_rgba(pixels, w, h, tile_w, tile_h, clean=ALPHA_KEEP):
    """image [H][W][4] -> (colour_tiles [n][tile_h][tile_w][3], alpha_tiles [n][tile_h][tile_w]): the tile split of the colour raster and of the alpha plane that
    split_rgba produces"""
    rgb, a = split_rgba(pixels, w, h, clean)
    return split_tiles(rgb, tile_w, tile_h), split_tiles(a[:, :, None], tile_w, tile_h)[:, :, :, 0]


def merge_tiles_rgba(colour_tiles, alpha_tiles, w, h):
    """the tile rasters -> image [H][W][4]: the tile merge of both, then the interleave; no replicated pixel shows"""
    rgb = merge_tiles(colour_tiles, w, h)
    a = merge_tiles(np.asarray(alpha_tiles, np.uint8)[:, :, :, None], w, h)[:, :, 0]
    return merge_rgba(rgb, a, w, h).reshape(h, w, 4)


def sub_grid(arr, nx, i0, j0, ni, nj):
    """the per-tile array [n]... of the full grid -> that of the sub-grid, row-major: sub-tile b ni + a is tile (j0 + b) nx + (i0 + a)"""
    return np.stack([arr[(j0 + b) * nx + i0 + a] for b in range(nj) for a in range(ni)])


def container(w, h, tile_w, tile_h, payloads):
    """the `frit` file around the per-tile files: header, offset table, payloads (include/fri_emit.h)"""
    nx, ny = grid(w, h, tile_w, tile_h)
    assert len(payloads) == nx * ny
    at = HEADER + 8 * (len(payloads) + 1)
    offsets = [at]
    for p in payloads:
        at += len(p)
        offsets.append(at)
    return MAGIC + struct.pack("<7I", 1, h, w, tile_h, tile_w, ny, nx) + struct.pack(f"<{len(offsets)}Q", *offsets) + b"".join(payloads)


__all__ = ["ALPHA_CLEAN", "ALPHA_KEEP", "grid", "plane_index", "plane_order", "split_tiles_rgba", "merge_tiles_rgba", "sub_grid", "container"]
