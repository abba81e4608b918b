"""Tiled 4:2:0 coding restated in numpy by composition of the existing restatements (include/fri_hip.h, "Tiled 4:2:0 coding"): tests.tiled_ref.split_tiles then
tests.chroma420_ref.split420 per tile; merge420 per tile then merge_tiles; the plane order; and the shape walk of fri_hip_tile_shape420 on host-only plans'
owned_pixels(). No GPU involved."""
import numpy as np

from tests.chroma420_ref import chroma_shape, merge420, split420
from tests.tiled_ref import grid, merge_tiles, split_tiles


def plane_index(n, t, channel):
    """plane(t, Y) = t, plane(t, Cb) = n + 2 t, plane(t, Cr) = n + 2 t + 1"""
    return t if channel == 0 else n + 2 * t + channel - 1


def plane_order(per_tile):
    """per_tile: n triples (Y, Cb, Cr) of anything -> the 3 n items in plane order"""
    n = len(per_tile)
    out = [None] * (3 * n)
    for t, planes in enumerate(per_tile):
        for c in range(3):
            out[plane_index(n, t, c)] = planes[c]
    return out


def split_tiles420(img, tile_w, tile_h):
    """image [H][W][3] -> (y_tiles [n][tile_h][tile_w], c_tiles [n][2][ch][cw]): every tile of the tile split, split as an image of its own"""
    tiles = split_tiles(img, tile_w, tile_h)
    cw, ch = chroma_shape(tile_w, tile_h)
    y = np.empty((len(tiles), tile_h, tile_w), np.uint8)
    c = np.empty((len(tiles), 2, ch, cw), np.uint8)
    for t, tile in enumerate(tiles):
        y[t], c[t, 0], c[t, 1] = split420(tile, tile_w, tile_h)
    return y, c


def merge_tiles420(y_tiles, c_tiles, w, h, fill=0):
    """the planes of all tiles -> image [H][W][3]: every tile merged as an image of its own (the filter clamps to the tile's planes), then the tile merge"""
    n, tile_h, tile_w = y_tiles.shape
    tiles = np.stack([merge420(y_tiles[t], c_tiles[t, 0], c_tiles[t, 1], tile_w, tile_h).reshape(tile_h, tile_w, 3) for t in range(n)])
    return merge_tiles(tiles, w, h, fill)


def sub_grid(arr, nx, i0, j0, ni, nj):
    """the per-tile array [n]... of the full grid -> that of the sub-grid, row-major: sub-tile b ni + a is tile (j0 + b) nx + (i0 + a)"""
    return np.stack([arr[(j0 + b) * nx + i0 + a] for b in range(nj) for a in range(ni)])


def owns_every_pixel(w, h):
    import frave_amd as fa

    plan = fa.Plan(None, w, h, 1)
    whole = plan.owned_pixels() == w * h
    plan.close()
    return whole


def walk420(w, h, target):
    """fri_hip_tile_shape420 restated: the walk of fri_hip_tile_shape with both lattices asked"""
    def first(size):
        parts = max(1, (2 * size + target) // (2 * target))  # round half up
        return -(-size // parts)
    w0, h0 = first(w), first(h)
    for s in range(65):
        for a in range(s + 1):
            tw, th = w0 + a, h0 + s - a
            if owns_every_pixel(tw, th) and owns_every_pixel(*chroma_shape(tw, th)):
                return tw, th
    return None


__all__ = ["grid", "plane_index", "plane_order", "split_tiles420", "merge_tiles420", "sub_grid", "owns_every_pixel", "walk420"]
