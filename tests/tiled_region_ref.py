"""Region decode restated in numpy from the formulas of include/fri_emit.h ("Region decode"), independent of the library: the tile range of a region and the
region raster as a literal per-pixel definition over the sub-grid's tile raster. No GPU involved."""
import numpy as np


def region_tiles(w, h, tile_w, tile_h, x, y, rw, rh):
    """(i0, j0, ni, nj) of the region x, y, rw, rh of a w x h image, or None for a zero size or a region that leaves the image"""
    if min(w, h, tile_w, tile_h, rw, rh) < 1 or x < 0 or y < 0 or x + rw > w or y + rh > h:
        return None
    i0, j0 = x // tile_w, y // tile_h
    return i0, j0, (x + rw - 1) // tile_w - i0 + 1, (y + rh - 1) // tile_h - j0 + 1


def sub_grid(tiles, nx, i0, j0, ni, nj):
    """the file's tiles [ny nx][...] -> the sub-grid's [nj ni][...]: sub-tile b ni + a is tile (j0 + b) nx + (i0 + a)"""
    return np.stack([tiles[(j0 + b) * nx + (i0 + a)] for b in range(nj) for a in range(ni)])


def merge_region(sub, tile_w, tile_h, i0, j0, ni, x, y, rw, rh):
    """sub [nj ni][tile_h][tile_w][C] -> the region raster [rh][rw][C], pixel by pixel: region pixel (ry, rx) is image pixel (y + ry, x + rx), which is pixel
    (y + ry - j tile_h, x + rx - i tile_w) of tile (j, i) = sub-tile (j - j0) ni + (i - i0)"""
    sub = np.asarray(sub, np.uint8)
    out = np.empty((rh, rw, sub.shape[3]), np.uint8)
    for ry in range(rh):
        j = (y + ry) // tile_h
        for rx in range(rw):
            i = (x + rx) // tile_w
            out[ry, rx] = sub[(j - j0) * ni + (i - i0), y + ry - j * tile_h, x + rx - i * tile_w]
    return out
