"""Preview of regions restated in numpy from the definitions of include/fri_hip.h ("Preview of regions"), independent of the library: the source rectangles, the
tile list, the preview-region table word for word, the packed offsets, and a region's pixels as the crop of tests/preview_ref.py's thumbnail. No GPU involved."""
import numpy as np

from tests import preview_ref
from tests.tiled_regions_ref import NOT_LISTED, grid_of, tile_list


def thumbnail_size(w, h, shift):
    s = 1 << shift
    return -(-w // s), -(-h // s)


def source_rectangles(w, h, shift, regions):
    """the image rectangle (xs(X), ys(Y), xs(X + w - 1) - xs(X) + 1, ys(Y + h - 1) - ys(Y) + 1) of every region (X, Y, w, h) of the thumbnail at `shift`, or None
    where the definitions refuse: shift > 4, no region, a region that is empty or leaves the thumbnail"""
    if not 0 <= shift <= 4 or len(regions) < 1:
        return None
    s = 1 << shift
    tw, th = thumbnail_size(w, h, shift)
    out = []
    for X, Y, rw, rh in regions:
        if rw < 1 or rh < 1 or X < 0 or Y < 0 or X + rw > tw or Y + rh > th:
            return None
        xs = lambda v: min(v * s + s // 2, w - 1)  # noqa: E731
        ys = lambda v: min(v * s + s // 2, h - 1)  # noqa: E731
        out.append((xs(X), ys(Y), xs(X + rw - 1) - xs(X) + 1, ys(Y + rh - 1) - ys(Y) + 1))
    return out


def preview_tile_list(w, h, tile_w, tile_h, shift, regions):
    """the "Several regions" tile list of the source rectangles, or None where the definitions refuse"""
    source = source_rectangles(w, h, shift, regions)
    return None if source is None else tile_list(w, h, tile_w, tile_h, source)


def sampled_tiles(w, h, tile_w, tile_h, shift, regions):
    """the tiles that hold at least one sample of at least one region: a subset of the tile list, and all of it unless a tile side is below 2^shift"""
    s = 1 << shift
    nx, _ = grid_of(w, h, tile_w, tile_h)
    seen = set()
    for X, Y, rw, rh in regions:
        xs = np.minimum((X + np.arange(rw)) * s + s // 2, w - 1) // tile_w
        ys = np.minimum((Y + np.arange(rh)) * s + s // 2, h - 1) // tile_h
        seen |= {int(j) * nx + int(i) for j in np.unique(ys) for i in np.unique(xs)}
    return sorted(seen)


def packed_offsets(c, regions):
    """[off_0, ..., off_R]: region r's raster [h_r][w_r][C] sits at byte off_r, off_R is the total"""
    offs = [0]
    for _, _, rw, rh in regions:
        offs.append(offs[-1] + rw * rh * c)
    return offs


def preview_region_table(w, h, c, tile_w, tile_h, shift, regions):
    """the uint32 words of the preview-region table, 8 (R + 1) + nx ny of them, or None where the definitions refuse (also R > 65535 and n_groups >= 2^31)"""
    tiles = preview_tile_list(w, h, tile_w, tile_h, shift, regions)
    if tiles is None or len(regions) > 65535:
        return None
    nx, ny = grid_of(w, h, tile_w, tile_h)
    offs = packed_offsets(c, regions)
    words, first_group = [], 0
    for (X, Y, rw, rh), off in zip(regions, offs):
        words += [X, Y, rw, rh, off & 0xFFFFFFFF, off >> 32, first_group, -(-rw // 16)]
        first_group += -(-rw // 16) * -(-rh // 16)  # groups_r: the 16 x 16 blocks of the region
    if first_group >= 2**31:
        return None
    words += [0, 0, 0, 0, offs[-1] & 0xFFFFFFFF, offs[-1] >> 32, first_group, 0]
    slot = {t: k for k, t in enumerate(tiles)}
    words += [slot.get(t, NOT_LISTED) for t in range(nx * ny)]
    return np.array(words, np.uint32)


def crops(thumbnail, regions):
    """region r = thumbnail[Y : Y + h, X : X + w]"""
    return [thumbnail[Y:Y + rh, X:X + rw] for X, Y, rw, rh in regions]


def region_pixels(image, shift, regions):
    """the regions' pixels from the preview image P_L [H][W][C]: preview_ref.subsample(P_L, m)[Y : Y + h, X : X + w]"""
    return crops(preview_ref.subsample(image, shift), regions)
