"""Several regions per call restated in numpy from the definitions of include/fri_emit.h ("Several regions"), independent of the library: the tile list, the
region table word for word, and the packed output as a literal per-pixel definition over the tile-list raster. No GPU involved."""
import numpy as np

from tests.tiled_region_ref import region_tiles

NOT_LISTED = 0xFFFFFFFF


def grid_of(w, h, tile_w, tile_h):
    return -(-w // tile_w), -(-h // tile_h)


def tile_list(w, h, tile_w, tile_h, regions):
    """the strictly ascending list of the file-grid tiles t = j nx + i at least one region touches, or None for no regions or a region that is refused"""
    if len(regions) < 1:
        return None
    nx, _ = grid_of(w, h, tile_w, tile_h)
    touched = set()
    for region in dict.fromkeys(tuple(r) for r in regions):  # (a repeated region touches nothing new)
        r = region_tiles(w, h, tile_w, tile_h, *region)
        if r is None:
            return None
        i0, j0, ni, nj = r
        touched |= {(j0 + b) * nx + i0 + a for b in range(nj) for a in range(ni)}
    return sorted(touched)


def region_table(w, h, c, tile_w, tile_h, regions):
    """the uint32 words of the region table, 8 (R + 1) + nx ny of them, or None where the definitions refuse (R = 0, R > 65535, a bad region, n_groups >= 2^31)"""
    tiles = tile_list(w, h, tile_w, tile_h, regions)
    if tiles is None or len(regions) > 65535:
        return None
    nx, ny = grid_of(w, h, tile_w, tile_h)
    words, off, first_group = [], 0, 0
    for x, y, rw, rh in regions:
        words += [x, y, rw, rh, off & 0xFFFFFFFF, off >> 32, first_group, 0]
        off += rw * rh * c
        first_group += -(-(rh * -(-(rw * c) // 16)) // 256)  # groups_r = ceil(h ceil(w C / 16) / 256)
    if first_group >= 2**31:
        return None
    words += [0, 0, 0, 0, off & 0xFFFFFFFF, off >> 32, first_group, 0]
    slot = {t: k for k, t in enumerate(tiles)}
    words += [slot.get(t, NOT_LISTED) for t in range(nx * ny)]
    return np.array(words, np.uint32)


def merge_regions(raster, tiles, w, h, tile_w, tile_h, regions):
    """raster [T][tile_h][tile_w][C] in the order of `tiles` -> the packed output: region r's raster [h_r][w_r][C] at byte off_r. Region pixel (ry, rx) is image
    pixel (y + ry, x + rx), which is pixel (y + ry - j tile_h, x + rx - i tile_w) of tile (j, i), slot(j nx + i) of the raster. A tile that is not listed has no
    slot: reading it is an error here."""
    raster = np.asarray(raster, np.uint8)
    nx, _ = grid_of(w, h, tile_w, tile_h)
    slot = {t: k for k, t in enumerate(tiles)}
    out = []
    for x, y, rw, rh in regions:
        part = np.empty((rh, rw, raster.shape[3]), np.uint8)
        for ry in range(rh):
            j = (y + ry) // tile_h
            for rx in range(rw):
                i = (x + rx) // tile_w
                part[ry, rx] = raster[slot[j * nx + i], y + ry - j * tile_h, x + rx - i * tile_w]
        out.append(part.reshape(-1))
    return np.concatenate(out)


def merge_regions_fast(raster, tiles, w, h, tile_w, tile_h, regions):
    """merge_regions without the pixel loop, for the large shapes: the listed tiles are placed into an image-sized canvas (their in-image pixels only), the regions
    are its crops. Checked against merge_regions on the small shapes by the tests that use it."""
    raster = np.asarray(raster, np.uint8)
    nx, _ = grid_of(w, h, tile_w, tile_h)
    canvas = np.zeros((h, w, raster.shape[3]), np.uint8)
    for k, t in enumerate(tiles):
        j, i = divmod(t, nx)
        y0, x0 = j * tile_h, i * tile_w
        hh, ww = min(tile_h, h - y0), min(tile_w, w - x0)
        canvas[y0:y0 + hh, x0:x0 + ww] = raster[k, :hh, :ww]
    return np.concatenate([canvas[y:y + rh, x:x + rw].reshape(-1) for x, y, rw, rh in regions])
