"""Several regions of a tiled 4:2:0 file restated in numpy from the definitions of include/fri_emit.h ("Several regions of tiled 4:2:0 files"), independent of the
library: the 4:2:0 region table word for word, and the packed output as the crops of tests.tiled420_ref.merge_tiles420 on full-grid planes in which every unlisted
tile holds a poison value. No GPU involved."""
import numpy as np

from tests.tiled420_ref import merge_tiles420
from tests.tiled_regions_ref import NOT_LISTED, grid_of, tile_list

POISONS = (0x5A, 0xC3)  # two values an unlisted tile is filled with: what the regions show must not depend on which


def region_table420(w, h, tile_w, tile_h, regions):
    """the uint32 words of the 4:2:0 region table, 8 (R + 1) + nx ny of them, or None where the definitions refuse (R = 0, R > 65535, a bad region,
    n_groups >= 2^31, 3 W > 2^31 - 1). A lane owns 16 pixels: groups_r = ceil(h ceil(w / 16) / 256); off_r counts bytes, 3 w h a region."""
    tiles = tile_list(w, h, tile_w, tile_h, regions)
    if tiles is None or len(regions) > 65535 or 3 * w > 2**31 - 1:
        return None
    nx, ny = grid_of(w, h, tile_w, tile_h)
    words, off, first_group = [], 0, 0
    for x, y, rw, rh in regions:
        words += [x, y, rw, rh, off & 0xFFFFFFFF, off >> 32, first_group, 0]
        off += 3 * rw * rh
        first_group += -(-(rh * -(-rw // 16)) // 256)
    if first_group >= 2**31:
        return None
    words += [0, 0, 0, 0, off & 0xFFFFFFFF, off >> 32, first_group, 0]
    slot = {t: k for k, t in enumerate(tiles)}
    words += [slot.get(t, NOT_LISTED) for t in range(nx * ny)]
    return np.array(words, np.uint32)


def full_grid(planes, tiles, n_grid, poison):
    """the tile-list array [T]... -> the full grid's [n_grid]...: the listed tiles at their grid places, every other tile filled with `poison`"""
    planes = np.asarray(planes, np.uint8)
    out = np.full((n_grid,) + planes.shape[1:], poison, np.uint8)
    out[list(tiles)] = planes
    return out


def merge_regions420(y_tiles, c_tiles, tiles, w, h, tile_w, tile_h, regions):
    """y_tiles [T][tile_h][tile_w] and c_tiles [T][2][ch][cw] in the order of `tiles` -> the packed output: region r's raster [h_r][w_r][3] at byte off_r, the crop
    [y : y + h, x : x + w] of merge_tiles420 of the full grid's planes. Every pixel is upsampled within its own tile, so an unlisted tile never shows: the crops are
    made with two poison values and must agree."""
    nx, ny = grid_of(w, h, tile_w, tile_h)
    packed = []
    for poison in POISONS:
        image = merge_tiles420(full_grid(y_tiles, tiles, nx * ny, poison), full_grid(c_tiles, tiles, nx * ny, poison), w, h)
        packed.append(np.concatenate([np.ascontiguousarray(image[y:y + rh, x:x + rw]).reshape(-1) for x, y, rw, rh in regions]))
    assert np.array_equal(packed[0], packed[1]), "a region shows an unlisted tile"
    return packed[0]
