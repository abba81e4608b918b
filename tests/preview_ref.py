"""Preview decode restated in numpy from the definitions of include/fri_hip.h ("Preview decode"), on the oracle's inverse transform: the prefix count from the
valid mask, the planes of P_L (every Some node at or above 2^L set to 0), P_L itself for lossless files (per tile the oracle's inverse, the merge, the reversible
colour transform undone in numpy), and the subsample. No GPU involved, and nothing of the library's preview code."""
import numpy as np

from oracle import fri_oracle
from tests.tiled_ref import merge_tiles

NONE = -(2 ** 31)


def num_some_levels(valid_bits, levels):
    """the Some nodes with heap index < 2^levels: valid_bits bool [F][512]"""
    return int(np.count_nonzero(valid_bits[:, : 1 << levels]))


def prefix_planes(coefs, levels):
    """full planes [..., 512] with every Some node at or above 2^levels set to 0 (None stays None)"""
    out = np.array(coefs, np.int32, copy=True)
    tail = out[..., 1 << levels:]
    tail[tail != NONE] = 0
    return out


def expand(compact, valid_bits):
    """compact planes [..., F, 2^L] -> what K13 bounded by L leaves in full-stride planes [..., F, 512]: the initial 0 on every other Some node, None elsewhere"""
    full = np.where(valid_bits, 0, NONE).astype(np.int32)
    out = np.broadcast_to(full, compact.shape[:-2] + full.shape).copy()
    out[..., : compact.shape[-1]] = compact
    return out


def subsample(image, shift):
    """out(Y, X, c) = image(min(Y S + S / 2, H - 1), min(X S + S / 2, W - 1), c), S = 2^shift; [ceil(H / S)][ceil(W / S)][C]"""
    h, w = image.shape[:2]
    s = 1 << shift
    rows = np.minimum(np.arange(-(-h // s)) * s + s // 2, h - 1)
    cols = np.minimum(np.arange(-(-w // s)) * s + s // 2, w - 1)
    return image[rows][:, cols]


def lossless_preview_image(coefs, width, height, tile_w, tile_h, levels, rct=False):
    """P_L of a lossless tiled file from its full planes coefs [n_tiles][C][F][512]: per tile the oracle's inverse of the prefix planes (unquantised: the
    matrix is all ones), the merge, and for rct the planes (G, B - G + 128, R - G + 128) back to R, G, B mod 256; uint8 [H][W][C]"""
    n, c, f, _ = coefs.shape
    planes = prefix_planes(coefs, levels)
    tiles = np.empty((n, tile_h, tile_w, c), np.uint8)
    w = fri_oracle.Wavelet(np.zeros(tile_w * tile_h * c, np.uint8), tile_h, tile_w, c)
    assert w.num_cells == f
    for t in range(n):
        w.set_coefficients(planes[t])
        tiles[t] = w.to_raster().reshape(tile_h, tile_w, c)
    w.close()
    img = merge_tiles(tiles, width, height)
    if rct:
        y, cb, cr = (img[..., k].astype(np.int32) for k in range(3))
        img = np.stack([(cr + y - 128) & 255, y, (cb + y - 128) & 255], axis=-1).astype(np.uint8)
    return img
