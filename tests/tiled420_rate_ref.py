"""The size estimate of a tiled 4:2:0 file, fri_hip_estimate_size_tiled420_dev (include/fri_hip.h), restated on the host: the arrays in plane order are put into
tile order with tests/tiled420_ref.plane_index and handed to tests/tiled_rate_ref.py - a 4:2:0 tile is a `frif` payload of three channels, so the formula per tile
is the tiled estimate's, unchanged. No new formula, no GPU involved."""
import numpy as np

from tests import tiled_rate_ref
from tests.tiled420_ref import plane_index


def tile_order(per_plane):
    """[3 n]... in plane order -> [n][3]..."""
    a = np.asarray(per_plane)
    n = a.shape[0] // 3
    assert a.shape[0] == 3 * n
    return np.stack([np.stack([a[plane_index(n, t, ch)] for ch in range(3)]) for t in range(n)])


def estimate_file(hist, oob=None):
    """(file bytes, tile bytes uint64 [n]) of the tiled 4:2:0 file the histograms hist [3 n][10][1024] (oob [3 n]) code to"""
    return tiled_rate_ref.estimate_file(tile_order(np.asarray(hist, np.uint32)), None if oob is None else tile_order(np.asarray(oob, np.uint64)))


def tile_models(hist):
    """uint32 [3 n][10][3] in plane order: tiled_rate_ref.tile_models of every tile"""
    hist = np.asarray(hist, np.uint32)
    n = hist.shape[0] // 3
    per_tile = [tiled_rate_ref.tile_models(t) for t in tile_order(hist)]
    out = np.zeros((3 * n, 10, 3), np.uint32)
    for t in range(n):
        for ch in range(3):
            out[plane_index(n, t, ch)] = per_tile[t][ch]
    return out
