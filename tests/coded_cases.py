"""`frit` files for the coded-plane tests (tests/test_coded_parse_host.py, tests/test_gpu_decode.py): built on the CPU from oracle arrays the way
tests/test_tiled_host.py and tests/test_tiled420_host.py build theirs - per tile the oracle's coefficients, its prediction with the known-answer parameters, the
symbol streams, then the host emitter. Nothing here touches a GPU."""
import functools

import numpy as np

import frave_amd.emit as emit
from tests import rate_model
from tests.tiled420_ref import plane_order, split_tiles420
from tests.tiled_ref import mixed_image, split_tiles


def tile_streams(tile, tw, th, c, quality):
    """(streams [C][n], hist [C][10][1024], vp, wp [C][3][6]) of one tile from the oracle, quantised at `quality` (100: lossless)"""
    centers, coefs, bucket, pred, hist, oob, vp, wp = rate_model.oracle_arrays(np.ascontiguousarray(tile).reshape(-1), tw, th, c, quality)
    assert not oob.any()
    streams = []
    for ch in range(c):
        sym, bk = emit.channel_symbols(centers, coefs[ch], bucket[ch], pred[ch])
        streams.append((bk.astype(np.uint16) << 10) | sym)
    return np.stack(streams), hist, vp, wp


def file_of_image(img, tw, th, quality, **flags):
    """(frit bytes, value_params, width_params [n_tiles C][3][6]) of an image [H][W][C] in tw x th tiles. quality 100 writes a lossless file, anything else is
    recorded in it; flags: rct / ycbcr of emit.tiled_encode_from_streams (they only label the planes: the oracle codes what it is given)."""
    h, w, c = img.shape
    per = [tile_streams(t, tw, th, c, quality) for t in split_tiles(img, tw, th)]
    streams, hist, vp, wp = (np.stack([p[k] for p in per]) for k in range(4))
    frv = emit.tiled_encode_from_streams(w, h, tw, th, streams, hist, vp, wp, quality=0 if quality == 100 else quality, **flags)
    return frv, vp.reshape(-1, 3, 6), wp.reshape(-1, 3, 6)


@functools.lru_cache(maxsize=None)
def tiled_file(w, h, c, tw, th, quality, seed=3, **flags):
    return file_of_image(mixed_image(w, h, c, tw, seed), tw, th, quality, **flags)


@functools.lru_cache(maxsize=None)
def tiled420_file(w, h, tw, th, quality, seed=5):
    """(frit bytes, value_params, width_params [3 n][3][6] in plane order) of a tiled 4:2:0 file"""
    y_tiles, c_tiles = split_tiles420(mixed_image(w, h, 3, tw, seed), tw, th)
    per = []
    for t in range(len(y_tiles)):
        planes = []
        for plane in (y_tiles[t], c_tiles[t, 0], c_tiles[t, 1]):
            st, hist, vp, wp = tile_streams(plane, plane.shape[1], plane.shape[0], 1, quality)
            planes.append(dict(stream=st[0], hist=hist[0], vp=vp[0], wp=wp[0]))
        per.append(tuple(planes))
    planes = plane_order(per)
    streams = np.concatenate([p["stream"] for p in planes])
    hist, vp, wp = (np.stack([p[k] for p in planes]) for k in ("hist", "vp", "wp"))
    frv = emit.tiled_encode_from_streams420(w, h, tw, th, streams, per[0][0]["stream"].size, per[0][1]["stream"].size, hist, vp, wp, quality)
    return frv, vp, wp
