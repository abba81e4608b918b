"""The size estimate of a tiled (`frit`) file, fri_hip_estimate_size_tiled_dev (include/fri_hip.h), restated on the host on top of tests/rate_model.py's
context_cost. The yardstick of tests/test_tiled_rate_host.py and tests/test_gpu_tiled_search.py; no GPU involved.

    file = 32 + 8 (n_tiles + 1) + sum over the tiles of payload(t)
    payload(t) = rate_model.estimate_image with one change: a context without symbols costs 14 + 2 bytes and 0 bits instead of making the image uncodable

The emitter codes the tiles with FRI_EMIT_EMPTY_OK: a context without symbols gets the model of max_freq_bits = 0, which the floor raises to 8, lists no value and
codes nothing - its 14 container bytes, and the 8 flush bytes of a rANS state that never moved, 2 more than the 6 per state the channel's flush constant of 60
assumes. Every payload is rounded up to whole bytes on its own; an out-of-alphabet symbol or a used symbol of frequency 0 still makes a tile, and with it the
file, uncodable: UINT64_MAX.
"""
import numpy as np

from tests.rate_model import CHANNEL_BYTES, CONTEXT_BYTES, FRAC_BITS, HEADER_BYTES, UNCODABLE, context_cost

FRIT_HEADER = 32  # "frit", version, H, W, tile_h, tile_w, ny, nx
EMPTY_CONTEXT_BYTES = CONTEXT_BYTES + 2  # the container's 14 and what an unmoved rANS state flushes beyond the 6 bytes the channel's 60 count for it
EMPTY_MAX_FREQ_BITS = 8  # max_freq_bits = 0 raised to the floor; the normalised Laplace shape sums to 2^8


def estimate_tile(hist, oob=None):
    """Estimated payload bytes of one tile from its histograms hist [C][10][1024] (and out-of-alphabet counts oob [C])."""
    hist = np.asarray(hist, np.uint32).reshape(-1, 10, 1024)
    if oob is not None and np.asarray(oob).any():
        return UNCODABLE
    total = HEADER_BYTES * 8 << FRAC_BITS
    for ch in range(hist.shape[0]):
        total += CHANNEL_BYTES * 8 << FRAC_BITS
        for b in range(10):
            if not hist[ch, b].any():
                total += EMPTY_CONTEXT_BYTES * 8 << FRAC_BITS
                continue
            r = context_cost(hist[ch, b], b)
            if r is None:
                return UNCODABLE
            cost, n_off, _ = r
            total += cost + ((CONTEXT_BYTES + 2 * n_off) * 8 << FRAC_BITS)
    return -(-total // (8 << FRAC_BITS))


def tile_models(hist):
    """uint32 [C][10][3] = (max_freq_bits, n_off, status) of every context of a tile, as d_models reports them in columns 0, 1 and 3: status 0 ok, 1 no symbols
    (coded all the same), 2 a used symbol of frequency 0."""
    import frave_amd.emit as emit

    hist = np.asarray(hist, np.uint32).reshape(-1, 10, 1024)
    out = np.zeros((hist.shape[0], 10, 3), np.uint32)
    for ch in range(hist.shape[0]):
        for b in range(10):
            if not hist[ch, b].any():
                out[ch, b] = (EMPTY_MAX_FREQ_BITS, 0, 1)
                continue
            f, _, off, bits = emit.finalize_context(hist[ch, b], b)
            out[ch, b] = (bits, len(off), 2 if (f[hist[ch, b] > 0] == 0).any() else 0)
    return out


def estimate_tiles(hist, oob=None):
    """estimate_tile over hist [n_tiles][C][10][1024] (oob [n_tiles][C]): uint64 [n_tiles]"""
    hist = np.asarray(hist, np.uint32)
    n = hist.shape[0]
    oob = np.zeros((n, 1), np.uint64) if oob is None else np.asarray(oob, np.uint64).reshape(n, -1)
    return np.array([estimate_tile(hist[t], oob[t]) for t in range(n)], np.uint64)


def file_bytes(tile_bytes):
    """32 + 8 (n + 1) + the sum of the payloads; UINT64_MAX if any tile is uncodable"""
    tile_bytes = [int(v) for v in np.asarray(tile_bytes, np.uint64).reshape(-1)]
    if any(v == UNCODABLE for v in tile_bytes):
        return UNCODABLE
    return FRIT_HEADER + 8 * (len(tile_bytes) + 1) + sum(tile_bytes)


def estimate_file(hist, oob=None):
    """(file bytes, tile bytes uint64 [n_tiles]) of the tiled file the histograms hist [n_tiles][C][10][1024] code to"""
    tiles = estimate_tiles(hist, oob)
    return file_bytes(tiles), tiles
