"""Synthetic planes for the rANS coder tests (tests/test_rans_host.py on the host emitter, tests/test_gpu_rans.py on K11): name -> (streams uint16 [planes][n],
hist uint32 [planes][10][1024]), and the reference of a case from tests/rans_ref.py, computed once per process."""
import functools

import numpy as np

from tests import rans_ref

CHUNK, QUEUE, STITCH = 256, 512, 4096  # k11_rans.hip: kRansChunk, kRansQueue, kStitchThreads * kStitchPer
WIDTHS = [2.5, 4.5, 6.3, 8.5, 12.7, 16.0, 20.0, 24.0, 28.0, 36.0]
SHARE = np.array([47, 15, 10, 8, 6, 5, 4, 3, 1.5, 0.5]) / 100.0  # uneven contexts: the largest holds 47 % of a plane


def random_stream(n, seed, outliers=0.02, share=None):
    """n entries `bucket << 10 | symbol`: Laplace-like symbols of each context's own width, a few anywhere in 0..1022 (off-distribution values); share: the
    contexts' probabilities (SHARE unless given)"""
    rng = np.random.default_rng(seed)
    b = rng.choice(10, size=n, p=SHARE if share is None else share)
    k = np.rint(rng.laplace(0.0, np.array(WIDTHS)[b])).astype(np.int64)
    sym = np.where(k >= 0, 2 * k, -2 * k - 1)
    far = rng.random(n) < outliers
    sym = np.where(far, rng.integers(0, 1023, n), np.minimum(sym, 1022))
    return (b << 10 | sym).astype(np.uint16)


def _with_hist(streams):
    streams = np.ascontiguousarray(np.stack(streams), np.uint16)
    return streams, np.stack([rans_ref.histogram(s) for s in streams])


LENGTHS = [1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, QUEUE - 1, QUEUE, QUEUE + 1, STITCH - 1, STITCH, STITCH + 1, 65535, 65536, 65537, 70001]
BATCHES = [1, 3, 41]
SPECIAL = ["one_context", "one_each", "nine_empty", "freq_one", "off_heavy", "collapse", "symbol_1023"]


@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, arg = name.partition(":")
    if kind == "n":  # one plane of that length
        return _with_hist([random_stream(int(arg), 1000 + int(arg))])
    if kind == "batch":  # planes of 300 symbols, each its own content
        return _with_hist([random_stream(300, 7 * int(arg) + p, outliers=0.01 * (p % 5)) for p in range(int(arg))])
    rng = np.random.default_rng(5)
    if name == "one_context":  # all symbols in context 3
        s = random_stream(700, 11)
        return _with_hist([(s & 1023) | 3 << 10])
    if name == "one_each":  # ten symbols, one per context
        return _with_hist([np.array([b << 10 | (3 * b) for b in (4, 9, 0, 2, 7, 1, 8, 3, 6, 5)], np.uint16)])
    if name == "nine_empty":  # only context 6 is used: nine states flush 2^31 untouched
        return _with_hist([np.array([6 << 10 | v for v in (0, 1, 0, 2, 0, 0, 5, 1, 0, 3) * 13], np.uint16)])
    if name == "freq_one":  # context 0's only symbol has model frequency 1 (max_freq_bits at its floor of 8): the coder's `freq < 2` path
        # (an off-distribution only symbol always ends with 2 - the scale to 2^8 stretches the slot behind the whole shape - so: a tail symbol whose Laplace slot is 1)
        for sym in range(8, 64):
            c = rans_ref.Context()
            c.freqs[sym], c.max_freq_bits = 3, 1
            c.finalize(0)
            if c.freqs[sym] == 1:
                return _with_hist([np.array([0 << 10 | sym] + [2 << 10 | 1] * 20 + [0 << 10 | sym] * 2, np.uint16)])
    if name == "off_heavy":  # most symbols are off-distribution values: 150 of them per context, far out in three narrow contexts
        return _with_hist([(rng.choice([0, 1, 2], 6000) << 10 | (100 + 6 * rng.integers(0, 150, 6000))).astype(np.uint16)])
    if name == "collapse":  # a hundred off-distribution values push a small context's total past 2^8: the scaling empties used slots, which then steal
        far0, far1 = rng.choice(np.arange(100, 1000), 100, replace=False), rng.choice(np.arange(200, 900), 120, replace=False)
        a = np.concatenate([0 << 10 | rng.choice(far0, 200), (random_stream(200, 31) & 1023) | 5 << 10])
        return _with_hist([rng.permutation(a).astype(np.uint16), (1 << 10 | rng.choice(far1, 400)).astype(np.uint16)])
    if name == "symbol_1023":  # the last slot in use: its frequency wraps (emit.cpp, finalize) - the same outcome as the host, whatever it is
        s = random_stream(600, 23)
        s[::7] = (s[::7] & ~np.uint16(1023)) | 1023
        return _with_hist([s])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, empty_ok=True):
    """[rans_ref.Coded] per plane"""
    streams, hist = case(name)
    return [rans_ref.encode_plane(s, h, empty_ok) for s, h in zip(streams, hist)]
