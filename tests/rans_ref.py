"""A Python restatement of what the device rANS coder (K11, include/fri_hip.h fri_hip_rans_encode_planes_dev) must write for one plane: the emitter's model rule with
FRI_EMIT_EMPTY_OK (oracle/emit_oracle.py's Context.finalize, imported, over the counts) and the one-loop rans64 coder of host/emit.cpp's encode_symbols in the
fixed-width arithmetic of csrc/rans_step.hpp - every intermediate masked to the width the header gives it, so that a model rans64 was not made for (a frequency of
1, the wrapping last slot) codes to the same words. Pure Python integers: test infrastructure only."""
import numpy as np

from oracle.emit_oracle import ALPHABET, CONTEXTS, Context, prev_power_two, trailing_zeros

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
L = 1 << 31
TOO_SMALL, BAD_MODEL, ZERO_FREQ, BAD_BUCKET = 1, 2, 4, 8  # FRI_HIP_RANS_* status bits


def make_symbol(start, freq, scale_bits):
    """rans_step.hpp make_symbol: (x_max, rcp_freq, freq, bias, cmpl_freq, rcp_shift)"""
    one = 1 << (scale_bits & 63)
    cmpl = (one - freq) & M32
    x_max = ((((1 << 31) >> (scale_bits & 63)) << 32) * freq) & M64
    if freq < 2:
        return x_max, M64, freq, (start + ((one - 1) & M32)) & M32, cmpl, 0
    shift = 0
    while freq > (1 << shift):
        shift += 1
    x0 = freq - 1
    x1 = 1 << (shift + 31)
    t1 = x1 // freq
    x0 = (x0 + ((x1 % freq) << 32)) & M64
    t0 = x0 // freq
    return x_max, (t0 + (t1 << 32)) & M64, freq, start, cmpl, shift - 1


def put_symbol(x, e):
    """rans_step.hpp put_symbol: (new state, emitted word or None)"""
    x_max, rcp, _, bias, cmpl, rshift = e
    word = None
    if x >= x_max:
        word = x & M32
        x >>= 32
    q = ((x * rcp) >> 64) >> (rshift & 63)
    return (x + bias + q * cmpl) & M64, word


def put_division(x, start, freq, scale_bits):
    """rans_step.hpp put_division, the plain rans64 step"""
    x_max = ((((1 << 31) >> (scale_bits & 63)) << 32) * freq) & M64
    word = None
    if x >= x_max:
        word = x & M32
        x >>= 32
    return (((x // freq) << (scale_bits & 63)) + x % freq + start) & M64, word


def contexts_from_hist(hist, empty_ok=True):
    """[Context or None] x 10 from counts [10][1024]: emit.cpp contexts_from_hist. None: the emitter refuses the context (it divides by zero)."""
    out = []
    for b in range(CONTEXTS):
        c = Context()
        c.freqs = [int(v) for v in hist[b]]
        total = sum(c.freqs) & M32
        c.max_freq_bits = 0 if empty_ok and not any(c.freqs) else trailing_zeros(prev_power_two(total))
        try:
            c.finalize(b)
        except ZeroDivisionError:
            c = None
        out.append(c)
    return out


def collapsed_slots(counts, bucket):
    """the third word of K6's and K11's model report for a context with counts: the used symbols whose slot is empty after the scaling to 2^max_freq_bits, before
    the stealing loop gives each of them one count (emit.cpp finalize, :174-176)"""
    counts = [int(v) for v in counts]
    bits = max(8, trailing_zeros(prev_power_two(sum(counts) & M32)))
    f = [1 if n and not lv else lv for n, lv in zip(counts, _laplace_slots(bucket, bits))]
    total, cum = sum(f), [0]
    for v in f:
        cum.append(cum[-1] + v)
    scaled = [((1 << (bits & 31)) * c) // total for c in cum[:ALPHABET]]
    return sum(1 for j in range(ALPHABET - 1) if f[j] and scaled[j + 1] == scaled[j])


def _laplace_slots(bucket, bits):
    """fill_with_laplace's (u32)(lap * 2^bits) per symbol, with the platform's expf like the emitter (oracle/emit_oracle.py, Context.finalize)"""
    import ctypes

    from oracle.emit_oracle import WIDTHS, _libm, f32, unpack_signed

    width, scale, out = f32(WIDTHS[bucket]), f32(1 << (bits & 31)), []
    for j in range(ALPHABET):
        e = f32(_libm.expf(ctypes.c_float(float(-abs(f32(unpack_signed(j))) / width))))
        v = f32(f32(e / f32(f32(2.0) * width)) * scale)
        out.append(min(int(v), M32) if v > 0 else 0)
    return out


class Coded:
    """What K11 reports for one plane. status: the bits without TOO_SMALL (which depends on the caller's stride); words: uint32, flush included, meaningful when
    status == 0; zero_at / bucket_at: 1 + the highest index with a zero model frequency / a bucket above 9, else 0; max_freq_bits [10], off [10] lists (a refused
    context: 0 and whatever the counts list)."""


def encode_plane(stream, hist, empty_ok=True):
    stream = np.asarray(stream, np.uint16)
    ctxs = contexts_from_hist(np.asarray(hist).reshape(CONTEXTS, ALPHABET), empty_ok)
    out = Coded()
    out.status = BAD_MODEL if any(c is None for c in ctxs) else 0
    out.max_freq_bits = [0 if c is None else c.max_freq_bits for c in ctxs]
    out.off = [None if c is None else list(c.off) for c in ctxs]
    table = {}
    x = [L] * CONTEXTS
    n = len(stream)
    emitted = [None] * n
    out.zero_at = out.bucket_at = 0
    for k in range(n - 1, -1, -1):
        v = int(stream[k])
        b, sym = v >> 10, v & 1023
        if b >= CONTEXTS:
            out.bucket_at = out.bucket_at or k + 1
            continue
        c = ctxs[b]
        if c is None or c.freqs[sym] == 0:  # a step the device skips
            out.zero_at = out.zero_at or k + 1
            continue
        e = table.get(v)
        if e is None:
            e = table[v] = make_symbol(c.cdf[sym], c.freqs[sym], c.max_freq_bits)
        x[b], emitted[k] = put_symbol(x[b], e)
    if out.zero_at:
        out.status |= ZERO_FREQ
    if out.bucket_at:
        out.status |= BAD_BUCKET
    flush = []
    for s in range(CONTEXTS - 1, -1, -1):
        flush += [x[s] & M32, x[s] >> 32]
    out.words = np.array(flush + [w for w in emitted if w is not None], np.uint32)
    return out


def split(stream):
    """a uint16 stream -> [(symbol, bucket)], the form oracle.emit_oracle.rans_encode takes"""
    return [(int(v) & 1023, int(v) >> 10) for v in stream]


def histogram(stream):
    """the counts [10][1024] of a stream whose buckets are all in range"""
    s = np.asarray(stream, np.uint16)
    return np.bincount(s.astype(np.int64), minlength=CONTEXTS * ALPHABET)[: CONTEXTS * ALPHABET].reshape(CONTEXTS, ALPHABET).astype(np.uint32)
