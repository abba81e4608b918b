"""The .frv size estimate of fri_hip_estimate_size_dev (include/fri_hip.h) restated on the host, on top of the product emitter's own ANS models
(frave_amd.emit.finalize_context). The yardstick of tests/test_rate_host.py and tests/test_gpu_rate.py; no GPU involved.

    bytes = ceil((8 * container + sum over channels and contexts of ideal_bits) / 8)
    container = 18 + sum over channels (218 + sum over contexts (14 + 2 n_off))
    bits of a context = sum over used symbols s of count[s] * (max_freq_bits - log2 freq[s] + bias[s])    (the model's final freq, cdf and max_freq_bits)
    bias[s] = (cdf[s] - (freq[s] - 1) (M - freq[s]) / (2 freq[s])) / (2^31 ln(2^32) ln 2),  M = 2^max_freq_bits

The bias is what rans64 (state in [2^31, 2^63), 32-bit renormalisation) codes a symbol above or below its ideal cost on average: x' = floor(x / f) M +
x mod f + start is x M / f + start - (x mod f)(M - f) / f, with the state log-uniform and x mod f uniform. It is negligible for small images and some
60 bytes of a 4096^2 plane.

18 = the 16-byte header + EOI; 218 per channel = PRD + 36 f32 (146), DAT + u64 length (10), EOC (2) and 60 bytes for the flush of the ten rANS
states; 14 + 2 n_off per context = EHD, u32 max_freq_bits, u64 n_off and the off-distribution list. A context without symbols, an out-of-alphabet
symbol or a used symbol whose final frequency is 0 make the image uncodable: UINT64_MAX.
"""
import math

import numpy as np

UNCODABLE = 2 ** 64 - 1
HEADER_BYTES = 18  # "frif", height, width, metadata word, EOI
CHANNEL_BYTES = 146 + 10 + 2 + 60  # PRD + 36 f32, DAT + u64 length, EOC, rANS flush estimate
CONTEXT_BYTES = 14  # EHD + u32 max_freq_bits + u64 n_off (+ 2 per off-distribution value)
FRAC_BITS = 16  # the device's fixed point: a symbol's cost is rounded to 2^-16 bit


CODER_BIAS = 1.0 / (2 ** 31 * 32 * math.log(2) ** 2)


def context_model(counts, bucket, with_cdf=False):
    """(freqs, n_off, max_freq_bits) - and the cdf with with_cdf - of the encoder's model of one context, or None where the emitter refuses it (no symbols)."""
    import frave_amd.emit as emit

    try:
        f, cdf, off, bits = emit.finalize_context(np.asarray(counts, np.uint32), bucket)
    except emit.EmitError:
        return None
    return (f, len(off), bits, cdf) if with_cdf else (f, len(off), bits)


def context_cost(counts, bucket):
    """(bits in units of 2^-16 bit, n_off, max_freq_bits) of one context, or None when the context is uncodable."""
    m = context_model(counts, bucket, with_cdf=True)
    if m is None:
        return None
    f, n_off, bits, cdf = m
    counts = np.asarray(counts, np.uint64)
    used = counts > 0
    if (f[used] == 0).any():
        return None
    big = float(2 ** (bits & 63))
    cost = 0
    for s in np.nonzero(used)[0]:
        fr = float(f[s])
        per = bits - math.log2(fr) + (float(cdf[s]) - (fr - 1.0) * (big - fr) / (2.0 * fr)) * CODER_BIAS
        cost += int(np.rint(float(counts[s]) * per * 2 ** FRAC_BITS))
    return max(cost, 0), n_off, bits


def estimate_image(hist, oob=None):
    """Estimated .frv bytes of one image from its histograms hist [C][10][1024] (and out-of-alphabet counts oob [C])."""
    hist = np.asarray(hist, np.uint32).reshape(-1, 10, 1024)
    if oob is not None and np.asarray(oob).any():
        return UNCODABLE
    total = HEADER_BYTES * 8 << FRAC_BITS
    for ch in range(hist.shape[0]):
        total += CHANNEL_BYTES * 8 << FRAC_BITS
        for b in range(10):
            r = context_cost(hist[ch, b], b)
            if r is None:
                return UNCODABLE
            cost, n_off, _ = r
            total += cost + ((CONTEXT_BYTES + 2 * n_off) * 8 << FRAC_BITS)
    return -(-total // (8 << FRAC_BITS))


def estimate(hist, oob=None):
    """estimate_image over a batch hist [N][C][10][1024] (oob [N][C]): uint64 [N]."""
    hist = np.asarray(hist, np.uint32)
    n = hist.shape[0]
    oob = np.zeros((n, 1), np.uint64) if oob is None else np.asarray(oob, np.uint64).reshape(n, -1)
    return np.array([estimate_image(hist[i], oob[i]) for i in range(n)], np.uint64)


def oracle_arrays(img, w, h, c, quality):
    """(centers, coefs, bucket, prediction, hist, oob, value_params, width_params) of the CPU oracle for an image quantised at `quality`, predicted with the
    known-answer parameters: what emit.encode_image takes."""
    import frave_amd as fa
    from oracle import fri_oracle
    from tests.common import KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS

    W = fri_oracle.Wavelet(img, h, w, c)
    W.quantize(fa.quality_matrix(quality))
    coefs = W.coefficients()
    bs, ps, hs, oo = [], [], [], []
    for ch in range(c):
        b, p, hist, oob = W.predict(ch, KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS)
        bs.append(b), ps.append(p), hs.append(hist), oo.append(oob)
    vp = np.stack([np.asarray(KAT_VALUE_PARAMS, np.float32).reshape(3, 6)] * c)
    wp = np.stack([np.asarray(KAT_WIDTH_PARAMS, np.float32).reshape(3, 6)] * c)
    return W.centers(), coefs, np.stack(bs), np.stack(ps), np.stack(hs), np.array(oo, np.uint64), vp, wp
