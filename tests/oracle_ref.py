"""Plain references for K3 that involve no GPU code: the three dequantisers in numpy, the oracle's raster of dequantised coefficients (with the inverse
colour transform on top), the pixels the oracle's cells cover, and the [2 C + 1] distortion sums of fri_hip_measure_distortion_dev."""
import numpy as np

from tests.test_rct_host import inverse_rct

NONE = -(2 ** 31)
REFERENCE, MULTIPLY, MIDPOINT = 0, 1, 2  # fri_hip_plan_set_dequantiser
# heap index -> quantiser layer, floor(log2(i + 1))
LAYER = np.floor(np.log2(np.arange(512) + 1)).astype(np.int64)


def _wrap32(v):
    return ((np.asarray(v, np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)


def midpoint(coefs, qm):
    """FRI_HIP_DEQUANT_MIDPOINT in numpy: v q + (q - 1) / 2 (v > 0), v q - (q - 1) / 2 (v < 0), 0, None stays None; wrapping int32"""
    v = np.asarray(coefs, np.int64)
    q = np.asarray(qm, np.int64)[LAYER]
    m, h = v * q, (q - 1) // 2
    out = _wrap32(np.where(v > 0, m + h, np.where(v < 0, m - h, 0)))
    return np.where(v == NONE, NONE, out).astype(np.int32)


def divide(coefs, qm):
    """the reference's quantization::decode: trunc(v / q), None stays None"""
    v = np.asarray(coefs, np.int64)
    q = np.asarray(qm, np.int64)[LAYER]
    return np.where(v == NONE, NONE, np.trunc(v / q)).astype(np.int32)


def multiply(coefs, qm):
    """FRI_HIP_DEQUANT_MULTIPLY: v q, wrapping int32, None stays None"""
    v = np.asarray(coefs, np.int64)
    q = np.asarray(qm, np.int64)[LAYER]
    return np.where(v == NONE, NONE, _wrap32(v * q)).astype(np.int32)


DEQUANTISERS = {REFERENCE: divide, MULTIPLY: multiply, MIDPOINT: midpoint}


def oracle_coefficients(oracle, img, w, h, c, qm, rct=False):
    """the oracle's quantised coefficients [C][F][512] of img (of rct(img) for a colour-transformed plan)"""
    from tests.test_rct_host import rct as forward_rct

    src = forward_rct(img) if rct else img
    W = oracle.Wavelet(np.ascontiguousarray(src).reshape(-1), h, w, c)
    W.quantize(np.asarray(qm, np.int32))
    co = W.coefficients()
    W.close()
    return co


def oracle_owned(oracle, w, h, c):
    """bool [h * w * c]: bytes of the pixels some retained cell covers - the oracle's raster of an all-255 image's transform is 255 there, 0 elsewhere"""
    W = oracle.Wavelet(np.full(w * h * c, 255, np.uint8), h, w, c)
    back = W.to_raster()
    W.close()
    px = (back.reshape(-1, c) == 255).all(axis=1)
    return np.repeat(px, c)


def oracle_raster(oracle, coefs, qm, mode, w, h, c, rct=False, owned=None):
    """what K3 writes: the oracle's raster of the dequantised coefficients; for an RCT plan the inverse colour transform of the covered pixels (the others
    stay 0)"""
    W = oracle.Wavelet(np.zeros(w * h * c, np.uint8), h, w, c)
    W.set_coefficients(DEQUANTISERS[mode](coefs, qm))
    out = W.to_raster()
    W.close()
    if rct:
        own = oracle_owned(oracle, w, h, c) if owned is None else owned
        inv = inverse_rct(out.reshape(-1, 3)).reshape(-1)
        out = np.where(own, inv, 0).astype(np.uint8)
    return out


def numpy_measure(recon, ref, owned, c):
    """fri_hip_measure_distortion_dev's [2 C + 1] sums: per channel the sum of squared and the largest absolute difference over the owned bytes, then the
    number of owned pixels"""
    e = np.abs(np.asarray(recon, np.int64).reshape(-1) - np.asarray(ref, np.int64).reshape(-1)).reshape(-1, c)
    own = np.asarray(owned, bool).reshape(-1, c)
    out = []
    for ch in range(c):
        ec = e[:, ch][own[:, ch]]
        out += [int((ec * ec).sum()), int(ec.max()) if ec.size else 0]
    return out + [int(own[:, 0].sum())]
