"""The irreversible YCbCr transform of fri_hip_plan_set_colour_transform(FRI_HIP_COLOUR_YCBCR) and FRI_EMIT_YCBCR restated in numpy (include/fri_hip.h): the
JFIF / BT.601 full-range transform in libjpeg's 16-bit fixed point, 32-bit signed arithmetic, >> an arithmetic shift. The reference of every YCbCr test:
K1 codes the oracle's transform of ycc(pixels); K3 writes inverse_ycc(clamp(dequant(coefficients))) over the owned pixels and 0 elsewhere."""
import numpy as np

from tests.oracle_ref import DEQUANTISERS, oracle_owned

COLOUR_YCBCR = 3


def ycc(pixels):
    """forward, per pixel: (R, G, B) in 0..255 -> (Y, Cb, Cr) in 0..255, interleaved like the input"""
    p = np.asarray(pixels, np.uint8).reshape(-1, 3).astype(np.int32)
    r, g, b = p[:, 0], p[:, 1], p[:, 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return np.stack([y, cb, cr], axis=1).astype(np.uint8).reshape(np.shape(pixels))


def inverse_ycc(planes):
    """inverse of (Y, Cb, Cr) already clamped to 0..255 -> (R, G, B), each clamped to 0..255"""
    p = np.asarray(planes, np.uint8).reshape(-1, 3).astype(np.int32)
    y, db, dr = p[:, 0], p[:, 1] - 128, p[:, 2] - 128
    r = y + ((91881 * dr + 32768) >> 16)
    g = y + ((-22554 * db - 46802 * dr + 32768) >> 16)
    b = y + ((116130 * db + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=1), 0, 255).astype(np.uint8).reshape(np.shape(planes))


def oracle_coefficients_ycc(oracle, img, w, h, qm):
    """the oracle's quantised coefficients [3][F][512] of ycc(img)"""
    W = oracle.Wavelet(np.ascontiguousarray(ycc(img)).reshape(-1), h, w, 3)
    W.quantize(np.asarray(qm, np.int32))
    co = W.coefficients()
    W.close()
    return co


def oracle_raster_ycc(oracle, coefs, qm, mode, w, h, owned=None):
    """what K3 writes on a YCbCr plan: the oracle's (clamped) raster of the dequantised coefficients, turned into R, G, B over the owned pixels, 0 elsewhere"""
    W = oracle.Wavelet(np.zeros(w * h * 3, np.uint8), h, w, 3)
    W.set_coefficients(DEQUANTISERS[mode](coefs, qm))
    out = W.to_raster()
    W.close()
    own = oracle_owned(oracle, w, h, 3) if owned is None else owned
    return np.where(own, inverse_ycc(out.reshape(-1, 3)).reshape(-1), 0).astype(np.uint8)


def psnr(a, b):
    e = np.asarray(a, np.float64).reshape(-1) - np.asarray(b, np.float64).reshape(-1)
    mse = float((e * e).mean())
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)
