"""Plain references for K3 that involve no GPU code: the three dequantisers in numpy, the oracle's raster of dequantised coefficients (with the inverse
colour transform on top), the pixels the oracle's cells cover, and the [2 C + 1] distortion sums of fri_hip_measure_distortion_dev; for K4 the fit's
normal-equation sums over the oracle's neighbour values."""
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


def _fit_groups():
    """per heap node its layer group (level 8 -> 0, level 7 -> 1, levels 0-6 -> 2) and whether it is a row of the fit (heap nodes 0 and 1 are not)"""
    p = np.arange(512)
    level = np.floor(np.log2(np.maximum(p, 1))).astype(int)
    return np.where(level == 8, 0, np.where(level == 7, 1, 2)), p >= 2


def cpu_fit_sums(oracle, W, ch, value_params, nv=None):
    """the sums K4 accumulates for channel ch of the oracle Wavelet W: gram [3][7][7] and wtw [3][6][6] (exact int64), wtr [3][6] (float64); nv:
    W.neighbour_values(ch), if the caller has it"""
    co = W.coefficients()[ch].astype(np.int64)  # [F][512]
    some = co != oracle.NONE
    nv = (W.neighbour_values(ch) if nv is None else nv).astype(np.int64)  # [F][512][6]
    g, fit_row = _fit_groups()
    use = some & fit_row[None, :]
    gram = np.zeros((3, 7, 7), np.int64)
    wtw = np.zeros((3, 6, 6), np.int64)
    wtr = np.zeros((3, 6), np.float64)
    vp = np.asarray(value_params, np.float32)
    for grp in range(3):
        m = use & (g == grp)[None, :]
        v = nv[m]  # [n][6]
        val = co[m]
        u = np.concatenate([v, val[:, None]], axis=1)
        gram[grp] = u.T @ u
        # f32 prediction, left to right, one rounding per op (prediction.rs:199-204 / nalgebra gemv)
        vf = v.astype(np.float32)
        pf = vf[:, 0] * vp[grp, 0]
        for k in range(1, 6):
            pf = (pf + vf[:, k] * vp[grp, k]).astype(np.float32)
        res = np.abs(val.astype(np.float32) - pf).astype(np.float32)
        w = np.stack([np.ones(len(v), np.int64), np.abs(v[:, 0] - v[:, 3]), np.abs(v[:, 1] - v[:, 2]), np.abs(v[:, 4] - v[:, 5]), np.abs(v[:, 1] - v[:, 5]),
                      np.abs(v[:, 2] - v[:, 4])], axis=1)
        wtw[grp] = w.T @ w
        wtr[grp] = (w.astype(np.float64) * res.astype(np.float64)[:, None]).sum(0)
    return gram, wtw, wtr
