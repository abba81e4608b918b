"""4:2:0 chroma subsampling (include/fri_hip.h, "4:2:0 chroma subsampling") restated in numpy on top of tests/ycbcr_ref.py: the split of an R, G, B raster
into a luma plane and two half-resolution chroma planes, the (3, 1) / 4 triangle upsampling and the merge back to R, G, B. The reference of every 4:2:0 test;
no GPU code involved. All arithmetic is signed integer, >> an arithmetic shift."""
import numpy as np

from tests.ycbcr_ref import inverse_ycc, ycc


def chroma_shape(w, h):
    return (w + 1) // 2, (h + 1) // 2


def split420(pixels, w, h):
    """(Y [h][w], Cb [ch][cw], Cr [ch][cw]) uint8 of interleaved R, G, B: per pixel ycc, then each chroma sample is (the four of its 2 x 2 block + 2) >> 2
    with an odd last column or row replicated"""
    p = ycc(np.asarray(pixels, np.uint8).reshape(h, w, 3)).astype(np.int32)
    cw, ch = chroma_shape(w, h)
    x0, y0 = 2 * np.arange(cw), 2 * np.arange(ch)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    out = [p[:, :, 0].astype(np.uint8)]
    for c in (1, 2):
        q = p[:, :, c]
        s = q[np.ix_(y0, x0)] + q[np.ix_(y0, x1)] + q[np.ix_(y1, x0)] + q[np.ix_(y1, x1)]
        out.append(((s + 2) >> 2).astype(np.uint8))
    return tuple(out)


def upsample420(plane, w, h):
    """a chroma plane [ch][cw] at full resolution [h][w]: c = (9 p[j][i] + 3 p[j][i'] + 3 p[j'][i] + p[j'][i'] + 8) >> 4 with i = x >> 1, i' = i + 1 for odd x and
    i - 1 for even x, clamped to the plane; j, j' the same from y"""
    p = np.asarray(plane, np.uint8).astype(np.int32)
    ch, cw = p.shape
    x, y = np.arange(w), np.arange(h)
    i, j = x >> 1, y >> 1
    i2 = np.clip(np.where(x & 1, i + 1, i - 1), 0, cw - 1)
    j2 = np.clip(np.where(y & 1, j + 1, j - 1), 0, ch - 1)
    return (9 * p[np.ix_(j, i)] + 3 * p[np.ix_(j, i2)] + 3 * p[np.ix_(j2, i)] + p[np.ix_(j2, i2)] + 8) >> 4


def merge420(y, cb, cr, w, h):
    """R, G, B uint8 [h * w * 3] of the three planes: the chroma planes upsampled, then inverse_ycc per pixel"""
    planes = np.stack([np.asarray(y, np.uint8).reshape(h, w).astype(np.int32), upsample420(cb, w, h), upsample420(cr, w, h)], axis=2)
    return inverse_ycc(planes.astype(np.uint8).reshape(-1, 3)).reshape(-1)


def measure420(recon, ref):
    """fri_hip_measure_distortion420_dev's seven integers: per channel the sum of squared and the largest absolute difference, then the pixel count"""
    e = np.abs(np.asarray(recon, np.int64).reshape(-1, 3) - np.asarray(ref, np.int64).reshape(-1, 3))
    out = []
    for c in range(3):
        out += [int((e[:, c] ** 2).sum()), int(e[:, c].max())]
    return out + [e.shape[0]]


def planes_flat(y, cb, cr):
    """the three planes as one byte array, the layout of the device buffers: Y, then Cb, then Cr"""
    return np.concatenate([np.asarray(a, np.uint8).reshape(-1) for a in (y, cb, cr)])
