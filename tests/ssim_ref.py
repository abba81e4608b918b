"""The exact SSIM of fri_hip_measure_ssim (include/fri_hip.h) restated in numpy, vectorised over the 4 x 4 block sums: 8 x 8 windows at stride 4 (the x264 /
libvpx window set), integer sums, n and d exact in int64, v = rint(float(n) / float(d) x 2^32) with IEEE round-to-nearest-even throughout. The reference
of every SSIM test."""
import numpy as np

C1, C2 = 26634, 239708  # 64^2 (0.01 x 255)^2 and 64^2 (0.03 x 255)^2, truncated
ONE = 1 << 32  # the value of a window of identical pixels


def windows(w, h):
    """(nx, ny): the window grid of a w x h raster"""
    return w // 4 - 1, h // 4 - 1


def window_sums(a, b, w, h, c):
    """(Sa, Sb, Saa, Sbb, Sab), each int64 [c][ny][nx]: a window is 2 x 2 of the 4 x 4 blocks"""
    bx, by = w // 4, h // 4
    A = np.asarray(a, np.uint8).reshape(h, w, c)[: 4 * by, : 4 * bx].astype(np.int64)
    B = np.asarray(b, np.uint8).reshape(h, w, c)[: 4 * by, : 4 * bx].astype(np.int64)
    out = []
    for x in (A, B, A * A, B * B, A * B):
        blk = x.reshape(by, 4, bx, 4, c).sum(axis=(1, 3))  # [by][bx][c]
        win = blk[:-1, :-1] + blk[1:, :-1] + blk[:-1, 1:] + blk[1:, 1:]
        out.append(np.moveaxis(win, 2, 0))
    return tuple(out)


def values_of_sums(sa, sb, saa, sbb, sab):
    """the window values v (int64) of integer window sums"""
    sa, sb, saa, sbb, sab = (np.asarray(x, np.int64) for x in (sa, sb, saa, sbb, sab))
    n = (2 * sa * sb + C1) * (2 * (64 * sab - sa * sb) + C2)
    d = (sa * sa + sb * sb + C1) * (64 * saa - sa * sa + 64 * sbb - sb * sb + C2)
    return np.rint(n.astype(np.float64) / d.astype(np.float64) * float(ONE)).astype(np.int64)


def window_values(a, b, w, h, c):
    """v, int64 [c][ny][nx]"""
    return values_of_sums(*window_sums(a, b, w, h, c))


def measure(a, b, w, h, c):
    """what fri_hip_measure_ssim returns: int64 [c + 1] = per channel the sum of v, then nx ny"""
    nx, ny = windows(w, h)
    v = window_values(a, b, w, h, c)
    return np.array([int(v[ch].sum()) for ch in range(c)] + [nx * ny], np.int64)


def ssim(a, b, w, h, c):
    """SSIM of the image: the integer sum over the channels first, then one division"""
    m = measure(a, b, w, h, c)
    return float(int(m[:c].sum())) / (float(c * int(m[c])) * float(ONE))
