"""RGBA coding restated in numpy (include/fri_hip.h, "RGBA: a lossless alpha plane"): the forward split of interleaved R, G, B, A pixels into the colour raster
and the alpha plane, in both modes, and the merge. The reference of every alpha test."""
import numpy as np

ALPHA_KEEP, ALPHA_CLEAN = 0, 1


def split_rgba(pixels, w, h, clean=ALPHA_KEEP):
    """(rgb uint8 [h][w][3], a uint8 [h][w]) of pixels [h][w][4]. KEEP: copied unchanged. CLEAN: a pixel with A == 0 gets R = G = B = 0."""
    assert clean in (ALPHA_KEEP, ALPHA_CLEAN)
    p = np.asarray(pixels, np.uint8).reshape(h, w, 4)
    rgb, a = p[:, :, :3].copy(), p[:, :, 3].copy()
    if clean == ALPHA_CLEAN:
        rgb[a == 0] = 0
    return rgb, a


def merge_rgba(rgb, a, w, h):
    """pixels uint8 [h * w * 4]: (R, G, B) from the colour raster, A from the alpha plane"""
    out = np.empty((h, w, 4), np.uint8)
    out[:, :, :3] = np.asarray(rgb, np.uint8).reshape(h, w, 3)
    out[:, :, 3] = np.asarray(a, np.uint8).reshape(h, w)
    return out.reshape(-1)


def cleaned(pixels, w, h):
    """what a lossless file made with CLEAN decodes to"""
    return merge_rgba(*split_rgba(pixels, w, h, ALPHA_CLEAN), w, h)


def alpha_plane(kind, w, h, seed=0):
    """alpha planes of the tests: "zeros", "opaque", "random" (about a quarter zeros, the rest any value), "runs" (runs of 0 and 255 and a ramp)"""
    rng = np.random.default_rng(1000 + seed)
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    if kind == "opaque":
        return np.full((h, w), 255, np.uint8)
    if kind == "random":
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        a[rng.random((h, w)) < 0.25] = 0
        return a
    assert kind == "runs"
    a = np.zeros((h, w), np.uint8)
    a[:, w // 4 : w // 2] = 255
    a[h // 3 : 2 * h // 3, : w // 4] = 255
    ramp = (np.arange(w - w // 2, dtype=np.int64) * 255 // max(w - w // 2 - 1, 1)).astype(np.uint8)
    a[:, w // 2 :] = ramp[None, :]
    return a


def rgba_image(rgb, a):
    """interleave a colour image [h][w][3] with an alpha plane [h][w]"""
    h, w = a.shape
    return merge_rgba(rgb, a, w, h).reshape(h, w, 4)
