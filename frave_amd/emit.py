"""ctypes binding of frave_amd/libfri_emit.so: the host side of the encode path behind the kernels (symbol order, ANS model,
rANS streams, `frif` container; frave_amd/host/emit.hpp). No GPU involved."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libfri_emit.so")
_lib = None
RCT = 0x100  # FRI_EMIT_RCT: `channels = 3 | RCT` - the planes are Y, Cb, Cr of the reversible colour transform (include/fri_emit.h)
YCBCR = 0x400  # FRI_EMIT_YCBCR: `channels = 3 | YCBCR | QUALITY(q)` - the planes are Y, Cb, Cr of the irreversible JFIF transform (lossy files only)
S420 = 0x800  # FRI_EMIT_420: `channels = 3 | YCBCR | S420 | QUALITY(q)` in encode_image_from_streams - 4:2:0, Cb and Cr are streams of the half-resolution lattice
FRI_EMIT_ALPHA = ALPHA = 0x1000  # FRI_EMIT_ALPHA: `channels = 3 | ALPHA [| RCT | YCBCR | QUALITY(q)]` in encode_image_from_streams - a fourth, lossless channel: the alpha plane
FRI_EMIT_EMPTY_OK = EMPTY_OK = 0x2000  # FRI_EMIT_EMPTY_OK: in encode_image_from_streams - a context without symbols gets the model of max_freq_bits = 0 instead of the error


def QUALITY(q):
    """FRI_EMIT_QUALITY(q): q = 1..99, the planes were quantised with fri_hip_quality_matrix(q) (include/fri_emit.h)"""
    return int(q) << 16


def _arg(channels, rct, quality, ycbcr=False, s420=False, alpha=False):
    return channels | (RCT if rct else 0) | (YCBCR if ycbcr else 0) | (S420 if s420 else 0) | (ALPHA if alpha else 0) | QUALITY(quality or 0)


class EmitError(RuntimeError):
    pass


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):  # host-only C++ (g++): build on first use
            import subprocess

            subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "host"), _SO])
        L = C.CDLL(_SO)
        vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
        L.fri_emit_symbol_order.argtypes = [vp, u32, u32, vp]
        L.fri_emit_finalize_context.argtypes = [vp, u32, vp, vp, vp, vp, C.c_char_p, sz]
        L.fri_emit_channel_symbols.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp]
        L.fri_emit_encode_image.argtypes = [u32, u32, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, sz, vp, C.c_char_p, sz]
        L.fri_emit_check_image.argtypes = [vp, sz, u32, vp, u32, vp, vp, vp, C.c_char_p, sz]
        L.fri_emit_decode_image.argtypes = [vp, sz, vp, vp, sz, vp, C.c_char_p, sz]
        L.fri_emit_rans_selfcheck.argtypes = [C.c_uint64, C.c_uint64, C.c_char_p, sz]
        L.fri_emit_stream_order.argtypes = [vp, u32, vp, vp, vp]
        L.fri_emit_encode_image_from_streams.argtypes = [u32, u32, u32, vp, C.c_uint64, vp, vp, vp, vp, sz, vp, C.c_char_p, sz]
        L.fri_tiled_encode_from_streams.argtypes = [u32, u32, u32, u32, u32, vp, C.c_uint64, vp, vp, vp, u32, vp, sz, vp, C.c_char_p, sz]
        L.fri_tiled_encode_from_streams420.argtypes = [u32, u32, u32, u32, u32, vp, C.c_uint64, C.c_uint64, vp, vp, vp, u32, vp, sz, vp, C.c_char_p, sz]
        L.fri_tiled_encode_from_streams_rgba.argtypes = [u32, u32, u32, u32, u32, vp, C.c_uint64, vp, vp, vp, u32, vp, sz, vp, C.c_char_p, sz]
        L.fri_tiled_encode_from_coded.argtypes = [u32, u32, u32, u32, u32, vp, C.c_uint64, vp, vp, vp, vp, vp, u32, vp, sz, vp, C.c_char_p, sz]
        L.fri_tiled_encode_from_coded420.argtypes = [u32, u32, u32, u32, u32, vp, C.c_uint64, vp, vp, vp, vp, vp, u32, vp, sz, vp, C.c_char_p, sz]
        L.fri_coded_encode_image.argtypes = [u32, u32, u32, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, sz, vp, C.c_char_p, sz]
        L.fri_tiled_info.argtypes = [vp, sz, vp]
        L.fri_tiled_decode.argtypes = [vp, sz, u32, vp, vp, sz, C.c_char_p, sz]
        L.fri_tiled_decode_levels.argtypes = [vp, sz, u32, u32, vp, vp, sz, C.c_char_p, sz]
        L.fri_tiled_parse_coded.argtypes = [vp, sz, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, vp, vp, C.c_char_p, sz]
        L.fri_tiled_region_tiles.argtypes = [u32, u32, u32, u32, u32, u32, u32, u32, vp]
        L.fri_tiled_decode_region.argtypes = [vp, sz, u32, u32, u32, u32, u32, vp, vp, vp, sz, C.c_char_p, sz]
        L.fri_tiled_update_from_streams.argtypes = [vp, sz, u32, u32, u32, u32, u32, vp, C.c_uint64, vp, vp, vp, u32, vp, vp, sz, vp, C.c_char_p, sz]
        L.fri_tiled_regions_tiles.argtypes = [u32, u32, u32, u32, u32, vp, vp, sz, vp]
        L.fri_tiled_decode_tiles.argtypes = [vp, sz, u32, vp, sz, vp, vp, sz, C.c_char_p, sz]
        L.fri_tiled_parse_coded_tiles.argtypes = [vp, sz, vp, sz, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, vp, vp, C.c_char_p, sz]
        L.fri_tiled_preview_regions_tiles.argtypes = [u32, u32, u32, u32, u32, u32, vp, vp, sz, vp]
        L.fri_tiled_decode_tiles_levels.argtypes = [vp, sz, u32, vp, sz, u32, vp, vp, sz, C.c_char_p, sz]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def symbol_order(centers, level):
    """[(cell, heap index)] of `level` in stream order; centers = plan.centers() ([F][2] int32)."""
    c = np.ascontiguousarray(centers, np.int32)
    out = np.empty(len(c) << level, np.uint32)
    if load_library().fri_emit_symbol_order(_p(c), len(c), level, _p(out)) != 0:
        raise EmitError("fri_emit_symbol_order")
    return np.stack([out >> 9, out & 511], axis=1)


def finalize_context(counts, bucket):
    """(freqs, cdf, off_distribution_values, max_freq_bits) of the ANS model built from one context's measured counts."""
    f = np.ascontiguousarray(counts, np.uint32).copy()
    cdf = np.empty(1024, np.uint32)
    off = np.empty(1024, np.uint16)
    n_off, bits = C.c_uint32(0), C.c_uint32(0)
    err = C.create_string_buffer(256)
    rc = load_library().fri_emit_finalize_context(_p(f), bucket, _p(cdf), _p(off), C.addressof(n_off), C.addressof(bits), err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_emit_finalize_context: {rc}")
    return f, cdf, off[: n_off.value].copy(), bits.value


def channel_symbols(centers, coefs, bucket, prediction):
    c = np.ascontiguousarray(centers, np.int32)
    co, b, p = np.ascontiguousarray(coefs, np.int32), np.ascontiguousarray(bucket, np.uint8), np.ascontiguousarray(prediction, np.int32)
    sym = np.empty(len(c) * 512, np.uint16)
    bk = np.empty(len(c) * 512, np.uint8)
    n = C.c_uint64(0)
    if load_library().fri_emit_channel_symbols(_p(c), len(c), _p(co), _p(b), _p(p), _p(sym), _p(bk), C.addressof(n)) != 0:
        raise EmitError("fri_emit_channel_symbols")
    return sym[: n.value].copy(), bk[: n.value].copy()


def encode_image(width, height, centers, coefs, bucket, prediction, hist, value_params, width_params, rct=False, quality=0, ycbcr=False):
    """.frv bytes. coefs/bucket/prediction [C][F][512], hist [C][10][1024], params [C][3][6]. rct: the three planes are Y, Cb, Cr of the reversible colour
    transform (Plan.set_colour_transform): the file says YCbCr and carries the flag. quality: 0 (lossless) or 1..99, the quality whose matrix
    (frave_amd.quality_matrix) quantised the planes: the file records it. ycbcr: the planes are Y, Cb, Cr of the irreversible JFIF transform
    (COLOUR_YCBCR); needs C = 3 and a quality, not with rct."""
    c = np.ascontiguousarray(centers, np.int32)
    co, b, p = np.ascontiguousarray(coefs, np.int32), np.ascontiguousarray(bucket, np.uint8), np.ascontiguousarray(prediction, np.int32)
    h = np.ascontiguousarray(hist, np.uint32)
    vp, wp = np.ascontiguousarray(value_params, np.float32), np.ascontiguousarray(width_params, np.float32)
    channels = co.size // (len(c) * 512)
    assert co.size == channels * len(c) * 512 and b.size == co.size and p.size == co.size and h.size == channels * 10240 and vp.size == channels * 18 and wp.size == channels * 18
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    L = load_library()
    # one call in the common case: a symbol costs at most max_freq_bits (< 32) bits, so 4 bytes per coefficient + the container
    # overhead always suffice; the library reports the needed size (-3) if they should not
    out = np.empty(co.size * 4 + channels * (10 * 2070 + 256) + 64, np.uint8)
    arg = _arg(channels, rct, quality, ycbcr)
    rc = L.fri_emit_encode_image(width, height, arg, _p(c), len(c), _p(co), _p(b), _p(p), _p(h), _p(vp), _p(wp), _p(out), out.size, C.addressof(n), err, 256)
    if rc == -3:
        out = np.empty(n.value, np.uint8)
        rc = L.fri_emit_encode_image(width, height, arg, _p(c), len(c), _p(co), _p(b), _p(p), _p(h), _p(vp), _p(wp), _p(out), out.size, C.addressof(n), err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_emit_encode_image: {rc}")
    out = out[: n.value]
    return out.tobytes()


def stream_order(centers, valid_mask):
    """uint32 [num_some]: cell << 9 | heap index of every symbol of a channel, in stream order (None nodes taken out)."""
    c = np.ascontiguousarray(centers, np.int32)
    m = np.ascontiguousarray(valid_mask, np.uint32)
    out = np.empty(len(c) * 512, np.uint32)
    n = C.c_uint64(0)
    if load_library().fri_emit_stream_order(_p(c), len(c), _p(m), _p(out), C.addressof(n)) != 0:
        raise EmitError("fri_emit_stream_order")
    return out[: n.value].copy()


def encode_image_from_streams(width, height, streams, hist, value_params, width_params, rct=False, quality=0, ycbcr=False, n_luma=None, alpha=False, empty_ok=False):
    """.frv bytes from the device's symbol streams: streams uint16 [C][n_symbols] (bucket << 10 | symbol), hist [C][10][1024], params [C][3][6].
    rct, quality, ycbcr: see encode_image. n_luma: a 4:2:0 file (implies the flag; needs ycbcr and a quality) - streams is the concatenation Y [n_luma],
    Cb [n_c], Cr [n_c] that Plan420.encode_image420_symbols returns; the emitter works n_c out from the geometry. alpha: streams [4][n_symbols], hist
    [4][10][1024], params [4][3][6] - the three colour channels, which rct, quality and ycbcr describe, then the lossless alpha plane
    (PlanRGBA.encode_image_rgba_symbols returns them so); not with n_luma. empty_ok: FRI_EMIT_EMPTY_OK - a context without symbols is coded instead of refused."""
    st = np.ascontiguousarray(streams, np.uint16)
    h = np.ascontiguousarray(hist, np.uint32)
    channels = h.size // 10240
    planes = channels
    if alpha:  # the flag rides on the three colour channels; a wrong count reaches the library as it is and is refused there
        channels -= 1
    n_symbols = st.size // planes if n_luma is None else int(n_luma)
    vp, wp = np.ascontiguousarray(value_params, np.float32), np.ascontiguousarray(width_params, np.float32)
    assert (n_luma is not None or st.size == planes * n_symbols) and vp.size == planes * 18 and wp.size == planes * 18
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    out = np.empty(st.size * 4 + planes * (10 * 2070 + 256) + 64, np.uint8)
    rc = load_library().fri_emit_encode_image_from_streams(width, height, _arg(channels, rct, quality, ycbcr, n_luma is not None, alpha) | (EMPTY_OK if empty_ok else 0), _p(st), n_symbols, _p(h), _p(vp), _p(wp), _p(out), out.size, C.addressof(n), err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_emit_encode_image_from_streams: {rc}")
    return out[: n.value].tobytes()


def check_image(frv, centers, coefs, bucket, prediction, rct=False, quality=0, ycbcr=False):
    """Entropy-layer self-check: parse, rebuild the models from the container, decode every symbol, compare. Raises on mismatch (the colour transform
    flags and the quality included)."""
    c = np.ascontiguousarray(centers, np.int32)
    co, b, p = np.ascontiguousarray(coefs, np.int32), np.ascontiguousarray(bucket, np.uint8), np.ascontiguousarray(prediction, np.int32)
    data = np.frombuffer(frv, np.uint8)
    channels = co.size // (len(c) * 512)
    err = C.create_string_buffer(256)
    rc = load_library().fri_emit_check_image(_p(data), data.size, _arg(channels, rct, quality, ycbcr), _p(c), len(c), _p(co), _p(b), _p(p), err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_emit_check_image: {rc}")


def rans_selfcheck(n_symbols, seed=1):
    """The context-parallel rANS coder against the plain one-loop coder on n_symbols pseudo-random symbols. Raises on a difference."""
    err = C.create_string_buffer(256)
    rc = load_library().fri_emit_rans_selfcheck(n_symbols, seed, err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_emit_rans_selfcheck: {rc}")


class DecodedImage(tuple):
    """(width, height, channels, centers, coefs), and .rct: True if the planes are Y, Cb, Cr of the reversible colour transform; .quality: 0 for a
    lossless file, else the quality 1..99 whose matrix quantised the planes (decode with the midpoint dequantiser); .ycbcr: True if the planes are Y, Cb, Cr
    of the irreversible JFIF transform (decode with COLOUR_YCBCR); .s420: True for a 4:2:0 file - coefs is then the tuple (Y [F_y][512], Cb [F_c][512],
    Cr [F_c][512]), centers the luma lattice's (decode with Plan420.decode_image420 of the three concatenated); .alpha: True for a file with an alpha
    plane - channels stays 3 and coefs is [4][F][512], the colour planes then alpha (decode with PlanRGBA.decode_image_rgba)."""

    rct = False
    quality = 0
    ycbcr = False
    s420 = False
    alpha = False


def decode_image(frv):
    """A .frv back to coefficient planes (serialize::decode + entropy_coding::decode of the reference, host only).
    Returns (width, height, channels, centers [F][2] int32, coefs [channels][F][512] int32 with None = INT32_MIN); its .rct is the file's colour transform flag."""
    data = np.frombuffer(frv, np.uint8)
    info = np.zeros(4, np.uint32)
    err = C.create_string_buffer(256)
    L = load_library()
    rc = L.fri_emit_decode_image(_p(data), data.size, _p(info), None, 0, None, err, 256)
    if rc != -3:
        raise EmitError(err.value.decode() or f"fri_emit_decode_image: {rc}")
    w, h, c, f = (int(x) for x in info)
    rct = bool(c & RCT)
    ycbcr = bool(c & YCBCR)
    quality = (c >> 16) & 0x7F
    s420 = bool(c & S420)
    alpha = bool(c & ALPHA)
    c &= 0xFF
    if s420:  # F_c: the cells of the half-resolution lattice, from a host-only subsampled plan (no GPU involved)
        from .api import Plan420

        sub = Plan420(None, w, h)
        fc = sub.chroma.num_cells
        sub.close()
        coefs = np.empty((f + 2 * fc, 512), np.int32)
    else:
        coefs = np.empty((c + 1 if alpha else c, f, 512), np.int32)
    centers = np.empty((f, 2), np.int32)
    rc = L.fri_emit_decode_image(_p(data), data.size, _p(info), _p(coefs), coefs.size, _p(centers), err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_emit_decode_image: {rc}")
    out = DecodedImage((w, h, c, centers, (coefs[:f], coefs[f:f + fc], coefs[f + fc:]) if s420 else coefs))
    out.rct = rct
    out.quality = quality
    out.ycbcr = ycbcr
    out.s420 = s420
    out.alpha = alpha
    return out


# ---- the tile container `frit` (include/fri_emit.h) ---------------------------------------------------------------------------
class TiledInfo(tuple):
    """(width, height, tile_w, tile_h, nx, ny, channels, n_cells) of a tiled file, and .rct / .quality / .ycbcr / .s420 as DecodedImage has them: what every tile
    is. A tiled 4:2:0 file (.s420): n_cells is F_y, the cells of the tile's luma lattice. A tiled RGBA file (.alpha): channels stays 3, every tile has a fourth
    plane on the same lattice."""

    rct = False
    quality = 0
    ycbcr = False
    s420 = False
    alpha = False


def _tiled_info(info):
    w, h, tw, th, nx, ny, c, f = (int(x) for x in info)
    out = TiledInfo((w, h, tw, th, nx, ny, c & 0xFF, f))
    out.rct, out.ycbcr, out.quality, out.s420 = bool(c & RCT), bool(c & YCBCR), (c >> 16) & 0x7F, bool(c & S420)
    out.alpha = bool(c & ALPHA)
    return out


def _chroma_cells(ti):
    """F_c of a tiled 4:2:0 file: the cells of the lattice of a tile's chroma planes, from a host-only plan (no GPU involved)"""
    from .api import Plan

    sub = Plan(None, (ti[2] + 1) // 2, (ti[3] + 1) // 2, 1)
    fc = sub.num_cells
    sub.close()
    return fc


def _tiled_coefs(ti, n):
    """the array fri_tiled_decode[_region] fills for n tiles: [n][C][F][512], or flat in plane order - n (F_y + 2 F_c) x 512 - for a tiled 4:2:0 file, or
    the planes in plane order, [4 n][F][512] = [n][3][F][512] then [n][F][512], for a tiled RGBA file"""
    if ti.s420:
        return np.empty(n * (ti[7] + 2 * _chroma_cells(ti)) * 512, np.int32)
    if ti.alpha:
        return np.empty((4 * n, ti[7], 512), np.int32)
    return np.empty((n, ti[6], ti[7], 512), np.int32)


def tiled_encode_from_streams420(width, height, tile_w, tile_h, streams, n_luma, n_chroma, hist, value_params, width_params, quality, threads=0):
    """fri_tiled_encode_from_streams420: the `frit` bytes of a tiled 4:2:0 file from what PlanTiled420.encode_image_tiled420_symbols returns, all in plane order
    (plane(t, Y) = t, plane(t, Cb) = n + 2 t, plane(t, Cr) = n + 2 t + 1): streams uint16 [n][n_luma] then [n][2][n_chroma] (flat), hist [3 n][10][1024], params
    [3 n][3][6]; quality 1..99. The bytes do not depend on `threads`."""
    st = np.ascontiguousarray(streams, np.uint16).reshape(-1)
    h = np.ascontiguousarray(hist, np.uint32)
    vp, wp = np.ascontiguousarray(value_params, np.float32), np.ascontiguousarray(width_params, np.float32)
    n_tiles = -(-width // tile_w) * -(-height // tile_h)
    planes = 3 * n_tiles
    assert h.size == planes * 10240 and vp.size == planes * 18 and wp.size == planes * 18 and st.size == n_tiles * (n_luma + 2 * n_chroma)
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    out = np.empty(st.size * 4 + planes * (10 * 2070 + 256) + n_tiles * 72 + 64, np.uint8)
    args = (width, height, tile_w, tile_h, _arg(3, False, quality, True, True), _p(st), n_luma, n_chroma, _p(h), _p(vp), _p(wp), threads)
    L = load_library()
    rc = L.fri_tiled_encode_from_streams420(*args, _p(out), out.size, C.addressof(n), err, 256)
    if rc == -3:
        out = np.empty(n.value, np.uint8)
        rc = L.fri_tiled_encode_from_streams420(*args, _p(out), out.size, C.addressof(n), err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_tiled_encode_from_streams420: {rc}")
    return out[: n.value].tobytes()


def tiled_encode_from_streams_rgba(width, height, tile_w, tile_h, streams, hist, value_params, width_params, rct=False, quality=0, ycbcr=False, threads=0, flags=None):
    """fri_tiled_encode_from_streams_rgba: the `frit` bytes of a tiled RGBA file from what PlanTiledRgba.encode_image_tiled_rgba_symbols returns, all in plane
    order (plane(t, c) = 3 t + c, plane(t, A) = 3 n + t): streams uint16 [4 n][n_symbols], hist [4 n][10][1024], params [4 n][3][6]. rct / quality / ycbcr say
    how the colour was coded; the alpha planes are lossless. `flags`: the whole `channels` word in their place (for the refusals). The bytes do not depend on
    `threads`."""
    st = np.ascontiguousarray(streams, np.uint16)
    h = np.ascontiguousarray(hist, np.uint32)
    vp, wp = np.ascontiguousarray(value_params, np.float32), np.ascontiguousarray(width_params, np.float32)
    n_tiles = -(-width // tile_w) * -(-height // tile_h)
    planes = 4 * n_tiles
    assert h.size == planes * 10240 and vp.size == planes * 18 and wp.size == planes * 18 and st.size % planes == 0
    n_symbols = st.size // planes
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    out = np.empty(st.size * 4 + planes * (10 * 2070 + 256) + n_tiles * 72 + 64, np.uint8)
    word = _arg(3, rct, quality, ycbcr, False, True) if flags is None else int(flags)
    args = (width, height, tile_w, tile_h, word, _p(st), n_symbols, _p(h), _p(vp), _p(wp), threads)
    L = load_library()
    rc = L.fri_tiled_encode_from_streams_rgba(*args, _p(out), out.size, C.addressof(n), err, 256)
    if rc == -3:
        out = np.empty(n.value, np.uint8)
        rc = L.fri_tiled_encode_from_streams_rgba(*args, _p(out), out.size, C.addressof(n), err, 256)
    if rc != 0:
        e = EmitError(err.value.decode() or f"fri_tiled_encode_from_streams_rgba: {rc}")
        e.code = rc
        raise e
    return out[: n.value].tobytes()


def tiled_encode_from_streams(width, height, tile_w, tile_h, streams, hist, value_params, width_params, rct=False, quality=0, ycbcr=False, threads=0):
    """fri_tiled_encode_from_streams: the `frit` bytes from what PlanTiled.encode_image_tiled_symbols returns - streams uint16 [n_tiles][C][n_symbols], hist
    [n_tiles][C][10][1024], params [n_tiles][C][3][6]. Tiles are coded on `threads` workers (0: the hardware concurrency, capped at 16); the bytes do not depend
    on it. rct, quality, ycbcr: see encode_image - they hold for every tile."""
    st = np.ascontiguousarray(streams, np.uint16)
    h = np.ascontiguousarray(hist, np.uint32)
    vp, wp = np.ascontiguousarray(value_params, np.float32), np.ascontiguousarray(width_params, np.float32)
    n_tiles = -(-width // tile_w) * -(-height // tile_h)
    planes = h.size // 10240
    channels = planes // n_tiles
    assert planes == n_tiles * channels and h.size == planes * 10240 and vp.size == planes * 18 and wp.size == planes * 18 and st.size % planes == 0
    n_symbols = st.size // planes
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    out = np.empty(st.size * 4 + planes * (10 * 2070 + 256) + n_tiles * 72 + 64, np.uint8)
    args = (width, height, tile_w, tile_h, _arg(channels, rct, quality, ycbcr), _p(st), n_symbols, _p(h), _p(vp), _p(wp), threads)
    L = load_library()
    rc = L.fri_tiled_encode_from_streams(*args, _p(out), out.size, C.addressof(n), err, 256)
    if rc == -3:
        out = np.empty(n.value, np.uint8)
        rc = L.fri_tiled_encode_from_streams(*args, _p(out), out.size, C.addressof(n), err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_tiled_encode_from_streams: {rc}")
    return out[: n.value].tobytes()


def _coded(words, n_words, models, off_values, value_params, width_params):
    w = np.ascontiguousarray(words, np.uint32)
    nw, m, off = np.ascontiguousarray(n_words, np.uint32), np.ascontiguousarray(models, np.uint32), np.ascontiguousarray(off_values, np.uint16)
    vp, wp = np.ascontiguousarray(value_params, np.float32), np.ascontiguousarray(width_params, np.float32)
    planes = nw.size
    assert planes and w.size % planes == 0 and m.size == planes * 40 and off.size == planes * 10240 and vp.size == planes * 18 and wp.size == planes * 18
    return w, w.size // planes, nw, m, off, vp, wp, planes


def tiled_encode_from_coded(width, height, tile_w, tile_h, words, n_words, models, off_values, value_params, width_params, rct=False, quality=0, ycbcr=False, threads=0):
    """fri_tiled_encode_from_coded: the `frit` bytes from what PlanTiled.encode_image_tiled_coded returns - words uint32 [n_tiles C][word_stride], n_words
    [n_tiles C], models [n_tiles C][10][4], off_values uint16 [n_tiles C][10][1024], params [n_tiles][C][3][6]. Nothing is coded here; the file is
    tiled_encode_from_streams's, byte for byte."""
    w, stride, nw, m, off, vp, wp, planes = _coded(words, n_words, models, off_values, value_params, width_params)
    n_tiles = -(-width // tile_w) * -(-height // tile_h)
    channels = planes // n_tiles
    assert planes == n_tiles * channels
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    out = np.empty(int(nw.sum()) * 4 + planes * (10 * 2070 + 256) + n_tiles * 72 + 64, np.uint8)
    rc = load_library().fri_tiled_encode_from_coded(width, height, tile_w, tile_h, _arg(channels, rct, quality, ycbcr), _p(w), stride, _p(nw), _p(m), _p(off), _p(vp), _p(wp),
                                                    threads, _p(out), out.size, C.addressof(n), err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_tiled_encode_from_coded: {rc}")
    return out[: n.value].tobytes()


def tiled_encode_from_coded420(width, height, tile_w, tile_h, words, n_words, models, off_values, value_params, width_params, quality, threads=0):
    """fri_tiled_encode_from_coded420: the `frit` bytes of a tiled 4:2:0 file from what PlanTiled420.encode_image_tiled420_coded returns, all in plane order -
    words uint32 [3 n][word_stride], n_words [3 n], models [3 n][10][4], off_values uint16 [3 n][10][1024], params [3 n][3][6]; quality 1..99. Nothing is coded
    here; the file is tiled_encode_from_streams420's, byte for byte, and does not depend on `threads`."""
    w, stride, nw, m, off, vp, wp, planes = _coded(words, n_words, models, off_values, value_params, width_params)
    n_tiles = -(-width // tile_w) * -(-height // tile_h)
    assert planes == 3 * n_tiles
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    out = np.empty(int(nw.sum()) * 4 + planes * (10 * 2070 + 256) + n_tiles * 72 + 64, np.uint8)
    args = (width, height, tile_w, tile_h, _arg(3, False, quality, True, True), _p(w), stride, _p(nw), _p(m), _p(off), _p(vp), _p(wp), threads)
    L = load_library()
    rc = L.fri_tiled_encode_from_coded420(*args, _p(out), out.size, C.addressof(n), err, 256)
    if rc == -3:
        out = np.empty(n.value, np.uint8)
        rc = L.fri_tiled_encode_from_coded420(*args, _p(out), out.size, C.addressof(n), err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_tiled_encode_from_coded420: {rc}")
    return out[: n.value].tobytes()


def coded_encode_image(width, height, words, n_words, models, off_values, value_params, width_params, rct=False, quality=0, ycbcr=False):
    """fri_coded_encode_image: the `frif` bytes of an ordinary image of 1 or 3 channels from its coded planes (the layouts of tiled_encode_from_coded with C planes):
    encode_image_from_streams's file, byte for byte."""
    w, stride, nw, m, off, vp, wp, planes = _coded(words, n_words, models, off_values, value_params, width_params)
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    out = np.empty(int(nw.sum()) * 4 + planes * (10 * 2070 + 256) + 64, np.uint8)
    rc = load_library().fri_coded_encode_image(width, height, _arg(planes, rct, quality, ycbcr), _p(w), stride, _p(nw), _p(m), _p(off), _p(vp), _p(wp), _p(out), out.size,
                                               C.addressof(n), err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_coded_encode_image: {rc}")
    return out[: n.value].tobytes()


def tiled_info(frv):
    """fri_tiled_info: the TiledInfo of a `frit` file (header, table and every payload's header are checked; nothing is decoded)."""
    data = np.frombuffer(frv, np.uint8)
    info = np.zeros(8, np.uint32)
    rc = load_library().fri_tiled_info(_p(data), data.size, _p(info))
    if rc != 0:
        raise EmitError(f"fri_tiled_info: {rc}")
    return _tiled_info(info)


def tiled_decode(frv, threads=0):
    """fri_tiled_decode: (TiledInfo, coefs int32 [n_tiles][C][F][512] with None = INT32_MIN) - what PlanTiled.decode_image_tiled takes. Tiles are decoded on
    `threads` workers (0: the hardware concurrency, capped at 16). A tiled 4:2:0 file (TiledInfo.s420): coefs is flat and in plane order, [n][F_y][512] then
    [n][2][F_c][512] - what PlanTiled420.decode_image_tiled420 takes. A tiled RGBA file (TiledInfo.alpha): coefs is [4 n][F][512] in plane order - what
    PlanTiledRgba.decode_image_tiled_rgba takes."""
    data = np.frombuffer(frv, np.uint8)
    info = np.zeros(8, np.uint32)
    err = C.create_string_buffer(256)
    L = load_library()
    rc = L.fri_tiled_decode(_p(data), data.size, threads, _p(info), None, 0, err, 256)
    if rc != -3:
        raise EmitError(err.value.decode() or f"fri_tiled_decode: {rc}")
    ti = _tiled_info(info)
    coefs = _tiled_coefs(ti, ti[4] * ti[5])
    rc = L.fri_tiled_decode(_p(data), data.size, threads, _p(info), _p(coefs), coefs.size, err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_tiled_decode: {rc}")
    return ti, coefs


def tiled_decode_levels(frv, levels, threads=0):
    """fri_tiled_decode_levels: (TiledInfo, compact coefs int32 [n_tiles][C][F][2^levels]) - tiled_decode stopped behind the nodes with heap index < 2^levels (0: the
    DC alone, 1: DC and root, 9: everything), which are a prefix of every channel's stream; equal to tiled_decode's planes sliced to [..., :2^levels]. What
    PlanTiled.preview takes. EmitError for levels > 9 and for a tiled 4:2:0 file."""
    data = np.frombuffer(frv, np.uint8)
    info = np.zeros(8, np.uint32)
    err = C.create_string_buffer(256)
    L = load_library()
    if not 0 <= int(levels) <= 9:
        raise EmitError("fri_tiled_decode_levels: levels must be 0..9")
    rc = L.fri_tiled_decode_levels(_p(data), data.size, threads, int(levels), _p(info), None, 0, err, 256)
    if rc != -3:
        raise EmitError(err.value.decode() or f"fri_tiled_decode_levels: {rc}")
    ti = _tiled_info(info)
    coefs = np.empty((ti[4] * ti[5], ti[6], ti[7], 1 << int(levels)), np.int32)
    rc = L.fri_tiled_decode_levels(_p(data), data.size, threads, int(levels), _p(info), _p(coefs), coefs.size, err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_tiled_decode_levels: {rc}")
    return ti, coefs


def tiled_parse_coded(frv, word_stride=None):
    """fri_tiled_parse_coded: a `frit` file back to its coded planes, the inverse of tiled_encode_from_coded[420] and what PlanTiled[420].decode_coded takes -
    (TiledInfo, words uint32 [P][word_stride], n_words [P], models [P][10][4] = {max_freq_bits as the file carries it, n_off, 0, 0}, off_values uint16 [P][10][1024],
    value_params, width_params [P][3][6]), P = n_tiles C planes in the file's plane order. Nothing is decoded. word_stride: None sizes the rows by the longest plane
    (one size query first); a stride shorter than a plane raises an EmitError that names the plane and carries the complete counts as .n_words."""
    data = np.frombuffer(frv, np.uint8)
    info = np.zeros(8, np.uint32)
    err = C.create_string_buffer(256)
    L = load_library()
    rc = L.fri_tiled_parse_coded(_p(data), data.size, _p(info), 0, None, 0, None, None, None, None, None, err, 256)
    if rc != -3:
        raise EmitError(err.value.decode() or f"fri_tiled_parse_coded: {rc}")
    ti = _tiled_info(info)
    planes = ti[4] * ti[5] * ti[6]
    nw = np.zeros(planes, np.uint32)
    rc = L.fri_tiled_parse_coded(_p(data), data.size, _p(info), planes, None, 0, _p(nw), None, None, None, None, err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_tiled_parse_coded: {rc}")
    stride = max(int(nw.max()), 1) if word_stride is None else int(word_stride)
    words = np.zeros((planes, stride), np.uint32)
    models, off = np.zeros((planes, 10, 4), np.uint32), np.zeros((planes, 10, 1024), np.uint16)
    vp, wp = np.zeros((planes, 3, 6), np.float32), np.zeros((planes, 3, 6), np.float32)
    rc = L.fri_tiled_parse_coded(_p(data), data.size, _p(info), planes, _p(words), stride, _p(nw), _p(models), _p(off), _p(vp), _p(wp), err, 256)
    if rc != 0:
        e = EmitError(err.value.decode() or f"fri_tiled_parse_coded: {rc}")
        e.n_words = nw
        raise e
    return ti, words, nw, models, off, vp, wp


def tiled_region_tiles(width, height, tile_w, tile_h, x, y, w, h):
    """fri_tiled_region_tiles: (i0, j0, ni, nj), the sub-grid of tiles the region x, y, w, h (image pixels) touches. EmitError for a zero size or a region that
    leaves the image."""
    out = np.zeros(4, np.uint32)
    rc = load_library().fri_tiled_region_tiles(width, height, tile_w, tile_h, x, y, w, h, _p(out))
    if rc != 0:
        raise EmitError(f"fri_tiled_region_tiles: {rc}")
    return tuple(int(v) for v in out)


def tiled_decode_region(frv, x, y, w, h, threads=0):
    """fri_tiled_decode_region: (TiledInfo, (i0, j0, ni, nj), coefs int32 [nj ni][C][F][512]) - what PlanTiled.decode_region_tiled takes. The file is checked as
    tiled_decode checks it; only the tiles the region touches are decoded, and damage inside the body of an untouched tile is not looked at. A tiled 4:2:0 file:
    coefs is flat and in the sub-grid's plane order - what PlanTiled420.decode_region_tiled420 takes. A tiled RGBA file: coefs is [4 ni nj][F][512] in the
    sub-grid's plane order - what PlanTiledRgba.decode_region_tiled_rgba takes."""
    data = np.frombuffer(frv, np.uint8)
    info, tiles = np.zeros(8, np.uint32), np.zeros(4, np.uint32)
    err = C.create_string_buffer(256)
    L = load_library()
    rc = L.fri_tiled_decode_region(_p(data), data.size, threads, x, y, w, h, _p(info), _p(tiles), None, 0, err, 256)
    if rc != -3:
        raise EmitError(err.value.decode() or f"fri_tiled_decode_region: {rc}")
    ti = _tiled_info(info)
    coefs = _tiled_coefs(ti, int(tiles[2]) * int(tiles[3]))
    rc = L.fri_tiled_decode_region(_p(data), data.size, threads, x, y, w, h, _p(info), _p(tiles), _p(coefs), coefs.size, err, 256)
    if rc != 0:
        raise EmitError(err.value.decode() or f"fri_tiled_decode_region: {rc}")
    return ti, tuple(int(v) for v in tiles), coefs


def _regions(regions):
    """regions as the contiguous uint32 [R][4] array the C side reads; EmitError for anything that is not R >= 1 rows of (x, y, w, h) in 32 bits"""
    try:
        wide = np.asarray(regions, np.int64).reshape(-1, 4)
    except (ValueError, TypeError, OverflowError) as e:
        raise EmitError(f"regions must be rows of (x, y, w, h): {e}") from None
    if wide.shape[0] == 0 or (wide < 0).any() or (wide > 0xFFFFFFFF).any():
        raise EmitError("regions must be one or more rows of (x, y, w, h), each in 32 bits")
    return np.ascontiguousarray(wide, np.uint32)


def tiled_regions_tiles(width, height, tile_w, tile_h, regions):
    """fri_tiled_regions_tiles: the tile list of `regions` [(x, y, w, h), ...] - uint32 [T], the strictly ascending file-grid indices t = j nx + i of the tiles at
    least one region touches, each once. EmitError for no regions, a zero size or a region that leaves the image."""
    rg = _regions(regions)
    n = C.c_size_t(0)
    L = load_library()
    rc = L.fri_tiled_regions_tiles(width, height, tile_w, tile_h, rg.shape[0], _p(rg), None, 0, C.addressof(n))
    if rc != -3:
        raise EmitError(f"fri_tiled_regions_tiles: {rc}")
    out = np.zeros(n.value, np.uint32)
    rc = L.fri_tiled_regions_tiles(width, height, tile_w, tile_h, rg.shape[0], _p(rg), _p(out), out.size, C.addressof(n))
    if rc != 0:
        raise EmitError(f"fri_tiled_regions_tiles: {rc}")
    return out


def tiled_decode_tiles(frv, tiles, threads=0):
    """fri_tiled_decode_tiles: (TiledInfo, coefs int32 [T][C][F][512]) for the strictly ascending tile list `tiles` (file-grid indices), in list order - what
    PlanTiled.decode_regions_tiled takes. The file is checked as tiled_decode checks it; only the listed tiles are decoded, and damage inside the body of an
    unlisted tile is not looked at. A tiled 4:2:0 file: coefs is flat and in plane order with n = T; a tiled RGBA file: [4 T][F][512] in plane order. An EmitError carries the C return value as .code."""
    data = np.frombuffer(frv, np.uint8)
    tl = np.ascontiguousarray(tiles, np.uint32).reshape(-1)
    info = np.zeros(8, np.uint32)
    err = C.create_string_buffer(256)
    L = load_library()

    def fail(rc):
        e = EmitError(err.value.decode() or f"fri_tiled_decode_tiles: {rc}")
        e.code = rc
        return e

    rc = L.fri_tiled_decode_tiles(_p(data), data.size, threads, _p(tl), tl.size, _p(info), None, 0, err, 256)
    if rc != -3:
        raise fail(rc)
    ti = _tiled_info(info)
    coefs = _tiled_coefs(ti, tl.size)
    rc = L.fri_tiled_decode_tiles(_p(data), data.size, threads, _p(tl), tl.size, _p(info), _p(coefs), coefs.size, err, 256)
    if rc != 0:
        raise fail(rc)
    return ti, coefs


def tiled_preview_regions_tiles(width, height, tile_w, tile_h, shift, regions):
    """fri_tiled_preview_regions_tiles: the tile list of `regions` [(X, Y, w, h), ...] given in the coordinates of the thumbnail at `shift` - uint32 [T], the tile list
    tiled_regions_tiles makes of their source rectangles (include/fri_emit.h, "Preview of regions"). EmitError for no regions, a zero size, shift > 4 or a region
    that is empty or leaves the thumbnail."""
    rg = _regions(regions)
    n = C.c_size_t(0)
    L = load_library()
    if not 0 <= int(shift) <= 0xFFFFFFFF:
        raise EmitError("fri_tiled_preview_regions_tiles: shift must be 0..4")
    rc = L.fri_tiled_preview_regions_tiles(width, height, tile_w, tile_h, int(shift), rg.shape[0], _p(rg), None, 0, C.addressof(n))
    if rc != -3:
        raise EmitError(f"fri_tiled_preview_regions_tiles: {rc}")
    out = np.zeros(n.value, np.uint32)
    rc = L.fri_tiled_preview_regions_tiles(width, height, tile_w, tile_h, int(shift), rg.shape[0], _p(rg), _p(out), out.size, C.addressof(n))
    if rc != 0:
        raise EmitError(f"fri_tiled_preview_regions_tiles: {rc}")
    return out


def tiled_decode_tiles_levels(frv, tiles, levels, threads=0):
    """fri_tiled_decode_tiles_levels: (TiledInfo, compact coefs int32 [T][C][F][2^levels]) for the strictly ascending tile list `tiles`, in list order - tiled_decode_tiles
    stopped behind the nodes with heap index < 2^levels; equal to tiled_decode_levels's planes at the listed tiles and to tiled_decode_tiles's sliced to
    [..., :2^levels]. What PlanTiled.preview_regions takes. EmitError (with the C return value as .code) for levels > 9, a bad list, and a tiled 4:2:0 or RGBA file."""
    data = np.frombuffer(frv, np.uint8)
    tl = np.ascontiguousarray(tiles, np.uint32).reshape(-1)
    info = np.zeros(8, np.uint32)
    err = C.create_string_buffer(256)
    L = load_library()

    def fail(rc):
        e = EmitError(err.value.decode() or f"fri_tiled_decode_tiles_levels: {rc}")
        e.code = rc
        return e

    if not 0 <= int(levels) <= 9:
        raise EmitError("fri_tiled_decode_tiles_levels: levels must be 0..9")
    rc = L.fri_tiled_decode_tiles_levels(_p(data), data.size, threads, _p(tl), tl.size, int(levels), _p(info), None, 0, err, 256)
    if rc != -3:
        raise fail(rc)
    ti = _tiled_info(info)
    coefs = np.empty((tl.size, ti[6], ti[7], 1 << int(levels)), np.int32)
    rc = L.fri_tiled_decode_tiles_levels(_p(data), data.size, threads, _p(tl), tl.size, int(levels), _p(info), _p(coefs), coefs.size, err, 256)
    if rc != 0:
        raise fail(rc)
    return ti, coefs


def tiled_parse_coded_tiles(frv, tiles, word_stride=None):
    """fri_tiled_parse_coded_tiles: tiled_parse_coded for the strictly ascending tile list `tiles` - the same tuple with P = T C planes in list order (plane order
    with n = T for a tiled 4:2:0 file); only the listed payloads' markers are walked. What PlanTiled.decode_regions_coded takes. An EmitError carries the C return
    value as .code."""
    data = np.frombuffer(frv, np.uint8)
    tl = np.ascontiguousarray(tiles, np.uint32).reshape(-1)
    info = np.zeros(8, np.uint32)
    err = C.create_string_buffer(256)
    L = load_library()

    def fail(rc):
        e = EmitError(err.value.decode() or f"fri_tiled_parse_coded_tiles: {rc}")
        e.code = rc
        return e

    head = (_p(data), data.size, _p(tl), tl.size, _p(info))
    rc = L.fri_tiled_parse_coded_tiles(*head, 0, None, 0, None, None, None, None, None, err, 256)
    if rc != -3:
        raise fail(rc)
    ti = _tiled_info(info)
    planes = tl.size * ti[6]
    nw = np.zeros(planes, np.uint32)
    rc = L.fri_tiled_parse_coded_tiles(*head, planes, None, 0, _p(nw), None, None, None, None, err, 256)
    if rc != 0:
        raise fail(rc)
    stride = max(int(nw.max()), 1) if word_stride is None else int(word_stride)
    words = np.zeros((planes, stride), np.uint32)
    models, off = np.zeros((planes, 10, 4), np.uint32), np.zeros((planes, 10, 1024), np.uint16)
    vp, wp = np.zeros((planes, 3, 6), np.float32), np.zeros((planes, 3, 6), np.float32)
    rc = L.fri_tiled_parse_coded_tiles(*head, planes, _p(words), stride, _p(nw), _p(models), _p(off), _p(vp), _p(wp), err, 256)
    if rc != 0:
        e = fail(rc)
        e.n_words = nw
        raise e
    return ti, words, nw, models, off, vp, wp


def tiled_update_from_streams(frv, x, y, w, h, streams, hist, value_params, width_params, rct=False, quality=0, ycbcr=False, threads=0, flags=0):
    """fri_tiled_update_from_streams: (the updated `frit` bytes, (i0, j0, ni, nj)) - the file `frv` with the payloads of the tiles the region x, y, w, h touches
    coded from what PlanTiled.encode_region_tiled_symbols returns, in the sub-grid's order: streams uint16 [nj ni][C][n_symbols], hist [nj ni][C][10][1024],
    params [nj ni][C][3][6] (C is read from hist's second axis). Every other payload is copied and not looked into. rct, quality, ycbcr must be the file's own: the
    metadata word they make must be tile 0's. `flags` is or-ed into the channels word as it is. An EmitError carries the C return value as .code. The buffer of
    the first call is sized generously, so the touched tiles are coded once as a rule (a size query would code them too)."""
    data = np.frombuffer(frv, np.uint8)
    st = np.ascontiguousarray(streams, np.uint16)
    hi = np.ascontiguousarray(hist, np.uint32)
    vp, wp = np.ascontiguousarray(value_params, np.float32), np.ascontiguousarray(width_params, np.float32)
    assert hi.ndim == 4 and hi.shape[2:] == (10, 1024), "hist is [nj ni][C][10][1024]"
    planes, channels = hi.shape[0] * hi.shape[1], hi.shape[1]
    assert planes and vp.size == planes * 18 and wp.size == planes * 18 and st.size % planes == 0
    info, tiles = np.zeros(8, np.uint32), np.zeros(4, np.uint32)
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    L = load_library()
    # the arrays must hold the tiles the region touches before the library reads them (a malformed file or a bad region is the library's to refuse: it does so first)
    if L.fri_tiled_info(_p(data), data.size, _p(info)) == 0 and L.fri_tiled_region_tiles(*(int(v) for v in info[:4]), x, y, w, h, _p(tiles)) == 0:
        if int(tiles[2]) * int(tiles[3]) != hi.shape[0]:
            e = EmitError(f"fri_tiled_update_from_streams: the region touches {int(tiles[2]) * int(tiles[3])} tiles, the arrays hold {hi.shape[0]}")
            e.code = -1
            raise e
    args = (_p(data), data.size, x, y, w, h, _arg(channels, rct, quality, ycbcr) | flags, _p(st), st.size // planes, _p(hi), _p(vp), _p(wp), threads, _p(tiles))
    out = np.empty(data.size + st.size * 4 + planes * (10 * 2070 + 256) + hi.shape[0] * 72 + 64, np.uint8)  # the file and, generously, the new payloads: one call as a rule
    rc = L.fri_tiled_update_from_streams(*args, _p(out), out.size, C.addressof(n), err, 256)
    if rc == -3:
        out = np.empty(n.value, np.uint8)
        rc = L.fri_tiled_update_from_streams(*args, _p(out), out.size, C.addressof(n), err, 256)
    if rc != 0:
        e = EmitError(err.value.decode() or f"fri_tiled_update_from_streams: {rc}")
        e.code = rc
        raise e
    return out[: n.value].tobytes(), tuple(int(v) for v in tiles)
