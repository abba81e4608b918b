"""Reversible colour transform (fri_hip_plan_set_colour_transform, FRI_EMIT_RCT), host side: the transform itself, the setter's argument checks on host-only
plans, and the flagged container built from oracle coefficients of rct(pixels). CPU only."""
import ctypes as C
import struct

import numpy as np
import pytest

from oracle import emit_oracle, fri_oracle
from tests.common import KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS, gen_image

import frave_amd.emit as emit


def rct(pixels):
    """forward, per pixel mod 256: (R, G, B) -> (Y, Cb, Cr) = (G, B - G + 128, R - G + 128), interleaved like the input"""
    p = np.asarray(pixels, np.uint8).reshape(-1, 3).astype(np.int32)
    r, g, b = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([g, (b - g + 128) & 255, (r - g + 128) & 255], axis=1).astype(np.uint8).reshape(np.shape(pixels))


def inverse_rct(planes):
    """inverse: (Y, Cb, Cr) -> (R, G, B) = (Cr + Y - 128, Y, Cb + Y - 128) mod 256"""
    p = np.asarray(planes, np.uint8).reshape(-1, 3).astype(np.int32)
    y, cb, cr = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(cr + y - 128) & 255, y, (cb + y - 128) & 255], axis=1).astype(np.uint8).reshape(np.shape(planes))


def correlated_image(w, h, seed):
    """G: a smooth texture plus noise; R = G + 23, B = G - 31, each plus small noise of its own (clipped to 8 bits)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    g = 128 + 60 * np.sin(x / 9.0) * np.cos(y / 13.0) + 30 * np.sin((x + 2 * y) / 31.0) + rng.normal(0, 4, (h, w))
    r = g + 23 + rng.normal(0, 0.6, (h, w))
    b = g - 31 + rng.normal(0, 0.6, (h, w))
    return np.clip(np.rint(np.stack([r, g, b], axis=2)), 0, 255).astype(np.uint8)


def test_rct_is_a_bijection_on_all_8_bit_triples():
    v = np.arange(1 << 24, dtype=np.uint32)
    px = np.stack([v >> 16, (v >> 8) & 255, v & 255], axis=1).astype(np.uint8)
    f = rct(px)
    assert np.array_equal(inverse_rct(f), px)
    code = (f[:, 0].astype(np.uint32) << 16) | (f[:, 1].astype(np.uint32) << 8) | f[:, 2]
    assert np.unique(code).size == 1 << 24  # onto as well: every triple is the image of exactly one
    assert np.array_equal(f[:, 0], px[:, 1])  # Y is G


def test_setter_arguments_on_host_only_plans():
    import frave_amd as fa
    from frave_amd import api

    lib = fa.load_library()
    rgb, luma = fa.Plan(None, 64, 48, 3), fa.Plan(None, 64, 48, 1)
    assert rgb.colour_transform == api.COLOUR_NONE == 0 and api.COLOUR_RCT == 1
    assert lib.fri_hip_plan_set_colour_transform(None, api.COLOUR_NONE) == -1
    assert lib.fri_hip_plan_set_colour_transform(None, api.COLOUR_RCT) == -1
    with pytest.raises(fa.FriHipError) as e:
        luma.set_colour_transform(api.COLOUR_RCT)
    assert e.value.code == -1
    luma.set_colour_transform(api.COLOUR_NONE)  # the default is valid on every plan
    for bad in (2, -1, 0x100):
        with pytest.raises(fa.FriHipError) as e:
            rgb.set_colour_transform(bad)
        assert e.value.code == -1
    assert rgb.colour_transform == api.COLOUR_NONE
    rgb.set_colour_transform(api.COLOUR_RCT)
    assert rgb.colour_transform == api.COLOUR_RCT
    rgb.set_colour_transform(api.COLOUR_NONE)
    # a host-only plan still refuses to compute, whatever the mode
    rgb.set_colour_transform(api.COLOUR_RCT)
    with pytest.raises(fa.FriHipError) as e:
        rgb.transform_quant(np.zeros((48, 64, 3), np.uint8))
    assert e.value.code == -3
    rgb.close(), luma.close()


def _oracle_arrays(img, w, h):
    W = fri_oracle.Wavelet(img, h, w, 3)
    coefs = W.coefficients()
    bs, ps, hs = [], [], []
    for ch in range(3):
        b, p, hist, oob = W.predict(ch, KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS)
        assert oob == 0
        bs.append(b), ps.append(p), hs.append(hist)
    vp = np.stack([np.asarray(KAT_VALUE_PARAMS, np.float32).reshape(3, 6)] * 3)
    wp = np.stack([np.asarray(KAT_WIDTH_PARAMS, np.float32).reshape(3, 6)] * 3)
    return W, coefs, np.stack(bs), np.stack(ps), np.stack(hs), vp, wp


def _mdat(frv):
    return struct.unpack("<I", frv[12:16])[0]


@pytest.mark.parametrize("shape", [(160, 120), (96, 257)])
def test_flagged_container_differs_only_in_the_metadata_word(shape):
    w, h = shape
    img = gen_image("smooth", w, h, 3, 3)
    W, coefs, bucket, pred, hist, vp, wp = _oracle_arrays(rct(img), w, h)
    plain = emit.encode_image(w, h, W.centers(), coefs, bucket, pred, hist, vp, wp)
    flagged = emit.encode_image(w, h, W.centers(), coefs, bucket, pred, hist, vp, wp, rct=True)
    variant = 1  # TameTwindragon
    assert _mdat(plain) == 0x80000000 | variant << 28
    assert _mdat(flagged) == 0xC0000001 | variant << 28
    assert len(flagged) == len(plain) and flagged[:12] == plain[:12] and flagged[16:] == plain[16:]
    # the stream route writes the same bytes (streams = bucket << 10 | symbol in stream order)
    streams = []
    for ch in range(3):
        sym, bk = emit.channel_symbols(W.centers(), coefs[ch], bucket[ch], pred[ch])
        streams.append((bk.astype(np.uint16) << 10) | sym)
    assert emit.encode_image_from_streams(w, h, np.stack(streams), hist, vp, wp, rct=True) == flagged
    emit.check_image(flagged, W.centers(), coefs, bucket, pred, rct=True)
    with pytest.raises(emit.EmitError):  # the check compares the flag too
        emit.check_image(flagged, W.centers(), coefs, bucket, pred)
    with pytest.raises(emit.EmitError):
        emit.check_image(plain, W.centers(), coefs, bucket, pred, rct=True)
    # the product's decoder reports the flag and returns the same planes
    d_plain, d_flag = emit.decode_image(plain), emit.decode_image(flagged)
    assert d_plain.rct is False and d_flag.rct is True
    assert d_flag[:3] == (w, h, 3)
    assert np.array_equal(d_flag[3], d_plain[3]) and np.array_equal(d_flag[4], d_plain[4])
    assert np.array_equal(coefs, d_flag[4])
    # the reference's decoder (restated) reads only bits 28-31: it returns the Y, Cb, Cr planes
    ow, oh, oc, ocoefs = emit_oracle.decode_image(flagged)[:4]
    assert (ow, oh, oc) == (w, h, 3) and np.array_equal(ocoefs, d_flag[4])


def test_channels_with_unknown_high_bits_are_refused():
    w, h = 160, 120
    W, coefs, bucket, pred, hist, vp, wp = _oracle_arrays(rct(gen_image("smooth", w, h, 3, 3)), w, h)
    L = emit.load_library()
    c, co, b, p = (np.ascontiguousarray(a) for a in (W.centers(), coefs, bucket, pred))
    h_, vp_, wp_ = np.ascontiguousarray(hist, np.uint32), np.ascontiguousarray(vp), np.ascontiguousarray(wp)
    out = np.empty(coefs.size * 4 + 100000, np.uint8)
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def enc(arg):
        return L.fri_emit_encode_image(w, h, arg, P(c), len(c), P(co), P(b), P(p), P(h_), P(vp_), P(wp_), P(out), out.size, C.addressof(n), err, 256)

    assert enc(3) == 0 and enc(3 | emit.RCT) == 0
    for arg in (3 | 0x200, 3 | 0x80000000, 1 | emit.RCT, 2, 0x100):
        assert enc(arg) == -1, hex(arg)
    frv = out[: n.value].copy()
    for arg in (3 | 0x200, 1 | emit.RCT):
        assert L.fri_emit_check_image(P(frv), frv.size, arg, P(c), len(c), P(co), P(b), P(p), err, 256) == -1


def test_other_low_metadata_bits_stay_ignored():
    w, h = 160, 120
    W, coefs, bucket, pred, hist, vp, wp = _oracle_arrays(rct(gen_image("smooth", w, h, 3, 3)), w, h)
    plain = emit.encode_image(w, h, W.centers(), coefs, bucket, pred, hist, vp, wp)
    odd = bytearray(plain)
    odd[12:16] = struct.pack("<I", _mdat(plain) | 0x6)  # RGB with bits 1 and 2: not a flagged file
    d = emit.decode_image(bytes(odd))
    assert d.rct is False and np.array_equal(d[4], emit.decode_image(plain)[4])
    rgb_bit0 = bytearray(plain)
    rgb_bit0[12:16] = struct.pack("<I", _mdat(plain) | 0x1)  # bit 0 counts only with the YCbCr colour space
    assert emit.decode_image(bytes(rgb_bit0)).rct is False


def test_flagged_file_of_a_correlated_image_is_smaller():
    """Coded through the oracle's arrays and the emitter (KAT predictor parameters for both): R and B that follow G closely leave Cb and Cr with little to code.
    That this holds for natural photographs is not measured here."""
    w, h = 256, 192
    img = correlated_image(w, h, 7)
    plain = emit.encode_image(w, h, *_centered(_oracle_arrays(img, w, h)))
    flagged = emit.encode_image(w, h, *_centered(_oracle_arrays(rct(img), w, h)), rct=True)
    print(f"correlated {w}x{h}: RGB {len(plain)} B, RCT {len(flagged)} B ({len(flagged) / len(plain):.3f})")
    assert len(flagged) < 0.8 * len(plain)


def _centered(arrays):
    W, coefs, bucket, pred, hist, vp, wp = arrays
    return W.centers(), coefs, bucket, pred, hist, vp, wp
