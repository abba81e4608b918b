"""Lossy YCbCr colour coding (fri_hip_plan_set_colour_transform(FRI_HIP_COLOUR_YCBCR), FRI_EMIT_YCBCR), host side: the transform over every 8-bit triple,
the setter on host-only plans, the searches' argument checks, the emitter's flag and metadata word, the decoder's report and the size estimate of a YCbCr
file. CPU only."""
import ctypes as C
import struct

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd import api
from tests import rate_model
from tests.common import gen_image
from tests.test_rct_host import correlated_image
from tests.ycbcr_ref import inverse_ycc, psnr, ycc

VARIANT = 1  # TameTwindragon


def _all_triples():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([v >> 16, (v >> 8) & 255, v & 255], axis=1).astype(np.uint8)


def test_transform_range_and_round_trip_over_all_8_bit_triples():
    px = _all_triples()
    p = px.astype(np.int64)
    # the planes without the final cast: each stays inside 0..255, so K1's byte path and the 9-bit coefficient bound hold
    r, g, b = p[:, 0], p[:, 1], p[:, 2]
    for plane in ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16, (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
                  (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16):
        assert plane.min() >= 0 and plane.max() <= 255
    back = inverse_ycc(ycc(px))
    err = np.abs(back.astype(np.int32) - px.astype(np.int32))
    assert err.max() == 1  # lossy by construction, off by at most 1 per channel
    db = psnr(back, px)
    print(f"forward + inverse over the 2^24 cube: max error {err.max()}, {db:.2f} dB")
    assert 52.5 < db < 53.5
    assert np.array_equal(ycc(np.zeros((1, 3), np.uint8)), [[0, 128, 128]])


def test_setter_on_host_only_plans():
    lib = fa.load_library()
    rgb, luma = fa.Plan(None, 64, 48, 3), fa.Plan(None, 64, 48, 1)
    assert api.COLOUR_YCBCR == 3
    rgb.set_colour_transform(api.COLOUR_YCBCR)
    assert rgb.colour_transform == api.COLOUR_YCBCR
    rgb.set_colour_transform(api.COLOUR_RCT)  # the modes replace each other
    rgb.set_colour_transform(api.COLOUR_YCBCR)
    rgb.set_colour_transform(api.COLOUR_NONE)
    with pytest.raises(fa.FriHipError) as e:
        luma.set_colour_transform(api.COLOUR_YCBCR)
    assert e.value.code == -1
    for bad in (2, 4, 7):  # 2: "irreversible" without chroma planes means nothing
        with pytest.raises(fa.FriHipError) as e:
            rgb.set_colour_transform(bad)
        assert e.value.code == -1
    assert lib.fri_hip_plan_set_colour_transform(None, api.COLOUR_YCBCR) == -1
    rgb.set_colour_transform(api.COLOUR_YCBCR)
    with pytest.raises(fa.FriHipError) as e:  # a host-only plan still refuses to compute
        rgb.transform_quant(np.zeros((48, 64, 3), np.uint8))
    assert e.value.code == -3
    rgb.close(), luma.close()


def test_searches_take_ycbcr_plans_and_still_refuse_rct_plans():
    """On a host-only plan the searches get past their argument checks with YCbCr (and report "no device", -3), but not with the RCT (-1)."""
    L = api.load_library()
    P = fa.Plan(None, 64, 48, 3)
    px = np.zeros(P.pixel_bytes, np.uint8)
    qual, db, est = C.c_int32(0), C.c_double(0), C.c_uint64(0)
    for mode, want in ((api.COLOUR_YCBCR, -3), (api.COLOUR_RCT, -1)):
        P.set_colour_transform(mode)
        assert L.fri_hip_search_quality(P._h, api._p(px), 40.0, C.byref(qual), C.byref(db)) == want
        assert L.fri_hip_search_quality_dev(P._h, 16, 40.0, C.byref(qual), C.byref(db), None) == want
        assert L.fri_hip_search_quality_for_size(P._h, api._p(px), 5000, C.byref(qual), C.byref(est)) == want
        assert L.fri_hip_search_quality_for_size_dev(P._h, 16, 5000, C.byref(qual), C.byref(est), None) == want
    P.close()


# ---- the container (FRI_EMIT_YCBCR: colour space YCbCr, metadata bit 1) ----------------------------------------------------------------------------

def _mdat(frv):
    return struct.unpack("<I", frv[12:16])[0]


def _ycc_arrays(w, h, quality, kind="smooth"):
    img = gen_image(kind, w, h, 3, 3)
    centers, coefs, bucket, pred, hist, oob, vp, wp = rate_model.oracle_arrays(ycc(img), w, h, 3, quality)
    assert not oob.any()
    return centers, coefs, bucket, pred, hist, vp, wp


@pytest.mark.parametrize("shape", [(160, 120), (96, 257)])
@pytest.mark.parametrize("quality", [1, 50, 99])
def test_ycbcr_file_differs_only_in_the_metadata_word(shape, quality):
    from oracle import emit_oracle

    w, h = shape
    centers, coefs, bucket, pred, hist, vp, wp = _ycc_arrays(w, h, quality)
    lossy = emit.encode_image(w, h, centers, coefs, bucket, pred, hist, vp, wp, quality=quality)
    flagged = emit.encode_image(w, h, centers, coefs, bucket, pred, hist, vp, wp, quality=quality, ycbcr=True)
    assert _mdat(lossy) == 0x80000000 | VARIANT << 28 | quality << 8
    assert _mdat(flagged) == _mdat(lossy) | 0xC0000000 | 0x2  # colour space 0b11, bit 1 set, bit 0 clear
    assert _mdat(flagged) & 1 == 0
    assert len(flagged) == len(lossy) and flagged[:12] == lossy[:12] and flagged[16:] == lossy[16:]
    streams = []
    for ch in range(3):
        sym, bk = emit.channel_symbols(centers, coefs[ch], bucket[ch], pred[ch])
        streams.append((bk.astype(np.uint16) << 10) | sym)
    assert emit.encode_image_from_streams(w, h, np.stack(streams), hist, vp, wp, quality=quality, ycbcr=True) == flagged
    emit.check_image(flagged, centers, coefs, bucket, pred, quality=quality, ycbcr=True)
    with pytest.raises(emit.EmitError):  # the check compares the flag
        emit.check_image(flagged, centers, coefs, bucket, pred, quality=quality)
    with pytest.raises(emit.EmitError):
        emit.check_image(lossy, centers, coefs, bucket, pred, quality=quality, ycbcr=True)
    d = emit.decode_image(flagged)
    assert d.ycbcr is True and d.rct is False and d.quality == quality and d[:3] == (w, h, 3)
    assert np.array_equal(d[4], coefs)
    assert emit.decode_image(lossy).ycbcr is False
    # the reference's decoder (restated) reads only bits 28-31: it returns the Y, Cb, Cr planes
    ow, oh, oc, ocoefs = emit_oracle.decode_image(flagged)[:4]
    assert (ow, oh, oc) == (w, h, 3) and np.array_equal(ocoefs, coefs)


def test_decoder_reports_the_flag_in_info():
    w, h = 160, 120
    centers, coefs, bucket, pred, hist, vp, wp = _ycc_arrays(w, h, 37)
    frv = np.frombuffer(emit.encode_image(w, h, centers, coefs, bucket, pred, hist, vp, wp, quality=37, ycbcr=True), np.uint8)
    info = np.zeros(4, np.uint32)
    L = emit.load_library()
    assert L.fri_emit_decode_image(frv.ctypes.data_as(C.c_void_p), frv.size, info.ctypes.data_as(C.c_void_p), None, 0, None, None, 0) == -3
    assert int(info[2]) == 3 | emit.YCBCR | emit.QUALITY(37)


def test_ycbcr_flag_refusals():
    w, h = 160, 120
    centers, coefs, bucket, pred, hist, vp, wp = _ycc_arrays(w, h, 50)
    L = emit.load_library()
    cc, co, b, p = (np.ascontiguousarray(a) for a in (centers, coefs, bucket, pred))
    h_, vp_, wp_ = np.ascontiguousarray(hist, np.uint32), np.ascontiguousarray(vp), np.ascontiguousarray(wp)
    out = np.empty(coefs.size * 4 + 100000, np.uint8)
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def enc(arg):
        return L.fri_emit_encode_image(w, h, arg, P(cc), len(cc), P(co), P(b), P(p), P(h_), P(vp_), P(wp_), P(out), out.size, C.addressof(n), err, 256)

    assert emit.YCBCR == 0x400
    refused = (3 | emit.YCBCR, 1 | emit.YCBCR | emit.QUALITY(50), 3 | emit.YCBCR | emit.RCT | emit.QUALITY(50), 3 | emit.YCBCR | emit.RCT,
               3 | emit.YCBCR | emit.QUALITY(100), 3 | 0x200 | emit.QUALITY(50), 3 | emit.YCBCR | 0x200 | emit.QUALITY(50))
    for arg in refused:
        assert enc(arg) == -1, hex(arg)
    for q in (1, 99):
        assert enc(3 | emit.YCBCR | emit.QUALITY(q)) == 0
    assert enc(3 | emit.YCBCR | emit.QUALITY(50)) == 0
    frv = out[: n.value].copy()
    for arg in (3 | emit.YCBCR, 1 | emit.YCBCR | emit.QUALITY(50), 3 | emit.YCBCR | emit.RCT | emit.QUALITY(50)):
        assert L.fri_emit_check_image(P(frv), frv.size, arg, P(cc), len(cc), P(co), P(b), P(p), err, 256) == -1


def test_invalid_ycbcr_metadata():
    w, h = 160, 120
    centers, coefs, bucket, pred, hist, vp, wp = _ycc_arrays(w, h, 50)
    flagged = emit.encode_image(w, h, centers, coefs, bucket, pred, hist, vp, wp, quality=50, ycbcr=True)
    m = _mdat(flagged)

    def with_mdat(word):
        odd = bytearray(flagged)
        odd[12:16] = struct.pack("<I", word)
        return bytes(odd)

    with pytest.raises(emit.EmitError, match="Invalid metadata"):  # bits 0 and 1 both set
        emit.decode_image(with_mdat(m | 0x1))
    with pytest.raises(emit.EmitError, match="Invalid metadata"):  # bit 1 and quality 0
        emit.decode_image(with_mdat(m & ~(0x7F << 8)))
    # a YCbCr file with neither bit decodes as before (the planes, no flag)
    d = emit.decode_image(with_mdat(m & ~0x3))
    assert d.ycbcr is False and d.rct is False and d.quality == 50 and np.array_equal(d[4], coefs)
    # bit 1 of an RGB file stays ignored
    rgb = with_mdat((m & ~(0x3 << 30)) | 2 << 30)
    d = emit.decode_image(rgb)
    assert d.ycbcr is False and d.rct is False and np.array_equal(d[4], coefs)


def test_estimate_is_within_24_bytes_per_channel_of_a_ycbcr_file():
    w, h = 320, 240
    img = correlated_image(w, h, 5)
    for q in (1, 50, 90, 99):
        centers, coefs, bucket, pred, hist, oob, vp, wp = rate_model.oracle_arrays(ycc(img), w, h, 3, q)
        assert not oob.any()
        est = rate_model.estimate_image(hist, oob)
        frv = emit.encode_image(w, h, centers, coefs, bucket, pred, hist, vp, wp, quality=q, ycbcr=True)
        assert abs(est - len(frv)) <= 24 * 3, (q, est, len(frv))
