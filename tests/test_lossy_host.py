"""Lossy coding by quality, host side: fri_hip_quality_matrix against the frozen table of every quality, the new dequantiser mode and the argument checks
of the measure and search entry points on host-only plans. CPU only."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import frave_amd as fa
from frave_amd import api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quality_matrices.npy")


def test_quality_matrix_matches_the_frozen_table():
    want = np.load(GOLDEN)
    assert want.shape == (100, 32) and want.dtype == np.int32
    for q in range(1, 101):
        assert np.array_equal(fa.quality_matrix(q), want[q - 1]), q


def test_quality_matrix_properties():
    m = np.stack([fa.quality_matrix(q) for q in range(1, 101)])
    assert (m[99] == 1).all()  # 100: lossless
    assert (m[:, 0] == 1).all()  # the DC
    assert np.array_equal(m[:, 9], m[:, 8])  # layer 9 is heap node 511 alone
    assert (m[:, 10:] == 1).all()
    assert (m >= 1).all() and (np.diff(m, axis=0) <= 0).all()  # non-increasing in quality
    assert (m[:99, 8] > 1).all()  # every quality below 100 quantises


@pytest.mark.parametrize("q", [0, -1, 101, 1000])
def test_quality_matrix_refuses_out_of_range(q):
    with pytest.raises(fa.FriHipError) as e:
        fa.quality_matrix(q)
    assert e.value.code == -1


def test_set_dequantiser_takes_the_midpoint_mode():
    P = fa.Plan(None, 64, 48, 3)
    for mode in (False, True, fa.DEQUANT_REFERENCE, fa.DEQUANT_MULTIPLY, fa.DEQUANT_MIDPOINT):
        P.set_dequantiser(mode)
    with pytest.raises(fa.FriHipError):
        P.set_dequantiser(3)
    P.close()


def test_host_only_plan_refuses_measure_and_search():
    L = api.load_library()
    P = fa.Plan(None, 64, 48, 1)
    q = fa.quality_matrix(50)
    out = np.zeros(3, np.uint64)
    assert L.fri_hip_measure_distortion_dev(P._h, 16, api._p(q), 16, api._p(out), None) == -3
    px = np.zeros(P.pixel_bytes, np.uint8)
    qual, db = C.c_int32(-7), C.c_double(0)
    assert L.fri_hip_search_quality(P._h, api._p(px), 40.0, C.byref(qual), C.byref(db)) == -3
    assert L.fri_hip_search_quality_dev(P._h, 16, 40.0, C.byref(qual), C.byref(db), None) == -3
    assert qual.value == -7
    P.close()


@pytest.mark.parametrize("target", [float("nan"), 0.0, -3.0, -math.inf])
def test_search_refuses_bad_targets(target):
    L = api.load_library()
    P = fa.Plan(None, 64, 48, 3)
    px = np.zeros(P.pixel_bytes, np.uint8)
    qual, db = C.c_int32(0), C.c_double(0)
    assert L.fri_hip_search_quality(P._h, api._p(px), target, C.byref(qual), C.byref(db)) == -1
    assert L.fri_hip_search_quality_dev(P._h, 16, target, C.byref(qual), C.byref(db), None) == -1
    P.close()


def test_search_refuses_rct_plans():
    L = api.load_library()
    P = fa.Plan(None, 64, 48, 3)
    P.set_colour_transform(api.COLOUR_RCT)
    px = np.zeros(P.pixel_bytes, np.uint8)
    qual, db = C.c_int32(0), C.c_double(0)
    assert L.fri_hip_search_quality(P._h, api._p(px), 40.0, C.byref(qual), C.byref(db)) == -1
    assert L.fri_hip_search_quality_dev(P._h, 16, 40.0, C.byref(qual), C.byref(db), None) == -1
    P.close()


def test_psnr_definition():
    assert fa.distortion_psnr(np.array([0, 0, 100], np.uint64), 1) == math.inf
    # one channel, 100 pixels, SSE 100: 10 log10(255^2)
    assert fa.distortion_psnr(np.array([100, 1, 100], np.uint64), 1) == pytest.approx(20 * math.log10(255), rel=1e-12)
    # pooled over three channels: N = 3 x pixels
    assert fa.distortion_psnr(np.array([50, 1, 0, 0, 250, 3, 100], np.uint64), 3) == pytest.approx(10 * math.log10(255 ** 2 * 300 / 300), rel=1e-12)


# ---- the container's quality field (FRI_EMIT_QUALITY, metadata bits 8..14) ---------------------------------------------------------------------

def _quantised_arrays(img, w, h, c, quality):
    from oracle import fri_oracle
    from tests.common import KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS

    W = fri_oracle.Wavelet(img, h, w, c)
    W.quantize(fa.quality_matrix(quality))
    coefs = W.coefficients()
    bs, ps, hs = [], [], []
    for ch in range(c):
        b, p, hist, oob = W.predict(ch, KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS)
        assert oob == 0
        bs.append(b), ps.append(p), hs.append(hist)
    vp = np.stack([np.asarray(KAT_VALUE_PARAMS, np.float32).reshape(3, 6)] * c)
    wp = np.stack([np.asarray(KAT_WIDTH_PARAMS, np.float32).reshape(3, 6)] * c)
    return W.centers(), coefs, np.stack(bs), np.stack(ps), np.stack(hs), vp, wp


def _mdat(frv):
    import struct

    return struct.unpack("<I", frv[12:16])[0]


@pytest.mark.parametrize("shape", [(160, 120, 1), (96, 257, 3)])
@pytest.mark.parametrize("quality", [1, 50, 99])
def test_quality_field_differs_only_in_the_metadata_word(shape, quality):
    import frave_amd.emit as emit
    from oracle import emit_oracle
    from tests.common import gen_image

    w, h, c = shape
    img = gen_image("smooth", w, h, c, 3)
    centers, coefs, bucket, pred, hist, vp, wp = _quantised_arrays(img, w, h, c, quality)
    plain = emit.encode_image(w, h, centers, coefs, bucket, pred, hist, vp, wp)
    lossy = emit.encode_image(w, h, centers, coefs, bucket, pred, hist, vp, wp, quality=quality)
    assert _mdat(lossy) == _mdat(plain) | quality << 8 and (_mdat(plain) >> 8) & 0x7F == 0
    assert len(lossy) == len(plain) and lossy[:12] == plain[:12] and lossy[16:] == plain[16:]
    streams = []
    for ch in range(c):
        sym, bk = emit.channel_symbols(centers, coefs[ch], bucket[ch], pred[ch])
        streams.append((bk.astype(np.uint16) << 10) | sym)
    assert emit.encode_image_from_streams(w, h, np.stack(streams), hist, vp, wp, quality=quality) == lossy
    emit.check_image(lossy, centers, coefs, bucket, pred, quality=quality)
    for wrong in (0, quality % 99 + 1):  # the check compares the field
        with pytest.raises(emit.EmitError):
            emit.check_image(lossy, centers, coefs, bucket, pred, quality=wrong)
    d_plain, d_lossy = emit.decode_image(plain), emit.decode_image(lossy)
    assert d_plain.quality == 0 and d_lossy.quality == quality and d_lossy.rct is False
    assert d_lossy[:3] == (w, h, c)
    assert np.array_equal(d_lossy[4], d_plain[4]) and np.array_equal(d_lossy[4], coefs)
    # the reference's decoder (restated) reads only bits 28-31: it returns the same (quantised) planes - the wrong pixels if dequantised as lossless
    ow, oh, oc, ocoefs = emit_oracle.decode_image(lossy)[:4]
    assert (ow, oh, oc) == (w, h, c) and np.array_equal(ocoefs, coefs)


def test_quality_field_refusals():
    import ctypes as C
    import struct

    import frave_amd.emit as emit
    from tests.common import gen_image

    w, h = 160, 120
    centers, coefs, bucket, pred, hist, vp, wp = _quantised_arrays(gen_image("smooth", w, h, 3, 3), w, h, 3, 50)
    L = emit.load_library()
    cc, co, b, p = (np.ascontiguousarray(a) for a in (centers, coefs, bucket, pred))
    h_, vp_, wp_ = np.ascontiguousarray(hist, np.uint32), np.ascontiguousarray(vp), np.ascontiguousarray(wp)
    out = np.empty(coefs.size * 4 + 100000, np.uint8)
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def enc(arg):
        return L.fri_emit_encode_image(w, h, arg, P(cc), len(cc), P(co), P(b), P(p), P(h_), P(vp_), P(wp_), P(out), out.size, C.addressof(n), err, 256)

    for arg in (3 | emit.QUALITY(100), 3 | emit.QUALITY(127), 3 | emit.RCT | emit.QUALITY(50), 3 | 0x200, 3 | 0x80000000, 1 | emit.RCT, 0x100):
        assert enc(arg) == -1, hex(arg)
    assert enc(3 | emit.QUALITY(50)) == 0
    frv = out[: n.value].copy()
    for arg in (3 | emit.QUALITY(100), 3 | emit.RCT | emit.QUALITY(50)):
        assert L.fri_emit_check_image(P(frv), frv.size, arg, P(cc), len(cc), P(co), P(b), P(p), err, 256) == -1
    # a file whose field holds 100..127 is invalid metadata
    for bad in (100, 127):
        odd = bytearray(frv.tobytes())
        odd[12:16] = struct.pack("<I", (_mdat(frv.tobytes()) & ~(0x7F << 8)) | bad << 8)
        with pytest.raises(emit.EmitError, match="Invalid metadata"):
            emit.decode_image(bytes(odd))
