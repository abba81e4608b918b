"""4:2:0 chroma subsampling, host side (include/fri_hip.h "4:2:0 chroma subsampling", FRI_EMIT_420): the host-only subsampled plan, the numpy restatement against
literal per-pixel loops, the emitter's flag - round trip, container bytes, refusals, invalid metadata - and the size model of a 4:2:0 file. CPU only."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd import api
from frave_amd.api import Plan420  # noqa: F401  (without the feature the module fails here)
from tests import rate_model
from tests.chroma420_ref import chroma_shape, merge420, split420, upsample420
from tests.common import gen_image
from tests.test_rct_host import correlated_image
from tests.ycbcr_ref import inverse_ycc, ycc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = 1  # TameTwindragon
SHAPES = [(64, 48), (97, 61), (3, 5), (17, 9), (1, 700), (700, 1), (1023, 767)]


# ---- the host-only plan ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_host_only_plan_owns_two_ordinary_plans(shape):
    w, h = shape
    cw, ch = chroma_shape(w, h)
    P = fa.Plan420(None, w, h)
    assert (P.cw, P.ch) == (cw, ch)
    for view, (pw, ph) in ((P.luma, (w, h)), (P.chroma, (cw, ch))):
        ref = fa.Plan(None, pw, ph, 1)
        assert (view.width, view.height, view.channels) == (pw, ph, 1)
        assert view.num_cells == ref.num_cells and view.num_some == ref.num_some and view.pixel_bytes == ref.pixel_bytes
        assert np.array_equal(view.centers(), ref.centers()) and np.array_equal(view.valid_mask(), ref.valid_mask())
        ref.close()
    assert P.num_symbols == P.luma.num_some + 2 * P.chroma.num_some
    assert P.coef_count == (P.luma.num_cells + 2 * P.chroma.num_cells) * 512
    P.close()


def test_host_only_plan_refuses_to_compute():
    w, h = 64, 48
    P = fa.Plan420(None, w, h)
    px = np.zeros((h, w, 3), np.uint8)
    calls = [lambda: P.split420_dev(16, 16, 16), lambda: P.merge420_dev(16, 16, 16), lambda: P.measure_distortion420_dev(16, 16, 16, 16),
             lambda: P.encode_image420_symbols(px, 50), lambda: P.decode_image420(np.zeros(P.coef_count, np.int32), 50),
             lambda: P.search_quality(px, 40.0), lambda: P.search_quality(16, 40.0), lambda: P.search_quality_ssim(px, 0.9), lambda: P.search_quality_ssim(16, 0.9),
             lambda: P.search_quality_for_size(px, 5000), lambda: P.search_quality_for_size(16, 5000),
             lambda: P.luma.transform_quant(np.zeros((h, w), np.uint8))]
    for call in calls:
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -3
    P.close()


def test_plan_and_search_argument_errors():
    L = api.load_library()
    h = C.c_void_p()
    for w, hh in ((0, 10), (10, 0)):
        assert L.fri_hip_plan420_create(None, w, hh, C.byref(h)) == -1
    assert L.fri_hip_plan420_create(None, 8, 8, None) == -1
    assert L.fri_hip_plan420_destroy(None) == 0 and L.fri_hip_plan420_luma(None) is None and L.fri_hip_plan420_chroma(None) is None
    P = fa.Plan420(None, 64, 48)
    px = np.zeros(P.pixel_bytes, np.uint8)
    qual, v, est = C.c_int32(0), C.c_double(0), C.c_uint64(0)
    for bad in (float("nan"), 0.0, -3.0):
        assert L.fri_hip_search_quality420(P._h, api._p(px), bad, C.byref(qual), C.byref(v)) == -1
        assert L.fri_hip_search_quality420_dev(P._h, 16, bad, C.byref(qual), C.byref(v), None) == -1
        assert L.fri_hip_search_quality_ssim420(P._h, api._p(px), bad, C.byref(qual), C.byref(v)) == -1
    assert L.fri_hip_search_quality_ssim420_dev(P._h, 16, 1.5, C.byref(qual), C.byref(v), None) == -1
    assert L.fri_hip_search_quality_for_size420(P._h, api._p(px), 0, C.byref(qual), C.byref(est)) == -1
    assert L.fri_hip_search_quality_for_size420_dev(P._h, 16, 0, C.byref(qual), C.byref(est), None) == -1
    for q in (0, 100, -1):  # a 4:2:0 file has a quality of 1..99 (checked once the device is there: a host-only plan says -3 first)
        assert L.fri_hip_encode_image420_symbols(P._h, api._p(px), q, None, None, None, None, None) == -3
    P.close()
    thin = fa.Plan420(None, 7, 64)  # no SSIM window: refused before the device check
    assert L.fri_hip_search_quality_ssim420(thin._h, api._p(px), 0.9, C.byref(qual), C.byref(v)) == -1
    assert L.fri_hip_search_quality_ssim420_dev(thin._h, 16, 0.9, C.byref(qual), C.byref(v), None) == -1
    thin.close()


# ---- the restatement against literal loops -------------------------------------------------------------------------------------------------------------------------

def _literal_split(img, w, h):
    p = ycc(img).reshape(h, w, 3).astype(int)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    y = np.zeros((h, w), np.uint8)
    cb, cr = np.zeros((ch, cw), np.uint8), np.zeros((ch, cw), np.uint8)
    for yy in range(h):
        for xx in range(w):
            y[yy, xx] = p[yy, xx, 0]
    for j in range(ch):
        for i in range(cw):
            xs, ys = (2 * i, min(2 * i + 1, w - 1)), (2 * j, min(2 * j + 1, h - 1))
            cb[j, i] = (sum(int(p[b, a, 1]) for a in xs for b in ys) + 2) >> 2
            cr[j, i] = (sum(int(p[b, a, 2]) for a in xs for b in ys) + 2) >> 2
    return y, cb, cr


def _literal_merge(y, cb, cr, w, h):
    ch, cw = cb.shape
    out = np.zeros((h, w, 3), np.uint8)
    for yy in range(h):
        for xx in range(w):
            i, j = xx >> 1, yy >> 1
            i2 = min(max(i + 1 if xx & 1 else i - 1, 0), cw - 1)
            j2 = min(max(j + 1 if yy & 1 else j - 1, 0), ch - 1)
            up = [(9 * int(p[j, i]) + 3 * int(p[j, i2]) + 3 * int(p[j2, i]) + int(p[j2, i2]) + 8) >> 4 for p in (cb, cr)]
            out[yy, xx] = inverse_ycc(np.array([[y[yy, xx], up[0], up[1]]], np.uint8))[0]
    return out.reshape(-1)


@pytest.mark.parametrize("shape", [(1, 1), (2, 1), (1, 2), (3, 5), (5, 3), (4, 4), (7, 6), (17, 9), (1, 9), (9, 1)])
def test_restatement_equals_literal_loops(shape):
    w, h = shape
    img = gen_image("noise", w, h, 3, w * 31 + h)
    got, want = split420(img, w, h), _literal_split(img, w, h)
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a, b)
    rng = np.random.default_rng(w * 100 + h)
    cw, ch = chroma_shape(w, h)
    y, cb, cr = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (ch, cw), (ch, cw)))  # any planes, saturated ones included: the decoder's come from K3
    assert np.array_equal(merge420(y, cb, cr, w, h), _literal_merge(y, cb, cr, w, h))
    # a constant plane stays constant (the filter's weights sum to 16), and the filter stays inside 0..255
    assert (upsample420(np.full((ch, cw), 201, np.uint8), w, h) == 201).all()
    up = upsample420(cb, w, h)
    assert up.shape == (h, w) and up.min() >= 0 and up.max() <= 255


# ---- the emitter (FRI_EMIT_420) ------------------------------------------------------------------------------------------------------------------------------------

def _mdat(frv):
    return struct.unpack("<I", frv[12:16])[0]


def _plane_arrays(plane, quality):
    """the oracle's arrays of one plane coded as a C = 1 image, and its symbol stream"""
    ph, pw = plane.shape
    centers, coefs, bucket, pred, hist, oob, vp, wp = rate_model.oracle_arrays(np.ascontiguousarray(plane).reshape(-1), pw, ph, 1, quality)
    assert not oob.any()
    sym, bk = emit.channel_symbols(centers, coefs[0], bucket[0], pred[0])
    return dict(w=pw, h=ph, centers=centers, coefs=coefs[0], hist=hist[0], vp=vp[0], wp=wp[0], stream=(bk.astype(np.uint16) << 10) | sym)


def _file420(w, h, quality, kind="smooth", seed=3):
    img = correlated_image(w, h, seed) if kind == "correlated" else gen_image(kind, w, h, 3, seed)
    ch = [_plane_arrays(p, quality) for p in split420(img, w, h)]
    streams = np.concatenate([c["stream"] for c in ch])
    hist, vp, wp = (np.stack([c[k] for c in ch]) for k in ("hist", "vp", "wp"))
    frv = emit.encode_image_from_streams(w, h, streams, hist, vp, wp, quality=quality, ycbcr=True, n_luma=ch[0]["stream"].size)
    return frv, ch, (streams, hist, vp, wp)


@pytest.mark.parametrize("shape", [(160, 120), (97, 257)])
@pytest.mark.parametrize("quality", [1, 50, 99])
def test_emitter_round_trip_and_container(shape, quality):
    w, h = shape
    frv, ch, _ = _file420(w, h, quality)
    # the metadata word: colour space YCbCr, bits 1 and 2 set, bit 0 clear, the quality in bits 8..14
    assert _mdat(frv) == 0xC0000000 | VARIANT << 28 | quality << 8 | 0x4 | 0x2
    assert frv[:4] == b"frif" and struct.unpack("<II", frv[4:12]) == (h, w) and frv[-2:] == b"\xff\xdf"
    # each channel's bytes are the bytes the same stream gets in a C = 1 file of its own lattice
    body = b""
    for c in ch:
        single = emit.encode_image_from_streams(c["w"], c["h"], c["stream"], c["hist"], c["vp"], c["wp"], quality=quality)
        body += single[16:-2]
    assert frv[16:-2] == body
    # the product decoder gives the three planes back exactly and reports the flag
    d = emit.decode_image(frv)
    assert d.s420 is True and d.ycbcr is True and d.rct is False and d.quality == quality and d[:3] == (w, h, 3)
    assert np.array_equal(d[3], ch[0]["centers"])
    for got, c in zip(d[4], ch):
        assert got.shape == c["coefs"].shape and np.array_equal(got, c["coefs"])
    sub = fa.Plan420(None, w, h)
    assert d[4][0].shape[0] == sub.luma.num_cells and d[4][1].shape[0] == sub.chroma.num_cells
    # through the C ABI: the size query, a buffer one element short, the exact buffer
    L = emit.load_library()
    data = np.frombuffer(frv, np.uint8)
    info = np.zeros(4, np.uint32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.fri_emit_decode_image(P(data), data.size, P(info), None, 0, None, None, 0) == -3
    assert [int(x) for x in info] == [w, h, 3 | emit.YCBCR | emit.S420 | emit.QUALITY(quality), sub.luma.num_cells]
    buf = np.zeros(sub.coef_count, np.int32)
    info[:] = 0
    assert L.fri_emit_decode_image(P(data), data.size, P(info), P(buf), buf.size - 1, None, None, 0) == -3
    assert int(info[2]) == 3 | emit.YCBCR | emit.S420 | emit.QUALITY(quality) and int(info[3]) == sub.luma.num_cells
    assert L.fri_emit_decode_image(P(data), data.size, P(info), P(buf), buf.size, None, None, 0) == 0
    assert np.array_equal(buf, np.concatenate([c["coefs"].reshape(-1) for c in ch]))
    sub.close()


def test_flag_refusals():
    w, h, q = 160, 120, 50
    frv, ch, (streams, hist, vp, wp) = _file420(w, h, q)
    L = emit.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.empty(streams.size * 4 + 100000, np.uint8)
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    n_luma = ch[0]["stream"].size
    h_, vp_, wp_ = np.ascontiguousarray(hist, np.uint32), np.ascontiguousarray(vp), np.ascontiguousarray(wp)

    def from_streams(arg, n_symbols=n_luma):
        return L.fri_emit_encode_image_from_streams(w, h, arg, P(streams), n_symbols, P(h_), P(vp_), P(wp_), P(out), out.size, C.addressof(n), err, 256)

    assert emit.S420 == 0x800
    good = 3 | emit.YCBCR | emit.S420 | emit.QUALITY(q)
    assert from_streams(good) == 0 and out[: n.value].tobytes() == frv
    for arg in (3 | emit.S420 | emit.QUALITY(q),                    # without FRI_EMIT_YCBCR
                3 | emit.YCBCR | emit.S420,                          # without a quality
                3 | emit.YCBCR | emit.S420 | emit.RCT | emit.QUALITY(q), 3 | emit.S420 | emit.RCT,  # with FRI_EMIT_RCT
                1 | emit.YCBCR | emit.S420 | emit.QUALITY(q), 1 | emit.S420,  # with one channel
                3 | emit.YCBCR | emit.S420 | emit.QUALITY(100), 3 | emit.S420):
        assert from_streams(arg) == -1, hex(arg)
    # an n_symbols that is not the W x H lattice's count
    for bad in (n_luma - 1, n_luma + 1, ch[1]["stream"].size, streams.size // 3):
        assert from_streams(good, bad) == -1, bad
    # the array route does not take the flag
    cc, co, b = np.ascontiguousarray(ch[0]["centers"]), np.zeros((3,) + ch[0]["coefs"].shape, np.int32), np.zeros((3,) + ch[0]["coefs"].shape, np.uint8)
    for arg in (good, 3 | emit.S420 | emit.QUALITY(q), 3 | emit.S420):
        assert L.fri_emit_encode_image(w, h, arg, P(cc), len(cc), P(co), P(b), P(co), P(h_), P(vp_), P(wp_), P(out), out.size, C.addressof(n), err, 256) == -1
        data = np.frombuffer(frv, np.uint8)
        assert L.fri_emit_check_image(P(data), data.size, arg, P(cc), len(cc), P(co), P(b), P(co), err, 256) == -1


def test_invalid_420_metadata_and_ignored_bit():
    w, h, q = 97, 257, 40
    frv, ch, _ = _file420(w, h, q)
    m = _mdat(frv)

    def with_mdat(data, word):
        odd = bytearray(data)
        odd[12:16] = struct.pack("<I", word)
        return bytes(odd)

    with pytest.raises(emit.EmitError, match="Invalid metadata"):  # bit 2 without bit 1 in a YCbCr file
        emit.decode_image(with_mdat(frv, m & ~0x2))
    with pytest.raises(emit.EmitError, match="Invalid metadata"):  # bit 2 with bit 0
        emit.decode_image(with_mdat(frv, m | 0x1))
    with pytest.raises(emit.EmitError, match="Invalid metadata"):
        emit.decode_image(with_mdat(frv, (m | 0x1) & ~0x2))
    # bit 2 of a Luma or RGB file stays ignored: the committed files decode as before with the bit flipped
    for name in ("emit_mixed_96x257_rgb.frv", "emit_mixed_129x65_luma.frv"):
        gold = open(os.path.join(ROOT, "tests", "golden", name), "rb").read()
        assert _mdat(gold) >> 30 in (1, 2) and not _mdat(gold) & 0x4
        a, b = emit.decode_image(gold), emit.decode_image(with_mdat(gold, _mdat(gold) | 0x4))
        assert b.s420 is False and b.ycbcr is False and b.rct is False and a[:3] == b[:3]
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    # a plain YCbCr file (bit 1 alone) is no 4:2:0 file
    centers, coefs, bucket, pred, hist, oob, vp, wp = rate_model.oracle_arrays(ycc(gen_image("smooth", 160, 120, 3, 3)), 160, 120, 3, q)
    d = emit.decode_image(emit.encode_image(160, 120, centers, coefs, bucket, pred, hist, vp, wp, quality=q, ycbcr=True))
    assert d.ycbcr is True and d.s420 is False and np.array_equal(d[4], coefs)


def test_estimate_is_within_24_bytes_per_channel_of_a_420_file():
    """the size model over the three histograms as one C = 3 image: one 18-byte header, one final rounding (the bound of tests/test_ycbcr_host.py)"""
    w, h = 320, 240
    for q in (1, 50, 90, 99):
        frv, ch, (streams, hist, vp, wp) = _file420(w, h, q, "correlated", 5)
        est = rate_model.estimate_image(hist, np.zeros(3, np.uint64))
        assert abs(est - len(frv)) <= 24 * 3, (q, est, len(frv))
