"""RGBA coding, host side (include/fri_hip.h "RGBA: a lossless alpha plane", FRI_EMIT_ALPHA): the numpy restatement, the emitter's flag - container bytes, round
trip, refusals, invalid metadata - and the host-only RGBA plan. CPU only."""
import ctypes as C
import functools
import os
import struct

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd import api
from frave_amd.api import PlanRGBA  # noqa: F401  (without the feature the module fails here)
from tests import rate_model
from tests.alpha_ref import ALPHA_CLEAN, ALPHA_KEEP, alpha_plane, cleaned, merge_rgba, rgba_image, split_rgba
from tests.common import KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS, gen_image
from tests.test_rct_host import correlated_image, rct
from tests.ycbcr_ref import ycc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = 1  # TameTwindragon
W, H = 96, 65
# (name, what the colour planes hold, the emitter's arguments, colour space field, metadata bits 0..2, quality of the colour planes' matrix)
MODES = [("plain", lambda p: p, dict(), 2, 0x0, 100), ("rct", rct, dict(rct=True), 3, 0x1, 100), ("ycbcr50", ycc, dict(ycbcr=True, quality=50), 3, 0x2, 50)]
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (3, 5), (17, 9), (64, 48), (1, 70), (70, 1)])
@pytest.mark.parametrize("kind", ["zeros", "opaque", "random", "runs"])
def test_restatement_round_trips_and_clean_zeroes_exactly_the_transparent_colour(shape, kind):
    w, h = shape
    x = rgba_image(gen_image("noise", w, h, 3, w + 7 * h), alpha_plane(kind, w, h, w * h))
    rgb, a = split_rgba(x, w, h, ALPHA_KEEP)
    assert rgb.shape == (h, w, 3) and a.shape == (h, w)
    assert np.array_equal(rgb, x[:, :, :3]) and np.array_equal(a, x[:, :, 3])
    assert np.array_equal(merge_rgba(rgb, a, w, h), x.reshape(-1))
    # CLEAN against a literal per-pixel loop: the alpha is untouched, the colour is 0 where A == 0 and untouched elsewhere
    crgb, ca = split_rgba(x, w, h, ALPHA_CLEAN)
    assert np.array_equal(ca, a)
    for yy in range(h):
        for xx in range(w):
            want = (0, 0, 0) if x[yy, xx, 3] == 0 else tuple(x[yy, xx, :3])
            assert tuple(crgb[yy, xx]) == want
    assert np.array_equal(cleaned(x, w, h), merge_rgba(crgb, ca, w, h))
    if kind == "opaque":
        assert np.array_equal(crgb, rgb)
    if kind == "zeros":
        assert not crgb.any()
    with pytest.raises(AssertionError):
        split_rgba(x, w, h, 2)


# ---- the emitter (FRI_EMIT_ALPHA) ----------------------------------------------------------------------------------------------------------------------------

def _mdat(frv):
    return struct.unpack("<I", frv[12:16])[0]


def _with_mdat(data, word):
    odd = bytearray(data)
    odd[12:16] = struct.pack("<I", word)
    return bytes(odd)


def _streams(centers, coefs, bucket, pred):
    out = []
    for ch in range(coefs.shape[0]):
        sym, bk = emit.channel_symbols(centers, coefs[ch], bucket[ch], pred[ch])
        out.append((bk.astype(np.uint16) << 10) | sym)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _inputs(mode):
    """the four channels' inputs from oracle planes of a 96 x 65 RGBA image: lossless alpha holding runs of 0 and 255 and a ramp; the colour planes of `mode`"""
    name, forward, kwargs, cs, bits, quality = next(m for m in MODES if m[0] == mode)
    rgb, a = correlated_image(W, H, 11), alpha_plane("runs", W, H)
    assert (a == 0).any() and (a == 255).any() and np.unique(a).size > 16
    centers, coefs, bucket, pred, hist, oob, vp, wp = rate_model.oracle_arrays(np.ascontiguousarray(forward(rgb)).reshape(-1), W, H, 3, quality)
    # the alpha plane: lossless, and predicted with parameters of its own (dyadic like the known-answer ones), so that they must land in the fourth channel
    from oracle import fri_oracle

    avp, awp = (KAT_VALUE_PARAMS * np.float32(0.5)).astype(np.float32), (KAT_WIDTH_PARAMS * np.float32(2)).astype(np.float32)
    A = fri_oracle.Wavelet(a.reshape(-1), H, W, 1)
    A.quantize(np.ones(32, np.int32))
    acenters, acoefs = A.centers(), A.coefficients()
    ab, ap, ah, aoob = A.predict(0, avp, awp)
    A.close()
    abucket, apred, ahist, avp, awp = ab[None], ap[None], ah[None], avp[None], awp[None]
    assert not oob.any() and not aoob and np.array_equal(centers, acenters)
    colour = dict(streams=_streams(centers, coefs, bucket, pred), hist=hist, vp=vp, wp=wp, coefs=coefs)
    alpha = dict(streams=_streams(acenters, acoefs, abucket, apred), hist=ahist, vp=avp, wp=awp, coefs=acoefs)
    four = tuple(np.concatenate([colour[k], alpha[k]]) for k in ("streams", "hist", "vp", "wp"))
    return colour, alpha, four, centers


@pytest.mark.parametrize("mode", [m[0] for m in MODES])
def test_alpha_file_is_the_colour_file_with_bit_3_and_the_luma_channel_behind(mode):
    name, forward, kwargs, cs, bits, quality = next(m for m in MODES if m[0] == mode)
    colour, alpha, (streams, hist, vp, wp), centers = _inputs(mode)
    assert streams.shape[0] == 4 and hist.shape == (4, 10, 1024) and vp.shape == (4, 3, 6)
    frv = emit.encode_image_from_streams(W, H, streams, hist, vp, wp, alpha=True, **kwargs)
    rgb_file = emit.encode_image_from_streams(W, H, colour["streams"], colour["hist"], colour["vp"], colour["wp"], **kwargs)
    luma_file = emit.encode_image_from_streams(W, H, alpha["streams"], alpha["hist"], alpha["vp"], alpha["wp"])
    q = kwargs.get("quality", 0)
    assert _mdat(rgb_file) == cs << 30 | VARIANT << 28 | q << 8 | bits and _mdat(luma_file) == 1 << 30 | VARIANT << 28
    assert rgb_file[-2:] == b"\xff\xdf" and luma_file[-2:] == b"\xff\xdf"
    want = _with_mdat(rgb_file, _mdat(rgb_file) | 0x8)[:-2] + luma_file[16:-2] + rgb_file[-2:]
    assert frv == want
    # the decoder returns the four oracle planes and the flag
    d = emit.decode_image(frv)
    assert d.alpha is True and d[:3] == (W, H, 3) and d.rct is bool(kwargs.get("rct")) and d.ycbcr is bool(kwargs.get("ycbcr")) and d.quality == q and d.s420 is False
    assert np.array_equal(d[3], centers)
    assert d[4].shape == (4,) + colour["coefs"].shape[1:]
    assert np.array_equal(d[4][:3], colour["coefs"]) and np.array_equal(d[4][3], alpha["coefs"][0])
    # the colour file itself is no alpha file
    plain = emit.decode_image(rgb_file)
    assert plain.alpha is False and plain[4].shape[0] == 3
    # through the C ABI: the size query, a buffer one element short (-3 with info filled), the exact buffer
    L = emit.load_library()
    data = np.frombuffer(frv, np.uint8)
    f = len(centers)
    flags = 3 | emit.FRI_EMIT_ALPHA | (emit.RCT if kwargs.get("rct") else 0) | (emit.YCBCR if kwargs.get("ycbcr") else 0) | emit.QUALITY(q)
    info = np.zeros(4, np.uint32)
    assert L.fri_emit_decode_image(P(data), data.size, P(info), None, 0, None, None, 0) == -3
    assert [int(x) for x in info] == [W, H, flags, f]
    buf = np.zeros(4 * f * 512, np.int32)
    info[:] = 0
    assert L.fri_emit_decode_image(P(data), data.size, P(info), P(buf), buf.size - 1, None, None, 0) == -3
    assert [int(x) for x in info] == [W, H, flags, f]
    assert L.fri_emit_decode_image(P(data), data.size, P(info), P(buf), 3 * f * 512, None, None, 0) == -3  # (room for the colour planes only)
    assert L.fri_emit_decode_image(P(data), data.size, P(info), P(buf), buf.size, None, None, 0) == 0
    assert np.array_equal(buf.reshape(4, f, 512), d[4])


def test_flag_refusals():
    colour, alpha, (streams, hist, vp, wp), centers = _inputs("ycbcr50")
    L = emit.load_library()
    out = np.empty(streams.size * 4 + 200000, np.uint8)
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    n_symbols = streams.shape[1]
    st, h_, vp_, wp_ = (np.ascontiguousarray(x) for x in (streams, hist, vp, wp))

    def from_streams(arg, w=W, h=H):
        return L.fri_emit_encode_image_from_streams(w, h, arg, P(st), n_symbols, P(h_), P(vp_), P(wp_), P(out), out.size, C.addressof(n), err, 256)

    assert emit.FRI_EMIT_ALPHA == 0x1000
    for good in (3 | emit.FRI_EMIT_ALPHA, 3 | emit.FRI_EMIT_ALPHA | emit.RCT, 3 | emit.FRI_EMIT_ALPHA | emit.QUALITY(50), 3 | emit.FRI_EMIT_ALPHA | emit.YCBCR | emit.QUALITY(50)):
        assert from_streams(good) == 0, hex(good)
        assert _mdat(out[: n.value].tobytes()) & 0x8
    for arg in (1 | emit.FRI_EMIT_ALPHA, 1 | emit.FRI_EMIT_ALPHA | emit.QUALITY(50),  # with one channel
                3 | emit.FRI_EMIT_ALPHA | emit.YCBCR | emit.S420 | emit.QUALITY(50), 3 | emit.FRI_EMIT_ALPHA | emit.S420,  # with FRI_EMIT_420
                4 | emit.FRI_EMIT_ALPHA, 4, 2 | emit.FRI_EMIT_ALPHA,  # the flag rides on three channels
                3 | emit.FRI_EMIT_ALPHA | emit.YCBCR, 3 | emit.FRI_EMIT_ALPHA | emit.RCT | emit.QUALITY(50), 3 | emit.FRI_EMIT_ALPHA | emit.QUALITY(100)):  # what is refused without it
        assert from_streams(arg) == -1, hex(arg)
    with pytest.raises(emit.EmitError):  # the binding: two planes with the flag are one channel with it
        emit.encode_image_from_streams(W, H, streams[:2], hist[:2], vp[:2], wp[:2], alpha=True)
    # the array route and the check do not take the flag
    frv = emit.encode_image_from_streams(W, H, streams, hist, vp, wp, alpha=True, ycbcr=True, quality=50)
    data = np.frombuffer(frv, np.uint8)
    cc = np.ascontiguousarray(centers)
    co, b = np.zeros((4,) + colour["coefs"].shape[1:], np.int32), np.zeros((4,) + colour["coefs"].shape[1:], np.uint8)
    for arg in (3 | emit.FRI_EMIT_ALPHA, 3 | emit.FRI_EMIT_ALPHA | emit.RCT, 3 | emit.FRI_EMIT_ALPHA | emit.YCBCR | emit.QUALITY(50), 1 | emit.FRI_EMIT_ALPHA):
        assert L.fri_emit_encode_image(W, H, arg, P(cc), len(cc), P(co), P(b), P(co), P(h_), P(vp_), P(wp_), P(out), out.size, C.addressof(n), err, 256) == -1, hex(arg)
        assert L.fri_emit_check_image(P(data), data.size, arg, P(cc), len(cc), P(co), P(b), P(co), err, 256) == -1, hex(arg)


def test_invalid_alpha_metadata_and_ignored_bit():
    for mode in ("plain", "ycbcr50"):
        name, forward, kwargs, cs, bits, quality = next(m for m in MODES if m[0] == mode)
        colour, alpha, (streams, hist, vp, wp), centers = _inputs(mode)
        frv = emit.encode_image_from_streams(W, H, streams, hist, vp, wp, alpha=True, **kwargs)
        m = _mdat(frv)
        assert m & 0x8 and not m & 0x4
        with pytest.raises(emit.EmitError, match="Invalid metadata"):  # bit 3 together with bit 2
            emit.decode_image(_with_mdat(frv, m | 0x4))
        L = emit.load_library()
        odd = np.frombuffer(_with_mdat(frv, m | 0x4), np.uint8)
        info = np.zeros(4, np.uint32)
        err = C.create_string_buffer(256)
        assert L.fri_emit_decode_image(P(odd), odd.size, P(info), None, 0, None, err, 256) == -2 and err.value == b"Invalid metadata"
        # without bit 3 the fourth channel is one too many; a three-channel file with bit 3 is one short
        with pytest.raises(emit.EmitError, match="Malformed image bytes"):
            emit.decode_image(_with_mdat(frv, m & ~0x8))
        rgb_file = emit.encode_image_from_streams(W, H, colour["streams"], colour["hist"], colour["vp"], colour["wp"], **kwargs)
        with pytest.raises(emit.EmitError, match="Malformed image bytes"):
            emit.decode_image(_with_mdat(rgb_file, _mdat(rgb_file) | 0x8))
    # bit 3 of a Luma file stays ignored, as all flag bits of Luma files are: the committed file decodes as before with the bit flipped
    gold = open(os.path.join(ROOT, "tests", "golden", "emit_mixed_129x65_luma.frv"), "rb").read()
    assert _mdat(gold) >> 30 == 1 and not _mdat(gold) & 0x8
    for extra in (0x8, 0x8 | 0x4):
        a, b = emit.decode_image(gold), emit.decode_image(_with_mdat(gold, _mdat(gold) | extra))
        assert b.alpha is False and b.s420 is False and a[:3] == b[:3] == (129, 65, 1)
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    # and the committed RGB file has no alpha
    rgb_gold = emit.decode_image(open(os.path.join(ROOT, "tests", "golden", "emit_mixed_96x257_rgb.frv"), "rb").read())
    assert rgb_gold.alpha is False and rgb_gold[4].shape[0] == 3


# ---- the host-only plan ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(64, 48), (97, 61), (3, 5), (1, 700), (333, 251)])
def test_host_only_plan_owns_two_ordinary_plans_on_one_lattice(shape):
    w, h = shape
    R = fa.PlanRGBA(None, w, h)
    for view, c in ((R.colour, 3), (R.alpha, 1)):
        ref = fa.Plan(None, w, h, c)
        assert (view.width, view.height, view.channels) == (w, h, c)
        assert view.num_cells == ref.num_cells and view.num_some == ref.num_some and view.pixel_bytes == ref.pixel_bytes
        assert np.array_equal(view.centers(), ref.centers()) and np.array_equal(view.valid_mask(), ref.valid_mask())
        ref.close()
    assert R.colour.num_cells == R.alpha.num_cells == R.num_cells and R.colour.num_some == R.alpha.num_some == R.num_some
    assert np.array_equal(R.colour.centers(), R.alpha.centers())
    assert R.pixel_bytes == 4 * w * h and R.coef_count == 4 * R.num_cells * 512
    R.close()


def test_host_only_plan_refuses_to_compute_and_argument_errors():
    w, h = 64, 48
    R = fa.PlanRGBA(None, w, h)
    px = np.zeros((h, w, 4), np.uint8)
    calls = [lambda: R.split_rgba_dev(16, 16, 16), lambda: R.split_rgba_dev(16, 16, 16, clean=api.ALPHA_CLEAN), lambda: R.merge_rgba_dev(16, 16, 16),
             lambda: R.encode_symbols_rgba_dev(16, 16, 16, 16, 16), lambda: R.encode_image_rgba_symbols(px), lambda: R.encode_image_rgba_symbols(px, clean=api.ALPHA_CLEAN),
             lambda: R.decode_image_rgba(np.zeros(R.coef_count, np.int32)), lambda: R.colour.transform_quant(np.zeros((h, w, 3), np.uint8)),
             lambda: R.alpha.transform_quant(np.zeros((h, w), np.uint8))]
    for call in calls:
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -3
    R.close()
    assert (api.ALPHA_KEEP, api.ALPHA_CLEAN) == (0, 1)
    L = api.load_library()
    hd = C.c_void_p()
    for ww, hh in ((0, 10), (10, 0)):
        assert L.fri_hip_plan_rgba_create(None, ww, hh, C.byref(hd)) == -1
    assert L.fri_hip_plan_rgba_create(None, 8, 8, None) == -1
    with pytest.raises(fa.FriHipError):  # larger than the pixel index of an ordinary plan
        fa.PlanRGBA(None, 65536, 65536)
    assert L.fri_hip_plan_rgba_destroy(None) == 0 and L.fri_hip_plan_rgba_colour(None) is None and L.fri_hip_plan_rgba_alpha(None) is None
    assert L.fri_hip_split_rgba_dev(None, 16, 0, 16, 16, None) == -1 and L.fri_hip_merge_rgba_dev(None, 16, 16, 16, None) == -1
    # four channels on an ordinary plan stay refused: alpha lives in a plan of its own
    with pytest.raises(fa.FriHipError) as e:
        fa.Plan(None, 10, 10, 4)
    assert e.value.code == -1
