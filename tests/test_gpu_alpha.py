"""RGBA coding on the device (fri_hip_plan_rgba, K9: k9_alpha.hip) against tests/alpha_ref.py, the existing plans and the CPU oracle:

- the split (both modes) and the merge exactly equal to the restatement, over whole and ragged pixel counts (N mod 16 = 6, 15, 9, 0, 12, 12, 1, 0, and N < 16), three
  kinds of alpha plane, device pointers on and one byte off a 256-byte boundary, between guard bytes;
- fri_hip_encode_image_rgba_symbols and fri_hip_encode_symbols_rgba_dev against the existing route on an ordinary C = 3 and an ordinary C = 1 plan;
- end to end through the emitter, its decoder and fri_hip_decode_image_rgba: lossless files return the input (the cleaned input with CLEAN), a YCbCr file the
  oracle's midpoint raster of the split colour and the exact alpha;
- graph capture of the raster kernels; the alpha plan's dequantiser setting survives a decode;
- fri_driver encode-file of a PAM and decode-file back to one."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from frave_amd.api import ALPHA_CLEAN, ALPHA_KEEP, PlanRGBA  # noqa: F401  (without the feature the module fails here)
from tests.alpha_ref import alpha_plane, cleaned, merge_rgba, rgba_image, split_rgba
from tests.common import gen_image
from tests.oracle_ref import MIDPOINT, MULTIPLY, REFERENCE
from tests.test_gpu_instances import Guarded
from tests.test_rct_host import correlated_image
from tests.ycbcr_ref import COLOUR_YCBCR, oracle_coefficients_ycc, oracle_raster_ycc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELAXED = 2  # hipStreamCaptureModeRelaxed
SHAPES = [(2, 3), (3, 5), (17, 9), (64, 48), (1, 700), (700, 1), (1023, 767), (1920, 1080)]
KINDS = ["zeros", "opaque", "random"]
COLOUR_NONE, COLOUR_RCT = 0, 1
# (name, colour transform of the colour plan, quality of its matrix or 0 for lossless, the emitter's arguments)
MODES = [("plain", COLOUR_NONE, 0, dict()), ("rct", COLOUR_RCT, 0, dict(rct=True)), ("ycbcr50", COLOUR_YCBCR, 50, dict(ycbcr=True, quality=50))]


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


def test_shapes_cover_every_tail():
    assert [w * h % 16 for w, h in SHAPES] == [6, 15, 9, 0, 12, 12, 1, 0] and SHAPES[0][0] * SHAPES[0][1] < 16 and SHAPES[1][0] * SHAPES[1][1] < 16


@functools.lru_cache(maxsize=4)
def _reference(kind, w, h):
    """(pixels, per mode the split's colour raster and alpha plane, the cleaned pixels) of the restatement"""
    a = alpha_plane(kind, w, h, w + h)
    if kind == "random" and a.size >= 1000:
        assert 0.2 < (a == 0).mean() < 0.3
    img = rgba_image(gen_image("noise", w, h, 3, 7), a)
    flat = np.ascontiguousarray(img).reshape(-1)
    split = {clean: tuple(np.ascontiguousarray(p).reshape(-1) for p in split_rgba(img, w, h, clean)) for clean in (ALPHA_KEEP, ALPHA_CLEAN)}
    return flat, split


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_and_merge_equal_the_restatement(ctx, shape, kind):
    import torch

    import frave_amd as fa

    w, h = shape
    n = w * h
    img, split = _reference(kind, w, h)
    R = fa.PlanRGBA(ctx, w, h)
    assert R.pixel_bytes == 4 * n
    for offset in (0, 1):
        src = Guarded(torch, 4 * n, offset=offset, salt=1)
        src.put(torch, [img])
        for clean in (ALPHA_KEEP, ALPHA_CLEAN):
            want_rgb, want_a = split[clean]
            rgb = Guarded(torch, 3 * n, offset=offset, salt=2)
            a = Guarded(torch, n, offset=offset, salt=3)
            R.split_rgba_dev(src.ptr, rgb.ptr, a.ptr, clean=clean)
            (got_rgb,), intact_rgb = rgb.get(torch)
            (got_a,), intact_a = a.get(torch)
            assert intact_rgb and intact_a, "the split wrote outside its buffers"
            bad = got_rgb != want_rgb
            assert not bad.any(), (shape, kind, offset, clean, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
            bad = got_a != want_a
            assert not bad.any(), (shape, kind, offset, clean, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
            # the merge of those planes, between guards
            back = Guarded(torch, 4 * n, offset=offset, salt=4)
            R.merge_rgba_dev(rgb.ptr, a.ptr, back.ptr)
            (got,), intact = back.get(torch)
            assert intact, "the merge wrote outside its raster"
            want = merge_rgba(want_rgb, want_a, w, h)
            bad = got != want
            assert not bad.any(), (shape, kind, offset, clean, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
            if clean == ALPHA_KEEP:
                assert np.array_equal(got, img)
            # the inputs come back intact
            (again_rgb,), ok_rgb = rgb.get(torch)
            (again_a,), ok_a = a.get(torch)
            assert ok_rgb and ok_a and np.array_equal(again_rgb, want_rgb) and np.array_equal(again_a, want_a)
        (again,), ok = src.get(torch)
        assert ok and np.array_equal(again, img)
    for bad_clean in (2, -1, 255):
        with pytest.raises(fa.FriHipError) as e:
            R.split_rgba_dev(src.ptr, rgb.ptr, a.ptr, clean=bad_clean)
        assert e.value.code == -1
    R.close()


def _image(w, h, seed, kind="random"):
    return rgba_image(correlated_image(w, h, seed), alpha_plane(kind, w, h, seed))


def _plan(ctx, w, h, transform):
    import frave_amd as fa

    R = fa.PlanRGBA(ctx, w, h)
    R.set_stream_order()
    R.colour.set_colour_transform(transform)
    return R


@pytest.mark.parametrize("shape", [(333, 251), (512, 384)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_is_the_existing_route_on_the_split_raster_and_the_alpha_plane(ctx, shape):
    import torch

    import frave_amd as fa

    w, h = shape
    img = _image(w, h, 30)
    for name, transform, quality, _ in MODES:
        qm = fa.quality_matrix(quality) if quality else np.ones(32, np.int32)
        R = _plan(ctx, w, h, transform)
        for clean in (ALPHA_KEEP, ALPHA_CLEAN):
            rgb, a = split_rgba(img, w, h, clean)
            sym, vp, wp, hist, oob = R.encode_image_rgba_symbols(img, qm, clean=clean)
            assert sym.shape == (4, R.num_some) and hist.shape == (4, 10, 1024) and vp.shape == wp.shape == (4, 3, 6) and oob.shape == (4,)
            Q3 = fa.Plan(ctx, w, h, 3)
            Q3.set_stream_order()
            Q3.set_colour_transform(transform)
            csym, cvp, cwp, chist, coob = Q3.encode_image_symbols(rgb, qm, fit=True)
            Q3.close()
            Q1 = fa.Plan(ctx, w, h, 1)
            Q1.set_stream_order()
            asym, avp, awp, ahist, aoob = Q1.encode_image_symbols(a, np.ones(32, np.int32), fit=True)
            Q1.close()
            for got, colour, alpha in ((sym, csym, asym), (vp, cvp, avp), (wp, cwp, awp), (hist, chist, ahist), (oob, coob, aoob)):
                assert np.array_equal(got[:3], colour), (name, clean)
                assert np.array_equal(got[3:], alpha), (name, clean)
            # the device form gives the same bits from device buffers, and with fit = 0 it reads all four channels' parameters
            d_px = torch.from_numpy(np.ascontiguousarray(img).reshape(-1).copy()).cuda()
            d_params = torch.zeros(4 * 36, dtype=torch.float32, device="cuda")
            d_sym = torch.zeros(4 * R.num_some, dtype=torch.int16, device="cuda")
            d_hist = torch.zeros(4 * 10 * 1024, dtype=torch.int32, device="cuda")
            d_oob = torch.zeros(8, dtype=torch.int64, device="cuda")
            for fit in (True, False):  # (the second pass reads the parameters the first one fitted)
                d_sym.zero_(), d_hist.zero_(), d_oob.fill_(5)
                R.encode_symbols_rgba_dev(d_px.data_ptr(), d_params.data_ptr(), d_sym.data_ptr(), d_hist.data_ptr(), d_oob.data_ptr(), d_oob.data_ptr() + 32 if fit else None,
                                          clean=clean, qmatrix=qm, fit=fit)
                torch.cuda.synchronize()
                assert np.array_equal(d_sym.cpu().numpy().view(np.uint16).reshape(4, -1), sym), (name, clean, fit)
                assert np.array_equal(d_hist.cpu().numpy().view(np.uint32).reshape(4, 10, 1024), hist), (name, clean, fit)
                params = d_params.cpu().numpy().reshape(4, 2, 3, 6)
                assert np.array_equal(params[:, 0], vp) and np.array_equal(params[:, 1], wp), (name, clean, fit)
                counts = d_oob.cpu().numpy().astype(np.uint64)
                assert np.array_equal(counts[:4], oob) and (not fit or not counts[4:].any())
            assert np.array_equal(d_px.cpu().numpy(), np.ascontiguousarray(img).reshape(-1))
        for bad_clean in (2, -1):
            with pytest.raises(fa.FriHipError) as e:
                R.encode_image_rgba_symbols(img, qm, clean=bad_clean)
            assert e.value.code == -1
        R.close()
    # without the stream order on both inner plans the encode is refused
    R = fa.PlanRGBA(ctx, w, h)
    R.colour.set_stream_order()
    with pytest.raises(fa.FriHipError) as e:
        R.encode_image_rgba_symbols(img)
    assert e.value.code == -1
    R.close()


@pytest.mark.parametrize("shape", [(200, 120), (333, 251)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_end_to_end_through_the_emitter(ctx, oracle, shape):
    import frave_amd as fa
    import frave_amd.emit as emit

    w, h = shape
    img = _image(w, h, 41)
    flat = np.ascontiguousarray(img).reshape(-1)
    for name, transform, quality, kwargs in MODES:
        qm = fa.quality_matrix(quality) if quality else np.ones(32, np.int32)
        R = _plan(ctx, w, h, transform)
        R.colour.set_dequantiser(MIDPOINT if quality else REFERENCE)
        for clean in (ALPHA_KEEP, ALPHA_CLEAN):
            sym, vp, wp, hist, oob = R.encode_image_rgba_symbols(img, qm, clean=clean)
            assert not oob.any()
            frv = emit.encode_image_from_streams(w, h, sym, hist, vp, wp, alpha=True, **kwargs)
            d = emit.decode_image(frv)
            assert d.alpha and d[:3] == (w, h, 3) and d.rct is bool(kwargs.get("rct")) and d.ycbcr is bool(kwargs.get("ycbcr")) and d.quality == quality
            got = R.decode_image_rgba(d[4], qm)
            rgb, a = split_rgba(img, w, h, clean)
            if not quality:  # lossless: the input, or the restatement's cleaned image
                want = flat if clean == ALPHA_KEEP else cleaned(img, w, h)
                assert np.array_equal(got, want), (name, clean)
            else:  # the oracle's coefficients of the split raster's planes and its midpoint raster; the alpha exactly
                want_co = oracle_coefficients_ycc(oracle, rgb, w, h, qm)
                assert np.array_equal(d[4][:3], want_co), (name, clean)
                want_rgb = oracle_raster_ycc(oracle, want_co, qm, MIDPOINT, w, h)
                assert np.array_equal(got.reshape(-1, 4)[:, :3].reshape(-1), want_rgb), (name, clean)
                assert np.array_equal(got.reshape(-1, 4)[:, 3], a.reshape(-1)), (name, clean)
        R.close()


def test_raster_kernels_replay_from_a_graph_and_the_alpha_plan_keeps_its_dequantiser(ctx, hip):
    import torch

    import frave_amd as fa

    w, h = 333, 251
    n = w * h
    R = fa.PlanRGBA(ctx, w, h)
    imgs = [np.ascontiguousarray(_image(w, h, 50 + i, k)).reshape(-1) for i, k in enumerate(KINDS)]
    d_rgba = torch.from_numpy(imgs[0].copy()).cuda()
    d_rgb = torch.empty(3 * n, dtype=torch.uint8, device="cuda")
    d_a = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_back = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    R.split_rgba_dev(d_rgba.data_ptr(), d_rgb.data_ptr(), d_a.data_ptr(), clean=ALPHA_CLEAN, stream=s.cuda_stream)
    R.merge_rgba_dev(d_rgb.data_ptr(), d_a.data_ptr(), d_back.data_ptr(), stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    for img in imgs:  # every replay works on what the pixel buffer holds now
        d_rgba.copy_(torch.from_numpy(img.copy()))
        d_rgb.fill_(9), d_a.fill_(9), d_back.fill_(9)
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(ex, sp) == 0
        s.synchronize()
        rgb, a = split_rgba(img, w, h, ALPHA_CLEAN)
        assert np.array_equal(d_rgb.cpu().numpy(), rgb.reshape(-1)) and np.array_equal(d_a.cpu().numpy(), a.reshape(-1))
        assert np.array_equal(d_back.cpu().numpy(), cleaned(img, w, h))
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    # the encode chain refuses a capturing stream, as its inner calls do, and leaves the graph empty
    R.set_stream_order()
    d_params = torch.zeros(4 * 36, dtype=torch.float32, device="cuda")
    d_sym = torch.zeros(4 * R.num_some, dtype=torch.int16, device="cuda")
    d_hist = torch.zeros(4 * 10 * 1024, dtype=torch.int32, device="cuda")
    d_oob = torch.zeros(8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    try:
        with pytest.raises(fa.FriHipError) as e:
            R.encode_symbols_rgba_dev(d_rgba.data_ptr(), d_params.data_ptr(), d_sym.data_ptr(), d_hist.data_ptr(), d_oob.data_ptr(), stream=s.cuda_stream)
        assert e.value.code == -1 and "graph" in str(e.value)
    finally:
        assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0
    n_nodes = C.c_size_t(12345)
    rc = hip.hipGraphGetNodes(graph, None, C.byref(n_nodes))
    hip.hipGraphDestroy(graph)
    assert rc == 0 and n_nodes.value == 0
    # the alpha plan's dequantiser setting survives decode_image_rgba, which decodes alpha with the reference's whatever is set
    img = _image(w, h, 60)
    qm = fa.quality_matrix(40)
    lossy = np.ascontiguousarray(split_rgba(img, w, h)[1])
    co_a = R.alpha.transform_quant(lossy, qm)  # an alpha plane quantised at quality 40: the three dequantisers give three different rasters
    rasters = {}
    for mode in (REFERENCE, MULTIPLY, MIDPOINT):
        R.alpha.set_dequantiser(mode)
        rasters[mode] = R.alpha.inverse_transform(co_a, qm)
    assert not np.array_equal(rasters[REFERENCE], rasters[MULTIPLY]) and not np.array_equal(rasters[MULTIPLY], rasters[MIDPOINT])
    sym, vp, wp, hist, oob = R.encode_image_rgba_symbols(img)
    import frave_amd.emit as emit

    d = emit.decode_image(emit.encode_image_from_streams(w, h, sym, hist, vp, wp, alpha=True))
    for mode in (MULTIPLY, MIDPOINT, REFERENCE):
        R.alpha.set_dequantiser(mode)
        assert np.array_equal(R.decode_image_rgba(d[4]), np.ascontiguousarray(img).reshape(-1))
        assert np.array_equal(R.alpha.inverse_transform(co_a, qm), rasters[mode]), mode
    R.close()


def _pam(w, h, pixels):
    return b"P7\nWIDTH %d\nHEIGHT %d\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n" % (w, h) + np.ascontiguousarray(pixels, np.uint8).tobytes()


def test_driver_rgba_file(ctx, oracle, tmp_path):
    """fri_driver encode-file of a PAM (the C++ mirror: device chain, emitter) passes its self-check - the file decodes to the direct RGBA round trip - and
    decode-file writes a PAM of the expected pixels; a file with alpha goes to no other format"""
    import struct

    import frave_amd as fa

    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h = 333, 251
    img = _image(w, h, 3)
    src = tmp_path / "in.pam"
    src.write_bytes(_pam(w, h, img))
    qm = fa.quality_matrix(50)
    crgb, ca = split_rgba(img, w, h, ALPHA_CLEAN)
    lossy = merge_rgba(oracle_raster_ycc(oracle, oracle_coefficients_ycc(oracle, crgb, w, h, qm), qm, MIDPOINT, w, h), ca, w, h)
    cases = (("rct", ["--rct"], 0xC0000009, np.ascontiguousarray(img).reshape(-1)), ("ycc", ["--ycbcr", "--quality", "50", "--clean-alpha"], 0xC000000A, lossy))
    for name, flags, bits, want in cases:
        dst, back = tmp_path / f"{name}.frv", tmp_path / f"{name}.pam"
        out = subprocess.run([driver, "encode-file", str(src), str(dst)] + flags, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "self-check" in out.stdout
        frv = dst.read_bytes()
        mdat = struct.unpack("<I", frv[12:16])[0]
        assert (mdat & 0xC000000F) == bits, hex(mdat)
        out = subprocess.run([driver, "decode-file", str(dst), str(back)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        got = back.read_bytes()
        assert got[: len(got) - 4 * w * h] == _pam(w, h, img)[: -4 * w * h]  # the same header
        assert np.array_equal(np.frombuffer(got[-4 * w * h :], np.uint8), want), name
        for other in ("bad.ppm", "bad.bmp") if name == "rct" else ():  # a file with alpha goes to a PAM only
            out = subprocess.run([driver, "decode-file", str(dst), str(tmp_path / other)], capture_output=True, text=True, timeout=120)
            assert out.returncode != 0 and "alpha" in out.stderr and not (tmp_path / other).exists()
    # a search on the colour alone
    dst = tmp_path / "psnr.frv"
    out = subprocess.run([driver, "encode-file", str(src), str(dst), "--ycbcr", "--psnr", "38"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "self-check" in out.stdout, out.stdout + out.stderr
    # what RGBA does not take, and --clean-alpha without alpha
    for bad in (["--size", "20000"], ["--bpp", "4"], ["--420", "--quality", "50"], ["--ycbcr"]):
        out = subprocess.run([driver, "encode-file", str(src), str(tmp_path / "bad.frv")] + bad, capture_output=True, text=True, timeout=120)
        assert out.returncode != 0, bad
    ppm = tmp_path / "in.ppm"
    ppm.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(img[:, :, :3]).tobytes())
    out = subprocess.run([driver, "encode-file", str(ppm), str(tmp_path / "bad.frv"), "--clean-alpha"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0
    rgbfile = tmp_path / "rgb.frv"
    out = subprocess.run([driver, "encode-file", str(ppm), str(rgbfile), "--rct"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    out = subprocess.run([driver, "decode-file", str(rgbfile), str(tmp_path / "none.pam")], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "alpha" in out.stderr
    broken = tmp_path / "short.pam"
    broken.write_bytes(_pam(w, h, img)[:-5])
    out = subprocess.run([driver, "encode-file", str(broken), str(tmp_path / "bad.frv")], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0
    grey_alpha = tmp_path / "ga.pam"
    grey_alpha.write_bytes(b"P7\nWIDTH 4\nHEIGHT 4\nDEPTH 2\nMAXVAL 255\nTUPLTYPE GRAYSCALE_ALPHA\nENDHDR\n" + bytes(32))
    out = subprocess.run([driver, "encode-file", str(grey_alpha), str(tmp_path / "bad.frv")], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0
