"""4:2:0 chroma subsampling on the device (fri_hip_plan420, K8: k8_chroma420.hip) against tests/chroma420_ref.py and the CPU oracle:

- the split, the merge and the measuring merge exactly equal to the restatement, over whole and ragged shapes, three kinds of image, device pointers on and one
  byte off a 256-byte boundary, between guard bytes;
- fri_hip_encode_image420_symbols against the existing route on two ordinary C = 1 plans and against the oracle, through the emitter and its decoder and
  fri_hip_decode_image420;
- the three searches against Python bisections over the piecewise entry points;
- graph capture of the raster kernels, the searches' refusal of a capturing stream;
- the size of a 4:2:0 file against the 4:4:4 YCbCr file of the same image at equal quality."""
import ctypes as C
import functools

import numpy as np
import pytest

from frave_amd.api import Plan420  # noqa: F401  (without the feature the module fails here)
from tests.chroma420_ref import chroma_shape, measure420, merge420, planes_flat, split420
from tests.common import gen_image
from tests.later_cases import C420_SATURATED
from tests.oracle_ref import MIDPOINT, oracle_raster
from tests.test_gpu_instances import Guarded
from tests.test_rct_host import correlated_image
from tests.ycbcr_ref import COLOUR_YCBCR, psnr

pytestmark = pytest.mark.gpu
RELAXED = 2  # hipStreamCaptureModeRelaxed
SHAPES = [(3, 5), (17, 9), (64, 48), (1, 700), (700, 1), (1023, 767), (1920, 1080), (4096, 4096)]
KINDS = ["noise", "smooth", "correlated"]


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


def _image(kind, w, h, seed):
    return correlated_image(w, h, seed) if kind == "correlated" else gen_image(kind, w, h, 3, seed)


@functools.lru_cache(maxsize=2)
def _reference(kind, w, h):
    """(pixels, the split's three planes as one array, the planes the merge is fed, its raster, the measuring merge's seven integers) of the restatement"""
    img = np.ascontiguousarray(_image(kind, w, h, 7)).reshape(-1)
    y, cb, cr = split420(img, w, h)
    planes = planes_flat(y, cb, cr)
    if kind == "noise":  # independent bytes in all three planes: the saturating corners of the inverse transform, which planes of a real image never reach
        cw, ch = chroma_shape(w, h)
        rng = np.random.default_rng(w * 7 + h)
        y, cb, cr = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8)
    fed = planes_flat(y, cb, cr)
    recon = merge420(y, cb, cr, w, h)
    return img, planes, fed, recon, measure420(recon, img)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_merge_and_measure_equal_the_restatement(ctx, shape, kind):
    import torch

    import frave_amd as fa

    w, h = shape
    img, planes, fed, recon, sums = _reference(kind, w, h)
    P = fa.Plan420(ctx, w, h)
    n_y = w * h
    assert planes.size == P.plane_bytes and sums[6] == n_y
    for offset in (0, 1):
        src = Guarded(torch, P.pixel_bytes, offset=offset, salt=1)
        src.put(torch, [img])
        out = Guarded(torch, P.plane_bytes, offset=offset, salt=2)
        P.split420_dev(src.ptr, out.ptr, out.ptr + n_y)
        (got,), intact = out.get(torch)
        assert intact, "the split wrote outside its planes"
        bad = got != planes
        assert not bad.any(), (shape, kind, offset, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
        assert src.get(torch)[1]
        # the merge of given planes, between guards
        pl = Guarded(torch, P.plane_bytes, offset=offset, salt=3)
        pl.put(torch, [fed])
        rgb = Guarded(torch, P.pixel_bytes, offset=offset, salt=4)
        P.merge420_dev(pl.ptr, pl.ptr + n_y, rgb.ptr)
        (got,), intact = rgb.get(torch)
        assert intact, "the merge wrote outside its raster"
        bad = got != recon
        assert not bad.any(), (shape, kind, offset, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
        # the measuring form: the seven integers, twice in a row, and nothing stored
        for _ in range(2):
            d_out = torch.full((7,), 77, dtype=torch.int64, device="cuda")
            P.measure_distortion420_dev(pl.ptr, pl.ptr + n_y, src.ptr, d_out.data_ptr())
            torch.cuda.synchronize()
            assert [int(x) for x in d_out.cpu().numpy().astype(np.uint64)] == sums, (shape, kind, offset)
        assert src.get(torch)[1] and pl.get(torch)[1]
        (again,), _ = src.get(torch)
        assert np.array_equal(again, img)
    P.close()


def test_measuring_merge_on_the_saturated_pair(ctx):
    """the reconstruction all 255 (Y = 255 under neutral chroma) against a reference of zeros, whole strips in whole workgroups: the largest sums the
    measuring kernel's 32-bit partials can meet, against the analytic values"""
    import torch

    import frave_amd as fa

    w, h = C420_SATURATED
    P = fa.Plan420(ctx, w, h)
    n_y = w * h
    planes = np.concatenate([np.full(n_y, 255, np.uint8), np.full(P.plane_bytes - n_y, 128, np.uint8)])
    y, cb, cr = planes[:n_y].reshape(h, w), planes[n_y : n_y + P.cw * P.ch].reshape(P.ch, P.cw), planes[n_y + P.cw * P.ch :].reshape(P.ch, P.cw)
    assert (merge420(y, cb, cr, w, h) == 255).all()  # the restatement agrees that this is the saturated reconstruction
    pl = Guarded(torch, P.plane_bytes, offset=1, salt=1)
    pl.put(torch, [planes])
    ref = Guarded(torch, P.pixel_bytes, offset=1, salt=2)
    ref.put(torch, [np.zeros(P.pixel_bytes, np.uint8)])
    d_out = torch.full((7,), 77, dtype=torch.int64, device="cuda")
    P.measure_distortion420_dev(pl.ptr, pl.ptr + n_y, ref.ptr, d_out.data_ptr())
    torch.cuda.synchronize()
    assert [int(x) for x in d_out.cpu().numpy().astype(np.uint64)] == [255 * 255 * n_y, 255] * 3 + [n_y]
    assert pl.get(torch)[1] and ref.get(torch)[1]
    P.close()


def _plain_route(ctx, plane, quality):
    """fri_hip_encode_image_symbols of one plane on an ordinary C = 1 plan"""
    import frave_amd as fa

    ph, pw = plane.shape
    Q = fa.Plan(ctx, pw, ph, 1)
    Q.set_stream_order()
    out = Q.encode_image_symbols(plane, fa.quality_matrix(quality), fit=True)
    Q.close()
    return out


@pytest.mark.parametrize("shape", [(512, 384), (333, 251), (1023, 767)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_image420_symbols_is_the_existing_route_on_the_split_planes(ctx, shape):
    import frave_amd as fa

    w, h = shape
    img = correlated_image(w, h, 30)
    P = fa.Plan420(ctx, w, h)
    P.set_stream_order()
    for q in (35, 80):
        sym, vp, wp, hist, oob = P.encode_image420_symbols(img, q)
        at = 0
        for k, plane in enumerate(split420(img, w, h)):
            rsym, rvp, rwp, rhist, roob = _plain_route(ctx, plane, q)
            n = rsym.size
            assert np.array_equal(sym[at : at + n], rsym.reshape(-1)), (q, k, "stream")
            assert np.array_equal(hist[k], rhist[0]) and np.array_equal(vp[k], rvp[0]) and np.array_equal(wp[k], rwp[0]) and oob[k] == roob[0], (q, k)
            at += n
        assert at == sym.size == P.num_symbols
    for bad in (0, 100, -5):  # a 4:2:0 file has a quality of 1..99
        with pytest.raises(fa.FriHipError) as e:
            P.encode_image420_symbols(img, bad)
        assert e.value.code == -1
        with pytest.raises(fa.FriHipError) as e:
            P.decode_image420(np.zeros(P.coef_count, np.int32), bad)
        assert e.value.code == -1
    P.close()


def _file420(P, img, quality):
    import frave_amd.emit as emit

    sym, vp, wp, hist, oob = P.encode_image420_symbols(img, quality)
    assert not oob.any()
    return emit.encode_image_from_streams(P.width, P.height, sym, hist, vp, wp, quality=quality, ycbcr=True, n_luma=P.luma.num_some)


@pytest.mark.parametrize("shape", [(640, 480), (577, 431)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_file_round_trip_against_the_oracle(ctx, oracle, shape):
    """encode -> emitter (FRI_EMIT_420) -> decoder gives the oracle's quantised coefficients of the restatement's planes; fri_hip_decode_image420 of them gives the
    restatement's merge of the oracle's midpoint-dequantised rasters"""
    import frave_amd as fa
    import frave_amd.emit as emit

    w, h = shape
    img = correlated_image(w, h, 41)
    P = fa.Plan420(ctx, w, h)
    P.set_stream_order()
    planes = split420(img, w, h)
    for q in (20, 60, 95):
        qm = fa.quality_matrix(q)
        d = emit.decode_image(_file420(P, img, q))
        assert d.s420 and d.ycbcr and not d.rct and d.quality == q and d[:3] == (w, h, 3)
        rasters = []
        for got, plane in zip(d[4], planes):
            ph, pw = plane.shape
            W = oracle.Wavelet(np.ascontiguousarray(plane).reshape(-1), ph, pw, 1)
            W.quantize(qm)
            want = W.coefficients()
            W.close()
            assert np.array_equal(got, want[0]), q
            rasters.append(oracle_raster(oracle, want, qm, MIDPOINT, pw, ph, 1).reshape(ph, pw))
        want_px = merge420(rasters[0], rasters[1], rasters[2], w, h)
        got_px = P.decode_image420(np.concatenate([c.reshape(-1) for c in d[4]]), q)
        assert np.array_equal(got_px, want_px), q
        print(shape, q, f"{psnr(got_px, img):.2f} dB")
    P.close()


class _Pieces:
    """the probes of the searches out of the piecewise entry points: the split once, then per quality K1 and K3 (midpoint) on both inner plans and the merge"""

    def __init__(self, ctx, img, w, h):
        import torch

        import frave_amd as fa

        self.torch, self.fa = torch, fa
        self.P = fa.Plan420(ctx, w, h)
        self.P.set_stream_order()
        self.rgb3 = fa.Plan(ctx, w, h, 3)  # the measuring entry points of a plain C = 3 plan: K7 and the rate kernel
        P = self.P
        self.img = img
        self.d_rgb = torch.from_numpy(np.ascontiguousarray(img).reshape(-1).copy()).cuda()
        self.d_planes = torch.empty(P.plane_bytes, dtype=torch.uint8, device="cuda")
        self.d_recon = torch.empty(P.plane_bytes, dtype=torch.uint8, device="cuda")
        self.d_back = torch.empty(P.pixel_bytes, dtype=torch.uint8, device="cuda")
        self.d_coefs = torch.empty(P.coef_count, dtype=torch.int32, device="cuda")
        self.n_y, self.n_c = w * h, P.cw * P.ch
        self.fy, self.fc = P.luma.num_cells * 512, P.chroma.num_cells * 512
        P.split420_dev(self.d_rgb.data_ptr(), self.d_planes.data_ptr(), self.d_planes.data_ptr() + self.n_y)
        P.luma.set_dequantiser(MIDPOINT), P.chroma.set_dequantiser(MIDPOINT)
        self.probes = []

    def round_trip(self, q):
        P, qm = self.P, self.fa.quality_matrix(q)
        pl, co, rc = self.d_planes.data_ptr(), self.d_coefs.data_ptr(), self.d_recon.data_ptr()
        self.probes.append(q)
        P.luma.transform_quant_dev(pl, co, qm)
        P.chroma.transform_quant_dev(pl + self.n_y, co + 4 * self.fy, qm, n_images=2, pixel_stride=self.n_c, coef_stride=self.fc)
        P.luma.inverse_transform_dev(co, rc, qm)
        P.chroma.inverse_transform_batch_dev(2, co + 4 * self.fy, self.fc, rc + self.n_y, self.n_c, qm)

    def psnr(self, q):
        self.round_trip(q)
        d_out = self.torch.empty(7, dtype=self.torch.int64, device="cuda")
        self.P.measure_distortion420_dev(self.d_recon.data_ptr(), self.d_recon.data_ptr() + self.n_y, self.d_rgb.data_ptr(), d_out.data_ptr())
        self.torch.cuda.synchronize()
        return self.fa.distortion_psnr(d_out.cpu().numpy().astype(np.uint64), 3)

    def ssim(self, q):
        self.round_trip(q)
        self.P.merge420_dev(self.d_recon.data_ptr(), self.d_recon.data_ptr() + self.n_y, self.d_back.data_ptr())
        self.torch.cuda.synchronize()
        return self.fa.ssim_of(self.rgb3.measure_ssim(self.img, self.d_back.cpu().numpy()), 3)[0]

    def size(self, q):
        self.probes.append(q)
        sym, vp, wp, hist, oob = self.P.encode_image420_symbols(self.img, q)
        return self.rgb3.estimate_size(hist, oob)

    def close(self):
        self.P.close(), self.rgb3.close()


def _lowest_reaching(value_of, target, top):
    """the header's bisection for PSNR and SSIM: lo = 0, hi = 100, 100 never probed; `top` is reported for 100"""
    lo, hi, hi_v = 0, 100, top
    while hi - lo > 1:
        mid = (lo + hi) // 2
        v = value_of(mid)
        if v >= target:
            hi, hi_v = mid, v
        else:
            lo = mid
    return hi, hi_v


def test_searches_are_the_bisections_over_the_piecewise_entry_points(ctx):
    import frave_amd as fa

    w, h = 640, 480
    img = correlated_image(w, h, 12)
    K = _Pieces(ctx, img, w, h)
    P = K.P
    for target in (30.0, 38.0, 80.0):
        want = _lowest_reaching(K.psnr, target, float("inf"))
        for got in (P.search_quality(img, target), P.search_quality(K.d_rgb.data_ptr(), target)):
            # the same integers go into both PSNRs; numpy's log10 and libm's may differ in the last place
            assert got[0] == want[0] and (got[1] == want[1] or got[1] == pytest.approx(want[1], abs=1e-9)), (target, got, want)
    assert want == (100, float("inf"))  # 80 dB: no quality 1..99 reaches it - "code losslessly"
    q, db = P.search_quality(img, 38.0)
    assert 1 < q < 100 and db >= 38.0
    for target in (0.9, 0.97, 1.0):
        want = _lowest_reaching(K.ssim, target, 1.0)
        assert P.search_quality_ssim(img, target) == want, target
        assert P.search_quality_ssim(K.d_rgb.data_ptr(), target) == want, target
    # the size search: lo = 0, hi = 100 (qualities 1..99), lo moves up while the estimate fits
    n1, n99 = len(_file420(P, img, 1)), len(_file420(P, img, 99))
    for budget in (n1 + 1000, (n1 + n99) // 2, n99 + 1000, 10 ** 9):
        lo, hi, lo_est, last = 0, 100, 0, None
        K.probes.clear()
        while hi - lo > 1:
            mid = (lo + hi) // 2
            last = K.size(mid)
            if last != 2 ** 64 - 1 and last <= budget:
                lo, lo_est = mid, last
            else:
                hi = mid
        assert len(K.probes) <= 7
        assert lo >= 1
        assert P.search_quality_for_size(img, budget) == (lo, lo_est), budget
        assert P.search_quality_for_size(K.d_rgb.data_ptr(), budget) == (lo, lo_est), budget
        if budget == 10 ** 9:
            assert lo == 99  # everything fits, and a 4:2:0 file has no quality 100
        frv = _file420(P, img, lo)
        assert abs(len(frv) - lo_est) <= 24 * 3, (budget, lo, lo_est, len(frv))  # the size model's bound for YCbCr files (tests/test_ycbcr_host.py)
    with pytest.raises(fa.FriHipError) as e:  # nothing fits
        P.search_quality_for_size(img, 100)
    assert e.value.code == -7
    qual, est = C.c_int32(5), C.c_uint64(0)
    assert fa.load_library().fri_hip_search_quality_for_size420(P._h, fa.api._p(np.ascontiguousarray(img).reshape(-1)), 100, C.byref(qual), C.byref(est)) == -7
    assert qual.value == 0 and est.value == K.size(1)
    K.close()


def test_raster_kernels_replay_from_a_graph_and_searches_refuse_capture(ctx, hip):
    import torch

    import frave_amd as fa

    w, h = 333, 251
    P = fa.Plan420(ctx, w, h)
    n_y = w * h
    imgs = [np.ascontiguousarray(_image(k, w, h, 50 + i)).reshape(-1) for i, k in enumerate(KINDS)]
    d_rgb = torch.from_numpy(imgs[0].copy()).cuda()
    d_planes = torch.empty(P.plane_bytes, dtype=torch.uint8, device="cuda")
    d_back = torch.empty(P.pixel_bytes, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(7, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    P.split420_dev(d_rgb.data_ptr(), d_planes.data_ptr(), d_planes.data_ptr() + n_y, stream=s.cuda_stream)
    P.merge420_dev(d_planes.data_ptr(), d_planes.data_ptr() + n_y, d_back.data_ptr(), stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    for img in imgs:  # every replay works on what the pixel buffer holds now
        d_rgb.copy_(torch.from_numpy(img.copy()))
        d_planes.fill_(9), d_back.fill_(9), d_out.fill_(9)
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(ex, sp) == 0
        s.synchronize()
        y, cb, cr = split420(img, w, h)
        assert np.array_equal(d_planes.cpu().numpy(), planes_flat(y, cb, cr))
        back = merge420(y, cb, cr, w, h)
        assert np.array_equal(d_back.cpu().numpy(), back)
        # (the measuring form on the stream, behind the replay)
        P.measure_distortion420_dev(d_planes.data_ptr(), d_planes.data_ptr() + n_y, d_rgb.data_ptr(), d_out.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        assert [int(x) for x in d_out.cpu().numpy().astype(np.uint64)] == measure420(back, img)
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    # the searches read every probe back: they refuse a capturing stream and leave the graph empty
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    try:
        for call in (lambda: P.search_quality(d_rgb.data_ptr(), 38.0, stream=s.cuda_stream), lambda: P.search_quality_ssim(d_rgb.data_ptr(), 0.9, stream=s.cuda_stream),
                     lambda: P.search_quality_for_size(d_rgb.data_ptr(), 50000, stream=s.cuda_stream)):
            with pytest.raises(fa.FriHipError) as e:
                call()
            assert e.value.code == -1 and "graph" in str(e.value)
    finally:
        assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0
    n_nodes = C.c_size_t(12345)
    rc = hip.hipGraphGetNodes(graph, None, C.byref(n_nodes))
    hip.hipGraphDestroy(graph)
    assert rc == 0 and n_nodes.value == 0
    q, db = P.search_quality(d_rgb.data_ptr(), 36.0, stream=s.cuda_stream)  # and work afterwards
    assert 1 <= q <= 100
    P.close()


def test_420_file_is_smaller_than_the_444_file_at_equal_quality(ctx):
    """Half the samples are coded: a sanity condition, not a tuned number. The ratios and both R, G, B PSNRs are printed; no threshold on either."""
    import frave_amd as fa
    import frave_amd.emit as emit

    w, h = 1024, 768
    P = fa.Plan420(ctx, w, h)
    P.set_stream_order()
    Q = fa.Plan(ctx, w, h, 3)
    Q.set_colour_transform(COLOUR_YCBCR)
    Q.set_dequantiser(MIDPOINT)
    Q.set_stream_order()
    for name, img in (("correlated", correlated_image(w, h, 8)), ("smooth", gen_image("smooth", w, h, 3, 2)), ("noise", gen_image("noise", w, h, 3, 2))):
        for q in (25, 75):
            qm = fa.quality_matrix(q)
            f420 = _file420(P, img, q)
            sym, vp, wp, hist, oob = Q.encode_image_symbols(img, qm, fit=True)
            assert not oob.any()
            f444 = emit.encode_image_from_streams(w, h, sym, hist, vp, wp, quality=q, ycbcr=True)
            d = emit.decode_image(f420)
            db420 = psnr(P.decode_image420(np.concatenate([c.reshape(-1) for c in d[4]]), q), img)
            db444 = psnr(Q.inverse_transform(emit.decode_image(f444)[4], qm), img)
            print(f"{name} {w}x{h} q{q}: 4:2:0 {len(f420)} B {db420:.2f} dB, 4:4:4 {len(f444)} B {db444:.2f} dB, ratio {len(f420) / len(f444):.3f}")
            assert len(f420) < len(f444), (name, q)
    P.close(), Q.close()


def test_driver_420_file(tmp_path):
    """fri_driver encode-file --420 (the C++ mirror: search, device chain, emitter) passes its self-check - the file decodes to the direct 4:2:0 round trip -
    and decode-file, which needs no flag, gives that image back; the file carries metadata bits 1 and 2 and is smaller than the 4:4:4 file of the same target"""
    import os
    import struct
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "frave_amd", "host")])
    w, h = 641, 479
    img = correlated_image(w, h, 3)
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + img.tobytes())
    sizes = {}
    for name, flags in (("444", ["--ycbcr", "--psnr", "38"]), ("420", ["--420", "--psnr", "38"]), ("420q", ["--420", "--quality", "70"]), ("420s", ["--420", "--ssim", "0.95"]),
                        ("420b", ["--420", "--bpp", "6"])):
        dst, back = tmp_path / f"{name}.frv", tmp_path / f"{name}.ppm"
        out = subprocess.run([driver, "encode-file", str(src), str(dst)] + flags, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        frv = dst.read_bytes()
        mdat = struct.unpack("<I", frv[12:16])[0]
        assert (mdat & 0xC0000007) == (0xC0000006 if name != "444" else 0xC0000002), hex(mdat)
        out = subprocess.run([driver, "decode-file", str(dst), str(back)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        px = np.frombuffer(back.read_bytes()[-w * h * 3 :], np.uint8)
        if "--psnr" in flags:
            assert psnr(px, img) >= 38.0
        if name == "420b":
            assert len(frv) <= w * h * 6 // 8
        sizes[name] = len(frv)
    print("driver sizes", sizes)
    assert sizes["420"] < sizes["444"]
    # --420 needs an RGB image and a lossy target, and excludes --rct
    for bad in (["--420"], ["--420", "--rct", "--quality", "50"], ["--420", "--rct"]):
        out = subprocess.run([driver, "encode-file", str(src), str(tmp_path / "bad.frv")] + bad, capture_output=True, text=True, timeout=120)
        assert out.returncode != 0, bad
    grey = tmp_path / "in.pgm"
    grey.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + img[:, :, 1].tobytes())
    out = subprocess.run([driver, "encode-file", str(grey), str(tmp_path / "bad.frv"), "--420", "--quality", "50"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0
