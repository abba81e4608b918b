"""Lossy coding by quality on the device: K3's midpoint dequantiser against the oracle's raster of numpy-dequantised coefficients, K3's measuring
instances against numpy's distortion of that raster, and fri_hip_search_quality against a Python replay of its bisection. Bit-exact throughout."""
import math

import numpy as np
import pytest

from tests.common import gen_image
from tests.oracle_ref import LAYER, midpoint

pytestmark = pytest.mark.gpu
NONE = -(2 ** 31)
MIDPOINT = 2


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


def _image(w, h, c, seed):
    img = gen_image("noise", w, h, c, seed)
    img[: h // 2] = gen_image("smooth", w, h // 2, c, seed + 1)
    return img


def _recon_oracle(oracle, coefs, qm, w, h, c):
    W = oracle.Wavelet(np.zeros(w * h * c, np.uint8), h, w, c)
    W.set_coefficients(midpoint(coefs, qm))
    return W.to_raster()


# 512 x 384: rows of a multiple of 16 bytes (the lists kernel); 1001 x 613: the scanning kernel
SHAPES = [(512, 384, 1), (512, 384, 3), (1001, 613, 1), (1001, 613, 3)]


@pytest.mark.parametrize("shape", SHAPES)
def test_midpoint_dequantiser_is_the_oracle(ctx, oracle, shape):
    import frave_amd as fa

    w, h, c = shape
    img = _image(w, h, c, 5)
    P = fa.Plan(ctx, w, h, c)
    P.set_dequantiser(MIDPOINT)
    for q in (1, 37, 75, 99):
        qm = fa.quality_matrix(q)
        coefs = P.transform_quant(img, qm)
        got = P.inverse_transform(coefs, qm)
        assert np.array_equal(got, _recon_oracle(oracle, coefs, qm, w, h, c)), q
    qm = fa.quality_matrix(100)
    assert np.array_equal(P.inverse_transform(P.transform_quant(img, qm), qm), img.reshape(-1))
    P.close()


def test_midpoint_dequantiser_4096(ctx, oracle):
    import frave_amd as fa

    w = h = 4096
    img = _image(w, h, 1, 9)
    P = fa.Plan(ctx, w, h, 1)
    P.set_dequantiser(MIDPOINT)
    qm = fa.quality_matrix(37)
    coefs = P.transform_quant(img, qm)
    assert np.array_equal(P.inverse_transform(coefs, qm), _recon_oracle(oracle, coefs, qm, w, h, 1))
    P.close()


def _owned(P, d_co, qm):
    """bytes K3 writes: K3 into a 0x00-filled and a 0xFF-filled buffer agree exactly on them"""
    import torch

    outs = []
    for fill in (0, 255):
        buf = torch.full((P.pixel_bytes,), fill, dtype=torch.uint8, device="cuda")
        P.inverse_transform_dev(d_co.data_ptr(), buf.data_ptr(), qm)
        torch.cuda.synchronize()
        outs.append(buf.cpu().numpy())
    return outs[0] == outs[1], outs[0]


def _measure(P, d_co, d_ref, qm):
    import torch

    d_out = torch.full((2 * P.channels + 1,), 77, dtype=torch.int64, device="cuda")  # the entry point zeroes it
    P.measure_distortion_dev(d_co.data_ptr(), d_ref.data_ptr(), d_out.data_ptr(), qm)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().astype(np.uint64)


def _numpy_measure(recon, ref, owned, c):
    e = np.abs(recon.astype(np.int64) - ref.astype(np.int64)).reshape(-1, c)
    own = owned.reshape(-1, c)
    out = []
    for ch in range(c):
        ec = e[:, ch][own[:, ch]]
        out += [int((ec * ec).sum()), int(ec.max()) if ec.size else 0]
    return out + [int(own[:, 0].sum())]


@pytest.mark.parametrize("shape", SHAPES + [(4096, 4096, 1)])
@pytest.mark.parametrize("mode", [MIDPOINT, 1])
def test_measure_matches_numpy(ctx, shape, mode):
    import torch

    import frave_amd as fa

    w, h, c = shape
    img = _image(w, h, c, 21)
    P = fa.Plan(ctx, w, h, c)
    P.set_dequantiser(mode)
    d_px = torch.from_numpy(img.reshape(-1).copy()).cuda()
    d_co = torch.empty(P.coef_count, dtype=torch.int32, device="cuda")
    for q in ((1, 37, 75, 100) if w < 4096 else (37, 100)):
        qm = fa.quality_matrix(q)
        P.transform_quant_dev(d_px.data_ptr(), d_co.data_ptr(), qm)
        owned, recon = _owned(P, d_co, qm)
        got = _measure(P, d_co, d_px, qm)
        assert [int(x) for x in got] == _numpy_measure(recon, img.reshape(-1), owned, c), q
        assert np.array_equal(_measure(P, d_co, d_px, qm), got)  # the same in every run
        if q == 100:
            assert all(int(got[2 * ch]) == 0 for ch in range(c))
        assert int(got[2 * c]) == w * h  # ordinary shapes: every pixel is owned
    P.close()


def test_measure_with_rct_is_lossless_at_100(ctx):
    import torch

    import frave_amd as fa

    for w, h in ((512, 384), (1001, 613)):
        img = _image(w, h, 3, 4)
        P = fa.Plan(ctx, w, h, 3)
        P.set_colour_transform(1)
        d_px = torch.from_numpy(img.reshape(-1).copy()).cuda()
        d_co = torch.empty(P.coef_count, dtype=torch.int32, device="cuda")
        qm = fa.quality_matrix(100)
        P.transform_quant_dev(d_px.data_ptr(), d_co.data_ptr(), qm)
        got = _measure(P, d_co, d_px, qm)
        assert [int(got[0]), int(got[2]), int(got[4]), int(got[6])] == [0, 0, 0, w * h]
        P.close()


def _replay(P, d_px, target):
    """fri_hip_search_quality's bisection, probe by probe, through the public entry points"""
    import torch

    import frave_amd as fa

    P.set_dequantiser(MIDPOINT)
    d_co = torch.empty(P.coef_count, dtype=torch.int32, device="cuda")
    lo, hi, hi_db = 0, 100, math.inf
    while hi - lo > 1:
        mid = (lo + hi) // 2
        qm = fa.quality_matrix(mid)
        P.transform_quant_dev(d_px.data_ptr(), d_co.data_ptr(), qm)
        db = fa.distortion_psnr(_measure(P, d_co, d_px, qm), P.channels)
        if db >= target:
            hi, hi_db = mid, db
        else:
            lo = mid
    return hi, hi_db


@pytest.mark.parametrize("shape", [(640, 480, 1), (1001, 613, 3)])
def test_search_is_the_bisection(ctx, shape):
    import torch

    import frave_amd as fa

    w, h, c = shape
    img = _image(w, h, c, 33)
    P = fa.Plan(ctx, w, h, c)
    d_px = torch.from_numpy(img.reshape(-1).copy()).cuda()
    for target in (30.0, 40.0, 50.0):
        q_host, db_host = P.search_quality(img, target)
        q_dev, db_dev = P.search_quality(d_px.data_ptr(), target)
        assert (q_host, db_host) == (q_dev, db_dev)
        q_ref, db_ref = _replay(P, d_px, target)
        assert q_host == q_ref and db_host == pytest.approx(db_ref, rel=1e-12), target
        assert db_host >= target
    assert P.search_quality(img, 1e9) == (100, math.inf)
    P.close()


def test_search_leaves_the_dequantiser(ctx, oracle):
    """the search probes with the midpoint dequantiser; the plan's own setting (here the reference's division) stays what the caller set"""
    import frave_amd as fa

    w, h = 256, 192
    img = _image(w, h, 1, 8)
    P = fa.Plan(ctx, w, h, 1)
    P.set_dequantiser(False)
    P.search_quality(img, 35.0)
    qm = fa.quality_matrix(20)
    coefs = P.transform_quant(img, qm)
    W = oracle.Wavelet(np.zeros(w * h, np.uint8), h, w, 1)
    v = coefs.astype(np.int64)
    deq = np.where(coefs == NONE, NONE, np.trunc(v / np.asarray(qm, np.int64)[LAYER])).astype(np.int32)
    W.set_coefficients(deq)
    assert np.array_equal(P.inverse_transform(coefs, qm), W.to_raster())
    P.close()


@pytest.mark.parametrize("shape", [(3, 300, 1), (2, 257, 3), (400, 2, 1), (401, 3, 3)])
def test_measure_on_thin_images(ctx, shape):
    """very thin images: some pixels belong to no retained cell (the lattice has holes, K3 zero-fills the image first), and the rim's partly owned dwords
    are read byte by byte - only the owned bytes count, derived from K3 into a 0x00-filled and a 0xFF-filled buffer"""
    import torch

    import frave_amd as fa

    w, h, c = shape
    img = _image(w, h, c, 17)
    P = fa.Plan(ctx, w, h, c)
    P.set_dequantiser(MIDPOINT)
    d_px = torch.from_numpy(img.reshape(-1).copy()).cuda()
    d_co = torch.empty(P.coef_count, dtype=torch.int32, device="cuda")
    for q in (20, 100):
        qm = fa.quality_matrix(q)
        P.transform_quant_dev(d_px.data_ptr(), d_co.data_ptr(), qm)
        got = _measure(P, d_co, d_px, qm)
        # the owned bytes: with holes K3 zero-fills the image first, so the 0x00 / 0xFF fills agree everywhere; a lossless round trip of an all-255 image
        # shows the cells' footprint instead
        recon = P.inverse_transform(d_co.cpu().numpy(), qm)
        owned, _ = _owned_by_cells(P, w, h, c)
        assert not owned.all() or int(got[2 * c]) == w * h
        assert [int(x) for x in got] == _numpy_measure(recon, img.reshape(-1), owned, c), q
        if q == 100:
            assert all(int(got[2 * ch]) == 0 for ch in range(c))
    P.close()


def _owned_by_cells(P, w, h, c):
    """pixels some retained cell covers: a lossless round trip of an all-255 image gives 255 there and the zero fill elsewhere"""
    full = np.full(w * h * c, 255, np.uint8)
    back = P.inverse_transform(P.transform_quant(full, np.ones(32, np.int32)), np.ones(32, np.int32))
    return back == 255, back


def _stream_file(P, img, quality, fit=True):
    import frave_amd as fa
    import frave_amd.emit as emit

    P.set_stream_order()
    qm = fa.quality_matrix(quality)
    sym, vp, wp, hist, oob = P.encode_image_symbols(img, qm, fit=fit)
    assert not oob.any()
    return emit.encode_image_from_streams(P.width, P.height, sym, hist, vp, wp, quality=quality if quality < 100 else 0)


@pytest.mark.parametrize("shape", [(160, 120, 1), (160, 120, 3), (4096, 4096, 1)])
def test_end_to_end_file_round_trip(ctx, shape):
    """K1 + chain -> emitter (quality field) -> product decoder -> K3 midpoint equals the direct K1 -> K3 midpoint round trip; q = 50 is smaller than lossless"""
    import frave_amd as fa
    import frave_amd.emit as emit

    w, h, c = shape
    img = _image(w, h, c, 40)
    P = fa.Plan(ctx, w, h, c)
    P.set_dequantiser(MIDPOINT)
    sizes = {}
    for q in ((25, 50, 90, 100) if w < 4096 else (50, 100)):
        frv = _stream_file(P, img, q)
        d = emit.decode_image(frv)
        assert d.quality == (q if q < 100 else 0) and d[:3] == (w, h, c)
        qm = fa.quality_matrix(d.quality or 100)
        got = P.inverse_transform(d[4], qm)
        want = P.inverse_transform(P.transform_quant(img, qm), qm)
        assert np.array_equal(got, want), q
        if q == 100:
            assert np.array_equal(got, img.reshape(-1))
        sizes[q] = len(frv)
    print("sizes", shape, sizes)
    assert sizes[50] < sizes[100]
    P.close()


def test_driver_lossy_files(ctx, tmp_path):
    import os
    import subprocess

    import frave_amd as fa

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "frave_amd", "host")])
    for c, magic, suffix in ((1, b"P5", "pgm"), (3, b"P6", "ppm")):
        w, h = 320, 200
        img = _image(w, h, c, 50 + c)
        src = tmp_path / f"in.{suffix}"
        src.write_bytes(magic + b"\n%d %d\n255\n" % (w, h) + img.tobytes())
        for flag in (["--quality", "75"], ["--psnr", "40"]):
            dst, back = tmp_path / f"out_{c}_{flag[0][2:]}.frv", tmp_path / f"back_{c}_{flag[0][2:]}.{suffix}"
            out = subprocess.run([driver, "encode-file", str(src), str(dst)] + flag, capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stdout + out.stderr
            assert "quality" in out.stdout, out.stdout
            import frave_amd.emit as emit

            d = emit.decode_image(dst.read_bytes())
            if flag[0] == "--quality":
                assert d.quality == 75
            else:
                P = fa.Plan(ctx, w, h, c)
                q, db = P.search_quality(img, 40.0)
                P.close()
                assert d.quality == (q if q < 100 else 0) and db >= 40.0
            out = subprocess.run([driver, "decode-file", str(dst), str(back)], capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stderr
            P = fa.Plan(ctx, w, h, c)
            P.set_dequantiser(MIDPOINT)
            qm = fa.quality_matrix(d.quality or 100)
            want = P.inverse_transform(P.transform_quant(img, qm), qm)
            P.close()
            data = back.read_bytes()
            assert data[-w * h * c :] == want.tobytes()
