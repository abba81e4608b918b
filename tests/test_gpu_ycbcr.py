"""Lossy YCbCr colour coding on the device (fri_hip_plan_set_colour_transform(FRI_HIP_COLOUR_YCBCR)) against tests/ycbcr_ref.py and the CPU oracle:

- every reachable YCbCr K1 instance: the oracle's coefficients of ycc(pixels), bit for bit (the RCT cases of tests/instance_cases.py, whose shapes, pointers
  and tilings reach every K1 cell, run again on YCbCr plans), the C16 chain form and the tuner's MEASURE form;
- every reachable YCbCr K3 instance (lists / scanning x NI x reference / multiply / midpoint, and MEASURE): inverse_ycc of the oracle's raster over the owned
  pixels, written between guard bytes, and the measure sums in R, G, B;
- the encode chain, the file round trip, both searches and the rate at equal distortion against plain RGB."""
import dataclasses
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.common import gen_image, random_params
from tests.instance_cases import CASES, knobs, qmatrix
from tests.oracle_ref import MIDPOINT, numpy_measure, oracle_owned
from tests.test_gpu_instances import GUARD, Guarded, _check_guards_i32, _guarded_coefs
from tests.test_rct_host import correlated_image
from tests.ycbcr_ref import COLOUR_YCBCR, oracle_coefficients_ycc, oracle_raster_ycc, psnr, ycc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the instance cases of the RCT plans (C = 3, every K1 / C16 / K3 / MEASURE cell the launchers can reach with a colour transform), on YCbCr plans
YCC_CASES = [dataclasses.replace(c, id=c.id.replace("3rct", "3ycc").replace("-rct-", "-ycc-"), rct=False) for c in CASES if c.rct]


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


def _plan(ctx, case):
    import frave_amd as fa

    w, h, c = case.shape
    with knobs(case.env()):
        P = fa.Plan(ctx, w, h, c)
    P.set_colour_transform(COLOUR_YCBCR)
    P.set_dequantiser(case.deq)
    return P


def _images(case):
    w, h, c = case.shape
    out = []
    for k in range(case.n_images):
        s = 1000 * case.seed + k
        img = correlated_image(w, h, s)
        img[: h // 3] = gen_image("noise", w, h // 3, c, s)  # saturated colours too: the clamps of the inverse
        out.append(np.ascontiguousarray(img).reshape(-1))
    return out


def _run_k1(ctx, oracle, case):
    import torch

    w, h, c = case.shape
    P = _plan(ctx, case)
    qm = qmatrix(case.quant)
    imgs = _images(case)
    px = Guarded(torch, P.pixel_bytes, case.n_images, case.pixel_stride, case.offset, case.seed)
    px.put(torch, imgs)
    co, co_ptr = _guarded_coefs(torch, P, case.n_images)
    P.transform_quant_dev(px.ptr, co_ptr, qm, n_images=case.n_images, pixel_stride=case.pixel_stride, coef_stride=P.coef_count)
    torch.cuda.synchronize()
    got = co.cpu().numpy()[GUARD // 4 : GUARD // 4 + case.n_images * P.coef_count].reshape(case.n_images, c, P.num_cells, 512)
    assert _check_guards_i32(co), "K1 wrote outside the coefficient planes"
    _, intact = px.get(torch)
    assert intact, "K1 wrote into its pixels' guards"
    for k, img in enumerate(imgs):
        want = oracle_coefficients_ycc(oracle, img, w, h, qm)
        assert np.array_equal(got[k], want), (case.id, k, int((got[k] != want).sum()))
    P.close()


def _run_c16(ctx, oracle, case):
    """the compact planes through the gather route and the direct route: streams, histograms and out-of-alphabet counts of the oracle's ycc(pixels)"""
    import torch

    from tests.test_gpu_instances import _oracle_symbols

    w, h, c = case.shape
    P = _plan(ctx, case)
    order = P.set_stream_order()
    qm = qmatrix(case.quant)
    imgs = _images(case)
    vp, wp = random_params(11 + case.seed, 0.1)
    params = np.broadcast_to(np.stack([np.asarray(vp, np.float32).reshape(3, 6), np.asarray(wp, np.float32).reshape(3, 6)]), (c, 2, 3, 6)).copy()
    want = [_oracle_symbols(oracle, ycc(img), w, h, c, qm, False, params, order) for img in imgs]
    n_img, n, plane = case.n_images, P.num_some, P.num_cells * 512
    px = Guarded(torch, P.pixel_bytes, n_img, case.pixel_stride, case.offset, case.seed)
    px.put(torch, imgs)
    for direct in (False, True):
        d_w = torch.full((n_img * c * plane,), 0xEEEE, dtype=torch.uint16, device="cuda")
        d_st = torch.full((n_img * c * n + 16,), 0xFFFF, dtype=torch.uint16, device="cuda")
        d_h = torch.full((n_img, c, 10, 1024), -1, dtype=torch.int32, device="cuda")
        d_o = torch.full((n_img, c), -1, dtype=torch.int64, device="cuda")
        d_par = torch.from_numpy(np.broadcast_to(params, (n_img, c, 2, 3, 6)).copy()).cuda()
        P.encode_symbols_batch_dev(n_img, px.ptr, case.pixel_stride, qm, False, d_par.data_ptr(), 0, c * plane, 0 if direct else d_w.data_ptr(), c * plane,
                                   d_st.data_ptr(), c * n, d_h.data_ptr(), d_o.data_ptr(), None)
        torch.cuda.synchronize()
        st = d_st.cpu().numpy()
        assert (st[n_img * c * n :] == 0xFFFF).all(), "the streams' tail was written"
        st = st[: n_img * c * n].reshape(n_img, c, n)
        hist, oob = d_h.cpu().numpy().view(np.uint32), d_o.cpu().numpy()
        for k in range(n_img):
            wsym, whist, woob = want[k]
            assert np.array_equal(hist[k], whist), (case.id, direct, k, "histograms")
            assert np.array_equal(oob[k], woob), (case.id, direct, k, "out-of-alphabet counts")
            for ch in range(c):
                if woob[ch] == 0:
                    assert np.array_equal(st[k, ch], wsym[ch]), (case.id, direct, k, ch)
    _, intact = px.get(torch)
    assert intact
    P.close()


def _k3_inputs(oracle, case):
    import torch

    w, h, c = case.shape
    qm = qmatrix(case.quant)
    imgs = _images(case)
    owned = oracle_owned(oracle, w, h, c)
    coefs = [oracle_coefficients_ycc(oracle, img, w, h, qm) for img in imgs]
    recon = [oracle_raster_ycc(oracle, co, qm, case.deq, w, h, owned) for co in coefs]
    d_co = torch.from_numpy(np.stack([co.reshape(-1) for co in coefs])).cuda()
    return qm, imgs, owned, recon, d_co


def _run_k3(ctx, oracle, case):
    import torch

    P = _plan(ctx, case)
    qm, imgs, owned, recon, d_co = _k3_inputs(oracle, case)
    out = Guarded(torch, P.pixel_bytes, case.n_images, case.pixel_stride, case.offset, case.seed)
    P.inverse_transform_batch_dev(case.n_images, d_co.data_ptr(), P.coef_count, out.ptr, case.pixel_stride, qm)
    got, intact = out.get(torch)
    assert intact, "K3 wrote into the guards or the gaps between images"
    for k in range(case.n_images):
        bad = got[k] != recon[k]
        assert not bad.any(), (case.id, k, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
    P.close()


def _run_measure(ctx, oracle, case):
    import torch

    w, h, c = case.shape
    P = _plan(ctx, case)
    qm, imgs, owned, recon, d_co = _k3_inputs(oracle, case)
    ref = Guarded(torch, P.pixel_bytes, 1, 0, case.offset, case.seed)
    ref.put(torch, imgs)
    d_out = torch.full((2 * c + 1,), 77, dtype=torch.int64, device="cuda")
    P.measure_distortion_dev(d_co.data_ptr(), ref.ptr, d_out.data_ptr(), qm)
    torch.cuda.synchronize()
    got = [int(x) for x in d_out.cpu().numpy().astype(np.uint64)]
    want = numpy_measure(recon[0], imgs[0], owned, c)  # in R, G, B against the R, G, B reference
    assert got == want, (case.id, got, want)
    _, intact = ref.get(torch)
    assert intact
    P.close()


RUN = {"k1": _run_k1, "c16": _run_c16, "k3": _run_k3, "measure": _run_measure}


@pytest.mark.parametrize("case", YCC_CASES, ids=lambda c: c.id)
def test_instance(ctx, oracle, case):
    RUN[case.kind](ctx, oracle, case)


def test_tuned_plan_and_measure_instance(ctx, oracle):
    """fri_hip_plan_tune_forward runs on the plan's mode (K1's YCbCr MEASURE instances); the tiling it keeps still gives the oracle's coefficients"""
    import frave_amd as fa

    w, h = 1024, 768
    img = correlated_image(w, h, 77)
    P = fa.Plan(ctx, w, h, 3)
    P.set_colour_transform(COLOUR_YCBCR)
    P.tune_forward()
    qm = fa.quality_matrix(60)
    assert np.array_equal(P.transform_quant(img, qm), oracle_coefficients_ycc(oracle, img, w, h, qm))
    assert np.array_equal(P.transform_quant(img), oracle_coefficients_ycc(oracle, img, w, h, np.ones(32, np.int32)))
    P.close()


@pytest.mark.parametrize("fit", [False, True])
def test_encode_image_symbols_is_the_plain_chain_of_ycc_planes(ctx, fit):
    import frave_amd as fa

    w, h = 512, 384
    img = correlated_image(w, h, 30)
    P, Q = fa.Plan(ctx, w, h, 3), fa.Plan(ctx, w, h, 3)
    P.set_colour_transform(COLOUR_YCBCR)
    P.set_stream_order(), Q.set_stream_order()
    qm = fa.quality_matrix(70)
    got = P.encode_image_symbols(img, qm, fit=fit)
    ref = Q.encode_image_symbols(ycc(img), qm, fit=fit)
    for a, b in zip(got, ref):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    P.close(), Q.close()


def _ycc_file(P, img, quality):
    import frave_amd as fa
    import frave_amd.emit as emit

    P.set_stream_order()
    sym, vp, wp, hist, oob = P.encode_image_symbols(img, fa.quality_matrix(quality), fit=True)
    assert not oob.any()
    return emit.encode_image_from_streams(P.width, P.height, sym, hist, vp, wp, quality=quality, ycbcr=True)


@pytest.mark.parametrize("shape", [(1024, 768), (4096, 4096)])
def test_file_round_trip(ctx, shape):
    """K1 + chain -> emitter (YCbCr flag) -> product decoder -> K3 (YCbCr, midpoint) gives the direct round trip's pixels"""
    import frave_amd as fa
    import frave_amd.emit as emit

    w, h = shape
    img = correlated_image(w, h, 41)
    P = fa.Plan(ctx, w, h, 3)
    P.set_colour_transform(COLOUR_YCBCR)
    P.set_dequantiser(MIDPOINT)
    for q in ((20, 60, 95) if w < 4096 else (60,)):
        frv = _ycc_file(P, img, q)
        d = emit.decode_image(frv)
        assert d.ycbcr and not d.rct and d.quality == q and d[:3] == (w, h, 3)
        qm = fa.quality_matrix(q)
        got = P.inverse_transform(d[4], qm)
        want = P.inverse_transform(P.transform_quant(img, qm), qm)
        assert np.array_equal(got, want), q
        print(shape, q, len(frv), f"{psnr(got, img):.2f} dB")
    P.close()


def test_searches_on_ycbcr_plans(ctx):
    """search_quality: the PSNR (in R, G, B) of the quality it returns reaches the target and one quality lower does not; search_quality_for_size: a quality
    in 1..99 whose estimate is within 24 C bytes of the file the emitter writes"""
    import frave_amd as fa

    w, h = 640, 480
    img = correlated_image(w, h, 12)
    P = fa.Plan(ctx, w, h, 3)
    P.set_colour_transform(COLOUR_YCBCR)
    P.set_dequantiser(MIDPOINT)

    def db_of(q):
        qm = fa.quality_matrix(q)
        return psnr(P.inverse_transform(P.transform_quant(img, qm), qm), img)

    q, db = P.search_quality(img, 38.0)
    assert 1 < q < 100 and db >= 38.0 and db == pytest.approx(db_of(q), abs=1e-9) and db_of(q - 1) < 38.0
    q100, db100 = P.search_quality(img, 60.0)  # beyond what YCbCr reaches: "code losslessly"
    assert q100 == 100
    n1, n99 = len(_ycc_file(P, img, 1)), len(_ycc_file(P, img, 99))
    for budget in (n1 + 1000, (n1 + n99) // 2, n99 + 1000, 10 ** 9):
        qs, est = P.search_quality_for_size(img, budget)
        assert 1 <= qs <= 99 and est <= budget
        if budget == 10 ** 9:
            assert qs == 99  # everything fits, and a YCbCr file has no quality 100
        frv = _ycc_file(P, img, qs)
        assert abs(len(frv) - est) <= 24 * 3, (budget, qs, est, len(frv))
    P.close()


def _file_at_psnr(ctx, img, target, colour):
    import frave_amd as fa

    w, h = img.shape[1], img.shape[0]
    P = fa.Plan(ctx, w, h, 3)
    P.set_colour_transform(colour)
    P.set_dequantiser(MIDPOINT)
    q, db = P.search_quality(img, target)
    assert q < 100
    qm = fa.quality_matrix(q)
    back = P.inverse_transform(P.transform_quant(img, qm), qm)
    P.set_stream_order()
    sym, vp, wp, hist, oob = P.encode_image_symbols(img, qm, fit=True)
    import frave_amd.emit as emit

    frv = emit.encode_image_from_streams(w, h, sym, hist, vp, wp, quality=q, ycbcr=colour == COLOUR_YCBCR)
    P.close()
    return len(frv), q, psnr(back, img)


def test_rate_at_equal_distortion(ctx):
    """At 40 dB in R, G, B, the YCbCr file of a correlated image is smaller than the plain RGB one. Smooth and noise images are printed, not asserted."""
    w, h = 1024, 768
    img = correlated_image(w, h, 8)
    n_rgb, q_rgb, db_rgb = _file_at_psnr(ctx, img, 40.0, 0)
    n_ycc, q_ycc, db_ycc = _file_at_psnr(ctx, img, 40.0, COLOUR_YCBCR)
    print(f"correlated {w}x{h} at 40 dB: RGB q{q_rgb} {n_rgb} B ({db_rgb:.2f} dB), YCbCr q{q_ycc} {n_ycc} B ({db_ycc:.2f} dB), ratio {n_ycc / n_rgb:.3f}")
    assert db_rgb >= 40.0 and db_ycc >= 40.0
    assert n_ycc < n_rgb
    for kind in ("smooth", "noise"):
        im = gen_image(kind, w, h, 3, 2)
        try:
            a, b = _file_at_psnr(ctx, im, 40.0, 0), _file_at_psnr(ctx, im, 40.0, COLOUR_YCBCR)
            print(f"{kind} at 40 dB: RGB {a[0]} B q{a[1]}, YCbCr {b[0]} B q{b[1]}, ratio {b[0] / a[0]:.3f}")
        except AssertionError:
            print(f"{kind}: 40 dB needs quality 100 in one of the modes")


def test_driver_ycbcr_file(tmp_path):
    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h = 320, 200
    img = correlated_image(w, h, 3)
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + img.tobytes())
    sizes = {}
    for flag in ([], ["--ycbcr"]):
        dst, back = tmp_path / f"out{len(flag)}.frv", tmp_path / f"back{len(flag)}.ppm"
        out = subprocess.run([driver, "encode-file", str(src), str(dst), "--psnr", "40"] + flag, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        frv = dst.read_bytes()
        mdat = struct.unpack("<I", frv[12:16])[0]
        assert (mdat & 0xC0000003) == (0xC0000002 if flag else 0x80000000), hex(mdat)
        out = subprocess.run([driver, "decode-file", str(dst), str(back)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        px = np.frombuffer(back.read_bytes()[-w * h * 3 :], np.uint8)
        assert psnr(px, img) >= 40.0
        sizes[bool(flag)] = len(frv)
    print("driver sizes at 40 dB", sizes)
    assert sizes[True] < sizes[False]
    # --ycbcr needs a lossy target and excludes --rct
    for bad in (["--ycbcr"], ["--ycbcr", "--rct", "--quality", "50"]):
        out = subprocess.run([driver, "encode-file", str(src), str(tmp_path / "bad.frv")] + bad, capture_output=True, text=True, timeout=120)
        assert out.returncode != 0, bad
