"""Reversible colour transform on the device (fri_hip_plan_set_colour_transform): K1 with RCT codes oracle(rct(pixels)), K3 with RCT writes
inverse_rct(K3 without it), and the whole round trip is lossless - through every route that reaches the kernels. Bit-exact throughout."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.common import KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS, gen_image
from tests.test_rct_host import correlated_image, inverse_rct, rct

pytestmark = pytest.mark.gpu
RCT = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


def _image(w, h, seed):
    """noise with a smooth band and a correlated band: every leaf value, and R / B that sit close to G"""
    img = gen_image("noise", w, h, 3, seed)
    img[: h // 3] = gen_image("smooth", w, h // 3, 3, seed + 1)
    if h >= 6:
        img[h // 3 : 2 * (h // 3)] = correlated_image(w, h // 3, seed)
    return img


def _rct_dev(px):
    """rct() of a flat uint8 tensor on the device (images too large for host copies)"""
    import torch

    p = px.view(-1, 3).to(torch.int32)
    return torch.stack([p[:, 1], (p[:, 2] - p[:, 1] + 128) & 255, (p[:, 0] - p[:, 1] + 128) & 255], dim=1).to(torch.uint8).view(-1)


def _inverse_rct_dev(px):
    import torch

    p = px.view(-1, 3).to(torch.int32)
    return torch.stack([(p[:, 2] + p[:, 0] - 128) & 255, p[:, 0], (p[:, 1] + p[:, 0] - 128) & 255], dim=1).to(torch.uint8).view(-1)


def _rct_plan(ctx, w, h):
    import frave_amd as fa

    P = fa.Plan(ctx, w, h, 3)
    P.set_colour_transform(RCT)
    return P


# the small shapes of test_gpu_parity.py, odd widths / heights, and 1080p
SHAPES = [(64, 48), (100, 37), (33, 17), (300, 200), (129, 65), (256, 192), (257, 191), (333, 777), (1021, 67), (1920, 1080)]


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_is_the_oracle_of_rct_pixels(ctx, oracle, shape):
    w, h = shape
    img = _image(w, h, 11)
    P = _rct_plan(ctx, w, h)
    want = oracle.Wavelet(rct(img), h, w, 3).coefficients()
    assert np.array_equal(P.transform_quant(img), want)
    q = np.ones(32, np.int32)
    q[:10] = [1, 2, 3, 1, 2, 1, 4, 1, 2, 3]
    W = oracle.Wavelet(rct(img), h, w, 3)
    W.quantize(q)
    assert np.array_equal(P.transform_quant(img, q), W.coefficients())
    # and the default mode is back to the plain transform
    P.set_colour_transform(0)
    assert np.array_equal(P.transform_quant(img), oracle.Wavelet(img, h, w, 3).coefficients())
    P.close()


@pytest.mark.parametrize("offset", [1, 2, 3, 7, 13])
def test_forward_from_unaligned_pointers(ctx, oracle, offset):
    import torch

    w, h = 301, 77
    img = _image(w, h, 5)
    P = _rct_plan(ctx, w, h)
    buf = torch.zeros(P.pixel_bytes + 64, dtype=torch.uint8, device="cuda")
    buf[offset : offset + P.pixel_bytes] = torch.from_numpy(img.reshape(-1).copy()).cuda()
    d_co = torch.empty(P.coef_count, dtype=torch.int32, device="cuda")
    P.transform_quant_dev(buf.data_ptr() + offset, d_co.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_co.cpu().numpy().reshape(3, -1, 512), oracle.Wavelet(rct(img), h, w, 3).coefficients())
    P.close()


def test_batch_form(ctx, oracle):
    w, h = 640, 360
    imgs = [_image(w, h, 20 + k) for k in range(9)]
    P = _rct_plan(ctx, w, h)
    outs = P.transform_quant_batch(imgs)  # nine images in one launch
    for img, got in zip(imgs, outs):
        assert np.array_equal(got, oracle.Wavelet(rct(img), h, w, 3).coefficients())
    P.close()


def test_every_candidate_tiling(ctx, oracle):
    """The RGB candidates fri_hip_plan_tune_forward chooses from, pinned one by one (as tests/test_gpu_tune.py does for planes)."""
    import frave_amd as fa

    w, h = 1024, 768
    img = _image(w, h, 8)
    want = oracle.Wavelet(rct(img), h, w, 3).coefficients()
    keys = ("FRI_HIP_TUNING", "FRI_HIP_STRIDED_SHARES", "FRI_HIP_BAND_ROWS", "FRI_HIP_CELLS_PER_TILE", "FRI_HIP_RANK_WEIGHTS")
    saved = {k: os.environ.get(k) for k in keys}
    try:
        os.environ["FRI_HIP_TUNING"] = "1"
        for spec in ({"FRI_HIP_STRIDED_SHARES": "1", "FRI_HIP_BAND_ROWS": "12"}, {"FRI_HIP_STRIDED_SHARES": "1", "FRI_HIP_BAND_ROWS": "24"},
                     {"FRI_HIP_STRIDED_SHARES": "0", "FRI_HIP_BAND_ROWS": "16"}, {"FRI_HIP_STRIDED_SHARES": "1", "FRI_HIP_BAND_ROWS": "8"},
                     {"FRI_HIP_STRIDED_SHARES": "0", "FRI_HIP_BAND_ROWS": "32"}):
            for k in keys[1:]:
                os.environ.pop(k, None)
            os.environ.update(spec)
            P = _rct_plan(ctx, w, h)
            assert np.array_equal(P.transform_quant(img), want), spec
            assert np.array_equal(P.inverse_transform(want), img.reshape(-1)), spec
            P.close()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    # the tuner on an RCT plan: the winner still gives the oracle's coefficients of rct(pixels)
    P = _rct_plan(ctx, w, h)
    assert P.tune_forward(16)["tuned"] in (True, False)
    assert np.array_equal(P.transform_quant(img), want)
    P.close()


def test_4096_and_samples_at_16384(ctx, oracle):
    import torch

    w = h = 4096
    img = _image(w, h, 3)
    P = _rct_plan(ctx, w, h)
    assert np.array_equal(P.transform_quant(img), oracle.Wavelet(rct(img), h, w, 3).coefficients())
    P.close()
    w = h = 16384
    P = _rct_plan(ctx, w, h)
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    d_px = torch.randint(0, 256, (P.pixel_bytes,), dtype=torch.uint8, device="cuda", generator=g)
    d_px[: w * 3 * 2000] = torch.from_numpy(correlated_image(w, 2000, 4).reshape(-1)).cuda()
    d_co = torch.empty(P.coef_count, dtype=torch.int32, device="cuda")
    P.transform_quant_dev(d_px.data_ptr(), d_co.data_ptr())
    torch.cuda.synchronize()
    centers = P.centers()
    pick = np.random.default_rng(9).choice(len(centers), 2000, replace=False)
    pick = np.concatenate([pick, np.arange(64), np.arange(len(centers) - 64, len(centers))])
    want, kept = oracle.cell_coefficients(_rct_dev(d_px).cpu().numpy(), h, w, 3, centers[pick])
    assert kept.all()
    got = d_co.view(3, -1, 512)[:, torch.from_numpy(pick).cuda()].permute(1, 0, 2).cpu().numpy()
    assert np.array_equal(got, want)
    del d_co, d_px
    torch.cuda.empty_cache()
    P.close()


@pytest.mark.parametrize("fit", [False, True])
def test_encode_chains(ctx, oracle, fit):
    """encode_image (with and without the fit) and encode_image_symbols (K1's C16 instance) on an RCT plan: what the plain chain makes of rct(pixels),
    and the coefficients are the oracle's"""
    import frave_amd as fa

    w, h = 512, 384
    img = _image(w, h, 30)
    P, Q = _rct_plan(ctx, w, h), fa.Plan(ctx, w, h, 3)
    vp = np.stack([np.asarray(KAT_VALUE_PARAMS, np.float32).reshape(3, 6)] * 3)
    wp = np.stack([np.asarray(KAT_WIDTH_PARAMS, np.float32).reshape(3, 6)] * 3)
    got = P.encode_image(img, fit=fit, value_params=vp, width_params=wp)
    ref = Q.encode_image(rct(img), fit=fit, value_params=vp, width_params=wp)
    assert np.array_equal(got[0], oracle.Wavelet(rct(img), h, w, 3).coefficients())
    for a, b in zip(got, ref):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    P.set_stream_order(), Q.set_stream_order()
    got = P.encode_image_symbols(img, fit=fit, value_params=vp, width_params=wp)
    ref = Q.encode_image_symbols(rct(img), fit=fit, value_params=vp, width_params=wp)
    for a, b in zip(got, ref):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    P.close(), Q.close()


@pytest.mark.parametrize("shape", [(333, 777), (1021, 67), (512, 512)])
def test_inverse_scanning_and_lists_kernels(ctx, shape):
    """odd widths: the scanning K3; 512 x 512 (rows of a multiple of 16 bytes): the lists kernel"""
    import frave_amd as fa

    w, h = shape
    img = _image(w, h, 40)
    P, Q = _rct_plan(ctx, w, h), fa.Plan(ctx, w, h, 3)
    co = P.transform_quant(img)
    got = P.inverse_transform(co)
    assert np.array_equal(got, inverse_rct(Q.inverse_transform(co)))
    assert np.array_equal(got, img.reshape(-1))
    rnd = np.random.default_rng(1).integers(-300, 300, co.shape).astype(np.int32)  # coefficients no encoder makes: the clamp comes first
    rnd[co == -(2 ** 31)] = -(2 ** 31)
    assert np.array_equal(P.inverse_transform(rnd), inverse_rct(Q.inverse_transform(rnd)))
    P.close(), Q.close()


def test_inverse_at_16384(ctx):
    """more than 400 000 cells: the inverse runs on the forward plan's shares (the lists kernel); on the device, in place of host copies of 3 GB"""
    import torch

    import frave_amd as fa

    w = h = 16384
    P = _rct_plan(ctx, w, h)
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    d_px = torch.randint(0, 256, (P.pixel_bytes,), dtype=torch.uint8, device="cuda", generator=g)
    d_co = torch.empty(P.coef_count, dtype=torch.int32, device="cuda")
    P.transform_quant_dev(d_px.data_ptr(), d_co.data_ptr())
    out_rct = torch.empty_like(d_px)
    P.inverse_transform_dev(d_co.data_ptr(), out_rct.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out_rct, d_px)  # lossless
    Q = fa.Plan(ctx, w, h, 3)
    out_plain = torch.empty_like(d_px)
    Q.inverse_transform_dev(d_co.data_ptr(), out_plain.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out_rct, _inverse_rct_dev(out_plain))
    del d_co, d_px, out_rct, out_plain
    torch.cuda.empty_cache()
    P.close(), Q.close()


@pytest.mark.parametrize("shape", [(512, 512), (257, 191), (33, 17), (1920, 1080), (4096, 4096)])
def test_lossless_round_trip(ctx, shape):
    w, h = shape
    img = _image(w, h, 50)
    import frave_amd as fa

    P, Q = _rct_plan(ctx, w, h), fa.Plan(ctx, w, h, 3)
    back = P.inverse_transform(P.transform_quant(img)).reshape(-1, 3)
    white = np.full((h, w, 3), 255, np.uint8)
    covered = (Q.inverse_transform(Q.transform_quant(white)).reshape(-1, 3) == 255).all(axis=1)  # pixels of a retained cell (a thin image has others)
    assert np.array_equal(back[covered], img.reshape(-1, 3)[covered])
    assert (back[~covered] == 0).all()  # the others stay 0 in all three channels
    P.close(), Q.close()


def test_graph_replay(ctx, oracle):
    import torch

    hip = C.CDLL("libamdhip64.so")
    w, h = 640, 360
    P = _rct_plan(ctx, w, h)
    imgs = [_image(w, h, 60 + k) for k in range(3)]
    d_px = torch.from_numpy(imgs[0].reshape(-1).copy()).cuda()
    d_co = torch.empty(P.coef_count, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, 2) == 0  # relaxed; one stream, one kernel node
    P.transform_quant_dev(d_px.data_ptr(), d_co.data_ptr(), stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    P.set_colour_transform(0)  # the captured launch keeps the mode of its capture
    for img in imgs:
        d_px.copy_(torch.from_numpy(img.reshape(-1).copy()))
        d_co.fill_(7)
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(ex, sp) == 0
        s.synchronize()
        assert np.array_equal(d_co.cpu().numpy().reshape(3, -1, 512), oracle.Wavelet(rct(img), h, w, 3).coefficients())
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    P.close()


def test_multi_with_rct_on_both_plans(oracle):
    import frave_amd as fa

    w, h = 320, 240
    imgs = [_image(w, h, 70 + k) for k in range(4)]
    M = fa.Multi([0, 0], w, h, 3)
    M.set_colour_transform(RCT)
    for img, got in zip(imgs, M.transform_quant(imgs)):
        assert np.array_equal(got, oracle.Wavelet(rct(img), h, w, 3).coefficients())
    coefs = M.encode_image(imgs, fit=True)[0]
    for img, co in zip(imgs, coefs):
        assert np.array_equal(co, oracle.Wavelet(rct(img), h, w, 3).coefficients())
    M.close()


def test_driver_rct_file_round_trip(tmp_path):
    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h = 320, 200
    img = correlated_image(w, h, 3)
    src = tmp_path / "in.ppm"
    ppm = b"P6\n%d %d\n255\n" % (w, h) + img.tobytes()
    src.write_bytes(ppm)
    sizes = {}
    for flag in ([], ["--rct"]):
        dst, back = tmp_path / f"out{len(flag)}.frv", tmp_path / f"back{len(flag)}.ppm"
        out = subprocess.run([driver, "encode-file", str(src), str(dst)] + flag, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        frv = dst.read_bytes()
        assert (struct.unpack("<I", frv[12:16])[0] & 0xC0000001) == (0xC0000001 if flag else 0x80000000)
        out = subprocess.run([driver, "decode-file", str(dst), str(back)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert back.read_bytes() == ppm
        sizes[bool(flag)] = len(frv)
    print("driver sizes", sizes)
    assert sizes[True] < sizes[False]
