"""SSIM on the device (K7, fri_hip_measure_ssim*; fri_hip_search_quality_ssim*) against tests/ssim_ref.py, bit for bit:

- K7 on shapes from 8 x 8 to 4096 x 4096, luma and RGB, on identical rasters, 0 against 255, noise against smooth and K3's midpoint reconstruction against
  its source, through the host form and the device form at byte offsets that start no row on a dword;
- the n-image form with garbage between the images, three runs;
- the search against a replay of its bisection built from K1, K3 and the oracle, on plain and YCbCr plans, and its refusals;
- a file at the quality found, decoded by the product decoder and K3, and fri_driver encode-file --ssim."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import ssim_ref
from tests.common import gen_image
from tests.later_cases import SSIM_BAND_CASES, SSIM_EDGE_SHAPES
from tests.oracle_ref import MIDPOINT
from tests.test_rct_host import correlated_image
from tests.ycbcr_ref import COLOUR_YCBCR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 8, 1), (9, 13, 3), (8, 300, 1), (300, 9, 3), (640, 480, 1), (1001, 613, 3), (4096, 4096, 1), (2048, 1536, 3)]
SHAPES += SSIM_EDGE_SHAPES  # W / 4 = 1 and 2 mod 128: the last strip `full` with its third block the row's last, and a last strip of one lane with two blocks
RELAXED = 2  # hipStreamCaptureModeRelaxed


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


def _image(w, h, c, seed):
    img = correlated_image(w, h, seed)
    return np.ascontiguousarray(img if c == 3 else img[:, :, 1:2]).reshape(-1)


def _pairs(ctx, w, h, c):
    import frave_amd as fa

    n = w * h * c
    noise = gen_image("noise", w, h, c, 5).reshape(-1)
    smooth = gen_image("smooth", w, h, c, 6).reshape(-1)
    src = _image(w, h, c, 7)
    R = fa.Plan(ctx, w, h, c)
    R.set_dequantiser(MIDPOINT)
    qm = fa.quality_matrix(30)
    recon = R.inverse_transform(R.transform_quant(src, qm), qm)
    R.close()
    return [("identical", noise, noise.copy()), ("0-255", np.zeros(n, np.uint8), np.full(n, 255, np.uint8)), ("noise-smooth", noise, smooth),
            ("k3-midpoint", src, recon)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_k7_equals_the_oracle(ctx, shape):
    import torch

    import frave_amd as fa

    w, h, c = shape
    P = fa.Plan(ctx, w, h, c)
    nx, ny = ssim_ref.windows(w, h)
    for name, a, b in _pairs(ctx, w, h, c):
        want = ssim_ref.measure(a, b, w, h, c)
        got = P.measure_ssim(a, b)
        assert np.array_equal(got, want), (name, got, want)
        if name == "identical":
            assert list(got) == [nx * ny << 32] * c + [nx * ny]
        # the device form at byte offsets 1 and 3: no row of either raster starts on a dword
        n = P.pixel_bytes
        buf = torch.from_numpy(np.random.default_rng(1).integers(0, 256, 2 * n + 16, dtype=np.uint8)).cuda()
        buf[1 : 1 + n] = torch.from_numpy(a)
        buf[n + 3 : 2 * n + 3] = torch.from_numpy(b)
        d_out = torch.full((c + 1,), -7, dtype=torch.int64, device="cuda")
        P.measure_ssim_dev(buf.data_ptr() + 1, buf.data_ptr() + n + 3, d_out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), want), name
        print(shape, name, fa.ssim_of(got, c)[0])
    P.close()


@pytest.mark.parametrize("shape", [(300, 9, 3), (640, 480, 1), (1001, 613, 3)], ids=lambda s: "x".join(map(str, s)))
def test_n_image_form_equals_single_calls(ctx, shape):
    import torch

    import frave_amd as fa

    w, h, c = shape
    P = fa.Plan(ctx, w, h, c)
    n, k = P.pixel_bytes, 3
    stride = n + 37  # image k starts at byte 37 k: no dword alignment for k > 0
    rng = np.random.default_rng(11)
    A = rng.integers(0, 256, k * stride, dtype=np.uint8)  # garbage in the gaps
    B = rng.integers(0, 256, k * stride, dtype=np.uint8)
    want = []
    for i in range(k):
        a = _image(w, h, c, 20 + i)
        b = np.clip(a.astype(np.int32) + rng.integers(-9 * i - 1, 9 * i + 2, n), 0, 255).astype(np.uint8)
        A[i * stride : i * stride + n], B[i * stride : i * stride + n] = a, b
        want.append(P.measure_ssim(a, b))
        assert np.array_equal(want[-1], ssim_ref.measure(a, b, w, h, c))
    d_a, d_b = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    runs = []
    for _ in range(3):
        d_out = torch.full((k, c + 1), 12345, dtype=torch.int64, device="cuda")
        P.measure_ssim_dev(d_a.data_ptr(), d_b.data_ptr(), d_out.data_ptr(), n_images=k, pixel_stride=stride)
        torch.cuda.synchronize()
        runs.append(d_out.cpu().numpy())
    assert all(np.array_equal(r, runs[0]) for r in runs)
    assert np.array_equal(runs[0], np.stack(want))
    P.close()


@pytest.mark.parametrize("case", [c for c, _ in SSIM_BAND_CASES], ids=lambda c: "x".join(map(str, c)))
def test_n_image_form_with_bands_above_four_rows(ctx, case):
    """launch_ssim's band size above 4 and at its clamp of 64 (tests/later_cases.py has the arithmetic, tests/test_later_cases_host.py checks it): a ragged
    last band, waves whose band starts past the last window row. Narrow, tall rasters, many images; every image against tests/ssim_ref.py."""
    import torch

    import frave_amd as fa

    w, h, c, k = case
    P = fa.Plan(ctx, w, h, c)
    n = P.pixel_bytes
    stride = n + 5  # image k starts at byte 5 k (+ 1 and + 3 below): no dword alignment
    rng = np.random.default_rng(k)
    A = rng.integers(0, 256, k * stride, dtype=np.uint8)  # garbage in the gaps
    B = rng.integers(0, 256, k * stride, dtype=np.uint8)
    want = []
    for i in range(k):
        a = A[i * stride : i * stride + n]
        if i % 3 == 0:  # every third pair is close: source and source + small noise
            B[i * stride : i * stride + n] = np.clip(a.astype(np.int32) + rng.integers(-6, 7, n), 0, 255).astype(np.uint8)
        want.append(ssim_ref.measure(a, B[i * stride : i * stride + n], w, h, c))
    d_a = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), A])).cuda()
    d_b = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), B])).cuda()
    d_out = torch.full((k, c + 1), 12345, dtype=torch.int64, device="cuda")
    P.measure_ssim_dev(d_a.data_ptr() + 1, d_b.data_ptr() + 3, d_out.data_ptr(), n_images=k, pixel_stride=stride)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(got, np.stack(want)), np.flatnonzero((got != np.stack(want)).any(axis=1))[:8].tolist()
    P.close()


def _replay(ctx, img, w, h, c, colour):
    """the bisection of fri_hip_search_quality_ssim restated: K1 (transform_quant_dev, quality_matrix(q)), K3 (inverse_transform_dev, midpoint), the oracle"""
    import torch

    import frave_amd as fa

    R = fa.Plan(ctx, w, h, c)
    if colour:
        R.set_colour_transform(colour)
    R.set_dequantiser(MIDPOINT)
    d_px = torch.from_numpy(img).cuda()
    d_co = torch.empty(R.coef_count, dtype=torch.int32, device="cuda")
    d_rec = torch.empty(R.pixel_bytes, dtype=torch.uint8, device="cuda")
    memo = {}

    def ssim_at(q):
        if q not in memo:
            qm = fa.quality_matrix(q)
            R.transform_quant_dev(d_px.data_ptr(), d_co.data_ptr(), qm)
            R.inverse_transform_dev(d_co.data_ptr(), d_rec.data_ptr(), qm)
            torch.cuda.synchronize()
            memo[q] = ssim_ref.ssim(img, d_rec.cpu().numpy(), w, h, c)
        return memo[q]

    def search(target):
        lo, hi, best = 0, 100, 1.0
        while hi - lo > 1:
            mid = (lo + hi) // 2
            s = ssim_at(mid)
            if s >= target:
                hi, best = mid, s
            else:
                lo = mid
        return hi, best

    return search, ssim_at, R


@pytest.mark.parametrize("case", [(640, 480, 1, 0), (1001, 613, 3, 0), (1001, 613, 3, COLOUR_YCBCR)], ids=["640x480x1", "1001x613x3", "1001x613x3-ycbcr"])
def test_search_equals_the_replay(ctx, case):
    import torch

    import frave_amd as fa

    w, h, c, colour = case
    img = _image(w, h, c, 31)
    P = fa.Plan(ctx, w, h, c)
    if colour:
        P.set_colour_transform(colour)
    qm = fa.quality_matrix(40)
    before = P.inverse_transform(P.transform_quant(img, qm), qm)  # the plan's own dequantiser (the reference's division)
    search, ssim_at, R = _replay(ctx, img, w, h, c, colour)
    d_px = torch.from_numpy(img).cuda()
    found = []
    for target in (0.80, 0.95, 0.99):
        want = search(target)
        assert P.search_quality_ssim(img, target) == want, target
        assert P.search_quality_ssim(d_px.data_ptr(), target) == want, target
        q, s = want
        assert s >= target and (q == 1 or ssim_at(q - 1) < target)
        found.append(want)
    print(case, found)
    assert found[0][0] < 100 and found[0][0] <= found[2][0]
    assert P.search_quality_ssim(img, 1.0) == (100, 1.0)  # no lossy quality reaches 1 on these images: "code losslessly"
    after = P.inverse_transform(P.transform_quant(img, qm), qm)
    assert np.array_equal(before, after)  # the plan's dequantiser is as it was ...
    assert not np.array_equal(after, R.inverse_transform(R.transform_quant(img, qm), qm))  # ... and it is not the midpoint one
    P.close(), R.close()


def test_search_refusals(ctx):
    import torch

    import frave_amd as fa

    w, h = 64, 48
    img = _image(w, h, 3, 2)
    P = fa.Plan(ctx, w, h, 3)
    P.set_colour_transform(fa.api.COLOUR_RCT)
    with pytest.raises(fa.FriHipError) as e:
        P.search_quality_ssim(img, 0.9)
    assert e.value.code == -1
    P.set_colour_transform(fa.api.COLOUR_NONE)
    want = P.search_quality_ssim(img, 0.9)
    hip = C.CDLL("libamdhip64.so")
    d_px = torch.from_numpy(img).cuda()
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    try:
        with pytest.raises(fa.FriHipError) as e:
            P.search_quality_ssim(d_px.data_ptr(), 0.9, stream=s.cuda_stream)
        assert e.value.code == -1 and "graph" in str(e.value)
    finally:
        graph = C.c_void_p()
        hip.hipStreamEndCapture(sp, C.byref(graph))
        if graph.value:
            hip.hipGraphDestroy(graph)
    assert P.search_quality_ssim(d_px.data_ptr(), 0.9, stream=s.cuda_stream) == want
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(fa.FriHipError):
            P.search_quality_ssim(img, bad)
    P.close()


@pytest.mark.parametrize("case", [(640, 480, 1, 0), (1001, 613, 3, COLOUR_YCBCR)], ids=["640x480x1", "1001x613x3-ycbcr"])
def test_file_at_the_found_quality_decodes_to_the_reported_ssim(ctx, case):
    import frave_amd as fa
    import frave_amd.emit as emit

    w, h, c, colour = case
    img = _image(w, h, c, 51)
    P = fa.Plan(ctx, w, h, c)
    if colour:
        P.set_colour_transform(colour)
    q, s = P.search_quality_ssim(img, 0.95)
    assert 1 <= q < 100 and s >= 0.95
    qm = fa.quality_matrix(q)
    P.set_stream_order()
    sym, vp, wp, hist, oob = P.encode_image_symbols(img, qm, fit=True)
    assert not oob.any()
    frv = emit.encode_image_from_streams(w, h, sym, hist, vp, wp, quality=q, ycbcr=bool(colour))
    d = emit.decode_image(frv)
    assert d.quality == q and d.ycbcr == bool(colour)
    P.set_dequantiser(MIDPOINT)
    back = P.inverse_transform(d[4], fa.quality_matrix(d.quality))
    assert ssim_ref.ssim(img, back, w, h, c) == s
    assert fa.ssim_of(P.measure_ssim(img, back), c)[0] == s
    print(case, q, s, len(frv))
    P.close()


def test_driver_encodes_to_an_ssim(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    w, h = 320, 200
    img = correlated_image(w, h, 4)
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + img.tobytes())
    for flag in ([], ["--ycbcr"]):
        dst, back = tmp_path / f"out{len(flag)}.frv", tmp_path / f"back{len(flag)}.ppm"
        out = subprocess.run([driver, "encode-file", str(src), str(dst), "--ssim", "0.95"] + flag, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "target SSIM 0.9500: quality" in out.stdout and "decoded SSIM" in out.stdout, out.stdout
        frv = dst.read_bytes()
        mdat = struct.unpack("<I", frv[12:16])[0]
        out2 = subprocess.run([driver, "decode-file", str(dst), str(back)], capture_output=True, text=True, timeout=300)
        assert out2.returncode == 0, out2.stderr
        px = np.frombuffer(back.read_bytes()[-w * h * 3 :], np.uint8)
        s = ssim_ref.ssim(img.reshape(-1), px, w, h, 3)
        assert s >= 0.95
        assert f"decoded SSIM {s:.6f}" in out.stdout
        if flag and "lossless RCT" not in out.stdout:
            assert (mdat & 0xC0000003) == 0xC0000002, hex(mdat)
        print(flag, len(frv), s, out.stdout.splitlines()[0])
