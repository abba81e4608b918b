"""Lossy coding to a target size on the device: the rate kernel's models against the emitter's own (emit.finalize_context) on oracle and crafted histograms,
its estimate against tests/rate_model.py and against the files the product emitter writes from the device chain, the batch form, and
fri_hip_search_quality_for_size against a Python replay of its bisection over estimate_size; fri_driver encode-file --size / --bpp."""
import numpy as np
import pytest

from tests import rate_model
from tests.common import gen_image

pytestmark = pytest.mark.gpu
UNCODABLE = rate_model.UNCODABLE


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


def _device_estimate(P, hist, oob=None):
    """fri_hip_estimate_size_dev over a batch hist [N][C][10][1024]: (bytes uint64 [N], models uint32 [N][C][10][4])"""
    import torch

    hist = np.ascontiguousarray(hist, np.uint32)
    n = hist.shape[0]
    d_hist = torch.from_numpy(hist.reshape(-1).view(np.int32).copy()).cuda()
    d_oob = None if oob is None else torch.from_numpy(np.ascontiguousarray(oob, np.uint64).reshape(-1).view(np.int64).copy()).cuda()
    d_bytes = torch.full((n,), 77, dtype=torch.int64, device="cuda")  # the entry point zeroes it
    d_models = torch.full((n * P.channels * 10 * 4,), -1, dtype=torch.int32, device="cuda")
    P.estimate_size(d_hist.data_ptr(), None if d_oob is None else d_oob.data_ptr(), n_images=n, d_bytes=d_bytes.data_ptr(), d_models=d_models.data_ptr())
    torch.cuda.synchronize()
    return d_bytes.cpu().numpy().view(np.uint64), d_models.cpu().numpy().view(np.uint32).reshape(n, P.channels, 10, 4)


def _check_models(hist, models):
    """every context the emitter can code: the device's max_freq_bits and off-distribution count are the emitter's"""
    import frave_amd.emit as emit

    hist = hist.reshape(-1, 10, 1024)
    models = models.reshape(-1, 10, 4)
    for k in range(hist.shape[0]):
        for b in range(10):
            try:
                f, _cdf, off, bits = emit.finalize_context(hist[k, b], b)
            except emit.EmitError:
                assert models[k, b, 3] == 1, (k, b)  # no symbols
                continue
            assert (models[k, b, 0], models[k, b, 1]) == (bits, len(off)), (k, b)
            used = hist[k, b] > 0
            assert models[k, b, 3] == (2 if (f[used] == 0).any() else 0), (k, b)


def _crafted():
    """[N][1][10][1024] histograms covering the model's corners"""
    rng = np.random.default_rng(7)
    out = []
    h = np.ones((10, 1024), np.uint32)  # every symbol once: ~1000 off-distribution values per context and collapsing slots
    out.append(h)
    h = np.ones((10, 1024), np.uint32)
    h[:, :8] = 50  # a peak and a long tail of ones
    h[:, 900:] = 3
    out.append(h)
    h = np.zeros((10, 1024), np.uint32)  # single-symbol contexts, on and off the Laplace peak
    for b in range(10):
        h[b, (0, 1, 7, 100, 1023, 2, 512, 999, 3, 40)[b]] = (1, 2, 300, 4096, 77, 1 << 20, 5, 123456, 9, 1 << 26)[b]
    out.append(h)
    h = np.zeros((10, 1024), np.uint32)  # 2^26 counts in one context, spread and concentrated
    h[:, 0] = 1000
    h[4, :64] = 1 << 20
    h[9, 0] = 1 << 26
    h[9, 1:40] = 12345
    h[9, 700] = 1
    out.append(h)
    for b_heavy in range(3):  # random geometric-tailed contexts
        h = (rng.geometric(0.02 + 0.05 * b_heavy, (10, 1024)) * (rng.random((10, 1024)) < 0.4)).astype(np.uint32)
        h[:, 0] += 1
        out.append(h)
    h = np.ones((10, 1024), np.uint32)
    h[6] = 0  # an empty context: uncodable
    out.append(h)
    return np.stack(out)[:, None]


def test_models_and_bytes_on_crafted_histograms(ctx):
    import frave_amd as fa

    P = fa.Plan(ctx, 320, 240, 1)
    hist = _crafted()
    got, models = _device_estimate(P, hist)
    _check_models(hist, models)
    want = rate_model.estimate(hist)
    assert got[-1] == UNCODABLE and want[-1] == UNCODABLE
    for g, w in zip(got, want):
        assert (g == UNCODABLE) == (w == UNCODABLE)
        if w != UNCODABLE:
            assert abs(int(g) - int(w)) <= 1, (g, w)
    # out-of-alphabet symbols make an image uncodable; NULL counts are not looked at
    oob = np.zeros((len(hist), 1), np.uint64)
    oob[1] = 3
    got2, _ = _device_estimate(P, hist, oob)
    assert got2[1] == UNCODABLE and np.array_equal(np.delete(got2, 1), np.delete(got, 1))
    P.close()


@pytest.mark.parametrize("shape", [(300, 200, 1), (1024, 768, 1), (160, 120, 3), (320, 240, 3)])
def test_models_and_bytes_on_oracle_histograms(ctx, oracle, shape):
    import frave_amd as fa

    w, h, c = shape
    P = fa.Plan(ctx, w, h, c)
    hists, oobs = [], []
    for kind in ("smooth", "noise"):
        img = gen_image(kind, w, h, c, 2)
        for q in (100, 1, 50, 90):
            _, _, _, _, hist, oob, _, _ = rate_model.oracle_arrays(img, w, h, c, q)
            hists.append(hist), oobs.append(oob)
    hist, oob = np.stack(hists), np.stack(oobs)
    got, models = _device_estimate(P, hist, oob)
    _check_models(hist, models)
    want = rate_model.estimate(hist, oob)
    assert np.all(np.abs(got.astype(np.int64) - want.astype(np.int64)) <= 1), (got, want)
    for k in range(len(hist)):  # the host form
        assert P.estimate_size(hist[k], oob[k]) == got[k]
    P.close()


def _stream_file(P, img, q):
    import frave_amd as fa
    import frave_amd.emit as emit

    sym, vp, wp, hist, oob = P.encode_image_symbols(img, fa.quality_matrix(q))
    assert not oob.any()
    return emit.encode_image_from_streams(P.width, P.height, sym, hist, vp, wp, quality=q if q < 100 else 0), hist, oob


@pytest.mark.parametrize("shape", [(4096, 4096, 1), (1024, 768, 3)])
def test_estimate_of_chain_histograms_is_within_24_bytes_per_channel_of_the_file(ctx, shape):
    import frave_amd as fa

    w, h, c = shape
    img = gen_image("noise", w, h, c, 3)
    img[: h // 2] = gen_image("smooth", w, h // 2, c, 4)
    P = fa.Plan(ctx, w, h, c)
    P.set_stream_order()
    for q in (1, 50, 90, 100):
        frv, hist, oob = _stream_file(P, img, q)
        est = P.estimate_size(hist, oob)
        print(shape, q, "estimate", est, "file", len(frv), "gap", est - len(frv))
        assert abs(est - len(frv)) <= 24 * c, (q, est, len(frv))
        assert abs(est - rate_model.estimate_image(hist, oob)) <= 1
    P.close()


def test_batch_equals_single_images_and_repeats_bit_for_bit(ctx):
    import frave_amd as fa

    w, h, c = 320, 240, 3
    P = fa.Plan(ctx, w, h, c)
    P.set_stream_order()
    hists, oobs, single = [], [], []
    for k in range(8):
        img = gen_image("noise" if k % 2 else "smooth", w, h, c, 10 + k)
        _, _, _, hist, oob = P.encode_image_symbols(img, fa.quality_matrix((10, 35, 60, 85, 100, 5, 50, 95)[k]))
        hists.append(hist), oobs.append(oob)
        single.append(P.estimate_size(hist, oob))
    hist, oob = np.stack(hists), np.stack(oobs)
    a_bytes, a_models = _device_estimate(P, hist, oob)
    b_bytes, b_models = _device_estimate(P, hist, oob)
    assert np.array_equal(a_bytes, np.array(single, np.uint64))
    assert np.array_equal(a_bytes, b_bytes) and np.array_equal(a_models, b_models)
    assert len(set(single)) == 8
    P.close()


def _replay(P, img, max_bytes):
    """fri_hip_search_quality_for_size's bisection through the public entry points: the chain's histograms, then estimate_size"""
    import frave_amd as fa

    lo, hi, lo_est = 0, 101, 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        _, _, _, hist, oob = P.encode_image_symbols(img, fa.quality_matrix(mid))
        est = P.estimate_size(hist, oob)
        if est != UNCODABLE and est <= max_bytes:
            lo, lo_est = mid, est
        else:
            hi = mid
    return lo, lo_est


def test_search_is_the_bisection(ctx):
    import torch

    import frave_amd as fa

    w, h, c = 640, 480, 1
    img = gen_image("smooth", w, h, c, 21)
    P = fa.Plan(ctx, w, h, c)
    P.set_stream_order()
    P.set_dequantiser(fa.DEQUANT_MIDPOINT)
    est = {}
    for q in range(1, 101):
        _, _, _, hist, oob = P.encode_image_symbols(img, fa.quality_matrix(q))
        est[q] = P.estimate_size(hist, oob)
    assert all(est[q] <= est[q + 1] for q in range(1, 100)), est  # the image's rate rises with quality: the bisection finds the boundary
    steps = [q for q in range(1, 100) if est[q] < est[q + 1]]
    assert len(steps) > 20
    probe = fa.quality_matrix(40)
    coefs = P.transform_quant(img, probe)
    before = (P.inverse_transform(coefs, probe), P.encode_image_symbols(img, probe)[0])
    d_px = torch.from_numpy(img.reshape(-1).copy()).cuda()
    for q in (steps[0], steps[len(steps) // 3], steps[len(steps) // 2], steps[-1]):
        for budget in (est[q], est[q + 1] - 1):
            got = P.search_quality_for_size(img, budget)
            assert got == (q, est[q]), (q, budget)
            assert P.search_quality_for_size(d_px.data_ptr(), budget) == got
            assert _replay(P, img, budget) == got
    assert P.search_quality_for_size(img, est[100] + 1000) == (100, est[100])
    with pytest.raises(fa.FriHipError) as e:
        P.search_quality_for_size(img, est[1] - 1)
    assert e.value.code == -7
    # the plan's dequantiser and stream order are what they were
    after = (P.inverse_transform(coefs, probe), P.encode_image_symbols(img, probe)[0])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    P.close()


def test_search_on_rgb(ctx):
    import frave_amd as fa

    w, h, c = 320, 200, 3
    img = gen_image("smooth", w, h, c, 22)
    P = fa.Plan(ctx, w, h, c)
    P.set_stream_order()
    _, _, _, hist, oob = P.encode_image_symbols(img, fa.quality_matrix(60))
    budget = P.estimate_size(hist, oob)
    q, e = P.search_quality_for_size(img, budget)
    assert (q, e) == _replay(P, img, budget) and q >= 60 and e <= budget
    P.close()


def test_driver_size_and_bpp(ctx, tmp_path):
    import os
    import re
    import subprocess

    import frave_amd as fa
    import frave_amd.emit as emit

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "frave_amd", "host")])
    for c, magic, suffix in ((1, b"P5", "pgm"), (3, b"P6", "ppm")):
        w, h = 320, 200
        img = gen_image("smooth", w, h, c, 60 + c)
        img[: h // 4] = gen_image("noise", w, h // 4, c, 70 + c)
        src = tmp_path / f"in.{suffix}"
        src.write_bytes(magic + b"\n%d %d\n255\n" % (w, h) + img.tobytes())
        P = fa.Plan(ctx, w, h, c)
        P.set_stream_order()
        est = {}
        for q in (1, 50, 100):
            _, _, _, hist, oob = P.encode_image_symbols(img, fa.quality_matrix(q))
            est[q] = P.estimate_size(hist, oob)
        P.close()
        lossless, middle = est[100], (est[1] + est[100]) // 2
        bpp = "%.3f" % (8 * est[50] / (w * h) + 0.01)
        for flag, budget in ((["--size", str(middle)], middle), (["--bpp", bpp], int(float(bpp) * w * h / 8)), (["--size", str(lossless + 5000)], lossless + 5000)):
            dst, back = tmp_path / f"out_{c}_{flag[1]}.frv", tmp_path / f"back_{c}_{flag[1]}.{suffix}"
            out = subprocess.run([driver, "encode-file", str(src), str(dst)] + flag, capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stdout + out.stderr
            m = re.search(r"target (\d+) bytes: quality (\d+), estimate (\d+) bytes, file (\d+) bytes", out.stdout)
            assert m, out.stdout
            assert int(m.group(1)) == budget
            data = dst.read_bytes()
            assert len(data) <= budget and len(data) == int(m.group(4))
            quality = int(m.group(2))
            d = emit.decode_image(data)
            assert d.quality == (quality if quality < 100 else 0) and d[:3] == (w, h, c)
            if budget > lossless:
                assert quality == 100
            out = subprocess.run([driver, "decode-file", str(dst), str(back)], capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stderr
        bad = subprocess.run([driver, "encode-file", str(src), str(tmp_path / "x.frv"), "--size", "100", "--quality", "50"], capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2
        tiny = subprocess.run([driver, "encode-file", str(src), str(tmp_path / "x.frv"), "--size", "100"], capture_output=True, text=True, timeout=300)
        assert tiny.returncode == 1 and "no quality fits" in tiny.stderr
