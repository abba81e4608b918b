"""The quality searches, the size estimate and the device rANS coder of tiled 4:2:0 coding on the device (include/fri_hip.h, "Tiled 4:2:0 coding"):

- K12's measuring kernel exactly against numpy (tests/tiled420_ref.merge_tiles420, then per-channel SSE, max and count) on every shape of the split and merge
  tests, random planes whose replicated samples differ from the image's edge, pointers 0, 1 and 3 bytes off; sums past 2^32; several strips per lane, ragged
  and clamped; graph capture;
- fri_hip_estimate_size_tiled420_dev against tests/tiled420_rate_ref.py on synthetic histograms with empty contexts and an out-of-alphabet count, and against the
  files the emitter writes from the device's streams;
- each search against a replay of its documented bisection in Python, the evaluator made of entry points that existed before the searches;
- fri_hip_encode_image_tiled420_coded + fri_tiled_encode_from_coded420 byte for byte the file of the host coder;
- fri_driver encode-file --tile-size-420 with --device-rans and with --target."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd import api
from frave_amd.api import TILED_ALLOW_HOLES, PlanTiled420, tile_shape420
from tests import ssim_ref, tiled420_rate_ref
from tests.common import gen_image
from tests.oracle_ref import MIDPOINT, REFERENCE
from tests.test_gpu_instances import Guarded
from tests.test_gpu_tiled420 import IMAGE, SHAPES
from tests.test_gpu_tiled_search import _bisect_lowest, _synthetic_hist
from tests.tiled420_ref import merge_tiles420, plane_order, split_tiles420
from tests.tiled_ref import mixed_image, parse_frit

for _name in ("measure_distortion_tiled420_dev", "estimate_size_tiled420", "estimate_size_tiled420_dev", "search_quality", "search_quality_ssim", "search_quality_for_size",
              "encode_image_tiled420_coded"):
    assert hasattr(PlanTiled420, _name), _name  # (without the feature the module fails here)
tiled_encode_from_coded420 = emit.tiled_encode_from_coded420

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELAXED = 2  # hipStreamCaptureModeRelaxed
UNCODABLE = 2 ** 64 - 1
assert len(SHAPES) == 9 and SHAPES[0] == (1, 1, 1, 1) and SHAPES[-1] == (1023, 767, 512, 512)


@pytest.fixture(scope="module")
def ctx():
    c = fa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


def _ids(s):
    return "x".join(map(str, s))


# ---- the measuring kernel -----------------------------------------------------------------------------------------------------------------------------------

def _numpy_measure(y_tiles, c_tiles, ref, w, h):
    """uint64 [7]: per channel the SSE and the largest absolute difference of the merged planes against ref, then W H"""
    d = merge_tiles420(y_tiles, c_tiles, w, h).astype(np.int64) - ref.reshape(h, w, 3).astype(np.int64)
    out = []
    for ch in range(3):
        out += [int((d[:, :, ch] ** 2).sum()), int(np.abs(d[:, :, ch]).max())]
    return np.array(out + [w * h], np.uint64)


def _device_measure(torch, T, d_y, d_c, d_ref, stream=0):
    d_out = torch.full((7,), -1, dtype=torch.int64, device="cuda")  # (the call zeroes it)
    T.measure_distortion_tiled420_dev(d_y, d_c, d_ref, d_out.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint64)


def _random_planes(T, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (T.n_tiles, T.tile_h, T.tile_w), dtype=np.uint8), rng.integers(0, 256, (T.n_tiles, 2, T.ch, T.cw), dtype=np.uint8))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_measure_equals_numpy_on_the_in_image_pixels(ctx, shape):
    import torch

    w, h, tw, th = shape
    T = PlanTiled420(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    ref = gen_image("noise", w, h, 3, w + h).reshape(-1)
    y, c = _random_planes(T, [w, h, tw, th])  # planes of their own noise: a replicated sample differs from the image's edge, so counting one shows
    want = _numpy_measure(y, c, ref, w, h)
    for offset in (0, 1, 3):
        d_y, d_c = Guarded(torch, y.size, offset=offset, salt=1), Guarded(torch, c.size, offset=offset, salt=2)
        d_y.put(torch, [y.reshape(-1)])
        d_c.put(torch, [c.reshape(-1)])
        d_ref = Guarded(torch, ref.size, offset=offset, salt=3)
        d_ref.put(torch, [ref])
        got = _device_measure(torch, T, d_y.ptr, d_c.ptr, d_ref.ptr)
        assert np.array_equal(got, want), (shape, offset, got.tolist(), want.tolist())
        for buf, host in ((d_ref, ref), (d_y, y.reshape(-1)), (d_c, c.reshape(-1))):  # the inputs are only read
            (back,), intact = buf.get(torch)
            assert intact and np.array_equal(back, host)
    T.close()


def test_measure_sums_pass_2_to_the_32_and_count_every_pixel_once(ctx):
    import torch

    w, h, tw, th = SHAPES[-1]
    T = PlanTiled420(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    d_y = torch.full((T.y_tile_bytes,), 255, dtype=torch.uint8, device="cuda")
    d_c = torch.full((T.c_tile_bytes,), 128, dtype=torch.uint8, device="cuda")  # grey: R = G = B = Y
    d_ref = torch.zeros(T.pixel_bytes, dtype=torch.uint8, device="cuda")
    got = _device_measure(torch, T, d_y.data_ptr(), d_c.data_ptr(), d_ref.data_ptr())
    assert 255 * 255 * w * h > 2 ** 32
    assert got.tolist() == [255 * 255 * w * h, 255] * 3 + [w * h]
    T.close()


# Past 512 workgroups of one-strip lanes a lane walks several strips, a whole grid apart; past 32 strips per lane the grid grows again (k12_tiles420.hip).
MEASURE_RAGGED = (2100, 1000, 701, 333)  # 132 000 strips, 516 workgroups: 2 strips per lane on 258 workgroups, whose second round ends 96 strips short
MEASURE_CLAMPED = (8300, 8250, 1024, 1024)  # 4 281 750 strips, 16 726 workgroups: 32 strips per lane, the clamp, on 523 workgroups


def test_measure_with_a_ragged_last_round_of_strips(ctx):
    import torch

    w, h, tw, th = MEASURE_RAGGED
    strips = -(-w // 16) * h
    groups = -(-strips // 256)
    per_lane = min(32, -(-groups // 512))
    assert per_lane == 2 and -(-groups // per_lane) * per_lane * 256 > strips  # (what the case is here for)
    T = PlanTiled420(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    ref = gen_image("noise", w, h, 3, 17).reshape(-1)
    y, c = _random_planes(T, 18)
    d_y, d_c, d_ref = Guarded(torch, y.size, offset=3, salt=1), Guarded(torch, c.size, offset=1, salt=2), Guarded(torch, ref.size, offset=1, salt=3)
    d_y.put(torch, [y.reshape(-1)])
    d_c.put(torch, [c.reshape(-1)])
    d_ref.put(torch, [ref])
    got = _device_measure(torch, T, d_y.ptr, d_c.ptr, d_ref.ptr)
    want = _numpy_measure(y, c, ref, w, h)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert d_y.get(torch)[1] and d_c.get(torch)[1] and d_ref.get(torch)[1]
    T.close()


def test_measure_past_the_clamp_of_strips_per_lane(ctx):
    """32 strips per lane, saturated - every merged byte 255 against a raster of zeros, the analytic sums: the worst case for the kernel's 32-bit sums per lane
    (32 x 16 x 255^2 < 2^25) and per wave (< 2^31)"""
    import torch

    w, h, tw, th = MEASURE_CLAMPED
    groups = -(-(-(-w // 16) * h) // 256)
    assert -(-groups // 512) > 32 and 32 * 16 * 255 * 255 * 64 < 2 ** 31
    T = PlanTiled420(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    d_y = torch.full((T.y_tile_bytes,), 255, dtype=torch.uint8, device="cuda")
    d_c = torch.full((T.c_tile_bytes,), 128, dtype=torch.uint8, device="cuda")
    d_ref = torch.zeros(T.pixel_bytes, dtype=torch.uint8, device="cuda")
    got = _device_measure(torch, T, d_y.data_ptr(), d_c.data_ptr(), d_ref.data_ptr())
    assert got.tolist() == [255 * 255 * w * h, 255] * 3 + [w * h]
    T.close()


def test_measure_replays_from_a_graph(ctx, hip):
    import torch

    w, h, tw, th = (257, 130, 100, 50)
    T = PlanTiled420(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    ref = gen_image("smooth", w, h, 3, 4).reshape(-1)
    planes = [_random_planes(T, 10 + k) for k in range(2)]
    d_ref = torch.from_numpy(ref.copy()).cuda()
    d_y = torch.from_numpy(planes[0][0].reshape(-1).copy()).cuda()
    d_c = torch.from_numpy(planes[0][1].reshape(-1).copy()).cuda()
    d_out = torch.zeros(7, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    T.measure_distortion_tiled420_dev(d_y.data_ptr(), d_c.data_ptr(), d_ref.data_ptr(), d_out.data_ptr(), stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    n_nodes = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 2  # the clearing of the sums, the measuring kernel
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    d_y.copy_(torch.from_numpy(planes[1][0].reshape(-1).copy()))  # replays measure what the buffers hold now, from zeroed sums each time
    d_c.copy_(torch.from_numpy(planes[1][1].reshape(-1).copy()))
    d_out.fill_(77)
    torch.cuda.synchronize()
    want = _numpy_measure(planes[1][0], planes[1][1], ref, w, h)
    for _ in range(2):
        assert hip.hipGraphLaunch(ex, sp) == 0
        s.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want)
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    T.close()


# ---- the plane-order estimate against the restatement ------------------------------------------------------------------------------------------------------------

def _device_estimate(torch, T, hist, oob=None, stream=0):
    n = T.n_tiles
    d_hist = torch.from_numpy(hist.reshape(-1).view(np.int32).copy()).cuda()
    d_oob = None if oob is None else torch.from_numpy(np.ascontiguousarray(oob, np.uint64).reshape(-1).view(np.int64).copy()).cuda()
    d_file = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    d_tiles = torch.full((n,), -5, dtype=torch.int64, device="cuda")
    d_models = torch.full((3 * n * 10 * 4,), -1, dtype=torch.int32, device="cuda")
    T.estimate_size_tiled420_dev(d_hist.data_ptr(), None if d_oob is None else d_oob.data_ptr(), d_file.data_ptr(), d_tiles.data_ptr(), d_models.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return int(d_file.cpu().numpy().view(np.uint64)[0]), d_tiles.cpu().numpy().view(np.uint64), d_models.cpu().numpy().view(np.uint32).reshape(3 * n, 10, 4)


def test_estimate_equals_the_restatement_on_synthetic_histograms(ctx, hip):
    import torch

    w, h, tw, th = IMAGE
    T = PlanTiled420(ctx, w, h, tw, th)
    n = T.n_tiles
    per_tile = _synthetic_hist(n, 3, 14)  # [n][3]: tile 1 with two empty contexts per channel, tile 2 with a channel (Cr) of ten empty contexts
    hist = np.stack(plane_order([tuple(per_tile[t]) for t in range(n)]))
    assert np.array_equal(tiled420_rate_ref.tile_order(hist), per_tile) and not hist[n + 2 * 2 + 1].any() and hist[2].any()
    want_file, want_tiles = tiled420_rate_ref.estimate_file(hist)
    assert want_file != UNCODABLE
    got_file, got_tiles, models = _device_estimate(torch, T, hist)
    gaps = got_tiles.astype(np.int64) - want_tiles.astype(np.int64)
    print("tile gaps", gaps.tolist(), "file gap", got_file - want_file)
    assert np.abs(gaps).max() <= 1, gaps.tolist()  # the bound of tests/test_gpu_rate.py per image
    assert got_file == 32 + 8 * (n + 1) + int(got_tiles.sum())
    assert np.array_equal(models[:, :, [0, 1, 3]], tiled420_rate_ref.tile_models(hist))
    assert (models[n + 2 * 2 + 1, :, 3] == 1).all() and (models[[1, n + 2, n + 3]][:, [3, 7], 3] == 1).all() and (models[0, :, 3] == 0).all()
    # the host form, with and without the per-tile output
    host_file, host_tiles = T.estimate_size_tiled420(hist)
    assert host_file == got_file and np.array_equal(host_tiles, got_tiles)
    total = C.c_uint64(0)
    assert api.load_library().fri_hip_estimate_size_tiled420(T._h, api._p(np.ascontiguousarray(hist)), None, C.byref(total), None) == 0 and total.value == got_file
    # an out-of-alphabet count in Cb of tile 1: that tile and the file are uncodable, the other tiles unchanged
    oob = np.zeros(3 * n, np.uint64)
    oob[n + 2 * 1] = 2
    bad_file, bad_tiles, _ = _device_estimate(torch, T, hist, oob)
    keep = [t for t in range(n) if t != 1]
    assert bad_file == UNCODABLE and int(bad_tiles[1]) == UNCODABLE and np.array_equal(bad_tiles[keep], got_tiles[keep])
    assert T.estimate_size_tiled420(hist, oob)[0] == UNCODABLE
    # capture and replay: the same bytes from what the buffers hold at the replay
    d_hist = torch.zeros(hist.size, dtype=torch.int32, device="cuda")
    d_file = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_tiles = torch.zeros(n, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    T.estimate_size_tiled420_dev(d_hist.data_ptr(), None, d_file.data_ptr(), d_tiles.data_ptr(), stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    d_hist.copy_(torch.from_numpy(hist.reshape(-1).view(np.int32).copy()))
    torch.cuda.synchronize()
    for _ in range(2):
        assert hip.hipGraphLaunch(ex, sp) == 0
        s.synchronize()
        assert int(d_file.cpu().numpy().view(np.uint64)[0]) == got_file and np.array_equal(d_tiles.cpu().numpy().view(np.uint64), got_tiles)
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    T.close()


# ---- shared: the image, its plan, the evaluator ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _image():
    w, h, tw, th = IMAGE
    img = mixed_image(w, h, 3, tw, 3)
    img.setflags(write=False)
    return img


@pytest.fixture(scope="module")
def plan(ctx):
    w, h, tw, th = IMAGE
    assert tile_shape420(w, h, 150) == (tw, th)
    T = PlanTiled420(ctx, w, h, tw, th)
    T.set_stream_order()
    yield T
    T.close()


@functools.lru_cache(maxsize=None)
def _symbols(T, q):
    """what the host coder's route takes at quality q - computed once per quality, read-only"""
    return T.encode_image_tiled420_symbols(_image(), q)


@pytest.mark.parametrize("quality", [30, 99])
def test_estimate_is_within_24_bytes_per_channel_of_the_emitters_payloads(plan, quality):
    w, h, tw, th = IMAGE
    T = plan
    sym, vp, wp, hist, oob = _symbols(T, quality)
    assert not oob.any()
    f = parse_frit(emit.tiled_encode_from_streams420(w, h, tw, th, sym, T.n_luma, T.n_chroma, hist, vp, wp, quality))
    est_file, est_tiles = T.estimate_size_tiled420(hist, oob)
    gaps = [int(est_tiles[t]) - len(f["payloads"][t]) for t in range(T.n_tiles)]
    print("quality", quality, "payload gaps", gaps, "file gap", est_file - f["offsets"][-1])
    assert max(map(abs, gaps)) <= 24 * 3, (quality, gaps)


# ---- the searches against a replay of their bisections -----------------------------------------------------------------------------------------------------------

_ctx_of_evaluator = {}


@functools.lru_cache(maxsize=None)
def _round_trip(q):
    """The tiled 4:2:0 round trip at quality q from entry points that existed before the searches: numpy split, per plane an ordinary C = 1 plan with the midpoint
    dequantiser (transform_quant, inverse_transform), numpy merge."""
    w, h, tw, th = IMAGE
    y, c = split_tiles420(_image(), tw, th)
    qm = fa.quality_matrix(q)
    out = []
    for planes in (y, c.reshape(-1, c.shape[2], c.shape[3])):
        Q = fa.Plan(_ctx_of_evaluator["ctx"], planes.shape[2], planes.shape[1], 1)
        Q.set_dequantiser(MIDPOINT)
        out.append(np.stack([Q.inverse_transform(Q.transform_quant(p, qm), qm).reshape(p.shape) for p in planes]))
        Q.close()
    return merge_tiles420(out[0], out[1].reshape(c.shape), w, h)


@functools.lru_cache(maxsize=None)
def _psnr_at(q):
    w, h = IMAGE[:2]
    d = _round_trip(q).astype(np.int64) - _image().astype(np.int64)
    m = []
    for ch in range(3):
        m += [int((d[:, :, ch] ** 2).sum()), int(np.abs(d[:, :, ch]).max())]
    return api.distortion_psnr(np.array(m + [w * h], np.uint64), 3)


@functools.lru_cache(maxsize=None)
def _ssim_at(q):
    w, h = IMAGE[:2]
    return ssim_ref.ssim(_image().reshape(-1), _round_trip(q).reshape(-1), w, h, 3)


def test_psnr_and_ssim_searches_replay_their_bisection(ctx, hip, plan):
    import torch

    _ctx_of_evaluator["ctx"] = ctx
    w, h, tw, th = IMAGE
    img = _image()
    T = plan
    # what the inner plans decode a plane to before the searches: the dequantiser set on them, which is not the midpoint one
    y, c = split_tiles420(img, tw, th)
    qm = fa.quality_matrix(30)
    before = []
    for inner, plane in ((T.luma, y[0]), (T.chroma, c[0, 0])):
        inner.set_dequantiser(REFERENCE)
        coefs = inner.transform_quant(plane, qm)
        back = inner.inverse_transform(coefs, qm)
        Q = fa.Plan(ctx, plane.shape[1], plane.shape[0], 1)
        Q.set_dequantiser(MIDPOINT)
        assert not np.array_equal(back, Q.inverse_transform(coefs, qm))  # (the check below can tell the two dequantisers apart)
        Q.close()
        before.append((inner, coefs, back))
    d_img = torch.from_numpy(img.reshape(-1).copy()).cuda()
    mid_db = 0.5 * (_psnr_at(20) + _psnr_at(70))
    for target in (mid_db, 200.0):
        want = _bisect_lowest(lambda q: (_psnr_at(q) >= target, _psnr_at(q)), float("inf"))
        got = T.search_quality(img, target)
        print("psnr target", target, "->", got)
        assert got == want  # the quality, and the PSNR as a double: the same integers through the same formula
        assert T.search_quality(d_img.data_ptr(), target) == want
    assert 1 < T.search_quality(img, mid_db)[0] < 100 and T.search_quality(img, 200.0) == (100, float("inf"))
    mid_ssim = 0.5 * (_ssim_at(20) + _ssim_at(70))
    for target in (mid_ssim, 1.0):
        want = _bisect_lowest(lambda q: (_ssim_at(q) >= target, _ssim_at(q)), 1.0)
        got = T.search_quality_ssim(img, target)
        print("ssim target", target, "->", got)
        assert got == want
        assert T.search_quality_ssim(d_img.data_ptr(), target) == want
    assert 1 < T.search_quality_ssim(img, mid_ssim)[0] < 100 and T.search_quality_ssim(img, 1.0) == (100, 1.0)
    # the _dev forms refuse a capturing stream before anything is enqueued
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    try:
        for call, target in ((T.search_quality, 30.0), (T.search_quality_ssim, 0.9), (T.search_quality_for_size, 10 ** 6)):
            with pytest.raises(fa.FriHipError) as e:
                call(d_img.data_ptr(), target, stream=s.cuda_stream)
            assert e.value.code == -1 and "graph" in str(e.value)
    finally:
        assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0
    n_nodes = C.c_size_t(12345)
    rc = hip.hipGraphGetNodes(graph, None, C.byref(n_nodes))
    hip.hipGraphDestroy(graph)
    assert rc == 0 and n_nodes.value == 0
    # the inner plans' dequantisers are as they were, and so are the caller's pixels
    for inner, coefs, back in before:
        assert np.array_equal(inner.inverse_transform(coefs, qm), back)
    assert np.array_equal(d_img.cpu().numpy(), img.reshape(-1))


def test_size_search_replays_its_bisection(ctx, plan):
    w, h, tw, th = IMAGE
    img = _image()
    T = plan
    n = T.n_tiles

    @functools.lru_cache(maxsize=None)
    def estimate(q):
        sym, vp, wp, hist, oob = _symbols(T, q)
        return tiled420_rate_ref.estimate_file(hist, oob)[0]

    budget = estimate(40) + 64
    lo, hi, lo_est, probed = 0, 100, 0, []
    while hi - lo > 1:  # fri_hip_search_quality_for_size420's bisection: a 4:2:0 file has a quality of 1..99
        mid = (lo + hi) // 2
        probed.append(mid)
        est = estimate(mid)
        if est != UNCODABLE and est <= budget:
            lo, lo_est = mid, est
        else:
            hi = mid
    assert all(abs(estimate(q) - budget) > n for q in probed), "the budget must not sit within the estimate's tolerance of a probe"
    q, est = T.search_quality_for_size(img, budget)
    print("budget", budget, "->", (q, est), "restatement", (lo, lo_est))
    assert q == lo and 1 <= q < 100 and abs(est - lo_est) <= n
    # a budget below quality 1: out of range, quality 0, the estimate of quality 1
    qual, v = C.c_int32(-7), C.c_uint64(0)
    px = np.ascontiguousarray(img.reshape(-1))
    assert api.load_library().fri_hip_search_quality_for_size_tiled420(T._h, api._p(px), 100, C.byref(qual), C.byref(v)) == -7
    assert qual.value == 0 and abs(v.value - estimate(1)) <= n
    with pytest.raises(fa.FriHipError) as e:
        T.search_quality_for_size(img, 100)
    assert e.value.code == -7
    # without the stream order on the inner plans the probes' chain is refused
    bare = PlanTiled420(ctx, w, h, tw, th)
    with pytest.raises(fa.FriHipError) as e:
        bare.search_quality_for_size(img, budget)
    assert e.value.code == -1
    bare.close()


# ---- the device coder ------------------------------------------------------------------------------------------------------------------------------------------

HOLES = (35, 23, 17, 9)  # chroma planes of 9 x 5 samples: too few nodes for all ten contexts


@pytest.mark.parametrize("case", [IMAGE + (60, 0), HOLES + (60, TILED_ALLOW_HOLES)], ids=_ids)
def test_coded_route_writes_the_file_of_the_host_coder(ctx, case):
    w, h, tw, th, quality, flags = case
    img = _image() if (w, h, tw, th) == IMAGE else mixed_image(w, h, 3, tw, 9)
    T = PlanTiled420(ctx, w, h, tw, th, flags)
    T.set_stream_order()
    n = T.n_tiles
    sym, vp, wp, hist, oob = T.encode_image_tiled420_symbols(img, quality)
    assert not oob.any()
    if flags:
        empty = hist.sum(axis=2) == 0
        print("empty contexts per plane", empty.sum(axis=1).tolist())
        assert empty[n:].any()  # some chroma context holds no symbol: FRI_HIP_RANS_EMPTY_OK is what codes it
    want = emit.tiled_encode_from_streams420(w, h, tw, th, sym, T.n_luma, T.n_chroma, hist, vp, wp, quality)
    first = T.encode_image_tiled420_coded(img, quality)
    words, n_words, models, off, status, cvp, cwp = first
    assert not status.any() and np.array_equal(cvp, vp) and np.array_equal(cwp, wp)
    assert (n_words[:n] <= T.n_luma + 20).all() and (n_words[n:] <= T.n_chroma + 20).all() and (n_words >= 20).all()
    for threads in (1, 4):
        assert emit.tiled_encode_from_coded420(w, h, tw, th, words, n_words, models, off, cvp, cwp, quality, threads=threads) == want
    again = T.encode_image_tiled420_coded(img, quality)  # two runs: identical outputs
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    # rows of 20 words hold the flush and nothing else: out of range, every plane's need reported, no row written
    planes = 3 * n
    small = np.full((planes, 20), 0xABCD, np.uint32)
    nw, m, st = np.zeros(planes, np.uint32), np.zeros((planes, 10, 4), np.uint32), np.zeros((planes, 4), np.uint32)
    o, v1, v2 = np.zeros((planes, 10, 1024), np.uint16), np.zeros((planes, 3, 6), np.float32), np.zeros((planes, 3, 6), np.float32)
    px = np.ascontiguousarray(img.reshape(-1))
    rc = api.load_library().fri_hip_encode_image_tiled420_coded(T._h, api._p(px), quality, api._p(v1), api._p(v2), api._p(small), 20, api._p(nw), api._p(m), api._p(o), api._p(st))
    assert rc == -7 and np.array_equal(nw, n_words) and (nw > 20).any()
    assert (small[nw > 20] == 0xABCD).all()
    with pytest.raises(fa.FriHipError) as e:
        T.encode_image_tiled420_coded(img, 0)
    assert e.value.code == -1
    T.close()


# ---- end to end through the driver -------------------------------------------------------------------------------------------------------------------------------

def test_driver_device_rans_and_targets(ctx, plan, tmp_path):
    _ctx_of_evaluator["ctx"] = ctx
    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h, tw, th = IMAGE
    img = _image()
    T = plan
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + img.tobytes())

    def run(dst, *args):
        return subprocess.run([driver, "encode-file", str(src), str(dst), *map(str, args)], capture_output=True, text=True, timeout=300)

    plain, coded = tmp_path / "plain.frv", tmp_path / "coded.frv"
    out = run(plain, "--tile-size-420", 150, "--quality", 60)
    assert out.returncode == 0 and "self-check" in out.stdout, out.stdout + out.stderr
    out = run(coded, "--tile-size-420", 150, "--quality", 60, "--device-rans")
    assert out.returncode == 0 and "self-check" in out.stdout and "K11" in out.stdout, out.stdout + out.stderr
    assert coded.read_bytes() == plain.read_bytes()
    sym, vp, wp, hist, oob = _symbols(T, 40)
    budget = T.estimate_size_tiled420(hist, oob)[0] + 64
    db, ss = f"{0.5 * (_psnr_at(20) + _psnr_at(70)):.6f}", f"{0.5 * (_ssim_at(20) + _ssim_at(70)):.6f}"  # (reachable in 4:2:0, whatever the image's colour noise costs)
    for target, search in ((f"psnr={db}", lambda: T.search_quality(img, float(db))), (f"ssim={ss}", lambda: T.search_quality_ssim(img, float(ss))),
                           (f"size={budget}", lambda: T.search_quality_for_size(img, budget))):
        dst = tmp_path / "target.frv"
        out = run(dst, "--tile-size-420", 150, "--target", target)
        assert out.returncode == 0 and "self-check" in out.stdout, out.stdout + out.stderr
        q, v = search()
        data = dst.read_bytes()
        info = emit.tiled_info(data)
        print(target, "search", (q, v), "file quality", info.quality, "bytes", len(data))
        assert 1 <= q <= 99 and info.s420 and f"search returned quality {q} " in out.stdout, out.stdout
        if target.startswith("size="):
            assert len(data) <= budget and q - 8 <= info.quality <= q  # (the file is checked against the budget: one quality down while it is over)
        else:
            assert info.quality == q
        dst.unlink()
    for bad in (["--tile-size", 150, "--quality", 60, "--target", "psnr=33"], ["--quality", 60, "--target", "psnr=33"], ["--tile-size-420", 150, "--quality", 60, "--target", "psnr=33"],
                ["--tile-size-420", 150, "--target", "psnr=0"], ["--tile-size-420", 150, "--target", "speed=3"]):
        out = run(tmp_path / "bad.frv", *bad)
        assert out.returncode != 0 and out.stderr and not (tmp_path / "bad.frv").exists(), bad
    out = run(tmp_path / "bad.frv", "--tile-size-420", 150, "--psnr", 35)
    assert out.returncode != 0 and "--target" in out.stderr and not (tmp_path / "bad.frv").exists()
