"""The quality searches and the size estimate over tiles on the device (include/fri_hip.h, "tiled coding"):

- K10's measuring kernel exactly against numpy (tests/tiled_ref.merge_tiles, then per-channel SSE, max and count) on every shape of the split and merge tests,
  replicated pixels filled with other values, pointers 0, 1 and 3 bytes off; sums past 2^32; graph capture;
- fri_hip_estimate_size_tiled_dev against tests/tiled_rate_ref.py on synthetic histograms with empty contexts and an out-of-alphabet count, and against the
  files the emitter writes from the device's streams;
- each search against a replay of its documented bisection in Python, the evaluator made of entry points that existed before the searches;
- fri_driver encode-file --tile-size with a target."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd import api
from frave_amd.api import TILED_ALLOW_HOLES, PlanTiled
from tests import ssim_ref, tiled_rate_ref
from tests.common import gen_image
from tests.later_cases import MEASURE_CLAMPED, MEASURE_RAGGED
from tests.oracle_ref import MIDPOINT, REFERENCE
from tests.test_gpu_instances import Guarded
from tests.tiled_ref import merge_tiles, mixed_image, parse_frit, split_tiles

for _name in ("measure_distortion_tiled_dev", "estimate_size_tiled", "estimate_size_tiled_dev", "search_quality", "search_quality_ssim", "search_quality_for_size"):
    assert hasattr(PlanTiled, _name), _name  # (without the feature the module fails here)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELAXED = 2  # hipStreamCaptureModeRelaxed
COLOUR_NONE, COLOUR_YCBCR = 0, 3
UNCODABLE = 2 ** 64 - 1
# (W, H, C, tile_w, tile_h)
SHAPES = [(1, 1, 1, 1, 1), (5, 3, 3, 2, 2), (17, 9, 1, 16, 4), (33, 20, 3, 16, 16), (50, 40, 1, 64, 64), (257, 130, 3, 100, 50), (1023, 767, 3, 512, 512)]
IMAGES = [(250, 250, 1, 125, 125), (334, 350, 3, 167, 117)]


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

def _numpy_measure(tiles, ref, w, h, c):
    """uint64 [2 C + 1]: per channel the SSE and the largest absolute difference of the merged tiles against ref, then W H"""
    d = merge_tiles(tiles, w, h).astype(np.int64) - ref.reshape(h, w, c).astype(np.int64)
    out = []
    for ch in range(c):
        out += [int((d[:, :, ch] ** 2).sum()), int(np.abs(d[:, :, ch]).max())]
    return np.array(out + [w * h], np.uint64)


def _device_measure(torch, T, d_tiles, d_ref, stream=0):
    d_out = torch.full((2 * T.channels + 1,), -1, dtype=torch.int64, device="cuda")  # (the call zeroes it)
    T.measure_distortion_tiled_dev(d_tiles, d_ref, d_out.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_measure_equals_numpy_on_the_in_image_pixels(ctx, shape):
    import torch

    w, h, c, tw, th = shape
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    ref = gen_image("noise", w, h, c, w + h).reshape(-1)
    # tiles of their own noise: the replicated pixels differ from the image's edge, so counting one shows
    tiles = gen_image("noise", tw, th * T.n_tiles, c, 99).reshape(T.n_tiles, th, tw, c)
    want = _numpy_measure(tiles, ref, w, h, c)
    for offset in (0, 1, 3):
        d_tiles = Guarded(torch, tiles.size, offset=offset, salt=1)
        d_tiles.put(torch, [tiles.reshape(-1)])
        d_ref = Guarded(torch, ref.size, offset=offset, salt=2)
        d_ref.put(torch, [ref])
        got = _device_measure(torch, T, d_tiles.ptr, d_ref.ptr)
        assert np.array_equal(got, want), (shape, offset, got.tolist(), want.tolist())
        (back,), intact = d_ref.get(torch)  # both inputs are only read
        assert intact and np.array_equal(back, ref)
        (back,), intact = d_tiles.get(torch)
        assert intact and np.array_equal(back, tiles.reshape(-1))
    T.close()


def test_measure_sums_pass_2_to_the_32_and_count_every_pixel_once(ctx):
    import torch

    w, h, c, tw, th = SHAPES[-1]
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    d_tiles = torch.full((T.tile_bytes,), 255, dtype=torch.uint8, device="cuda")
    d_ref = torch.zeros(T.pixel_bytes, dtype=torch.uint8, device="cuda")
    got = _device_measure(torch, T, d_tiles.data_ptr(), d_ref.data_ptr())
    assert 255 * 255 * w * h > 2 ** 32
    assert got.tolist() == [255 * 255 * w * h, 255] * c + [w * h]
    T.close()


def test_measure_with_a_ragged_last_round_of_strips(ctx):
    """more than one strip per lane and a workgroup count the strips per lane do not divide (tests/later_cases.py): the last round's workgroups past the end"""
    import torch

    shape, _ = MEASURE_RAGGED
    w, h, c, tw, th = shape
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    ref = gen_image("noise", w, h, c, 17).reshape(-1)
    tiles = np.random.default_rng(18).integers(0, 256, (T.n_tiles, th, tw, c), dtype=np.uint8)
    d_tiles = Guarded(torch, tiles.size, offset=3, salt=1)
    d_tiles.put(torch, [tiles.reshape(-1)])
    d_ref = Guarded(torch, ref.size, offset=1, salt=2)
    d_ref.put(torch, [ref])
    got = _device_measure(torch, T, d_tiles.ptr, d_ref.ptr)
    want = _numpy_measure(tiles, ref, w, h, c)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert d_tiles.get(torch)[1] and d_ref.get(torch)[1]
    T.close()


@pytest.mark.parametrize("content", ["saturated", "noise"])
def test_measure_past_the_clamp_of_strips_per_lane(ctx, content):
    """more than 16 384 workgroups of one-strip lanes: 32 strips per lane, the clamp. Saturated (every tile byte 255 against a raster of zeros, the analytic
    sums) is the worst case for the kernel's 32-bit sums per lane and per wave; noise is held to numpy, the reference summed in row blocks."""
    import torch

    shape, _ = MEASURE_CLAMPED
    w, h, c, tw, th = shape
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    if content == "saturated":
        d_tiles = torch.full((T.tile_bytes,), 255, dtype=torch.uint8, device="cuda")
        d_ref = torch.zeros(T.pixel_bytes, dtype=torch.uint8, device="cuda")
        want = [255 * 255 * w * h, 255] * c + [w * h]
    else:
        rng = np.random.default_rng(5)
        tiles = rng.integers(0, 256, (T.n_tiles, th, tw, c), dtype=np.uint8)
        ref = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        merged = merge_tiles(tiles, w, h)
        sse, worst = 0, 0
        for y in range(0, h, 512):  # no int64 array of the whole raster
            d = merged[y : y + 512].astype(np.int64) - ref[y : y + 512]
            sse, worst = sse + int((d * d).sum()), max(worst, int(np.abs(d).max()))
        want = [sse, worst, w * h]
        d_tiles, d_ref = torch.from_numpy(tiles.reshape(-1)).cuda(), torch.from_numpy(ref.reshape(-1)).cuda()
    got = _device_measure(torch, T, d_tiles.data_ptr(), d_ref.data_ptr())
    assert got.tolist() == want
    T.close()


def test_measure_replays_from_a_graph(ctx, hip):
    import torch

    w, h, c, tw, th = (257, 130, 3, 100, 50)
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    ref = gen_image("smooth", w, h, c, 4).reshape(-1)
    tiles = [gen_image("noise", tw, th * T.n_tiles, c, 10 + k).reshape(T.n_tiles, th, tw, c) for k in range(2)]
    d_ref = torch.from_numpy(ref.copy()).cuda()
    d_tiles = torch.from_numpy(tiles[0].reshape(-1).copy()).cuda()
    d_out = torch.zeros(2 * c + 1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    T.measure_distortion_tiled_dev(d_tiles.data_ptr(), d_ref.data_ptr(), d_out.data_ptr(), stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    d_tiles.copy_(torch.from_numpy(tiles[1].reshape(-1).copy()))  # replays measure what the buffer holds now, from zeroed sums each time
    d_out.fill_(77)
    torch.cuda.synchronize()
    for _ in range(2):
        assert hip.hipGraphLaunch(ex, sp) == 0
        s.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64), _numpy_measure(tiles[1], ref, w, h, c))
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    T.close()


# ---- the tiled estimate against the restatement ------------------------------------------------------------------------------------------------------------------

def _synthetic_hist(n, c, seed):
    """[n][C][10][1024]: geometric counts around the peak and one symbol far in the tail (an off-distribution value) in every context"""
    rng = np.random.default_rng(seed)
    hist = np.zeros((n, c, 10, 1024), np.uint32)
    for t in range(n):
        for ch in range(c):
            for b in range(10):
                k = 20 + 6 * b
                hist[t, ch, b, :k] = (rng.integers(1, 50, k) * np.exp(-np.arange(k) / (3.0 + b))).astype(np.uint32) * (1 + t)
                hist[t, ch, b, 0] += 100
                hist[t, ch, b, 700 + 10 * b + ch] = 1 + (t & 1)
    hist[1, :, 3] = 0  # tile 1: contexts 3 and 7 of every channel without symbols
    hist[1, :, 7] = 0
    hist[2, c - 1] = 0  # tile 2: a channel with all ten contexts empty
    return hist


def _device_estimate(torch, T, hist, oob=None, stream=0):
    n, c = T.n_tiles, T.channels
    d_hist = torch.from_numpy(hist.reshape(-1).view(np.int32).copy()).cuda()
    d_oob = None if oob is None else torch.from_numpy(np.ascontiguousarray(oob, np.uint64).reshape(-1).view(np.int64).copy()).cuda()
    d_file = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    d_tiles = torch.full((n,), -5, dtype=torch.int64, device="cuda")
    d_models = torch.full((n * c * 10 * 4,), -1, dtype=torch.int32, device="cuda")
    T.estimate_size_tiled_dev(d_hist.data_ptr(), None if d_oob is None else d_oob.data_ptr(), d_file.data_ptr(), d_tiles.data_ptr(), d_models.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return int(d_file.cpu().numpy().view(np.uint64)[0]), d_tiles.cpu().numpy().view(np.uint64), d_models.cpu().numpy().view(np.uint32).reshape(n, c, 10, 4)


@pytest.mark.parametrize("case", IMAGES, ids=_ids)
def test_estimate_equals_the_restatement_on_synthetic_histograms(ctx, hip, case):
    import torch

    w, h, c, tw, th = case
    T = PlanTiled(ctx, w, h, c, tw, th)
    n = T.n_tiles
    hist = _synthetic_hist(n, c, 11 + c)
    want_file, want_tiles = tiled_rate_ref.estimate_file(hist)
    assert want_file != UNCODABLE
    got_file, got_tiles, models = _device_estimate(torch, T, hist)
    gaps = got_tiles.astype(np.int64) - want_tiles.astype(np.int64)
    print(case, "tile gaps", gaps.tolist(), "file gap", got_file - want_file)
    assert np.abs(gaps).max() <= 1, gaps.tolist()  # the bound of tests/test_gpu_rate.py per image
    assert got_file == 32 + 8 * (n + 1) + int(got_tiles.sum()) and abs(got_file - want_file) <= n
    for t in range(n):
        assert np.array_equal(models[t][:, :, [0, 1, 3]], tiled_rate_ref.tile_models(hist[t])), t
    assert (models[1, :, [3, 7], 3] == 1).all() and (models[2, c - 1, :, 3] == 1).all() and (models[0, :, :, 3] == 0).all()
    # the host form, with and without the per-tile output
    host_file, host_tiles = T.estimate_size_tiled(hist)
    assert host_file == got_file and np.array_equal(host_tiles, got_tiles)
    total = C.c_uint64(0)
    assert api.load_library().fri_hip_estimate_size_tiled(T._h, api._p(np.ascontiguousarray(hist)), None, C.byref(total), None) == 0 and total.value == got_file
    # an out-of-alphabet count in the last tile: that tile and the file are uncodable, the other tiles unchanged
    oob = np.zeros((n, c), np.uint64)
    oob[n - 1, c - 1] = 2
    bad_file, bad_tiles, _ = _device_estimate(torch, T, hist, oob)
    assert bad_file == UNCODABLE and int(bad_tiles[n - 1]) == UNCODABLE and np.array_equal(bad_tiles[: n - 1], got_tiles[: n - 1])
    assert T.estimate_size_tiled(hist, oob)[0] == UNCODABLE
    # the untiled estimate on the inner plan keeps refusing a histogram with empty contexts
    assert T.tile.estimate_size(hist[1]) == UNCODABLE and T.tile.estimate_size(hist[0]) == int(got_tiles[0])
    # capture and replay: the same bytes from what the buffers hold at the replay
    d_hist = torch.zeros(hist.size, dtype=torch.int32, device="cuda")
    d_file = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_tiles = torch.zeros(n, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    T.estimate_size_tiled_dev(d_hist.data_ptr(), None, d_file.data_ptr(), d_tiles.data_ptr(), stream=s.cuda_stream)
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


# ---- the estimate against real files ----------------------------------------------------------------------------------------------------------------------------

FILE_CASES = [IMAGES[0] + ("mixed", 0), IMAGES[1] + ("mixed", 0), (128, 48, 1, 64, 48, "noise", TILED_ALLOW_HOLES)]


@pytest.mark.parametrize("case", FILE_CASES, ids=_ids)
def test_estimate_is_within_24_bytes_per_channel_of_the_emitters_payloads(ctx, case):
    w, h, c, tw, th, kind, flags = case
    img = mixed_image(w, h, c, tw, 3) if kind == "mixed" else gen_image(kind, w, h, c, 7)
    T = PlanTiled(ctx, w, h, c, tw, th, flags)
    T.set_stream_order()
    n = T.n_tiles
    for q in (100, 50):
        sym, vp, wp, hist, oob = T.encode_image_tiled_symbols(img, fa.quality_matrix(q))
        assert not oob.any()
        f = parse_frit(emit.tiled_encode_from_streams(w, h, tw, th, sym, hist, vp, wp, quality=q if q < 100 else 0))
        est_file, est_tiles = T.estimate_size_tiled(hist, oob)
        gaps = [int(est_tiles[t]) - len(f["payloads"][t]) for t in range(n)]
        print(case, q, "empty contexts", int((hist.sum(axis=3) == 0).sum()), "payload gaps", gaps, "file gap", est_file - f["offsets"][-1])
        assert max(map(abs, gaps)) <= 24 * c, (q, gaps)
        assert abs(est_file - f["offsets"][-1]) <= 24 * c * n, (q, est_file, f["offsets"][-1])
    T.close()


# ---- the searches against a replay of their bisections -----------------------------------------------------------------------------------------------------------

SEARCH_CASES = [IMAGES[0] + (COLOUR_NONE,), IMAGES[1] + (COLOUR_NONE,), IMAGES[1] + (COLOUR_YCBCR,)]
_ctx_of_evaluator = {}


def _search_image(case):
    w, h, c, tw, th, transform = case
    return mixed_image(w, h, c, tw, 5)


@functools.lru_cache(maxsize=None)
def _round_trip(case, q):
    """The tiled round trip at quality q from entry points that existed before the searches: numpy split, an ordinary plan of the tile's shape with the midpoint
    dequantiser (transform_quant, inverse_transform), numpy merge."""
    w, h, c, tw, th, transform = case
    Q = fa.Plan(_ctx_of_evaluator["ctx"], tw, th, c)
    Q.set_colour_transform(transform)
    Q.set_dequantiser(MIDPOINT)
    qm = fa.quality_matrix(q)
    per = [Q.inverse_transform(Q.transform_quant(tile, qm), qm).reshape(th, tw, c) for tile in split_tiles(_search_image(case), tw, th)]
    Q.close()
    return merge_tiles(np.stack(per), w, h)


def _psnr_at(case, q):
    w, h, c = case[:3]
    d = _round_trip(case, q).astype(np.int64) - _search_image(case).astype(np.int64)
    m = []
    for ch in range(c):
        m += [int((d[:, :, ch] ** 2).sum()), int(np.abs(d[:, :, ch]).max())]
    return api.distortion_psnr(np.array(m + [w * h], np.uint64), c)


def _ssim_at(case, q):
    w, h, c = case[:3]
    return ssim_ref.ssim(_search_image(case).reshape(-1), _round_trip(case, q).reshape(-1), w, h, c)


def _bisect_lowest(reaches, perfect):
    """fri_hip_search_quality's bisection: the lowest quality that reaches the target; 100 (never probed) with the perfect score"""
    lo, hi, hi_v = 0, 100, perfect
    while hi - lo > 1:
        mid = (lo + hi) // 2
        ok, v = reaches(mid)
        if ok:
            hi, hi_v = mid, v
        else:
            lo = mid
    return hi, hi_v


def _tiled(ctx, case):
    w, h, c, tw, th, transform = case
    T = PlanTiled(ctx, w, h, c, tw, th)
    T.set_stream_order()
    T.tile.set_colour_transform(transform)
    return T


@pytest.mark.parametrize("case", SEARCH_CASES, ids=_ids)
def test_psnr_and_ssim_searches_replay_their_bisection(ctx, hip, case):
    import torch

    _ctx_of_evaluator["ctx"] = ctx
    w, h, c, tw, th, transform = case
    img = _search_image(case)
    T = _tiled(ctx, case)
    T.tile.set_dequantiser(REFERENCE)
    # what the inner plan decodes a file's planes to before the searches: its own dequantiser and colour transform
    qm = fa.quality_matrix(30)
    Q = fa.Plan(ctx, tw, th, c)
    Q.set_colour_transform(transform)
    coefs = np.stack([Q.transform_quant(tile, qm) for tile in split_tiles(img, tw, th)])
    Q.close()
    before = T.decode_image_tiled(coefs, qm)
    assert not np.array_equal(before, merge_tiles_midpoint(ctx, case, coefs, qm))  # (the check below can tell the two dequantisers apart)
    d_img = torch.from_numpy(img.reshape(-1).copy()).cuda()
    mid_db = 0.5 * (_psnr_at(case, 20) + _psnr_at(case, 70))
    for target in (mid_db, 200.0):
        want = _bisect_lowest(lambda q: (_psnr_at(case, q) >= target, _psnr_at(case, q)), float("inf"))
        got = T.search_quality(img, target)
        print(case, "psnr target", target, "->", got)
        assert got == want  # the quality, and the PSNR as a double: the same integers through the same formula
        assert T.search_quality(d_img.data_ptr(), target) == want
    assert 1 < T.search_quality(img, mid_db)[0] < 100 and T.search_quality(img, 200.0) == (100, float("inf"))
    mid_ssim = 0.5 * (_ssim_at(case, 20) + _ssim_at(case, 70))
    for target in (mid_ssim, 1.0):
        want = _bisect_lowest(lambda q: (_ssim_at(case, q) >= target, _ssim_at(case, q)), 1.0)
        got = T.search_quality_ssim(img, target)
        print(case, "ssim target", target, "->", got)
        assert got == want
        assert T.search_quality_ssim(d_img.data_ptr(), target) == want
    assert 1 < T.search_quality_ssim(img, mid_ssim)[0] < 100
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
    # the inner plan's dequantiser and colour transform are as they were
    assert np.array_equal(T.decode_image_tiled(coefs, qm), before)
    assert np.array_equal(d_img.cpu().numpy(), img.reshape(-1))
    T.close()


def merge_tiles_midpoint(ctx, case, coefs, qm):
    w, h, c, tw, th, transform = case
    Q = fa.Plan(ctx, tw, th, c)
    Q.set_colour_transform(transform)
    Q.set_dequantiser(MIDPOINT)
    per = [Q.inverse_transform(co, qm).reshape(th, tw, c) for co in coefs]
    Q.close()
    return merge_tiles(np.stack(per), w, h).reshape(-1)


@pytest.mark.parametrize("case", SEARCH_CASES, ids=_ids)
def test_size_search_replays_its_bisection(ctx, case):
    w, h, c, tw, th, transform = case
    img = _search_image(case)
    T = _tiled(ctx, case)
    n = T.n_tiles

    @functools.lru_cache(maxsize=None)
    def estimate(q):
        sym, vp, wp, hist, oob = T.encode_image_tiled_symbols(img, fa.quality_matrix(q))
        return tiled_rate_ref.estimate_file(hist, oob)[0]

    budget = estimate(40) + 64
    lo, hi, lo_est, probed = 0, 100 if transform == COLOUR_YCBCR else 101, 0, []
    while hi - lo > 1:  # fri_hip_search_quality_for_size's bisection
        mid = (lo + hi) // 2
        probed.append(mid)
        est = estimate(mid)
        if est != UNCODABLE and est <= budget:
            lo, lo_est = mid, est
        else:
            hi = mid
    assert all(abs(estimate(q) - budget) > n for q in probed), "the budget must not sit within the estimate's tolerance of a probe"
    q, est = T.search_quality_for_size(img, budget)
    print(case, "budget", budget, "->", (q, est), "restatement", (lo, lo_est))
    assert q == lo and 1 <= q < 100 and abs(est - lo_est) <= n
    # a budget below quality 1: out of range, quality 0, the estimate of quality 1
    qual, v = C.c_int32(-7), C.c_uint64(0)
    px = np.ascontiguousarray(img.reshape(-1))
    assert api.load_library().fri_hip_search_quality_for_size_tiled(T._h, api._p(px), 100, C.byref(qual), C.byref(v)) == -7
    assert qual.value == 0 and abs(v.value - estimate(1)) <= n
    with pytest.raises(fa.FriHipError) as e:
        T.search_quality_for_size(img, 100)
    assert e.value.code == -7
    # a budget nothing exceeds: lossless where a lossless file exists, 99 on a YCbCr plan
    q, est = T.search_quality_for_size(img, 10 ** 9)
    assert q == (99 if transform == COLOUR_YCBCR else 100) and abs(est - estimate(q)) <= n
    # without the stream order on the inner plan the probes' chain is refused
    bare = PlanTiled(ctx, w, h, c, tw, th)
    with pytest.raises(fa.FriHipError) as e:
        bare.search_quality_for_size(img, budget)
    assert e.value.code == -1
    bare.close()
    T.close()


# ---- end to end through the driver -------------------------------------------------------------------------------------------------------------------------------

def test_driver_targets_hold_for_the_tiled_file(ctx, tmp_path):
    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h = 334, 350
    img = mixed_image(w, h, 3, 167, 8)
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + img.tobytes())
    tw, th = fa.tile_shape(w, h, 150)
    budget = 250000
    for flags, transform, search in ((["--psnr", "35"], COLOUR_NONE, lambda T: T.search_quality(img, 35.0)),
                                     (["--ycbcr", "--ssim", "0.95"], COLOUR_YCBCR, lambda T: T.search_quality_ssim(img, 0.95)),
                                     (["--size", str(budget)], COLOUR_NONE, lambda T: T.search_quality_for_size(img, budget))):
        dst = tmp_path / "target.frv"
        out = subprocess.run([driver, "encode-file", str(src), str(dst), "--tile-size", "150"] + flags, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "self-check" in out.stdout, out.stdout + out.stderr
        T = PlanTiled(ctx, w, h, 3, tw, th)
        T.set_stream_order()
        T.tile.set_colour_transform(transform)
        q, v = search(T)
        T.close()
        data = dst.read_bytes()
        info = emit.tiled_info(data)
        print(flags, "search", (q, v), "file quality", info.quality, "bytes", len(data), out.stdout.strip().splitlines()[0])
        assert info.quality == (q if q < 100 else 0), (flags, q, info.quality)
        assert f"quality {q}" in out.stdout
        if flags[0] == "--size":
            assert len(data) <= budget
