"""The size estimate of a tiled file, host side: the restatement (tests/tiled_rate_ref.py, the formula of fri_hip_estimate_size_tiled_dev) against the `frit` files
the product emitter writes from oracle-made planes - tiles with and without empty contexts -, the container and the empty-context rule exactly, and the argument
checks of the tiled measure, estimate and searches on host-only plans. CPU only."""
import ctypes as C
import functools

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd import api
from frave_amd.api import TILED_ALLOW_HOLES, PlanTiled
from tests import rate_model, tiled_rate_ref
from tests.common import gen_image
from tests.tiled_ref import grid, mixed_image, parse_frit, split_tiles

for _name in ("measure_distortion_tiled_dev", "estimate_size_tiled", "estimate_size_tiled_dev", "search_quality", "search_quality_ssim", "search_quality_for_size"):
    assert hasattr(PlanTiled, _name), _name  # (without the feature the module fails here)

# (name, W, H, C, tile_w, tile_h, empty contexts expected at quality 100: None = none at any quality)
INPUTS = [("mixed", 250, 250, 1, 125, 125, None), ("mixed", 334, 350, 3, 167, 117, None), ("noise", 256, 144, 1, 64, 48, 6), ("smooth", 200, 160, 3, 40, 40, 18)]
QUALITIES = (100, 1, 50, 90)


def _image(kind, w, h, c, tw):
    return mixed_image(w, h, c, tw, 3) if kind == "mixed" else gen_image(kind, w, h, c, 7)


def _streams(centers, coefs, bucket, pred):
    out = []
    for ch in range(coefs.shape[0]):
        sym, bk = emit.channel_symbols(centers, coefs[ch], bucket[ch], pred[ch])
        out.append((bk.astype(np.uint16) << 10) | sym)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _coded(case, q):
    """(streams [n][C][num_some], hist [n][C][10][1024], vp, wp [n][C][3][6]) of the case's tiles from the oracle at quality q, the known-answer parameters"""
    kind, w, h, c, tw, th, _ = case
    per = []
    for tile in split_tiles(_image(kind, w, h, c, tw), tw, th):
        centers, coefs, bucket, pred, hist, oob, vp, wp = rate_model.oracle_arrays(np.ascontiguousarray(tile).reshape(-1), tw, th, c, q)
        assert not oob.any()
        per.append((_streams(centers, coefs, bucket, pred), hist, vp, wp))
    return tuple(np.stack([p[k] for p in per]) for k in range(4))


@pytest.mark.parametrize("case", INPUTS, ids=lambda s: "-".join(map(str, s[:6])))
def test_estimate_is_within_24_bytes_per_channel_of_every_payload(case):
    """Every payload within 24 C bytes, the bound tests/test_rate_host.py holds per frif file, and the file within 24 C n_tiles. Measured with the restatement and
    the emitter: the worst payload gap 22 bytes at C = 3 and 8 at C = 1, the worst file gap 75."""
    kind, w, h, c, tw, th, empty_at_100 = case
    nx, ny = grid(w, h, tw, th)
    n = nx * ny
    for q in QUALITIES:
        streams, hist, vp, wp = _coded(case, q)
        empty = int((hist.sum(axis=3) == 0).sum())
        if empty_at_100 is None:
            assert empty == 0, (q, empty)
        elif q == 100:
            assert empty == empty_at_100 > 0, "the lossless planes of this input must leave contexts empty"
        frv = emit.tiled_encode_from_streams(w, h, tw, th, streams, hist, vp, wp, quality=q if q < 100 else 0)
        f = parse_frit(frv)
        est_file, est_tiles = tiled_rate_ref.estimate_file(hist)
        gaps = [int(est_tiles[t]) - len(f["payloads"][t]) for t in range(n)]
        print(case[:6], q, "empty", empty, "file", est_file - len(frv), "worst payload", max(map(abs, gaps)))
        assert max(map(abs, gaps)) <= 24 * c, (q, gaps)
        assert abs(est_file - len(frv)) <= 24 * c * n, (q, est_file, len(frv))
        assert est_file - len(frv) == sum(gaps)  # the container's header and table are exact


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("k", [0, 2, 10])
def test_container_and_empty_context_rule_are_exact(c, k):
    """One used symbol near the peak per context, k contexts of every channel emptied: 18 + C (218 + 10 x 14 + 2 k) + ceil(bits / 8) per tile, plus the table."""
    n = 3
    hist = np.zeros((n, c, 10, 1024), np.uint32)
    hist[:, :, :, 0] = 256
    hist[1, :, :, 0] = 300  # (tiles of different sizes)
    emptied = [3, 7, 0, 1, 2, 4, 5, 6, 8, 9][:k]
    hist[:, :, emptied] = 0
    want = []
    for t in range(n):
        bits = sum(rate_model.context_cost(hist[t, ch, b], b)[0] for ch in range(c) for b in range(10) if b not in emptied)
        want.append(18 + c * (218 + 10 * 14 + 2 * k) + -(-bits // 2 ** 19))
    total, tiles = tiled_rate_ref.estimate_file(hist)
    assert [int(v) for v in tiles] == want
    assert total == 32 + 8 * (n + 1) + sum(want)
    models = tiled_rate_ref.tile_models(hist[0])
    for b in range(10):
        assert tuple(models[0, b]) == ((8, 0, 1) if b in emptied else (8, 0, 0))
    if k:  # the untiled estimate refuses what the tiled one codes
        assert rate_model.estimate_image(hist[0]) == rate_model.UNCODABLE
    # an out-of-alphabet symbol in one tile: that tile and the file
    oob = np.zeros((n, c), np.uint64)
    oob[2, c - 1] = 1
    total, tiles = tiled_rate_ref.estimate_file(hist, oob)
    assert total == rate_model.UNCODABLE and [int(v) for v in tiles] == want[:2] + [rate_model.UNCODABLE]


# ---- the argument checks on host-only plans ---------------------------------------------------------------------------------------------------------------

def _host_plan(c=1):
    return PlanTiled(None, 250, 250, c, 125, 125)


SEARCHES = [("fri_hip_search_quality_tiled", C.c_double, 35.0), ("fri_hip_search_quality_ssim_tiled", C.c_double, 0.9), ("fri_hip_search_quality_for_size_tiled", C.c_uint64, 10000)]


@pytest.mark.parametrize("name,ctype,target", SEARCHES)
def test_searches_refuse_bad_arguments_and_host_only_plans(name, ctype, target):
    L = api.load_library()
    T = _host_plan(3)
    px = np.zeros(T.pixel_bytes, np.uint8)
    host, dev = getattr(L, name), getattr(L, name + "_dev")
    qual, v = C.c_int32(-7), ctype(5)
    # NULLs
    assert host(None, api._p(px), target, C.byref(qual), C.byref(v)) == -1
    assert host(T._h, None, target, C.byref(qual), C.byref(v)) == -1
    assert host(T._h, api._p(px), target, None, C.byref(v)) == -1
    assert host(T._h, api._p(px), target, C.byref(qual), None) == -1
    assert dev(None, 16, target, C.byref(qual), C.byref(v), None) == -1
    assert dev(T._h, None, target, C.byref(qual), C.byref(v), None) == -1
    # targets out of range: a zero budget, a NaN, a negative, an SSIM above 1
    bad = [0] if ctype is C.c_uint64 else [float("nan"), 0.0, -1.0] + ([1.5] if "ssim" in name else [])
    for t in bad:
        assert host(T._h, api._p(px), t, C.byref(qual), C.byref(v)) == -1, t
        assert dev(T._h, 16, t, C.byref(qual), C.byref(v), None) == -1, t
    # compute on a host-only plan, the outputs untouched
    assert host(T._h, api._p(px), target, C.byref(qual), C.byref(v)) == -3
    assert dev(T._h, 16, target, C.byref(qual), C.byref(v), None) == -3
    assert qual.value == -7 and v.value == 5
    # an RCT inner plan
    T.tile.set_colour_transform(api.COLOUR_RCT)
    assert host(T._h, api._p(px), target, C.byref(qual), C.byref(v)) == -1
    assert dev(T._h, 16, target, C.byref(qual), C.byref(v), None) == -1
    T.tile.set_colour_transform(api.COLOUR_YCBCR)
    assert host(T._h, api._p(px), target, C.byref(qual), C.byref(v)) == -3
    T.close()


def test_ssim_search_needs_an_image_of_8_by_8():
    L = api.load_library()
    T = PlanTiled(None, 7, 40, 1, 7, 20, TILED_ALLOW_HOLES)
    px = np.zeros(T.pixel_bytes, np.uint8)
    qual, v = C.c_int32(0), C.c_double(0)
    assert L.fri_hip_search_quality_ssim_tiled(T._h, api._p(px), 0.9, C.byref(qual), C.byref(v)) == -1
    assert L.fri_hip_search_quality_tiled(T._h, api._p(px), 30.0, C.byref(qual), C.byref(v)) == -3
    T.close()


def test_measure_and_estimate_refuse_bad_arguments_and_host_only_plans():
    L = api.load_library()
    T = _host_plan(1)
    hist = np.ones((T.n_tiles, 1, 10, 1024), np.uint32)
    total, tiles = C.c_uint64(7), np.full(T.n_tiles, 9, np.uint64)
    assert L.fri_hip_estimate_size_tiled(None, api._p(hist), None, C.byref(total), api._p(tiles)) == -1
    assert L.fri_hip_estimate_size_tiled(T._h, None, None, C.byref(total), api._p(tiles)) == -1
    assert L.fri_hip_estimate_size_tiled(T._h, api._p(hist), None, None, api._p(tiles)) == -1
    assert L.fri_hip_estimate_size_tiled(T._h, api._p(hist), None, C.byref(total), api._p(tiles)) == -3
    assert total.value == 7 and (tiles == 9).all()
    for args in [(None, 16, None, 16, 16, None, None), (T._h, None, None, 16, 16, None, None), (T._h, 16, None, None, 16, None, None), (T._h, 16, None, 16, None, None, None)]:
        assert L.fri_hip_estimate_size_tiled_dev(*args) == -1, args
    assert L.fri_hip_estimate_size_tiled_dev(T._h, 16, None, 16, 16, None, None) == -3
    for args in [(None, 16, 16, 16, None), (T._h, None, 16, 16, None), (T._h, 16, None, 16, None), (T._h, 16, 16, None, None)]:
        assert L.fri_hip_measure_distortion_tiled_dev(*args) == -1, args
    assert L.fri_hip_measure_distortion_tiled_dev(T._h, 16, 16, 16, None) == -3
    for call in (lambda: T.estimate_size_tiled(hist), lambda: T.estimate_size_tiled_dev(16, None, 16, 16), lambda: T.measure_distortion_tiled_dev(16, 16, 16),
                 lambda: T.search_quality(np.zeros(T.pixel_bytes, np.uint8), 30), lambda: T.search_quality_ssim(16, 0.9), lambda: T.search_quality_for_size(16, 1000)):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -3
    T.close()
