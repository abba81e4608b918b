"""The searches, the size estimate and the device coder of tiled 4:2:0 coding, host side (include/fri_hip.h "Tiled 4:2:0 coding";
fri_tiled_encode_from_coded420 of include/fri_emit.h). CPU only:

- the plane-order restatement of the estimate (tests/tiled420_rate_ref.py: a reorder in front of tests/tiled_rate_ref.py) against the payloads the emitter writes
  from oracle histograms;
- the container assembled from coded planes in plane order is byte for byte the container coded from the streams, on 1 and 4 threads; the size query; the refusals;
- a host-only plan refuses every new compute entry point with -3, bad arguments with -1;
- tests/tools/tiled420_coded_check.cpp, a program with its own main, under the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd import api
from frave_amd.api import PlanTiled420
from tests import rans_ref, tiled420_rate_ref
from tests.test_tiled420_host import H, QUALITIES, TH, TW, W, _inputs
from tests.tiled_ref import parse_frit

for _name in ("measure_distortion_tiled420_dev", "estimate_size_tiled420", "estimate_size_tiled420_dev", "search_quality", "search_quality_ssim", "search_quality_for_size",
              "encode_image_tiled420_coded"):
    assert hasattr(PlanTiled420, _name), _name  # (without the feature the module fails here)
tiled_encode_from_coded420 = emit.tiled_encode_from_coded420

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


# ---- the estimate in plane order ----------------------------------------------------------------------------------------------------------------------------

def test_tile_order_is_the_inverse_of_plane_order():
    n = 5
    planes = np.arange(3 * n)
    tiles = tiled420_rate_ref.tile_order(planes)
    assert tiles.tolist() == [[t, n + 2 * t, n + 2 * t + 1] for t in range(n)]


@pytest.mark.parametrize("quality", QUALITIES)
def test_restated_estimate_is_within_24_bytes_per_channel_of_the_emitters_payloads(quality):
    per, (streams, n_y, n_c, hist, vp, wp) = _inputs(quality)
    f = parse_frit(emit.tiled_encode_from_streams420(W, H, TW, TH, streams, n_y, n_c, hist, vp, wp, quality))
    est_file, est_tiles = tiled420_rate_ref.estimate_file(hist)
    n = len(per)
    gaps = [int(est_tiles[t]) - len(f["payloads"][t]) for t in range(n)]
    print("quality", quality, "payload gaps", gaps, "file gap", est_file - f["offsets"][-1])
    assert max(map(abs, gaps)) <= 24 * 3, gaps  # the bound of tests/test_gpu_tiled_search.py, per channel
    assert est_file == 32 + 8 * (n + 1) + int(est_tiles.sum())
    # an out-of-alphabet count in Cr of the last tile: that tile and the file are uncodable, the others unchanged
    oob = np.zeros(3 * n, np.uint64)
    oob[3 * n - 1] = 1
    bad_file, bad_tiles = tiled420_rate_ref.estimate_file(hist, oob)
    assert bad_file == 2 ** 64 - 1 and int(bad_tiles[n - 1]) == 2 ** 64 - 1 and np.array_equal(bad_tiles[: n - 1], est_tiles[: n - 1])


# ---- the container from coded planes ----------------------------------------------------------------------------------------------------------------------------

def coded_planes(streams, n_tiles, n_y, n_c, hist, pad=3):
    """(words [3 n][stride], n_words, models [3 n][10][4], off [3 n][10][1024]) in plane order from tests/rans_ref.py: every plane coded on the host"""
    chroma = streams[n_tiles * n_y:]
    planes = [streams[t * n_y:(t + 1) * n_y] for t in range(n_tiles)] + [chroma[k * n_c:(k + 1) * n_c] for k in range(2 * n_tiles)]
    refs = [rans_ref.encode_plane(s, h) for s, h in zip(planes, hist)]
    assert all(r.status == 0 for r in refs)
    stride = max(len(r.words) for r in refs) + pad
    words = np.full((len(refs), stride), 0xDEADBEEF, np.uint32)
    n_words = np.array([len(r.words) for r in refs], np.uint32)
    models = np.full((len(refs), 10, 4), 77, np.uint32)  # (the last two words are not read)
    off = np.full((len(refs), 10, 1024), 0xFFFF, np.uint16)
    for p, r in enumerate(refs):
        words[p, :len(r.words)] = r.words
        for b in range(10):
            models[p, b, :2] = r.max_freq_bits[b], len(r.off[b])
            off[p, b, :len(r.off[b])] = r.off[b]
    return words, n_words, models, off


@pytest.mark.parametrize("quality", QUALITIES)
def test_container_from_coded_planes_is_the_container_from_streams(quality):
    per, (streams, n_y, n_c, hist, vp, wp) = _inputs(quality)
    n = len(per)
    words, n_words, models, off = coded_planes(streams, n, n_y, n_c, hist)
    want = emit.tiled_encode_from_streams420(W, H, TW, TH, streams, n_y, n_c, hist, vp, wp, quality)
    for threads in (1, 4):
        assert emit.tiled_encode_from_coded420(W, H, TW, TH, words, n_words, models, off, vp, wp, quality, threads=threads) == want
    # the ABI: the size query, the refusals
    L = emit.load_library()
    size, err, out = C.c_size_t(0), C.create_string_buffer(256), np.zeros(len(want), np.uint8)
    arg = emit._arg(3, False, quality, True, True)  # 3 | YCBCR | 420 | QUALITY(q)

    def call(channels=arg, nw=n_words, m=models, cap=out.size, tile_w=TW, dst=out):
        nw, m = np.ascontiguousarray(nw, np.uint32), np.ascontiguousarray(m, np.uint32)
        return L.fri_tiled_encode_from_coded420(W, H, tile_w, TH, channels, P(words), words.shape[1], P(nw), P(m), P(off), P(vp), P(wp), 1, None if dst is None else P(dst), cap,
                                                C.addressof(size), err, 256)

    assert call() == 0 and size.value == len(want) and out.tobytes() == want
    assert call(cap=len(want) - 1) == -3 and size.value == len(want)
    assert call(dst=None, cap=0) == -3 and size.value == len(want)
    assert call(channels=arg | emit.EMPTY_OK) == 0
    assert call(channels=emit._arg(3, False, quality, True, False)) == -1  # without FRI_EMIT_420
    assert call(channels=arg | emit.ALPHA) == -1 and call(channels=emit._arg(3, False, 0, False, False)) == -1 and call(tile_w=0) == -1
    short, long_ = n_words.copy(), n_words.copy()
    short[n + 2 * 2] = 19  # Cb of tile 2
    long_[1] = words.shape[1] + 1
    assert call(nw=short) == -2 and b"tile 2: channel 1" in err.value
    assert call(nw=long_) == -2 and b"tile 1: channel 0" in err.value
    many = models.copy()
    many[n + 2 * 3 + 1, 4, 1] = 1025  # Cr of tile 3
    assert call(m=many) == -2 and b"tile 3: channel 2" in err.value
    # the 4:4:4 entry point keeps refusing FRI_EMIT_420
    assert L.fri_tiled_encode_from_coded(W, H, TW, TH, arg, P(words), words.shape[1], P(n_words), P(models), P(off), P(vp), P(wp), 1, P(out), out.size, C.addressof(size), err,
                                         256) == -1


# ---- the host-only plan -----------------------------------------------------------------------------------------------------------------------------------------

def test_host_only_plan_refuses_the_new_entry_points():
    p = PlanTiled420(None, W, H, TW, TH)
    n = p.n_tiles
    px = np.zeros((H, W, 3), np.uint8)
    hist = np.zeros((3 * n, 10, 1024), np.uint32)
    calls = [lambda: p.measure_distortion_tiled420_dev(16, 16, 16, 16), lambda: p.estimate_size_tiled420_dev(16, None, 16, 16), lambda: p.estimate_size_tiled420(hist),
             lambda: p.search_quality(px, 30.0), lambda: p.search_quality(16, 30.0), lambda: p.search_quality_ssim(px, 0.9), lambda: p.search_quality_ssim(16, 0.9),
             lambda: p.search_quality_for_size(px, 10 ** 6), lambda: p.search_quality_for_size(16, 10 ** 6), lambda: p.encode_image_tiled420_coded(px, 50)]
    for k, call in enumerate(calls):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -3, k
    bad = [lambda: p.measure_distortion_tiled420_dev(0, 16, 16, 16), lambda: p.measure_distortion_tiled420_dev(16, 16, 16, 0), lambda: p.estimate_size_tiled420_dev(0, None, 16, 16),
           lambda: p.estimate_size_tiled420_dev(16, None, 16, 0), lambda: p.search_quality(px, 0.0), lambda: p.search_quality(px, float("nan")), lambda: p.search_quality(0, 30.0),
           lambda: p.search_quality_ssim(px, 1.5), lambda: p.search_quality_ssim(px, 0.0), lambda: p.search_quality_for_size(px, 0)]
    for k, call in enumerate(bad):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -1, k
    L = api.load_library()
    assert L.fri_hip_measure_distortion_tiled420_dev(None, 16, 16, 16, 16, None) == -1
    assert L.fri_hip_estimate_size_tiled420(None, P(hist), None, P(np.zeros(1, np.uint64)), None) == -1
    assert L.fri_hip_encode_image_tiled420_coded(None, P(px), 50, 16, 16, 16, 64, 16, 16, 16, 16) == -1
    p.close()
    small = PlanTiled420(None, 7, 9, 7, 9, api.TILED_ALLOW_HOLES)  # SSIM needs W, H >= 8: refused before the device is asked for
    with pytest.raises(fa.FriHipError) as e:
        small.search_quality_ssim(np.zeros((9, 7, 3), np.uint8), 0.9)
    assert e.value.code == -1
    small.close()


# ---- under the host sanitizers -----------------------------------------------------------------------------------------------------------------------------------

def test_coded420_assembly_under_the_host_sanitizers(tmp_path):
    """A stand-alone program with its own main: nothing loaded into python is run under a sanitizer."""
    exe = tmp_path / "tiled420_coded_check"
    src = [os.path.join(ROOT, *parts) for parts in (("tests", "tools", "tiled420_coded_check.cpp"), ("frave_amd", "host", "emit.cpp"), ("frave_amd", "host", "emit_abi.cpp"),
                                                     ("frave_amd", "csrc", "geometry.cpp"))]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "frave_amd", "host"), "-o", str(exe)] + src)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
