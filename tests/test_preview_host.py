"""Preview decode, host side (include/fri_emit.h fri_tiled_decode_levels; include/fri_hip.h "Preview decode"): the level-limited decode against the full decode
sliced, its refusals and size query, the prefix counts against the valid mask and the stream order, a damaged stream that a low level does not see, the host-only
plan's refusals, and tests/preview_ref.py against the image it must give back at L = 9. CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.api as api
import frave_amd.emit as emit
from frave_amd.api import TILED_ALLOW_HOLES, PlanTiled
from tests import preview_ref
from tests.coded_cases import tiled420_file, tiled_file
from tests.tiled_ref import mixed_image, parse_frit

tiled_decode_levels = emit.tiled_decode_levels  # (without the feature the module fails here)
preview_size = api.preview_size

P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (W, H, C, tile_w, tile_h, quality, flags): lossless C = 1, RCT, quality 50, YCbCr 37
FILES = [(250, 250, 1, 125, 125, 100, {}), (334, 350, 3, 167, 117, 100, dict(rct=True)), (250, 250, 1, 125, 125, 50, {}), (334, 350, 3, 167, 117, 37, dict(ycbcr=True))]


def _file(case):
    w, h, c, tw, th, quality, flags = case
    return tiled_file(w, h, c, tw, th, quality, **flags)[0]


@pytest.mark.parametrize("case", FILES, ids=lambda c: "%dx%dx%d_q%d" % (c[0], c[1], c[2], c[5]))
def test_level_limited_decode_is_the_full_decode_sliced(case):
    frv = _file(case)
    ti, full = emit.tiled_decode(frv)
    assert (full == preview_ref.NONE).any()
    for levels in range(10):
        for threads in (1, 4):
            info, got = tiled_decode_levels(frv, levels, threads)
            assert tuple(info) == tuple(ti) and got.shape == full.shape[:3] + (1 << levels,)
            assert np.array_equal(got, full[..., : 1 << levels]), (levels, threads)
    assert np.array_equal(tiled_decode_levels(frv, 9)[1], full)  # L = 9 is the full planes


def test_refusals_and_the_size_query():
    frv = _file(FILES[0])
    L = emit.load_library()
    data = np.frombuffer(frv, np.uint8)
    ti, full = emit.tiled_decode(frv)
    want_info = [int(v) for v in ti[:8]]
    levels = 3
    buf = np.zeros(full.size >> (9 - levels), np.int32)
    for cap, ptr, rc in [(0, None, -3), (buf.size - 1, P(buf), -3), (buf.size, P(buf), 0)]:
        info = np.zeros(8, np.uint32)
        assert L.fri_tiled_decode_levels(P(data), data.size, 2, levels, P(info), ptr, cap, None, 0) == rc
        assert [int(x) for x in info] == want_info
    assert np.array_equal(buf.reshape(full.shape[:3] + (8,)), full[..., :8])
    info, err = np.zeros(8, np.uint32), C.create_string_buffer(256)
    assert L.fri_tiled_decode_levels(P(data), data.size, 2, 10, P(info), P(buf), buf.size, err, 256) == -1
    assert L.fri_tiled_decode_levels(None, data.size, 2, 3, P(info), P(buf), buf.size, err, 256) == -1
    assert L.fri_tiled_decode_levels(P(data), data.size, 2, 3, None, P(buf), buf.size, err, 256) == -1
    with pytest.raises(emit.EmitError):
        tiled_decode_levels(frv, 10)
    # what fri_tiled_decode refuses as malformed is malformed here too
    assert L.fri_tiled_decode_levels(P(data), data.size - 1, 2, 3, P(info), P(buf), buf.size, err, 256) == -2 and b"Malformed tiled image" in err.value
    # a tiled 4:2:0 file: -1, and the message names what to do instead - at every level, 9 included
    frv420 = tiled420_file(100, 70, 52, 50, 50)[0]
    d420 = np.frombuffer(frv420, np.uint8)
    for lv in (0, 4, 9):
        assert L.fri_tiled_decode_levels(P(d420), d420.size, 2, lv, P(info), None, 0, err, 256) == -1
        assert b"4:2:0" in err.value and b"fri_tiled_decode" in err.value
    with pytest.raises(emit.EmitError, match="fri_tiled_decode"):
        tiled_decode_levels(frv420, 5)


# shapes with holes (140 x 140, 64 x 64), thinner than a cell (300 x 5, 3 x 200, 1 x 1), and whole lattices
SHAPES = [(140, 140), (64, 64), (300, 5), (3, 200), (1, 1), (125, 125), (167, 117)]


@pytest.mark.parametrize("shape", SHAPES)
def test_prefix_counts_are_the_valid_masks_and_the_stream_orders(shape):
    w, h = shape
    plan = fa.Plan(None, w, h, 1)
    bits = plan.valid_bits()
    order = emit.stream_order(plan.centers(), plan.valid_mask())
    heaps = order & 511
    counts = [plan.num_some_levels(levels) for levels in range(10)]
    assert counts[9] == plan.num_some == order.size and counts[0] == plan.num_cells
    assert all(a <= b for a, b in zip(counts, counts[1:]))
    for levels in range(10):
        n = counts[levels]
        assert n == preview_ref.num_some_levels(bits, levels)
        # the stream-order entries with heap index < 2^L are exactly the first n entries
        assert (heaps[:n] < (1 << levels)).all() and (heaps[n:] >= (1 << levels)).all()
    with pytest.raises(fa.FriHipError) as e:
        plan.num_some_levels(10)
    assert e.value.code == -1
    plan.close()


def test_preview_size_and_argument_errors():
    assert preview_size(41, 17, 3) == (6, 3) and preview_size(41, 17, 0) == (41, 17) and preview_size(1, 1, 4) == (1, 1) and preview_size(4096, 4096, 2) == (1024, 1024)
    for bad in [(0, 4, 1), (4, 0, 1), (4, 4, 5)]:
        with pytest.raises(fa.FriHipError) as e:
            preview_size(*bad)
        assert e.value.code == -1


def test_host_only_tiled_plan_refuses_the_preview():
    p = PlanTiled(None, 250, 250, 1, 125, 125)
    calls = [lambda: p.preview(np.zeros((4, 1, p.num_cells, 4), np.int32), 2, 1), lambda: p.preview_tiles_dev(16, p.num_cells * 4, 4, 2, 1, 16)]
    for call in calls:
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -3
    p.close()


def cut_stream_file():
    """(frit bytes, plane, low level): the lossless C = 1 file with plane 1's rANS data cut to half its words - the host decoder accepts the low level, whose
    prefix ends long before the cut, and refuses the whole plane as truncated. Chosen and checked on the CPU; tests/test_gpu_preview.py runs K13 on it."""
    from tests.test_gpu_decode import _with_plane_data

    frv = _file(FILES[0])
    ti, words, n_words, models, off, vp, wp = emit.tiled_parse_coded(frv)
    plane, keep = 1, int(n_words[1]) // 2
    cut = _with_plane_data(frv, words[plane, : n_words[plane]], 1, plane, words[plane, :keep])
    parse_frit(cut)
    return cut, plane, 3


def test_damage_beyond_the_prefix_is_not_seen():
    cut, plane, low = cut_stream_file()
    ti, full = emit.tiled_decode(_file(FILES[0]))
    with pytest.raises(emit.EmitError, match="tile %d: channel 0: stream truncated" % plane):
        tiled_decode_levels(cut, 9)
    with pytest.raises(emit.EmitError, match="stream truncated"):
        emit.tiled_decode(cut)
    got = tiled_decode_levels(cut, low)[1]
    assert np.array_equal(got, full[..., : 1 << low])


def test_the_reference_gives_the_image_back_at_level_9():
    w, h, c, tw, th, quality, flags = FILES[0]
    ti, full = emit.tiled_decode(_file(FILES[0]))
    img = mixed_image(w, h, c, tw, 3)
    assert np.array_equal(preview_ref.lossless_preview_image(full, w, h, tw, th, 9), img)
    assert np.array_equal(preview_ref.subsample(img, 3)[:, :, 0], img[np.minimum(np.arange(32) * 8 + 4, h - 1)][:, np.minimum(np.arange(32) * 8 + 4, w - 1), 0])
    low = preview_ref.lossless_preview_image(full, w, h, tw, th, 0)  # the DC alone: every pixel of a cell carries one value
    assert low.shape == img.shape and len(np.unique(low)) <= ti[7] * 4 + 1
    compact = full[..., :8]
    plan = fa.Plan(None, tw, th, 1)
    assert np.array_equal(preview_ref.expand(compact, plan.valid_bits()), preview_ref.prefix_planes(full, 3))
    plan.close()
    assert TILED_ALLOW_HOLES == 1


def test_parser_and_level_limited_decoder_under_the_sanitizers(tmp_path):
    """A stand-alone program with its own main: nothing loaded into python is run under a sanitizer."""
    exe, src = tmp_path / "preview_host_check", tmp_path / "in.frv"
    host, csrc = os.path.join(ROOT, "frave_amd", "host"), os.path.join(ROOT, "frave_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "include"), "-I", host, "-I", csrc, "-o", str(exe), os.path.join(ROOT, "tests", "tools", "preview_host_check.cpp"),
                           os.path.join(host, "emit.cpp"), os.path.join(host, "emit_abi.cpp"), os.path.join(csrc, "geometry.cpp")])
    src.write_bytes(tiled_file(100, 70, 1, 52, 50, 100)[0])
    out = subprocess.run([str(exe), str(src)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
