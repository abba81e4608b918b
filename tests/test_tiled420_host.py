"""Tiled 4:2:0 coding, host side (include/fri_hip.h "Tiled 4:2:0 coding", fri_tiled_encode_from_streams420 of include/fri_emit.h): the shape walk over both
lattices, the host-only plan, the emitter and the decoder on oracle arrays in plane order - payload bytes, threads, size query, region decode - and the
refusals. CPU only."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd.api import TILED_ALLOW_HOLES, PlanTiled420, tile_shape, tile_shape420  # noqa: F401  (without the feature the module fails here)
from tests import rate_model
from tests.chroma420_ref import chroma_shape
from tests.tiled420_ref import grid, owns_every_pixel, plane_index, plane_order, split_tiles420, sub_grid, walk420
from tests.tiled_ref import mixed_image, parse_frit

tiled_encode_from_streams420 = emit.tiled_encode_from_streams420  # (without the feature the module fails here)

P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
W, H, TW, TH = 100, 70, 52, 50  # a 2 x 2 grid: the right column and the bottom row are partly replicated
QUALITIES = [1, 60]


# ---- the shape walk ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args,want,plain", [((4096, 4096, 512), (512, 512), None), ((334, 350, 150), (167, 175), None), ((1024, 1024, 128), (128, 135), (128, 128)),
                                            ((200, 100, 96), (103, 100), (100, 100))])
def test_tile_shape420_follows_the_walk_and_both_lattices_own_every_pixel(args, want, plain):
    got = tile_shape420(*args)
    assert got == want == tile_shape420(*args)
    if args[0] <= 1024:  # (the restated walk builds a plan per candidate: kept to the small images)
        assert walk420(*args) == got
    if plain is not None:
        assert tile_shape(*args) == plain
    tw, th = got
    assert owns_every_pixel(tw, th) and owns_every_pixel(*chroma_shape(tw, th))
    PlanTiled420(None, args[0], args[1], tw, th).close()  # create accepts it without ALLOW_HOLES


def test_tile_shape420_refuses_bad_arguments():
    for bad in [(0, 10, 8), (10, 0, 8), (10, 10, 0)]:
        with pytest.raises(fa.FriHipError) as e:
            tile_shape420(*bad)
        assert e.value.code == -1


# ---- the host-only plan ------------------------------------------------------------------------------------------------------------------------------

def test_host_only_plan_getters_refusals_and_no_device():
    assert owns_every_pixel(128, 128) and not owns_every_pixel(64, 64)
    with pytest.raises(fa.FriHipError) as e:  # the luma lattice is whole, the 64 x 64 chroma lattice leaves 8 samples to no cell
        PlanTiled420(None, 256, 256, 128, 128)
    assert e.value.code == -1
    PlanTiled420(None, 256, 256, 128, 128, TILED_ALLOW_HOLES).close()
    for w, h, tw, th, flags in [(0, 8, 4, 4, 1), (8, 0, 4, 4, 1), (8, 8, 0, 4, 1), (8, 8, 4, 0, 1), (256, 128, 1, 1, 1), (256, 256, 128, 128, 2), (256, 256, 128, 128, 3)]:
        with pytest.raises(fa.FriHipError) as e:  # zero sizes, 2 nx ny = 65536 > 65535, unknown flag bits
            PlanTiled420(None, w, h, tw, th, flags)
        assert e.value.code == -1, (w, h, tw, th, flags)
    PlanTiled420(None, 255, 128, 1, 1, TILED_ALLOW_HOLES).close()  # 2 nx ny = 65280
    p = PlanTiled420(None, W, H, TW, TH)
    cw, ch = chroma_shape(TW, TH)
    assert (p.nx, p.ny, p.tile_w, p.tile_h, p.n_tiles, p.cw, p.ch) == (2, 2, TW, TH, 4, cw, ch)
    for view, (pw, ph) in ((p.luma, (TW, TH)), (p.chroma, (cw, ch))):
        ref = fa.Plan(None, pw, ph, 1)
        assert (view.num_cells, view.num_some, view.pixel_bytes) == (ref.num_cells, ref.num_some, ref.pixel_bytes)
        assert np.array_equal(view.centers(), ref.centers())
        ref.close()
    assert p.region_tiles(51, 49, 2, 2) == (0, 0, 2, 2) and p.region_tiles(99, 69, 1, 1) == (1, 1, 1, 1) and p.buffer_tiles() == (0, 0)
    for bad in [(0, 0, 0, 1), (W, 0, 1, 1), (1, 0, W, 1)]:
        with pytest.raises(fa.FriHipError) as e:
            p.region_tiles(*bad)
        assert e.value.code == -1
    px = np.zeros((H, W, 3), np.uint8)
    calls = [lambda: p.split_tiles420_dev(16, 16, 16), lambda: p.merge_tiles420_dev(16, 16, 16), lambda: p.merge_tiles420_region_dev(16, 16, 0, 0, 1, 1, 16),
             lambda: p.encode_symbols_tiled420_dev(16, 50, 16, 16, 16, 16), lambda: p.encode_image_tiled420_symbols(px, 50),
             lambda: p.decode_image_tiled420(np.zeros(p.coef_count, np.int32), 50), lambda: p.decode_region_tiled420_dev(16, 50, 0, 0, 1, 1, 16),
             lambda: p.decode_region_tiled420(np.zeros(p.tile_coef_count, np.int32), 50, 0, 0, 1, 1)]
    for k, call in enumerate(calls):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -3, k
    p.close()


# ---- the emitter and the decoder from oracle arrays ---------------------------------------------------------------------------------------------------------------

def _plane_arrays(plane, quality):
    """the oracle's arrays of one plane coded as a C = 1 image, and its symbol stream (the pattern of tests/test_chroma420_host.py)"""
    ph, pw = plane.shape
    centers, coefs, bucket, pred, hist, oob, vp, wp = rate_model.oracle_arrays(np.ascontiguousarray(plane).reshape(-1), pw, ph, 1, quality)
    assert not oob.any()
    sym, bk = emit.channel_symbols(centers, coefs[0], bucket[0], pred[0])
    return dict(coefs=coefs[0], hist=hist[0], vp=vp[0], wp=wp[0], stream=(bk.astype(np.uint16) << 10) | sym)


@functools.lru_cache(maxsize=None)
def _inputs(quality):
    """per tile the (Y, Cb, Cr) oracle arrays, and the encoder's arguments in plane order"""
    assert owns_every_pixel(TW, TH) and owns_every_pixel(*chroma_shape(TW, TH))
    y_tiles, c_tiles = split_tiles420(mixed_image(W, H, 3, TW, 5), TW, TH)
    per = [tuple(_plane_arrays(p, quality) for p in (y_tiles[t], c_tiles[t, 0], c_tiles[t, 1])) for t in range(len(y_tiles))]
    planes = plane_order(per)
    streams = np.concatenate([p["stream"] for p in planes])
    hist, vp, wp = (np.stack([p[k] for p in planes]) for k in ("hist", "vp", "wp"))
    n_y, n_c = per[0][0]["stream"].size, per[0][1]["stream"].size
    return per, (streams, n_y, n_c, hist, vp, wp)


def _coefs_in_plane_order(per):
    return np.concatenate([p["coefs"].reshape(-1) for p in plane_order(per)])


def _tile_file(tile, quality):
    """the `frif` file of one tile: fri_emit_encode_image_from_streams with 3 | YCBCR | 420 | QUALITY(q) | EMPTY_OK"""
    streams = np.concatenate([c["stream"] for c in tile])
    hist, vp, wp = (np.stack([c[k] for c in tile]) for k in ("hist", "vp", "wp"))
    return emit.encode_image_from_streams(TW, TH, streams, hist, vp, wp, quality=quality, ycbcr=True, n_luma=tile[0]["stream"].size, empty_ok=True)


@pytest.mark.parametrize("quality", QUALITIES)
def test_container_payloads_threads_and_round_trip(quality):
    per, (streams, n_y, n_c, hist, vp, wp) = _inputs(quality)
    n = len(per)
    assert (grid(W, H, TW, TH), n) == ((2, 2), 4)
    frv = tiled_encode_from_streams420(W, H, TW, TH, streams, n_y, n_c, hist, vp, wp, quality, threads=1)
    assert frv == tiled_encode_from_streams420(W, H, TW, TH, streams, n_y, n_c, hist, vp, wp, quality, threads=4)
    f = parse_frit(frv)
    assert (f["W"], f["H"], f["tile_w"], f["tile_h"], f["nx"], f["ny"]) == (W, H, TW, TH, 2, 2)
    for t in range(n):
        assert f["payloads"][t] == _tile_file(per[t], quality), t
        assert struct.unpack_from("<I", f["payloads"][t], 12)[0] == 0xC0000000 | 1 << 28 | quality << 8 | 0x4 | 0x2
    F_y, F_c = per[0][0]["coefs"].shape[0], per[0][1]["coefs"].shape[0]
    info = emit.tiled_info(frv)
    assert tuple(info) == (W, H, TW, TH, 2, 2, 3, F_y) and (info.s420, info.ycbcr, info.rct, info.quality) == (True, True, False, quality)
    want = _coefs_in_plane_order(per)
    assert want.size == n * (F_y + 2 * F_c) * 512
    for threads in (1, 4):
        ti, got = emit.tiled_decode(frv, threads)
        assert tuple(ti) == tuple(info) and ti.s420 and got.shape == want.shape and np.array_equal(got, want)
    # through the C ABI: the size query, a buffer one element short (-3 with info filled), the exact buffer
    L = emit.load_library()
    data = np.frombuffer(frv, np.uint8)
    buf = np.zeros(want.size, np.int32)
    for cap, ptr, rc in [(0, None, -3), (buf.size - 1, P(buf), -3), (buf.size, P(buf), 0)]:
        got_info = np.zeros(8, np.uint32)
        assert L.fri_tiled_decode(P(data), data.size, 2, P(got_info), ptr, cap, None, 0) == rc
        assert [int(x) for x in got_info] == [W, H, TW, TH, 2, 2, 3 | emit.YCBCR | emit.S420 | emit.QUALITY(quality), F_y]
    assert np.array_equal(buf, want)


@pytest.mark.parametrize("region", [(99, 69, 1, 1), (50, 48, 4, 4), (0, 0, W, H), (3, 55, 20, 10)], ids=["one pixel", "across both borders", "whole image", "bottom left tile"])
def test_region_decode_returns_the_touched_tiles_planes(region):
    quality = 60
    per, (streams, n_y, n_c, hist, vp, wp) = _inputs(quality)
    frv = tiled_encode_from_streams420(W, H, TW, TH, streams, n_y, n_c, hist, vp, wp, quality)
    info, tiles, got = emit.tiled_decode_region(frv, *region)
    i0, j0, ni, nj = tiles
    assert tiles == emit.tiled_region_tiles(W, H, TW, TH, *region) and info.s420
    touched = [per[(j0 + b) * 2 + i0 + a] for b in range(nj) for a in range(ni)]
    assert np.array_equal(got, _coefs_in_plane_order(touched))
    if region == (0, 0, W, H):
        assert np.array_equal(got, emit.tiled_decode(frv)[1])
    # one element short: -3 with info and tiles filled
    L = emit.load_library()
    data = np.frombuffer(frv, np.uint8)
    buf, got_info, got_tiles = np.zeros(got.size - 1, np.int32), np.zeros(8, np.uint32), np.zeros(4, np.uint32)
    assert L.fri_tiled_decode_region(P(data), data.size, 1, *region, P(got_info), P(got_tiles), P(buf), buf.size, None, 0) == -3
    assert tuple(int(v) for v in got_tiles) == tiles and int(got_info[7]) == info[7]


def test_plane_order_helpers():
    assert [plane_index(4, t, c) for t in range(4) for c in range(3)] == [0, 4, 5, 1, 6, 7, 2, 8, 9, 3, 10, 11]
    assert np.array_equal(sub_grid(np.arange(6), 3, 1, 0, 2, 2), [1, 2, 4, 5])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals():
    quality = 60
    per, (streams, n_y, n_c, hist, vp, wp) = _inputs(quality)
    L = emit.load_library()
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    out = np.zeros(1 << 20, np.uint8)
    st, hh = np.ascontiguousarray(streams), np.ascontiguousarray(hist)

    def call(channels, ny=n_y, nc=n_c, tw=TW, cap=out.size):
        return L.fri_tiled_encode_from_streams420(W, H, tw, TH, channels, P(st), ny, nc, P(hh), P(vp), P(wp), 1, P(out), cap, C.addressof(n), err, 256)

    base = 3 | emit.YCBCR | emit.S420 | emit.QUALITY(quality)
    assert call(base) == 0 and call(base | emit.EMPTY_OK) == 0
    want_len = n.value
    assert call(base, cap=100) == -3 and n.value == want_len
    assert call(base, ny=n_y - 1) == -2 and call(base, nc=n_c + 1) == -2
    for bad in (3 | emit.YCBCR | emit.QUALITY(quality), 3 | emit.S420 | emit.QUALITY(quality), 3 | emit.YCBCR | emit.S420, 3 | emit.YCBCR | emit.S420 | emit.QUALITY(100),
                base | emit.ALPHA, base | emit.RCT, 1 | emit.YCBCR | emit.S420 | emit.QUALITY(quality)):
        assert call(bad) == -1, hex(bad)
    assert call(base, tw=0) == -1
    # the 4:4:4 entry point keeps refusing the flag
    assert L.fri_tiled_encode_from_streams(W, H, TW, TH, base, P(st), n_y, P(hh), P(vp), P(wp), 1, P(out), out.size, C.addressof(n), err, 256) == -1
    # one tile's payload replaced by a non-4:2:0 payload of the same tile shape: "Malformed tiled image"
    frv = tiled_encode_from_streams420(W, H, TW, TH, streams, n_y, n_c, hist, vp, wp, quality)
    f = parse_frit(frv)
    y = per[2][0]
    other = emit.encode_image_from_streams(TW, TH, y["stream"][None], y["hist"][None], y["vp"][None], y["wp"][None], quality=quality, empty_ok=True)
    assert other[:4] == b"frif" and struct.unpack_from("<2I", other, 4) == (TH, TW)
    for k in (0, 2):
        pl = list(f["payloads"])
        pl[k] = other
        table, at = [], f["offsets"][0]
        for p in pl:
            table.append(at)
            at += len(p)
        bad = np.frombuffer(frv[:32] + struct.pack("<5Q", *table, at) + b"".join(pl), np.uint8)
        info, buf = np.zeros(8, np.uint32), np.zeros(1 << 20, np.int32)
        assert L.fri_tiled_decode(P(bad), bad.size, 2, P(info), P(buf), buf.size, err, 256) == -2 and b"Malformed tiled image" in err.value, k
        assert L.fri_tiled_info(P(bad), bad.size, P(info)) == -2
    # bit 2 without bit 1, and bits 2 and 0, in every tile: invalid metadata, so no tiled file either
    for clear, set_ in ((0x2, 0), (0, 0x1)):
        b = bytearray(frv)
        for o in f["offsets"][:-1]:
            word = struct.unpack_from("<I", b, o + 12)[0]
            struct.pack_into("<I", b, o + 12, (word & ~clear) | set_)
        bad = np.frombuffer(bytes(b), np.uint8)
        info = np.zeros(8, np.uint32)
        assert L.fri_tiled_info(P(bad), bad.size, P(info)) == -2
