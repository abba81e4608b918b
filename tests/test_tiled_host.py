"""Tiled coding, host side (include/fri_hip.h "tiled coding", the `frit` container and FRI_EMIT_EMPTY_OK of include/fri_emit.h): the numpy restatement, the
container bytes against an independent parser, refusals, the tile-shape search and the owned-pixel count against the oracle, the host-only tiled plan, and the
emitter's rule for contexts without symbols. CPU only."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd.api import TILED_ALLOW_HOLES, PlanTiled, tile_shape  # noqa: F401  (without the feature the module fails here)
from tests import rate_model
from tests.common import KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS, gen_image
from tests.tiled_ref import grid, merge_tiles, mixed_image, parse_frit, split_tiles

P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
CASES = [(250, 250, 1, 125, 125), (334, 350, 3, 167, 117)]  # (W, H, C, tile_w, tile_h)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1), (5, 3, 3, 2, 2), (17, 9, 1, 16, 4), (33, 20, 3, 16, 16), (64, 48, 3, 64, 48), (50, 40, 1, 64, 64), (257, 130, 3, 100, 50)])
def test_restatement_replicates_the_edge_and_round_trips(shape):
    w, h, c, tw, th = shape
    img = gen_image("noise", w, h, c, w + 3 * h)
    nx, ny = grid(w, h, tw, th)
    tiles = split_tiles(img, tw, th)
    assert tiles.shape == (nx * ny, th, tw, c)
    for t in range(nx * ny):  # against a literal per-pixel loop on a few pixels of every tile
        j, i = divmod(t, nx)
        for y, x in {(0, 0), (th - 1, tw - 1), (th // 2, tw - 1), (th - 1, tw // 2)}:
            assert np.array_equal(tiles[t, y, x], img[min(j * th + y, h - 1), min(i * tw + x, w - 1)])
    assert np.array_equal(merge_tiles(tiles, w, h, fill=7), img)


# ---- owned pixels, the tile shape, the tiled plan -------------------------------------------------------------------------------------------------------------

def _oracle_owned(w, h):
    from oracle import fri_oracle

    W = fri_oracle.Wavelet(np.full(w * h, 255, np.uint8), h, w, 1)
    back = W.to_raster()
    W.close()
    return int(np.count_nonzero(back))


@pytest.mark.parametrize("shape,want", [((140, 140), 19586), ((150, 100), 14999), ((64, 64), 4088), ((128, 128), 128 * 128), ((167, 117), 167 * 117)])
def test_owned_pixels_is_the_oracle_rasters_nonzero_count(shape, want):
    w, h = shape
    plan = fa.Plan(None, w, h, 1)
    assert plan.owned_pixels() == want == _oracle_owned(w, h)
    plan.close()


def _walk(w, h, target):
    """fri_hip_tile_shape restated: the documented walk, with the owned-pixel getter as the test of a shape"""
    def first(size):
        parts = max(1, (2 * size + target) // (2 * target))  # round half up
        return -(-size // parts)
    w0, h0 = first(w), first(h)
    for s in range(65):
        for a in range(s + 1):
            tw, th = w0 + a, h0 + s - a
            plan = fa.Plan(None, tw, th, 1)
            whole = plan.owned_pixels() == tw * th
            plan.close()
            if whole:
                return tw, th
    return None


@pytest.mark.parametrize("args", [(250, 250, 125), (334, 350, 150), (140, 140, 140), (64, 64, 64), (1000, 700, 512), (127, 71, 100), (300, 140, 140)])
def test_tile_shape_is_deterministic_follows_the_walk_and_owns_every_pixel(args):
    w, h, target = args
    tw, th = tile_shape(w, h, target)
    assert (tw, th) == tile_shape(w, h, target) == _walk(w, h, target)
    assert _oracle_owned(tw, th) == tw * th
    PlanTiled(None, w, h, 1, tw, th).close()  # create accepts it without ALLOW_HOLES


def test_tile_shape_of_a_holed_start_moves_on_and_refuses_bad_arguments():
    assert tile_shape(140, 140, 140) != (140, 140) and tile_shape(64, 64, 64) != (64, 64)
    assert tile_shape(250, 250, 125) == (125, 125) and tile_shape(256, 256, 512) == (256, 256)
    for bad in [(0, 10, 8), (10, 0, 8), (10, 10, 0)]:
        with pytest.raises(fa.FriHipError) as e:
            tile_shape(*bad)
        assert e.value.code == -1


def test_tiled_plan_create_getters_and_refusals():
    p = PlanTiled(None, 334, 350, 3, 167, 117)
    assert (p.nx, p.ny, p.tile_w, p.tile_h, p.n_tiles) == (2, 3, 167, 117, 6)
    inner = fa.Plan(None, 167, 117, 3)
    assert (p.tile.num_cells, p.tile.num_some, p.tile.pixel_bytes) == (inner.num_cells, inner.num_some, inner.pixel_bytes)
    inner.close()
    p.close()
    for w, h, c, tw, th in [(0, 8, 1, 4, 4), (8, 0, 1, 4, 4), (8, 8, 1, 0, 4), (8, 8, 1, 4, 0), (128, 128, 2, 128, 128), (128, 128, 4, 128, 128), (300, 300, 1, 1, 1), (300, 300, 3, 2, 2)]:
        with pytest.raises(fa.FriHipError) as e:
            PlanTiled(None, w, h, c, tw, th, TILED_ALLOW_HOLES)
        assert e.value.code == -1, (w, h, c, tw, th)
    with pytest.raises(fa.FriHipError) as e:  # an unknown flag bit
        PlanTiled(None, 128, 128, 1, 128, 128, 2)
    assert e.value.code == -1
    # 140 x 140 tiles leave 14 pixels to no cell: refused unless asked for
    with pytest.raises(fa.FriHipError) as e:
        PlanTiled(None, 280, 280, 1, 140, 140)
    assert e.value.code == -1
    PlanTiled(None, 280, 280, 1, 140, 140, TILED_ALLOW_HOLES).close()


def test_host_only_tiled_plan_refuses_compute():
    p = PlanTiled(None, 250, 250, 1, 125, 125)
    with pytest.raises(fa.FriHipError) as e:
        p.encode_image_tiled_symbols(np.zeros((250, 250, 1), np.uint8))
    assert e.value.code == -3
    with pytest.raises(fa.FriHipError) as e:
        p.decode_image_tiled(np.zeros(p.coef_count, np.int32))
    assert e.value.code == -3
    for call in (p.split_tiles_dev, p.merge_tiles_dev):
        with pytest.raises(fa.FriHipError) as e:
            call(16, 32)
        assert e.value.code == -3
    with pytest.raises(fa.FriHipError) as e:
        p.encode_symbols_tiled_dev(16, 16, 16, 16, 16)
    assert e.value.code == -3
    p.close()


# ---- the container ------------------------------------------------------------------------------------------------------------------------------------

def _streams(centers, coefs, bucket, pred):
    out = []
    for ch in range(coefs.shape[0]):
        sym, bk = emit.channel_symbols(centers, coefs[ch], bucket[ch], pred[ch])
        out.append((bk.astype(np.uint16) << 10) | sym)
    return np.stack(out)


def _tile_arrays(tile, tw, th, c):
    """(streams [C][n], hist [C][10][1024], vp, wp [C][3][6], coefs [C][F][512]) of one tile from the oracle, lossless, the known-answer parameters"""
    centers, coefs, bucket, pred, hist, oob, vp, wp = rate_model.oracle_arrays(np.ascontiguousarray(tile).reshape(-1), tw, th, c, 100)
    assert not oob.any()
    return _streams(centers, coefs, bucket, pred), hist, vp, wp, coefs


@functools.lru_cache(maxsize=None)
def _inputs(case):
    w, h, c, tw, th = case
    tiles = split_tiles(mixed_image(w, h, c, tw, 3), tw, th)
    per = [_tile_arrays(t, tw, th, c) for t in tiles]
    return tuple(np.stack([p[k] for p in per]) for k in range(5))


@pytest.mark.parametrize("case", CASES)
def test_container_bytes_payloads_threads_and_round_trip(case):
    w, h, c, tw, th = case
    streams, hist, vp, wp, coefs = _inputs(case)
    nx, ny = grid(w, h, tw, th)
    n = nx * ny
    assert hist.shape == (n, c, 10, 1024) and (hist.sum(axis=3) > 0).all(), "every tile fills all ten contexts of every channel"
    frv = emit.tiled_encode_from_streams(w, h, tw, th, streams, hist, vp, wp, threads=1)
    assert frv == emit.tiled_encode_from_streams(w, h, tw, th, streams, hist, vp, wp, threads=4) == emit.tiled_encode_from_streams(w, h, tw, th, streams, hist, vp, wp)
    f = parse_frit(frv)
    assert (f["W"], f["H"], f["tile_w"], f["tile_h"], f["nx"], f["ny"]) == (w, h, tw, th, nx, ny)
    assert f["offsets"][0] == 32 + 8 * (n + 1) and f["offsets"][-1] == len(frv)
    for t in range(n):  # a payload is the tile's own file, with and without the empty-context rule (no context is empty here)
        want = emit.encode_image_from_streams(tw, th, streams[t], hist[t], vp[t], wp[t])
        assert f["payloads"][t] == want == emit.encode_image_from_streams(tw, th, streams[t], hist[t], vp[t], wp[t], empty_ok=True)
        assert np.array_equal(emit.decode_image(want)[4], coefs[t])
    info = emit.tiled_info(frv)
    assert tuple(info) == (w, h, tw, th, nx, ny, c, coefs.shape[2]) and (info.rct, info.ycbcr, info.quality) == (False, False, 0)
    for threads in (1, 4):
        ti, got = emit.tiled_decode(frv, threads)
        assert tuple(ti) == tuple(info) and got.shape == coefs.shape and np.array_equal(got, coefs)
    # fri_emit_decode_image is not taught the new magic
    with pytest.raises(emit.EmitError):
        emit.decode_image(frv)
    # through the C ABI: the size query, a buffer one element short (-3 with info filled), the exact buffer
    L = emit.load_library()
    data = np.frombuffer(frv, np.uint8)
    want_info = [w, h, tw, th, nx, ny, c, coefs.shape[2]]
    buf = np.zeros(coefs.size, np.int32)
    for cap, ptr, rc in [(0, None, -3), (buf.size - 1, P(buf), -3), (buf.size, P(buf), 0)]:
        got_info = np.zeros(8, np.uint32)
        assert L.fri_tiled_decode(P(data), data.size, 2, P(got_info), ptr, cap, None, 0) == rc
        assert [int(x) for x in got_info] == want_info
    assert np.array_equal(buf.reshape(coefs.shape), coefs)


def test_lossy_modes_ride_on_every_tile_and_420_and_alpha_are_refused():
    w, h, c, tw, th = CASES[1]
    streams, hist, vp, wp, coefs = _inputs(CASES[1])
    for kwargs, word in [(dict(rct=True), 3 << 30 | 1 << 28 | 1), (dict(quality=50), 2 << 30 | 1 << 28 | 50 << 8), (dict(ycbcr=True, quality=37), 3 << 30 | 1 << 28 | 37 << 8 | 2)]:
        frv = emit.tiled_encode_from_streams(w, h, tw, th, streams, hist, vp, wp, **kwargs)
        f = parse_frit(frv)
        assert all(struct.unpack_from("<I", p, 12)[0] == word for p in f["payloads"])
        assert f["payloads"][5] == emit.encode_image_from_streams(tw, th, streams[5], hist[5], vp[5], wp[5], **kwargs)
        info = emit.tiled_info(frv)
        assert (info.rct, info.ycbcr, info.quality) == (bool(kwargs.get("rct")), bool(kwargs.get("ycbcr")), kwargs.get("quality", 0))
    L = emit.load_library()
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    out = np.zeros(1 << 22, np.uint8)
    st, hh = np.ascontiguousarray(streams), np.ascontiguousarray(hist)
    base = 3 | emit.YCBCR | emit.QUALITY(50)
    for arg, rc in [(base, 0), (base | emit.EMPTY_OK, 0), (base | emit.S420, -1), (3 | emit.ALPHA, -1), (2, -1), (3 | emit.YCBCR, -1)]:
        assert L.fri_tiled_encode_from_streams(w, h, tw, th, arg, P(st), st.shape[2], P(hh), P(vp), P(wp), 1, P(out), out.size, C.addressof(n), err, 256) == rc, hex(arg)
    # a symbol count that is not the tile lattice's, and zero sizes
    assert L.fri_tiled_encode_from_streams(w, h, tw, th, 3, P(st), st.shape[2] - 1, P(hh), P(vp), P(wp), 1, P(out), out.size, C.addressof(n), err, 256) == -2
    assert L.fri_tiled_encode_from_streams(w, h, 0, th, 3, P(st), st.shape[2], P(hh), P(vp), P(wp), 1, P(out), out.size, C.addressof(n), err, 256) == -1
    # -3 with the needed size
    assert L.fri_tiled_encode_from_streams(w, h, tw, th, 3, P(st), st.shape[2], P(hh), P(vp), P(wp), 1, P(out), 100, C.addressof(n), err, 256) == -3
    assert n.value == len(emit.tiled_encode_from_streams(w, h, tw, th, streams, hist, vp, wp))


def _decode_rc(data):
    data = np.frombuffer(bytes(data), np.uint8)
    info = np.zeros(8, np.uint32)
    err = C.create_string_buffer(256)
    buf = np.zeros(1 << 22, np.int32)
    rc = emit.load_library().fri_tiled_decode(P(data), data.size, 2, P(info), P(buf), buf.size, err, 256)
    return rc, err.value.decode()


def test_malformed_files_are_refused():
    w, h, c, tw, th = CASES[0]
    streams, hist, vp, wp, coefs = _inputs(CASES[0])
    frv = emit.tiled_encode_from_streams(w, h, tw, th, streams, hist, vp, wp)
    f = parse_frit(frv)
    assert _decode_rc(frv)[0] == 0
    bad = []

    def patched(at, fmt, value):
        b = bytearray(frv)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)

    o = f["offsets"]
    bad.append(patched(32 + 8, "<Q", o[1] + 1))      # a shifted offset: the payload no longer starts with its magic
    bad.append(patched(32 + 8, "<Q", o[2]))          # not strictly increasing
    bad.append(patched(32 + 16, "<Q", o[1] - 8))     # decreasing
    bad.append(patched(32, "<Q", o[0] + 2))          # offset[0] is not the end of the table
    bad.append(patched(32 + 8 * 4, "<Q", o[4] + 1))  # offset[n] is not the file length
    bad.append(frv[:-1])                             # ... nor after a truncation
    bad.append(patched(4, "<I", 2))                  # version
    bad.append(patched(24, "<I", 3))                 # ny is not ceil(H / tile_h)
    bad.append(patched(16, "<I", 0))                 # tile_h = 0
    bad.append(patched(16, "<I", 126))               # a header whose tile is not the payloads'
    bad.append(patched(o[1] + 4, "<I", th + 1))      # a payload of another height
    bad.append(patched(o[3] + 8, "<I", tw - 1))      # ... of another width
    bad.append(patched(o[2] + 12, "<I", struct.unpack_from("<I", frv, o[2] + 12)[0] | 50 << 8))  # ... with another metadata word
    bad.append(f["payloads"][0])                     # a frif file
    bad.append(b"frit")
    # a payload of another size: the file of a 64 x 48 tile in the place of tile 1, the table adjusted
    small = _tile_arrays(gen_image("smooth", 64, 48, 1, 1), 64, 48, 1)
    other = emit.encode_image_from_streams(64, 48, small[0], small[1], small[2], small[3], empty_ok=True)
    pl = list(f["payloads"])
    pl[1] = other
    table, at = [], o[0]
    for p in pl:
        table.append(at)
        at += len(p)
    bad.append(frv[:32] + struct.pack("<5Q", *table, at) + b"".join(pl))
    for k, b in enumerate(bad):
        rc, msg = _decode_rc(b)
        assert rc == -2 and "Malformed tiled image" in msg, (k, rc, msg)
        with pytest.raises(ValueError):
            parse_frit(b)
        info = np.zeros(8, np.uint32)
        data = np.frombuffer(b, np.uint8)
        assert emit.load_library().fri_tiled_info(P(data), data.size, P(info)) == -2, k


# ---- contexts without symbols (FRI_EMIT_EMPTY_OK) -------------------------------------------------------------------------------------------------------------

EMPTY_CASES = [("noise", 64, 48, 1), ("smooth", 40, 40, 3)]  # (kind, W, H, empty contexts), seed 7


@pytest.mark.parametrize("case", EMPTY_CASES)
def test_empty_contexts_are_refused_without_the_flag_and_coded_with_it(case):
    kind, w, h, n_empty = case
    streams, hist, vp, wp, coefs = _tile_arrays(gen_image(kind, w, h, 1, 7), w, h, 1)
    assert int((hist[0].sum(axis=1) == 0).sum()) == n_empty
    with pytest.raises(emit.EmitError) as e:
        emit.encode_image_from_streams(w, h, streams, hist, vp, wp)
    assert "empty context" in str(e.value)
    frv = emit.encode_image_from_streams(w, h, streams, hist, vp, wp, empty_ok=True)
    d = emit.decode_image(frv)  # the existing decoder, unchanged
    assert d[:3] == (w, h, 1) and np.array_equal(d[4], coefs)
    # the flag is taken by the stream route only
    L = emit.load_library()
    n = C.c_size_t(0)
    dummy = np.zeros(16, np.uint8)
    assert L.fri_emit_encode_image(w, h, 1 | emit.EMPTY_OK, P(dummy), 1, P(dummy), P(dummy), P(dummy), P(dummy), P(dummy), P(dummy), None, 0, C.addressof(n), None, 0) == -1
    assert L.fri_emit_check_image(P(dummy), 16, 1 | emit.EMPTY_OK, P(dummy), 1, P(dummy), P(dummy), P(dummy), None, 0) == -1


def test_a_tiled_file_with_empty_contexts_round_trips():
    # 128 x 48 in 64 x 48 tiles: tile 0 is the noise image that leaves a context empty, tile 1 is smooth
    w, h, tw, th = 128, 48, 64, 48
    img = np.concatenate([gen_image("noise", 64, 48, 1, 7), gen_image("smooth", 64, 48, 1, 7)], axis=1)
    tiles = split_tiles(img, tw, th)
    assert np.array_equal(tiles[0], gen_image("noise", 64, 48, 1, 7))
    per = [_tile_arrays(t, tw, th, 1) for t in tiles]
    streams, hist, vp, wp, coefs = (np.stack([p[k] for p in per]) for k in range(5))
    assert (hist[0, 0].sum(axis=1) == 0).any()
    frv = emit.tiled_encode_from_streams(w, h, tw, th, streams, hist, vp, wp, threads=2)
    f = parse_frit(frv)
    assert f["payloads"][0] == emit.encode_image_from_streams(tw, th, streams[0], hist[0], vp[0], wp[0], empty_ok=True)
    ti, got = emit.tiled_decode(frv)
    assert np.array_equal(got, coefs)


def test_large_tiles_are_coded_by_one_loop_per_worker_and_give_the_image_emitters_bytes():
    """a tile of 65536 symbols or more: the image emitter codes it context-parallel, a tile worker with the plain one-loop coder - the same bytes"""
    tw, th = 300, 300
    plan = fa.Plan(None, tw, th, 1)
    n = plan.num_some
    plan.close()
    assert n >= 1 << 16
    rng = np.random.default_rng(5)
    bucket = rng.integers(0, 10, (2, 1, n)).astype(np.uint16)
    symbol = np.minimum(rng.geometric(0.05, (2, 1, n)) * (bucket + 1) // 4, 1023).astype(np.uint16)
    streams = (bucket << 10) | symbol
    hist = np.zeros((2, 1, 10, 1024), np.uint32)
    for t in range(2):
        np.add.at(hist[t, 0], (bucket[t, 0], symbol[t, 0]), 1)
    vp = np.stack([KAT_VALUE_PARAMS[None]] * 2).astype(np.float32)
    wp = np.stack([KAT_WIDTH_PARAMS[None]] * 2).astype(np.float32)
    frv = emit.tiled_encode_from_streams(2 * tw, th, tw, th, streams, hist, vp, wp, threads=2)
    f = parse_frit(frv)
    for t in range(2):
        assert f["payloads"][t] == emit.encode_image_from_streams(tw, th, streams[t], hist[t], vp[t], wp[t])
