"""Tiled RGBA coding on the host (fri_tiled_encode_from_streams_rgba, the tiled decoders on such files, the host-only fri_hip_plan_tiled_rgba) against
tests/tiled_rgba_ref.py and the per-tile emitter. No GPU involved: the streams come from the CPU oracle, as in tests/test_tiled_host.py and
tests/test_alpha_host.py."""
import ctypes as C
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd import api
from frave_amd.api import TILED_ALLOW_HOLES, PlanTiledRgba  # noqa: F401  (without the feature the module fails here)
from tests import rate_model
from tests.alpha_ref import alpha_plane, rgba_image
from tests.common import KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS
from tests.test_rct_host import correlated_image, rct
from tests.tiled_rgba_ref import ALPHA_KEEP, container, grid, merge_tiles_rgba, plane_index, plane_order, split_tiles_rgba
from tests.tiled_ref import parse_frit
from tests.ycbcr_ref import ycc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
# (name, the forward colour transform, the emitter's flags, the quality the oracle quantises at, metadata bits 0..3)
MODES = [("lossless", lambda p: p, dict(), 100, 0x8), ("rct", rct, dict(rct=True), 100, 0x9), ("q50", lambda p: p, dict(quality=50), 50, 0x8),
         ("ycbcr50", ycc, dict(ycbcr=True, quality=50), 50, 0xA)]
# (W, H, tile_w, tile_h): a 2 x 2 and a 3 x 3 grid whose last column and row reach past the image
GRIDS = [(60, 50, 32, 32), (70, 55, 24, 20)]


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (5, 3, 2, 2), (17, 9, 16, 4), (35, 23, 17, 9), (50, 40, 64, 64)])
def test_restatement_replicates_the_edge_cleans_and_round_trips(shape):
    w, h, tw, th = shape
    rng = np.random.default_rng(shape)
    img = rgba_image(rng.integers(1, 256, (h, w, 3), dtype=np.uint8), alpha_plane("random", w, h, w))
    nx, ny = grid(w, h, tw, th)
    for clean in (0, 1):
        colour, alpha = split_tiles_rgba(img, w, h, tw, th, clean)
        assert colour.shape == (nx * ny, th, tw, 3) and alpha.shape == (nx * ny, th, tw)
        for t in (0, nx * ny - 1):
            j, i = divmod(t, nx)
            for y, x in ((0, 0), (th - 1, tw - 1)):
                px = img[min(j * th + y, h - 1), min(i * tw + x, w - 1)]
                assert alpha[t, y, x] == px[3] and tuple(colour[t, y, x]) == ((0, 0, 0) if clean and px[3] == 0 else tuple(px[:3]))
        back = merge_tiles_rgba(colour, alpha, w, h)
        want = img.copy()
        if clean:
            want[img[:, :, 3] == 0, :3] = 0
        assert np.array_equal(back, want)
    assert [plane_index(2, t, c) for t in range(2) for c in range(4)] == [0, 1, 2, 6, 3, 4, 5, 7]
    assert plane_order([("a", "b", "c", "d"), ("e", "f", "g", "h")]) == ["a", "b", "c", "e", "f", "g", "d", "h"]


# ---- the emitter -------------------------------------------------------------------------------------------------------------------------------------------

def _streams(centers, coefs, bucket, pred):
    out = []
    for ch in range(coefs.shape[0]):
        sym, bk = emit.channel_symbols(centers, coefs[ch], bucket[ch], pred[ch])
        out.append((bk.astype(np.uint16) << 10) | sym)
    return np.stack(out)


def _tile_arrays(colour, alpha, tw, th, forward, quality):
    """(streams [4][n], hist [4][10][1024], vp, wp [4][3][6], coefs [4][F][512]) of one RGBA tile from the oracle: the colour planes of the mode, then the
    lossless alpha plane, predicted with parameters of its own so that they must land in the fourth channel"""
    from oracle import fri_oracle

    centers, coefs, bucket, pred, hist, oob, vp, wp = rate_model.oracle_arrays(np.ascontiguousarray(forward(colour)).reshape(-1), tw, th, 3, quality)
    avp, awp = (KAT_VALUE_PARAMS * np.float32(0.5)).astype(np.float32), (KAT_WIDTH_PARAMS * np.float32(2)).astype(np.float32)
    A = fri_oracle.Wavelet(np.ascontiguousarray(alpha).reshape(-1), th, tw, 1)
    A.quantize(np.ones(32, np.int32))
    acenters, acoefs = A.centers(), A.coefficients()
    ab, ap, ah, aoob = A.predict(0, avp, awp)
    A.close()
    assert not oob.any() and not aoob and np.array_equal(centers, acenters)
    streams = np.concatenate([_streams(centers, coefs, bucket, pred), _streams(acenters, acoefs, ab[None], ap[None])])
    return streams, np.concatenate([hist, ah[None]]), np.concatenate([vp, avp.reshape(1, 3, 6)]), np.concatenate([wp, awp.reshape(1, 3, 6)]), np.concatenate([coefs, acoefs])


@functools.lru_cache(maxsize=None)
def _inputs(mode, shape):
    """per tile: the four channels' arrays and the tile's own file; and the same arrays in plane order - computed once, read-only"""
    name, forward, kwargs, quality, bits = next(m for m in MODES if m[0] == mode)
    w, h, tw, th = shape
    img = rgba_image(correlated_image(w, h, 11), alpha_plane("runs", w, h))
    colour, alpha = split_tiles_rgba(img, w, h, tw, th, ALPHA_KEEP)
    per = [_tile_arrays(colour[t], alpha[t], tw, th, forward, quality) for t in range(len(colour))]
    files = [emit.encode_image_from_streams(tw, th, *p[:4], alpha=True, empty_ok=True, **kwargs) for p in per]
    ordered = tuple(np.stack(plane_order([tuple(p[k]) for p in per])) for k in range(5))
    for a in ordered:
        a.setflags(write=False)
    return per, files, ordered


@pytest.mark.parametrize("shape", GRIDS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", [m[0] for m in MODES])
def test_file_is_the_container_of_the_per_tile_alpha_files_and_decodes_in_plane_order(mode, shape):
    name, forward, kwargs, quality, bits = next(m for m in MODES if m[0] == mode)
    w, h, tw, th = shape
    per, files, (streams, hist, vp, wp, coefs) = _inputs(mode, shape)
    nx, ny = grid(w, h, tw, th)
    n = nx * ny
    assert streams.shape[0] == hist.shape[0] == 4 * n and coefs.shape[0] == 4 * n
    frv = emit.tiled_encode_from_streams_rgba(w, h, tw, th, streams, hist, vp, wp, threads=1, **kwargs)
    assert frv == container(w, h, tw, th, files)
    for threads in (2, 5):
        assert frv == emit.tiled_encode_from_streams_rgba(w, h, tw, th, streams, hist, vp, wp, threads=threads, **kwargs), threads
    f = parse_frit(frv)
    assert f["payloads"] == files and all(struct.unpack_from("<I", p, 12)[0] & 0xF == bits for p in f["payloads"])
    q = kwargs.get("quality", 0)
    info = emit.tiled_info(frv)
    F = coefs.shape[1]
    assert tuple(info) == (w, h, tw, th, nx, ny, 3, F) and info.alpha and not info.s420
    assert (info.rct, info.ycbcr, info.quality) == (bool(kwargs.get("rct")), bool(kwargs.get("ycbcr")), q)
    # the whole decode: the per-tile decodes in plane order, which are the oracle's planes
    per_decoded = [emit.decode_image(p) for p in files]
    assert all(d.alpha and d[4].shape == (4, F, 512) for d in per_decoded)
    want = np.stack(plane_order([tuple(d[4]) for d in per_decoded]))
    assert np.array_equal(want, coefs)
    for threads in (1, 4):
        ti, got = emit.tiled_decode(frv, threads)
        assert ti.alpha and tuple(ti) == tuple(info) and got.shape == (4 * n, F, 512) and np.array_equal(got, want), threads
    # regions and tile lists: the rows of the whole decode, in plane order with n = the tiles decoded
    def rows(tiles):
        return np.concatenate([np.concatenate([want[3 * t:3 * t + 3] for t in tiles]), np.stack([want[3 * n + t] for t in tiles])])

    for region in [(w - 1, h - 1, 1, 1), (0, 0, w, h), (tw - 2, th - 1, 5, 2), (0, h - 1, w, 1), (tw + 1, 0, 1, h)]:
        ti, tiles, part = emit.tiled_decode_region(frv, *region)
        i0, j0, ni, nj = tiles
        assert ti.alpha and tiles == emit.tiled_region_tiles(w, h, tw, th, *region)
        assert np.array_equal(part, rows([(j0 + b) * nx + i0 + a for b in range(nj) for a in range(ni)])), region
    for tiles in ([0], [n - 1], [0, n - 1], list(range(n)), [1, 2]):
        ti, part = emit.tiled_decode_tiles(frv, tiles)
        assert ti.alpha and np.array_equal(part, rows(tiles)), tiles
    # fri_emit_decode_image is not taught the magic
    with pytest.raises(emit.EmitError):
        emit.decode_image(frv)


def _abi(frv):
    return emit.load_library(), np.frombuffer(bytes(frv), np.uint8), np.zeros(8, np.uint32), C.create_string_buffer(256)


def test_channels_words_sizes_and_the_old_encoders():
    shape = GRIDS[0]
    w, h, tw, th = shape
    per, files, (streams, hist, vp, wp, coefs) = _inputs("ycbcr50", shape)
    L = emit.load_library()
    st, hh, vv, ww = (np.ascontiguousarray(x) for x in (streams, hist, vp, wp))
    n_symbols = st.shape[1]
    out = np.zeros(1 << 22, np.uint8)
    n, err = C.c_size_t(0), C.create_string_buffer(256)

    def rgba(arg, n_sym=n_symbols, tile_w=tw, cap=out.size):
        return L.fri_tiled_encode_from_streams_rgba(w, h, tile_w, th, arg, P(st), n_sym, P(hh), P(vv), P(ww), 1, P(out), cap, C.addressof(n), err, 256)

    A = emit.ALPHA
    for good in (3 | A, 3 | A | emit.RCT, 3 | A | emit.QUALITY(50), 3 | A | emit.YCBCR | emit.QUALITY(50), 3 | A | emit.EMPTY_OK):
        assert rgba(good) == 0, hex(good)
        assert struct.unpack_from("<I", out, 32 + 8 * 5 + 12)[0] & 0x8
    for bad in (3, 3 | emit.RCT, 3 | emit.YCBCR | emit.QUALITY(50),  # without the flag
                1 | A, 1 | A | emit.QUALITY(50), 4 | A, 2 | A, 4,  # the flag rides on three channels
                3 | A | emit.YCBCR | emit.S420 | emit.QUALITY(50), 3 | A | emit.S420,  # with FRI_EMIT_420
                3 | A | emit.YCBCR, 3 | A | emit.RCT | emit.QUALITY(50), 3 | A | emit.QUALITY(100), 3 | A | emit.RCT | emit.YCBCR | emit.QUALITY(50)):  # refused everywhere
        err.value = b""
        assert rgba(bad) == -1 and err.value == b"invalid argument", hex(bad)
    with pytest.raises(emit.EmitError) as e:
        emit.tiled_encode_from_streams_rgba(w, h, tw, th, streams, hist, vp, wp, flags=3 | A | emit.S420 | emit.YCBCR | emit.QUALITY(50))
    assert e.value.code == -1
    # a symbol count that is not the tile lattice's, a zero size, and -3 with the needed size
    base = 3 | A | emit.YCBCR | emit.QUALITY(50)
    assert rgba(base, n_sym=n_symbols - 1) == -2 and b"n_symbols" in err.value
    assert rgba(base, tile_w=0) == -1
    n.value = 0
    assert rgba(base, cap=100) == -3 and n.value == len(emit.tiled_encode_from_streams_rgba(w, h, tw, th, streams, hist, vp, wp, ycbcr=True, quality=50))
    assert L.fri_tiled_encode_from_streams_rgba(w, h, tw, th, base, P(st), n_symbols, P(hh), P(vv), P(ww), 1, None, 0, C.addressof(n), err, 256) == -3
    assert L.fri_tiled_encode_from_streams_rgba(w, h, tw, th, base, None, n_symbols, P(hh), P(vv), P(ww), 1, P(out), out.size, C.addressof(n), err, 256) == -1
    # the existing encoders keep refusing the flag
    words = np.zeros((4 * 4, 32), np.uint32)
    counts, models, off = np.full(16, 20, np.uint32), np.zeros((16, 10, 4), np.uint32), np.zeros((16, 10, 1024), np.uint16)
    for arg in (3 | A, base):
        assert L.fri_tiled_encode_from_streams(w, h, tw, th, arg, P(st), n_symbols, P(hh), P(vv), P(ww), 1, P(out), out.size, C.addressof(n), err, 256) == -1
        assert L.fri_tiled_encode_from_coded(w, h, tw, th, arg, P(words), 32, P(counts), P(models), P(off), P(vv), P(ww), 1, P(out), out.size, C.addressof(n), err, 256) == -1
        assert L.fri_tiled_encode_from_coded420(w, h, tw, th, arg | emit.S420, P(words), 32, P(counts), P(models), P(off), P(vv), P(ww), 1, P(out), out.size, C.addressof(n), err,
                                                256) == -1
    # the size queries of the decoders: -3 with `info` filled, for every capacity below 4 n F x 512
    frv = emit.tiled_encode_from_streams_rgba(w, h, tw, th, streams, hist, vp, wp, ycbcr=True, quality=50)
    L, data, info, err = _abi(frv)
    F = coefs.shape[1]
    want_info = [w, h, tw, th, 2, 2, base, F]
    buf = np.zeros(coefs.size, np.int32)
    for cap, ptr, rc in [(0, None, -3), (3 * 4 * F * 512, P(buf), -3), (buf.size - 1, P(buf), -3), (buf.size, P(buf), 0)]:
        info[:] = 0
        assert L.fri_tiled_decode(P(data), data.size, 2, P(info), ptr, cap, err, 256) == rc, cap
        assert [int(x) for x in info] == want_info
    assert np.array_equal(buf.reshape(coefs.shape), coefs)
    tiles = np.zeros(4, np.uint32)
    assert L.fri_tiled_decode_region(P(data), data.size, 2, 0, 0, 1, 1, P(info), P(tiles), P(buf), 4 * F * 512 - 1, err, 256) == -3 and list(tiles) == [0, 0, 1, 1]
    assert L.fri_tiled_decode_region(P(data), data.size, 2, 0, 0, 1, 1, P(info), P(tiles), P(buf), 4 * F * 512, err, 256) == 0
    lst = np.array([1, 3], np.uint32)
    assert L.fri_tiled_decode_tiles(P(data), data.size, 2, P(lst), 2, P(info), P(buf), 8 * F * 512 - 1, err, 256) == -3
    assert L.fri_tiled_decode_tiles(P(data), data.size, 2, P(lst), 2, P(info), P(buf), 8 * F * 512, err, 256) == 0


def _repacked(frv, payloads):
    """the container of `frv` around other payloads, the table adjusted"""
    f = parse_frit(frv)
    return container(f["W"], f["H"], f["tile_w"], f["tile_h"], payloads)


def test_malformed_tiled_rgba_files_and_what_stays_refused():
    shape = GRIDS[0]
    w, h, tw, th = shape
    per, files, (streams, hist, vp, wp, coefs) = _inputs("lossless", shape)
    frv = emit.tiled_encode_from_streams_rgba(w, h, tw, th, streams, hist, vp, wp)
    o = parse_frit(frv)["offsets"]

    def decode_rc(data):
        L, d, info, err = _abi(data)
        buf = np.zeros(coefs.size, np.int32)
        return L.fri_tiled_decode(P(d), d.size, 2, P(info), P(buf), buf.size, err, 256), err.value.decode()

    assert decode_rc(frv)[0] == 0
    # one payload swapped for the tile's non-alpha file (the colour channels alone): another metadata word
    rgb_file = emit.encode_image_from_streams(tw, th, *(a[:3] for a in per[1][:4]), empty_ok=True)
    rc, msg = decode_rc(_repacked(frv, [files[0], rgb_file, files[2], files[3]]))
    assert rc == -2 and "Malformed tiled image" in msg
    # ... and with the alpha word patched on: a payload that does not have four channels
    patched = bytearray(rgb_file)
    patched[12:16] = files[1][12:16]
    rc, msg = decode_rc(_repacked(frv, [files[0], bytes(patched), files[2], files[3]]))
    assert rc == -2 and "tile 1" in msg and "Malformed tiled image" in msg
    # ... and an RGB tiled file one of whose payloads has four channels
    plain = [emit.encode_image_from_streams(tw, th, *(a[:3] for a in p[:4]), empty_ok=True) for p in per]
    odd = bytearray(files[2])
    odd[12:16] = plain[2][12:16]
    rc, msg = decode_rc(_repacked(frv, [plain[0], plain[1], bytes(odd), plain[3]]))
    assert rc == -2 and "tile 2" in msg and "Malformed tiled image" in msg
    assert decode_rc(_repacked(frv, plain))[0] == 0  # (an RGB file: three planes per tile, and no alpha)
    assert not emit.tiled_info(_repacked(frv, plain)).alpha
    # bits 2 and 3 together, in every tile
    both = bytearray(frv)
    for t in range(4):
        word = struct.unpack_from("<I", both, o[t] + 12)[0]
        struct.pack_into("<I", both, o[t] + 12, word | 0x4)
    rc, msg = decode_rc(bytes(both))
    assert rc == -2 and "Malformed tiled image" in msg
    L, d, info, err = _abi(bytes(both))
    assert L.fri_tiled_info(P(d), d.size, P(info)) == -2
    # what has no tiled RGBA form: -1, and the message names the kind
    L, d, info, err = _abi(frv)
    buf = np.zeros(coefs.size, np.int32)
    nw = np.zeros(16, np.uint32)
    lst = np.array([0], np.uint32)
    tiles = np.zeros(4, np.uint32)
    out, n = np.zeros(len(frv) + 4096, np.uint8), C.c_size_t(0)
    st, hh, vv, ww = (np.ascontiguousarray(x) for x in (streams, hist, vp, wp))
    calls = {
        "decode_levels": lambda: L.fri_tiled_decode_levels(P(d), d.size, 2, 3, P(info), P(buf), buf.size, err, 256),
        "decode_levels, size query": lambda: L.fri_tiled_decode_levels(P(d), d.size, 2, 9, P(info), None, 0, err, 256),
        "parse_coded": lambda: L.fri_tiled_parse_coded(P(d), d.size, P(info), 16, None, 0, P(nw), None, None, None, None, err, 256),
        "parse_coded, size query": lambda: L.fri_tiled_parse_coded(P(d), d.size, P(info), 0, None, 0, None, None, None, None, None, err, 256),
        "parse_coded_tiles": lambda: L.fri_tiled_parse_coded_tiles(P(d), d.size, P(lst), 1, P(info), 16, None, 0, P(nw), None, None, None, None, err, 256),
        "update": lambda: L.fri_tiled_update_from_streams(P(d), d.size, 0, 0, 1, 1, 3, P(st), st.shape[1], P(hh), P(vv), P(ww), 1, P(tiles), P(out), out.size, C.addressof(n), err, 256),
    }
    for name, call in calls.items():
        err.value = b""
        assert call() == -1 and b"tiled RGBA" in err.value, (name, err.value)
    assert not out.any()
    for call in (lambda: emit.tiled_decode_levels(frv, 3), lambda: emit.tiled_parse_coded(frv)):
        with pytest.raises(emit.EmitError, match="tiled RGBA"):
            call()
    # the flag in the update's channels word stays "invalid argument"
    err.value = b""
    assert L.fri_tiled_update_from_streams(P(d), d.size, 0, 0, 1, 1, 3 | emit.ALPHA, P(st), st.shape[1], P(hh), P(vv), P(ww), 1, P(tiles), P(out), out.size, C.addressof(n), err,
                                           256) == -1 and err.value == b"invalid argument"
    # bit 3 of a Luma tile is ignored, as today
    from tests.common import gen_image
    from tests.tiled_ref import split_tiles

    lw, lh, ltw, lth = 40, 30, 24, 16
    grey = []
    for tile in split_tiles(gen_image("smooth", lw, lh, 1, 5), ltw, lth):
        centers, co, bucket, pred, hi, oob, v, wd = rate_model.oracle_arrays(np.ascontiguousarray(tile).reshape(-1), ltw, lth, 1, 100)
        grey.append((_streams(centers, co, bucket, pred), hi, v, wd, co))
    ls, lhist, lvp, lwp, lcoefs = (np.stack([g[k] for g in grey]) for k in range(5))
    luma = bytearray(emit.tiled_encode_from_streams(lw, lh, ltw, lth, ls, lhist, lvp, lwp))
    for at in parse_frit(bytes(luma))["offsets"][:-1]:
        struct.pack_into("<I", luma, at + 12, struct.unpack_from("<I", luma, at + 12)[0] | 0x8)
    ti, got = emit.tiled_decode(bytes(luma))
    assert not ti.alpha and ti[6] == 1 and np.array_equal(got, lcoefs)


# ---- the host-only plan ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", GRIDS + [(257, 130, 100, 50)], ids=lambda s: "x".join(map(str, s)))
def test_host_only_plan_has_the_grid_the_region_and_two_plans_on_one_lattice(shape):
    w, h, tw, th = shape
    T = PlanTiledRgba(None, w, h, tw, th, TILED_ALLOW_HOLES)
    nx, ny = grid(w, h, tw, th)
    assert T.grid() == (nx, ny, tw, th) and T.n_tiles == nx * ny
    for view, c in ((T.colour, 3), (T.alpha, 1)):
        ref = fa.Plan(None, tw, th, c)
        assert (view.width, view.height, view.channels) == (tw, th, c) and view.num_cells == ref.num_cells and view.num_some == ref.num_some
        assert np.array_equal(view.centers(), ref.centers())
        ref.close()
    assert T.num_cells == T.alpha.num_cells and T.num_some == T.alpha.num_some
    assert (T.pixel_bytes, T.colour_tile_bytes, T.alpha_tile_bytes) == (4 * w * h, 3 * nx * ny * tw * th, nx * ny * tw * th)
    assert T.coef_count == 4 * nx * ny * T.num_cells * 512 and T.num_symbols == 4 * nx * ny * T.num_some and T.buffer_tiles() == (0, 0)
    for region in [(0, 0, 1, 1), (w - 1, h - 1, 1, 1), (0, 0, w, h), (tw - 1, th - 1, 2, 2)]:
        assert T.region(*region) == emit.tiled_region_tiles(w, h, tw, th, *region)
    for bad in [(0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (2**32 - 1, 0, 2, 1)]:
        with pytest.raises(fa.FriHipError) as e:
            T.region(*bad)
        assert e.value.code == -1, bad
    # compute calls: no device
    px = np.zeros((h, w, 4), np.uint8)
    calls = [lambda: T.split_tiles_rgba_dev(16, 16, 16), lambda: T.split_tiles_rgba_dev(16, 16, 16, clean=api.ALPHA_CLEAN), lambda: T.merge_tiles_rgba_dev(16, 16, 16),
             lambda: T.merge_tiles_rgba_region_dev(16, 16, 0, 0, 1, 1, 16), lambda: T.encode_symbols_tiled_rgba_dev(16, 16, 16, 16, 16),
             lambda: T.decode_region_tiled_rgba_dev(16, 0, 0, 1, 1, 16), lambda: T.encode_image_tiled_rgba_symbols(px),
             lambda: T.decode_image_tiled_rgba(np.zeros(T.coef_count, np.int32)), lambda: T.decode_region_tiled_rgba(np.zeros(T.tile_coef_count, np.int32), 0, 0, 1, 1)]
    for k, call in enumerate(calls):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -3, k
    T.close()


def test_plan_create_refusals_and_null_arguments():
    L = api.load_library()
    hd = C.c_void_p()
    for args in ((0, 10, 4, 4, 0), (10, 0, 4, 4, 0), (10, 10, 0, 4, 0), (10, 10, 4, 0, 0), (10, 10, 4, 4, 2)):
        assert L.fri_hip_plan_tiled_rgba_create(None, *args, C.byref(hd)) == -1, args
    assert L.fri_hip_plan_tiled_rgba_create(None, 10, 10, 4, 4, 0, None) == -1
    # 3 nx ny planes in one batch launch: 148 x 148 tiles of one pixel are 65712 colour planes, 147 x 148 are 65268
    assert L.fri_hip_plan_tiled_rgba_create(None, 148, 148, 1, 1, 1, C.byref(hd)) == -1
    assert L.fri_hip_plan_tiled_rgba_create(None, 147, 148, 1, 1, 1, C.byref(hd)) == 0 and L.fri_hip_plan_tiled_rgba_destroy(hd) == 0
    # a tile shape whose lattice leaves pixels to no cell needs the flag (64 x 64: 8 of them)
    with pytest.raises(fa.FriHipError) as e:
        PlanTiledRgba(None, 128, 128, 64, 64)
    assert e.value.code == -1
    PlanTiledRgba(None, 128, 128, 64, 64, TILED_ALLOW_HOLES).close()
    tw, th = api.tile_shape(334, 350, 150)  # fri_hip_tile_shape is the tile-shape rule: the lattice is the same
    assert (tw, th) == (167, 175)
    PlanTiledRgba(None, 334, 350, tw, th).close()
    assert L.fri_hip_plan_tiled_rgba_destroy(None) == 0 and L.fri_hip_plan_tiled_rgba_colour(None) is None and L.fri_hip_plan_tiled_rgba_alpha(None) is None
    out = np.zeros(4, np.uint32)
    assert L.fri_hip_plan_tiled_rgba_grid(None, P(out)) == -1 and L.fri_hip_plan_tiled_rgba_region(None, 0, 0, 1, 1, P(out)) == -1
    assert L.fri_hip_split_tiles_rgba_dev(None, 16, 0, 16, 16, None) == -1 and L.fri_hip_merge_tiles_rgba_dev(None, 16, 16, 16, None) == -1
    assert L.fri_hip_merge_tiles_rgba_region_dev(None, 16, 16, 0, 0, 1, 1, 16, None) == -1


# ---- under the sanitizers ------------------------------------------------------------------------------------------------------------------------------------

def test_tiled_rgba_round_trip_under_the_sanitizers(tmp_path):
    """A stand-alone program with its own main: nothing loaded into python is run under a sanitizer."""
    exe = tmp_path / "tiled_rgba_host_check"
    host, csrc = os.path.join(ROOT, "frave_amd", "host"), os.path.join(ROOT, "frave_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "include"), "-I", host, "-I", csrc, "-o", str(exe), os.path.join(ROOT, "tests", "tools", "tiled_rgba_host_check.cpp"),
                           os.path.join(host, "emit.cpp"), os.path.join(host, "emit_abi.cpp"), os.path.join(csrc, "geometry.cpp")])
    shape = GRIDS[1]
    w, h, tw, th = shape
    per, files, (streams, hist, vp, wp, coefs) = _inputs("rct", shape)
    (tmp_path / "want.frv").write_bytes(container(w, h, tw, th, files))
    with open(tmp_path / "arrays.bin", "wb") as f:
        f.write(struct.pack("<7I", w, h, tw, th, 3 | emit.ALPHA | emit.RCT, streams.shape[1], coefs.shape[1]))
        f.write(streams.astype("<u2").tobytes() + hist.astype("<u4").tobytes() + vp.astype("<f4").tobytes() + wp.astype("<f4").tobytes() + coefs.astype("<i4").tobytes())
    out = subprocess.run([str(exe), str(tmp_path / "arrays.bin"), str(tmp_path / "want.frv")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
