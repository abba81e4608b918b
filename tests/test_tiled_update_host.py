"""Region update, host side (include/fri_emit.h "Region update"; fri_tiled_update_from_streams, fri_hip_plan_tiled_region_cover): the update against a Python
splice of two `frit` files by their tables, against the whole encode, and decoded; the refusals and return codes; the covered rectangle and the host-only plan;
and a stand-alone program under the sanitizers. Streams come from the CPU oracle, per tile. CPU only."""
import ctypes as C
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd.api import TILED_ALLOW_HOLES, PlanTiled
from tests import rate_model
from tests.coded_cases import tiled420_file, tiled_file
from tests.test_gpu_tiled_region import SHAPES, kernel_regions
from tests.test_tiled_region_host import CASES
from tests.tiled_ref import grid, mixed_image, parse_frit, split_tiles
from tests.tiled_region_ref import region_tiles, sub_grid
from tests.tiled_update_ref import region_cover, splice, split_region, split_region_fast, sub_tiles

tiled_update_from_streams = emit.tiled_update_from_streams  # (without the feature the module fails here ...
plan_region_cover = PlanTiled.region_cover  # ... or here)

P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_A, SEED_B = 3, 11
# name -> (case (W, H, C, tile_w, tile_h), the oracle's quality (100: lossless), emitter flags): 3 x 3 tiles, so that an interior tile exists, and a 2 x 2 file
MODES = {
    "lossless C = 1": (CASES[0], 100, {}),
    "quality C = 3": (CASES[1], 45, dict(quality=45)),
    "ycbcr + quality": (CASES[1], 45, dict(ycbcr=True, quality=45)),
    "rct": (CASES[1], 100, dict(rct=True)),
    "2 x 2, lossless C = 1": ((100, 70, 1, 52, 50), 100, {}),
    "2 x 2, quality C = 3": ((100, 70, 3, 52, 50), 40, dict(quality=40)),
}


def update_regions(case):
    """a one-pixel region in each corner, a region crossing a tile boundary (in both directions, off every tile corner), and the whole image"""
    w, h, c, tw, th = case
    return {
        "one pixel top left": (0, 0, 1, 1),
        "one pixel top right": (w - 1, 0, 1, 1),
        "one pixel bottom left": (0, h - 1, 1, 1),
        "one pixel bottom right": (w - 1, h - 1, 1, 1),
        "across a tile boundary": (tw - 3, th - 2, 7, 5),
        "whole image": (0, 0, w, h),
    }


@functools.lru_cache(maxsize=None)
def _tiles_of(case, quality, seed):
    """per tile of mixed_image(seed), from the oracle at `quality`: (streams [n][C][n_symbols], hist [n][C][10][1024], vp, wp [n][C][3][6], coefs [n][C][F][512])"""
    w, h, c, tw, th = case
    per = []
    for tile in split_tiles(mixed_image(w, h, c, tw, seed), tw, th):
        centers, coefs, bucket, pred, hist, oob, vp, wp = rate_model.oracle_arrays(np.ascontiguousarray(tile).reshape(-1), tw, th, c, quality)
        assert not oob.any()
        streams = []
        for ch in range(c):
            sym, bk = emit.channel_symbols(centers, coefs[ch], bucket[ch], pred[ch])
            streams.append((bk.astype(np.uint16) << 10) | sym)
        per.append((np.stack(streams), hist, vp, wp, coefs))
    out = tuple(np.stack([p[k] for p in per]) for k in range(5))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _whole_file(case, quality, seed, flags):
    w, h, c, tw, th = case
    st, hist, vp, wp, _ = _tiles_of(case, quality, seed)
    return emit.tiled_encode_from_streams(w, h, tw, th, st, hist, vp, wp, **dict(flags))


def _setup(mode):
    case, quality, flags = MODES[mode]
    key = tuple(sorted(flags.items()))
    return case, flags, _tiles_of(case, quality, SEED_A), _tiles_of(case, quality, SEED_B), _whole_file(case, quality, SEED_A, key), _whole_file(case, quality, SEED_B, key)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------

def test_region_split_is_the_sub_grids_rows_of_the_split_and_reads_only_the_covered_rectangle():
    for shape in SHAPES[:5]:
        w, h, c, tw, th = shape
        nx, ny = grid(w, h, tw, th)
        img = np.random.default_rng([w, h, c]).integers(0, 256, (h, w, c), dtype=np.uint8)
        whole = split_tiles(img, tw, th)
        for name, region in kernel_regions(shape).items():
            i0, j0, ni, nj = region_tiles(w, h, tw, th, *region)
            want = sub_grid(whole, nx, i0, j0, ni, nj)
            assert np.array_equal(split_region(img, tw, th, *region), want), (shape, name)
            assert np.array_equal(split_region_fast(img, tw, th, *region), want), (shape, name)
            cx, cy, cw, ch = region_cover(w, h, tw, th, *region)
            other = np.bitwise_not(img)  # every pixel outside the covered rectangle changed: the sub-grid's tiles stay what they are
            other[cy:cy + ch, cx:cx + cw] = img[cy:cy + ch, cx:cx + cw]
            assert np.array_equal(split_region(other, tw, th, *region), want), (shape, name)
    assert region_cover(100, 70, 52, 50, 99, 69, 1, 1) == (52, 50, 48, 20) and region_cover(100, 70, 52, 50, 51, 49, 2, 2) == (0, 0, 100, 70)
    assert region_cover(100, 70, 52, 50, 0, 0, 1, 1) == (0, 0, 52, 50) and region_cover(100, 70, 52, 50, 99, 0, 2, 1) is None


# ---- the update ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(MODES))
def test_update_is_the_splice_the_whole_encode_and_decodes(mode):
    case, flags, A, B, file_a, file_b = _setup(mode)
    w, h, c, tw, th = case
    nx, ny = grid(w, h, tw, th)
    img_a, img_b = mixed_image(w, h, c, tw, SEED_A), mixed_image(w, h, c, tw, SEED_B)
    assert file_a != file_b
    for name, region in update_regions(case).items():
        tiles = region_tiles(w, h, tw, th, *region)
        touched = sub_tiles(nx, *tiles)
        sub = [np.ascontiguousarray(B[k][touched]) for k in range(4)]  # B's streams, histograms and parameters, in the sub-grid's order
        want = splice(file_a, file_b, *region)
        for threads in (1, 4):  # the same bytes for every thread count
            got, got_tiles = tiled_update_from_streams(file_a, *region, *sub, threads=threads, **flags)
            assert got_tiles == tiles and got == want, (mode, name, threads)  # any A and B: the splice of the two whole files
        parse_frit(got)
        # an image that differs from A only inside the covered rectangle: its tiles are B's inside the sub-grid and A's outside it, and its whole file ...
        cx, cy, cw, ch = region_cover(w, h, tw, th, *region)
        patched = img_a.copy()
        patched[cy:cy + ch, cx:cx + cw] = img_b[cy:cy + ch, cx:cx + cw]
        pt, at, bt = split_tiles(patched, tw, th), split_tiles(img_a, tw, th), split_tiles(img_b, tw, th)
        assert all(np.array_equal(pt[t], bt[t] if t in touched else at[t]) for t in range(nx * ny))
        mixed = [np.stack([(B if t in touched else A)[k][t] for t in range(nx * ny)]) for k in range(4)]
        whole_of_patched = emit.tiled_encode_from_streams(w, h, tw, th, *mixed, **flags)
        assert got == whole_of_patched, (mode, name)  # ... is the updated file, byte for byte
        if name == "whole image":
            assert len(touched) == nx * ny and got == file_b
        else:
            assert len(touched) == 1 or name == "across a tile boundary" and len(touched) == 4
        # the updated file decodes to the planes of B's tiles inside the sub-grid and of A's tiles outside it
        ti, coefs = emit.tiled_decode(got)
        assert tuple(ti[:7]) == (w, h, tw, th, nx, ny, c)
        for t in range(nx * ny):
            assert np.array_equal(coefs[t], (B if t in touched else A)[4][t]), (mode, name, t)


def _update_rc(frv, region, arrays, channels_word, n_symbols=None, cap=None, threads=2):
    """(rc, message, tiles, out_len, bytes) of fri_tiled_update_from_streams through the C ABI into a buffer of `cap` bytes (None: plenty, 0: NULL)"""
    data = np.frombuffer(bytes(frv), np.uint8)
    st, hist, vp, wp = (np.ascontiguousarray(a) for a in arrays)
    tiles = np.full(4, 77, np.uint32)
    n = C.c_size_t(12345)
    err = C.create_string_buffer(256)
    buf = np.zeros(data.size + st.size * 4 + 4096 if cap is None else max(cap, 1), np.uint8)
    rc = emit.load_library().fri_tiled_update_from_streams(P(data), data.size, *region, channels_word, P(st), st.shape[-1] if n_symbols is None else n_symbols, P(hist), P(vp), P(wp),
                                                           threads, P(tiles), P(buf) if cap != 0 else None, buf.size if cap is None else cap, C.addressof(n), err, 256)
    return rc, err.value.decode(), [int(v) for v in tiles], n.value, buf


def test_refusals_and_return_codes():
    case, flags, A, B, file_a, file_b = _setup("2 x 2, lossless C = 1")
    w, h, c, tw, th = case
    assert file_a == tiled_file(w, h, c, tw, th, 100)[0]  # the file of tests/coded_cases.py
    region = (60, 10, 5, 5)  # tile 1
    assert region_tiles(w, h, tw, th, *region) == (1, 0, 1, 1)
    sub = [np.ascontiguousarray(B[k][[1]]) for k in range(4)]
    want = splice(file_a, file_b, *region)
    # the size query and a buffer one byte short: -3 with the exact size and `tiles` filled; the exact buffer: 0
    for cap, rc in [(0, -3), (len(want) - 1, -3), (len(want), 0)]:
        got_rc, msg, tiles, n, buf = _update_rc(file_a, region, sub, 1, cap=cap)
        assert got_rc == rc and tiles == [1, 0, 1, 1] and n == len(want), (cap, msg)
    assert buf[:n].tobytes() == want
    # a region fri_tiled_region_tiles refuses: -1, "invalid region", nothing written
    for bad in [(0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (0, 1, 1, h), (2**32 - 1, 0, 2, 1)]:
        rc, msg, tiles, n, buf = _update_rc(file_a, bad, sub, 1)
        assert rc == -1 and "invalid region" in msg and tiles == [77] * 4 and n == 12345 and not buf.any(), bad
        with pytest.raises(emit.EmitError) as e:
            tiled_update_from_streams(file_a, *bad, *sub)
        assert e.value.code == -1
    # FRI_EMIT_420 / FRI_EMIT_ALPHA in the channels word: -1
    for word in (3 | emit.YCBCR | emit.S420 | emit.QUALITY(50), 3 | emit.ALPHA, 1 | emit.S420, 1 | emit.ALPHA):
        assert _update_rc(file_a, region, sub, word)[0] == -1, hex(word)
    with pytest.raises(emit.EmitError) as e:
        tiled_update_from_streams(file_a, *region, *sub, flags=emit.ALPHA)
    assert e.value.code == -1
    # a tiled 4:2:0 file: -1, and the message says what to do
    frv420 = tiled420_file(100, 70, 52, 50, 50)[0]
    rc, msg, *_ = _update_rc(frv420, region, [np.ascontiguousarray(np.repeat(a, 3, axis=1)) for a in sub], 3 | emit.YCBCR | emit.QUALITY(50))
    assert rc == -1 and "4:2:0" in msg and "re-encoded whole" in msg
    # not a well-formed `frit` file (a `frif` file among them), a wrong n_symbols, a metadata word that is not tile 0's: -2
    o = parse_frit(file_a)["offsets"]
    for bad in (parse_frit(file_a)["payloads"][0], file_a[:-1], b"frit", file_a[:4] + struct.pack("<I", 2) + file_a[8:]):
        rc, msg, *_ = _update_rc(bad, region, sub, 1)
        assert rc == -2 and "Malformed tiled image" in msg
    rc, msg, *_ = _update_rc(file_a, region, sub, 1, n_symbols=sub[0].shape[-1] - 1)
    assert rc == -2 and "n_symbols" in msg
    for word in (1 | emit.QUALITY(50), 3, 3 | emit.RCT):  # another quality; another channel count (whose arrays would be larger: refused before they are read)
        rc, msg, tiles, n, buf = _update_rc(file_a, region, sub, word)
        assert rc == -2 and "metadata" in msg and n == 12345 and not buf.any(), hex(word)
    # the flag is always in force and may be passed
    assert _update_rc(file_a, region, sub, 1 | emit.EMPTY_OK)[0] == 0
    # a NULL pointer: -1
    L = emit.load_library()
    data = np.frombuffer(file_a, np.uint8)
    tiles, n = np.zeros(4, np.uint32), C.c_size_t(0)
    good = [P(data), data.size, *region, 1, P(sub[0]), sub[0].shape[-1], P(sub[1]), P(sub[2]), P(sub[3]), 1, P(tiles), None, 0, C.addressof(n), None, 0]
    assert L.fri_tiled_update_from_streams(*good) == -3
    for k in (0, 7, 9, 10, 11, 13, 16):
        args = list(good)
        args[k] = None
        assert L.fri_tiled_update_from_streams(*args) == -1, k
    # the Python wrapper refuses arrays that do not hold the region's tiles
    with pytest.raises(emit.EmitError):
        tiled_update_from_streams(file_a, 0, 0, w, h, *sub)


def test_damage_in_an_untouched_body_is_copied_and_a_damaged_header_is_refused():
    case, flags, A, B, file_a, file_b = _setup("lossless C = 1")
    w, h, c, tw, th = case
    region = (tw, th, tw, th)  # the centre tile, tile 4
    sub = [np.ascontiguousarray(B[k][[4]]) for k in range(4)]
    o = parse_frit(file_a)["offsets"]
    b = bytearray(file_a)
    for tile in (0, 3, 5, 8):  # the middle of the coded data, and the end marker
        b[(o[tile] + o[tile + 1]) // 2] ^= 0xFF
        b[o[tile + 1] - 1] ^= 0xFF
    damaged = bytes(b)
    with pytest.raises(emit.EmitError):
        emit.tiled_decode(damaged)
    got, tiles = tiled_update_from_streams(damaged, *region, *sub)
    want = bytearray(splice(file_a, file_b, *region))
    shift = len(parse_frit(file_b)["payloads"][4]) - (o[5] - o[4])
    for tile in (0, 3, 5, 8):  # the same bytes damaged in the splice: after tile 4 they have moved by the change of its length
        d = shift if tile > 4 else 0
        want[(o[tile] + o[tile + 1]) // 2 + d] ^= 0xFF
        want[o[tile + 1] - 1 + d] ^= 0xFF
    assert tiles == (1, 1, 1, 1) and got == bytes(want)
    # damage inside the touched payload is replaced with it
    b = bytearray(file_a)
    b[(o[4] + o[5]) // 2] ^= 0xFF
    assert tiled_update_from_streams(bytes(b), *region, *sub)[0] == splice(file_a, file_b, *region)
    # a damaged 16-byte header anywhere - of a touched or an untouched payload - is -2
    for tile in range(9):
        for at in (0, 5, 9, 13):
            b = bytearray(file_a)
            b[o[tile] + at] ^= 0x01
            rc, msg, *_ = _update_rc(bytes(b), region, sub, 1)
            assert rc == -2, (tile, at, msg)
            assert "Malformed tiled image" in msg or (tile == 0 and at == 13 and "metadata" in msg), (tile, at, msg)


# ---- the host-only tiled plan ----------------------------------------------------------------------------------------------------------------------------

def test_host_only_plan_gives_the_covered_rectangle_and_refuses_compute():
    for shape in SHAPES:
        w, h, c, tw, th = shape
        p = PlanTiled(None, w, h, c, tw, th, TILED_ALLOW_HOLES)
        for name, region in kernel_regions(shape).items():
            assert p.region_cover(*region) == region_cover(w, h, tw, th, *region), (shape, name)
        cx, cy, cw, ch = p.region_cover(0, 0, w, h)
        assert (cx, cy, cw, ch) == (0, 0, w, h)
        for bad in [(0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (2**32 - 1, 0, 2, 1)]:
            with pytest.raises(fa.FriHipError) as e:
                p.region_cover(*bad)
            assert e.value.code == -1
        p.close()
    w, h, c, tw, th = CASES[1]
    p = PlanTiled(None, w, h, c, tw, th)
    assert fa.load_library().fri_hip_plan_tiled_region_cover(p._h, 0, 0, 1, 1, None) == -1
    whole = (w * c, 0, 0, w, h)  # the whole raster as the source: pitch, origin, size
    img = np.zeros((h, w, c), np.uint8)
    # the compute entry points: -3 on a host-only plan ...
    for call in (lambda: p.split_tiles_region_dev(16, *whole, 0, 0, 8, 8, 32), lambda: p.encode_symbols_region_tiled_dev(16, *whole, 0, 0, 8, 8, 16, 16, 16, 16),
                 lambda: p.encode_region_tiled_symbols(img, 0, 0, 8, 8)):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -3
    # ... and -1 for bad arguments, before the device is asked for: a NULL pointer, a bad region, a source rectangle that does not contain the covered rectangle
    # or leaves the image, a pitch shorter than a row of the source
    cx, cy, cw, ch = p.region_cover(tw + 1, th + 1, 2, 2)  # the centre tile
    assert (cx, cy, cw, ch) == (tw, th, tw, th)
    bad_calls = [
        lambda: p.split_tiles_region_dev(0, *whole, 0, 0, 8, 8, 32),
        lambda: p.split_tiles_region_dev(16, *whole, 0, 0, 8, 8, 0),
        lambda: p.split_tiles_region_dev(16, *whole, w - 1, 0, 2, 1, 32),
        lambda: p.split_tiles_region_dev(16, *whole, 0, 0, 0, 1, 32),
        lambda: p.split_tiles_region_dev(16, w * c - 1, 0, 0, w, h, 0, 0, 8, 8, 32),                  # the pitch
        lambda: p.split_tiles_region_dev(16, cw * c, cx + 1, cy, cw - 1, ch, tw + 1, th + 1, 2, 2, 32),  # starts one column late
        lambda: p.split_tiles_region_dev(16, cw * c, cx, cy + 1, cw, ch - 1, tw + 1, th + 1, 2, 2, 32),  # ... one row late
        lambda: p.split_tiles_region_dev(16, cw * c, cx, cy, cw - 1, ch, tw + 1, th + 1, 2, 2, 32),      # ends one column early
        lambda: p.split_tiles_region_dev(16, cw * c, cx, cy, cw, ch - 1, tw + 1, th + 1, 2, 2, 32),      # ... one row early
        lambda: p.split_tiles_region_dev(16, (w + 1) * c, 0, 0, w + 1, h, 0, 0, 8, 8, 32),             # leaves the image
        lambda: p.split_tiles_region_dev(16, w * c, 0, 1, w, h, 0, th, 8, 8, 32),
        lambda: p.split_tiles_region_dev(16, w * c, 0, 0, 0, h, 0, 0, 8, 8, 32),
        lambda: p.encode_symbols_region_tiled_dev(0, *whole, 0, 0, 8, 8, 16, 16, 16, 16),
        lambda: p.encode_symbols_region_tiled_dev(16, *whole, 0, 0, 8, 8, 0, 16, 16, 16),
        lambda: p.encode_symbols_region_tiled_dev(16, *whole, 0, 0, 8, 8, 16, 0, 16, 16),
        lambda: p.encode_symbols_region_tiled_dev(16, *whole, 0, 0, 8, 8, 16, 16, 0, 16),
        lambda: p.encode_symbols_region_tiled_dev(16, *whole, 0, 0, 8, 8, 16, 16, 16, 0),
        lambda: p.encode_symbols_region_tiled_dev(16, *whole, 0, h, 1, 1, 16, 16, 16, 16),
        lambda: p.encode_symbols_region_tiled_dev(16, cw * c, cx, cy, cw - 1, ch, tw + 1, th + 1, 2, 2, 16, 16, 16, 16),
        lambda: p.encode_region_tiled_symbols(img, 0, 0, w + 1, 1),
        lambda: p.encode_region_tiled_symbols(img, 0, 0, 0, 1),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -1, k
    # the staged covered rectangle and any rectangle around it are good sources: only the missing device is in the way
    for src in [(cw * c, cx, cy, cw, ch), (cw * c + 5, cx, cy, cw, ch), ((cw + 3) * c, cx - 2, cy - 1, cw + 3, ch + 2)]:
        with pytest.raises(fa.FriHipError) as e:
            p.split_tiles_region_dev(16, *src, tw + 1, th + 1, 2, 2, 32)
        assert e.value.code == -3, src
    p.close()


# ---- a stand-alone program under the sanitizers --------------------------------------------------------------------------------------------------------------

def test_update_under_the_sanitizers(tmp_path):
    """A stand-alone program with its own main: nothing loaded into python is run under a sanitizer."""
    exe = tmp_path / "tiled_update_host_check"
    host, csrc = os.path.join(ROOT, "frave_amd", "host"), os.path.join(ROOT, "frave_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "include"), "-I", host, "-I", csrc, "-o", str(exe), os.path.join(ROOT, "tests", "tools", "tiled_update_host_check.cpp"),
                           os.path.join(host, "emit.cpp"), os.path.join(host, "emit_abi.cpp"), os.path.join(csrc, "geometry.cpp")])
    case, flags, A, B, file_a, file_b = _setup("2 x 2, lossless C = 1")
    w, h, c, tw, th = case
    region = (60, 0, 8, 70)  # the right column: tiles 1 and 3
    touched = sub_tiles(2, *region_tiles(w, h, tw, th, *region))
    assert touched == [1, 3]
    sub = [np.ascontiguousarray(B[k][touched]) for k in range(4)]
    (tmp_path / "in.frv").write_bytes(file_a)
    (tmp_path / "want.frv").write_bytes(splice(file_a, file_b, *region))
    with open(tmp_path / "arrays.bin", "wb") as f:
        f.write(struct.pack("<7IQ", *region, 1, len(touched), c, sub[0].shape[-1]))
        f.write(sub[0].astype("<u2").tobytes() + sub[1].astype("<u4").tobytes() + sub[2].astype("<f4").tobytes() + sub[3].astype("<f4").tobytes())
    out = subprocess.run([str(exe), str(tmp_path / "in.frv"), str(tmp_path / "arrays.bin"), str(tmp_path / "want.frv")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
