"""Region decode, host side (include/fri_emit.h "Region decode"; fri_tiled_region_tiles, fri_tiled_decode_region, fri_hip_plan_tiled_region): the tile-range
arithmetic against tests/tiled_region_ref.py, the region decode against fri_tiled_decode on 3 x 3 grids - a region can then have untouched tiles on every side -
damage inside and outside the touched tiles, malformed files, and the host-only tiled plan. CPU only."""
import ctypes as C
import struct

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd.api import TILED_ALLOW_HOLES, PlanTiled
from tests.test_tiled_host import _inputs, _tile_arrays
from tests.common import gen_image
from tests.tiled_ref import grid, parse_frit
from tests.tiled_region_ref import region_tiles, sub_grid

tiled_decode_region, tiled_region_tiles = emit.tiled_decode_region, emit.tiled_region_tiles  # (without the feature the module fails here ...
plan_region_tiles = PlanTiled.region_tiles  # ... or here)

P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
CASES = [(375, 375, 1, 125, 125), (450, 330, 3, 167, 117)]  # (W, H, C, tile_w, tile_h): 3 x 3 tiles; the second's last column and row are partial


def regions(case):
    w, h, c, tw, th = case
    return {
        "centre tile": (tw, th, tw, th),
        "one pixel in a corner tile": (w - 1, h - 1, 1, 1),
        "across all nine": (tw - 3, th - 2, tw + 7, th + 5),
        "last partial column": (2 * tw, 0, w - 2 * tw, h),
        "whole image": (0, 0, w, h),
    }


def frit_of(case, **kwargs):
    w, h, c, tw, th = case
    streams, hist, vp, wp, coefs = _inputs(case)
    return emit.tiled_encode_from_streams(w, h, tw, th, streams, hist, vp, wp, **kwargs)


def _region_rc(data, region, cap=None, threads=2):
    """(rc, message, info, tiles, coefs) of fri_tiled_decode_region through the C ABI, into a buffer of `cap` elements (None: plenty)"""
    data = np.frombuffer(bytes(data), np.uint8)
    info, tiles = np.zeros(8, np.uint32), np.zeros(4, np.uint32)
    err = C.create_string_buffer(256)
    buf = np.zeros(1 << 22 if cap is None else max(cap, 1), np.int32)
    rc = emit.load_library().fri_tiled_decode_region(P(data), data.size, threads, *region, P(info), P(tiles), P(buf) if cap != 0 else None, buf.size if cap is None else cap, err, 256)
    return rc, err.value.decode(), [int(v) for v in info], [int(v) for v in tiles], buf


# ---- the arithmetic --------------------------------------------------------------------------------------------------------------------------------------

def test_tile_range_of_every_region_of_a_small_image():
    w, h, tw, th = 7, 5, 3, 2
    plan = PlanTiled(None, w, h, 1, tw, th, TILED_ALLOW_HOLES)
    L = emit.load_library()
    out = np.zeros(4, np.uint32)
    valid = 0
    for x in range(w + 1):
        for y in range(h + 1):
            for rw in range(w + 2):
                for rh in range(h + 2):
                    want = region_tiles(w, h, tw, th, x, y, rw, rh)
                    if want is None:  # a zero size, or the region leaves the image
                        assert L.fri_tiled_region_tiles(w, h, tw, th, x, y, rw, rh, P(out)) == -1, (x, y, rw, rh)
                        with pytest.raises(fa.FriHipError) as e:
                            plan.region_tiles(x, y, rw, rh)
                        assert e.value.code == -1
                        continue
                    valid += 1
                    assert tiled_region_tiles(w, h, tw, th, x, y, rw, rh) == plan.region_tiles(x, y, rw, rh) == want, (x, y, rw, rh)
    assert valid == (w * (w + 1) // 2) * (h * (h + 1) // 2)  # every valid region was tried: x + w = W and w = 1 among them
    assert tiled_region_tiles(w, h, tw, th, 6, 4, 1, 1) == (2, 2, 1, 1) and tiled_region_tiles(w, h, tw, th, 2, 1, 2, 2) == (0, 0, 2, 2)
    plan.close()


def test_tile_range_near_two_to_the_32_and_zero_sizes():
    big = 2**32 - 1
    tw, th = 65536, 4096
    for x, y, rw, rh in [(0, 0, big, big), (big - 1, big - 1, 1, 1), (big - 5, 7, 5, 2**31), (65535, 4095, 2, 2), (2**31, 2**31, 2**31 - 1, 2**31 - 1)]:
        assert tiled_region_tiles(big, big, tw, th, x, y, rw, rh) == region_tiles(big, big, tw, th, x, y, rw, rh), (x, y, rw, rh)
    assert tiled_region_tiles(big, big, tw, th, 0, 0, big, big) == (0, 0, 65536, 2**20)
    L = emit.load_library()
    out = np.zeros(4, np.uint32)
    # x + w = 2^32 wraps to 0 in 32 bits: compared in 64 it leaves the image
    for x, y, rw, rh in [(1, 0, big, 1), (0, 1, 1, big), (big, 0, 1, 1), (0, big, 1, 1), (2**31, 0, 2**31, 1), (big, big, big, big)]:
        assert L.fri_tiled_region_tiles(big, big, tw, th, x, y, rw, rh, P(out)) == -1, (x, y, rw, rh)
    for args in [(0, 5, 3, 2, 0, 0, 1, 1), (7, 0, 3, 2, 0, 0, 1, 1), (7, 5, 0, 2, 0, 0, 1, 1), (7, 5, 3, 0, 0, 0, 1, 1), (7, 5, 3, 2, 0, 0, 0, 1), (7, 5, 3, 2, 0, 0, 1, 0)]:
        assert L.fri_tiled_region_tiles(*args, P(out)) == -1, args
    assert L.fri_tiled_region_tiles(7, 5, 3, 2, 0, 0, 1, 1, None) == -1
    with pytest.raises(emit.EmitError):
        tiled_region_tiles(7, 5, 3, 2, 6, 0, 2, 1)


# ---- the decode ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda s: "x".join(map(str, s)))
def test_region_decode_gives_the_touched_tiles_of_the_whole_decode(case):
    w, h, c, tw, th = case
    nx, ny = grid(w, h, tw, th)
    assert (nx, ny) == (3, 3)
    frv = frit_of(case)
    whole_info, whole = emit.tiled_decode(frv, 2)
    assert np.array_equal(whole, _inputs(case)[4])
    F = whole.shape[2]
    for name, region in regions(case).items():
        want_range = region_tiles(w, h, tw, th, *region)
        i0, j0, ni, nj = want_range
        want = sub_grid(whole, nx, i0, j0, ni, nj)
        for threads in (1, 4):  # the same bytes for every thread count
            info, tiles, got = tiled_decode_region(frv, *region, threads=threads)
            assert tuple(info) == tuple(whole_info) and tiles == want_range, name
            assert got.shape == want.shape == (ni * nj, c, F, 512) and np.array_equal(got, want), (name, threads)
        # the size query and a buffer one element short: -3 with info and tiles filled; the exact buffer: 0
        for cap, rc in [(0, -3), (want.size - 1, -3), (want.size, 0)]:
            got_rc, msg, got_info, got_tiles, buf = _region_rc(frv, region, cap)
            assert got_rc == rc and got_info == [w, h, tw, th, nx, ny, c, F] and got_tiles == list(want_range), (name, cap, msg)
        assert np.array_equal(buf[: want.size].reshape(want.shape), want)
    # the touched tiles really are a subset: the centre tile is 1 tile, the corner pixel 1, the rectangle 9, the last column 3
    assert [region_tiles(w, h, tw, th, *r)[2:] for r in regions(case).values()] == [(1, 1), (1, 1), (3, 3), (1, 3), (3, 3)]
    # the whole-image region returns what fri_tiled_decode returns
    info, tiles, got = tiled_decode_region(frv, 0, 0, w, h)
    assert tiles == (0, 0, 3, 3) and np.array_equal(got, whole)


def test_bad_regions_and_null_pointers_are_refused():
    case = CASES[0]
    w, h, c, tw, th = case
    frv = frit_of(case)
    for region in [(0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (0, 1, 1, h), (2**32 - 1, 0, 2, 1)]:
        rc, msg, info, tiles, _ = _region_rc(frv, region)
        assert rc == -1 and "invalid region" in msg, region
        with pytest.raises(emit.EmitError):
            tiled_decode_region(frv, *region)
    L = emit.load_library()
    data = np.frombuffer(frv, np.uint8)
    info, tiles = np.zeros(8, np.uint32), np.zeros(4, np.uint32)
    assert L.fri_tiled_decode_region(None, data.size, 1, 0, 0, 1, 1, P(info), P(tiles), None, 0, None, 0) == -1
    assert L.fri_tiled_decode_region(P(data), data.size, 1, 0, 0, 1, 1, None, P(tiles), None, 0, None, 0) == -1
    assert L.fri_tiled_decode_region(P(data), data.size, 1, 0, 0, 1, 1, P(info), None, None, 0, None, 0) == -1


@pytest.mark.parametrize("case", CASES, ids=lambda s: "x".join(map(str, s)))
def test_damage_outside_the_region_is_not_looked_at_and_damage_inside_names_the_files_tile(case):
    w, h, c, tw, th = case
    frv = frit_of(case)
    o = parse_frit(frv)["offsets"]
    centre = regions(case)["centre tile"]
    _, _, want = tiled_decode_region(frv, *centre)

    def flipped(tile, back):  # a byte inside the body of a payload, `back` bytes before its end
        b = bytearray(frv)
        b[o[tile + 1] - back] ^= 0xFF
        return bytes(b)

    # the last bytes of a payload are its end marker: fri_tiled_decode refuses the file when any tile's is damaged ...
    for tile in (0, 2, 3, 5, 8):
        bad = flipped(tile, 1)
        with pytest.raises(emit.EmitError) as e:
            emit.tiled_decode(bad)
        assert f"tile {tile}:" in str(e.value)
        # ... the region decode of the centre tile (tile 4) does not look at it
        info, tiles, got = tiled_decode_region(bad, *centre)
        assert tiles == (1, 1, 1, 1) and np.array_equal(got, want), tile
    # ... nor at the middle of an untouched payload's coded data, whatever that does to the tile
    b = bytearray(frv)
    for tile in (1, 3, 5, 7):
        b[(o[tile] + o[tile + 1]) // 2] ^= 0xFF
    assert np.array_equal(tiled_decode_region(bytes(b), *centre)[2], want)
    # inside a touched payload: the error names the tile's index in the file's grid, not in the sub-grid
    with pytest.raises(emit.EmitError) as e:
        tiled_decode_region(flipped(4, 1), *centre)
    assert "tile 4:" in str(e.value)
    x, y, rw, rh = regions(case)["last partial column"]  # tiles 2, 5, 8 = sub-tiles 0, 1, 2
    for tile in (5, 8):
        rc, msg, *_ = _region_rc(flipped(tile, 1), (x, y, rw, rh))
        assert rc == -2 and msg.startswith(f"tile {tile}:"), msg
    rc, msg, *_ = _region_rc(flipped(4, 1), (x, y, rw, rh))  # tile 4 is not in that column
    assert rc == 0, msg
    # the lowest failing tile of the region, whatever the thread count
    b = bytearray(flipped(5, 1))
    b[o[9] - 1] ^= 0xFF
    for threads in (1, 4):
        rc, msg, *_ = _region_rc(bytes(b), (x, y, rw, rh), threads=threads)
        assert rc == -2 and msg.startswith("tile 5:"), msg


def test_malformed_files_are_refused_whatever_the_region():
    case = CASES[0]
    w, h, c, tw, th = case
    frv = frit_of(case)
    f = parse_frit(frv)
    o, n = f["offsets"], 9

    def patched(at, fmt, value):
        b = bytearray(frv)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)

    bad = [
        patched(32 + 8, "<Q", o[1] + 1),          # a shifted offset: the payload no longer starts with its magic
        patched(32 + 8, "<Q", o[2]),              # not strictly increasing
        patched(32 + 16, "<Q", o[1] - 8),         # decreasing
        patched(32, "<Q", o[0] + 2),              # offset[0] is not the end of the table
        patched(32 + 8 * n, "<Q", o[n] + 1),      # offset[n] is not the file length
        frv[:-1],                                 # ... nor after a truncation
        patched(4, "<I", 2),                      # version
        patched(24, "<I", 4),                     # ny is not ceil(H / tile_h)
        patched(16, "<I", 0),                     # tile_h = 0
        patched(16, "<I", 126),                   # a header whose tile is not the payloads'
        patched(o[1] + 4, "<I", th + 1),          # a payload of another height
        patched(o[3] + 8, "<I", tw - 1),          # ... of another width
        patched(o[8] + 12, "<I", struct.unpack_from("<I", frv, o[8] + 12)[0] | 50 << 8),  # ... with another metadata word
        f["payloads"][0],                         # a frif file
        b"frit",
    ]
    # a payload of another size: the file of a 64 x 48 tile in the place of tile 8, the table adjusted
    small = _tile_arrays(gen_image("smooth", 64, 48, 1, 1), 64, 48, 1)
    pl = list(f["payloads"])
    pl[8] = emit.encode_image_from_streams(64, 48, small[0], small[1], small[2], small[3], empty_ok=True)
    table, at = [], o[0]
    for p in pl:
        table.append(at)
        at += len(p)
    bad.append(frv[:32] + struct.pack("<10Q", *table, at) + b"".join(pl))
    whole_rc = emit.load_library().fri_tiled_decode
    for k, b in enumerate(bad):
        data = np.frombuffer(b, np.uint8)
        info = np.zeros(8, np.uint32)
        assert whole_rc(P(data), data.size, 2, P(info), None, 0, None, 0) == -2, k  # what fri_tiled_decode refuses ...
        for name, region in list(regions(case).items()) + [("tile 0", (0, 0, 1, 1)), ("an invalid region", (0, 0, 0, 0))]:
            rc, msg, *_ = _region_rc(b, region)  # ... is refused whatever the region: none of these touches the damaged tile's body
            assert rc == -2 and "Malformed tiled image" in msg, (k, name, rc, msg)
            rc, msg, *_ = _region_rc(b, region, cap=0)
            assert rc == -2, (k, name)


# ---- the host-only tiled plan ----------------------------------------------------------------------------------------------------------------------------

def test_host_only_plan_gives_the_range_and_refuses_compute():
    w, h, c, tw, th = CASES[1]
    p = PlanTiled(None, w, h, c, tw, th)
    for region in regions(CASES[1]).values():
        assert p.region_tiles(*region) == region_tiles(w, h, tw, th, *region)
    with pytest.raises(fa.FriHipError) as e:
        p.merge_tiles_region_dev(16, 0, 0, 8, 8, 32)
    assert e.value.code == -3
    with pytest.raises(fa.FriHipError) as e:
        p.decode_region_tiled_dev(16, 0, 0, 8, 8, 32)
    assert e.value.code == -3
    with pytest.raises(fa.FriHipError) as e:
        p.decode_region_tiled(np.zeros(c * p.num_cells * 512, np.int32), 0, 0, 8, 8)
    assert e.value.code == -3
    # a bad region and a null pointer are invalid arguments, with or without a device
    for call in (lambda: p.merge_tiles_region_dev(16, w - 1, 0, 2, 1, 32), lambda: p.decode_region_tiled_dev(16, 0, 0, 0, 1, 32), lambda: p.merge_tiles_region_dev(0, 0, 0, 1, 1, 32),
                 lambda: p.decode_region_tiled_dev(16, 0, 0, 1, 1, 0), lambda: p.region_tiles(0, h, 1, 1)):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -1
    p.close()
