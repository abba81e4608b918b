"""Several regions per call, host side (include/fri_emit.h "Several regions"; fri_tiled_regions_tiles, fri_tiled_decode_tiles, fri_tiled_parse_coded_tiles,
fri_hip_plan_tiled_regions): the tile list and the region table against tests/tiled_regions_ref.py, the tile-list decode and parse against the rows of the whole
file's on the 3 x 3 grids of tests/test_tiled_region_host.py, damage inside and outside the listed tiles, every refusal, and the host-only tiled plan. CPU only."""
import ctypes as C
import functools

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd.api import TILED_ALLOW_HOLES, PlanTiled
from tests import rate_model
from tests.test_tiled_host import _inputs, _streams
from tests.test_tiled_region_host import CASES, frit_of, regions as named_regions
from tests.tiled_ref import grid, mixed_image, parse_frit, split_tiles
from tests.tiled_regions_ref import NOT_LISTED, region_table, tile_list

tiled_regions_tiles, tiled_decode_tiles, tiled_parse_coded_tiles = emit.tiled_regions_tiles, emit.tiled_decode_tiles, emit.tiled_parse_coded_tiles  # (without the feature
plan_regions = PlanTiled.regions  # the module fails here)

P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def region_sets(case):
    """name -> [(x, y, w, h), ...] on a 3 x 3-tile image"""
    w, h, c, tw, th = case
    named = named_regions(case)
    every = list(named.values())
    return {
        "all of them and a repeat": every + [every[0]],  # overlapping (the whole image is among them), repeated, sizes differ
        "two pixels in opposite corners": [(0, 0, 1, 1), (w - 1, h - 1, 1, 1)],  # two tiles that are not neighbours
        "one region": [named["across all nine"]],
        "the whole image": [(0, 0, w, h)],
        "centre and last column": [named["centre tile"], named["last partial column"]],  # tiles 2, 4, 5, 8: neither a sub-grid nor the grid
        "the same pixel three times": [(tw, th, 1, 1)] * 3,
    }


@functools.lru_cache(maxsize=None)
def lossy_inputs(case, quality=50):
    """test_tiled_host._inputs at a quality: the oracle's arrays of every tile, quantised"""
    w, h, c, tw, th = case
    per = []
    for tile in split_tiles(mixed_image(w, h, c, tw, 3), tw, th):
        centers, coefs, bucket, pred, hist, oob, vp, wp = rate_model.oracle_arrays(np.ascontiguousarray(tile).reshape(-1), tw, th, c, quality)
        assert not oob.any()
        per.append((_streams(centers, coefs, bucket, pred), hist, vp, wp, coefs))
    return tuple(np.stack([p[k] for p in per]) for k in range(5))


def files_of(case):
    """name -> (frit bytes, the coefficients it was made from): lossless and lossy"""
    w, h, c, tw, th = case
    streams, hist, vp, wp, coefs = lossy_inputs(case)
    return {"lossless": (frit_of(case), _inputs(case)[4]), "quality 50": (emit.tiled_encode_from_streams(w, h, tw, th, streams, hist, vp, wp, quality=50), coefs)}


# ---- the tile list and the region table ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda s: "x".join(map(str, s)))
def test_list_and_table_are_the_restatements(case):
    w, h, c, tw, th = case
    plan = PlanTiled(None, w, h, c, tw, th)  # host only
    for name, regs in region_sets(case).items():
        want_list, want_table = tile_list(w, h, tw, th, regs), region_table(w, h, c, tw, th, regs)
        got = tiled_regions_tiles(w, h, tw, th, regs)
        assert got.dtype == np.uint32 and got.tolist() == want_list, name
        tiles, table = plan.regions(regs)
        assert tiles.tolist() == want_list and table.dtype == np.uint32 and np.array_equal(table, want_table), name
        assert table.size == 8 * (len(regs) + 1) + 9
        # what the words say: the slots invert the list, the last row holds the totals
        slot = table[8 * (len(regs) + 1):]
        assert [int(slot[t]) for t in want_list] == list(range(len(want_list))) and (slot == NOT_LISTED).sum() == 9 - len(want_list)
        assert int(table[8 * len(regs) + 4]) == sum(r[2] * r[3] * c for r in regs)
    assert tile_list(w, h, tw, th, region_sets(case)["centre and last column"]) == [2, 4, 5, 8]
    assert tile_list(w, h, tw, th, region_sets(case)["two pixels in opposite corners"]) == [0, 8]
    assert tile_list(w, h, tw, th, region_sets(case)["the whole image"]) == list(range(9))
    plan.close()


def test_list_and_table_of_many_small_regions_on_a_small_grid():
    w, h, c, tw, th = 23, 17, 3, 5, 4  # 5 x 5 tiles, the last column and row partial
    plan = PlanTiled(None, w, h, c, tw, th, TILED_ALLOW_HOLES)
    rng = np.random.default_rng(15)
    for trial in range(40):
        regs = []
        for _ in range(int(rng.integers(1, 9))):
            x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
            regs.append((x, y, int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1))))
        tiles, table = plan.regions(regs)
        assert tiles.tolist() == tile_list(w, h, tw, th, regs) == tiled_regions_tiles(w, h, tw, th, regs).tolist(), regs
        assert np.array_equal(table, region_table(w, h, c, tw, th, regs)), regs
    # a region of more than one group: first_group moves by ceil(h ceil(w C / 16) / 256)
    regs = [(0, 0, 23, 17), (1, 1, 1, 1), (0, 0, 23, 17)]
    table = plan.regions(regs)[1]
    assert [int(table[8 * r + 6]) for r in range(4)] == [0, 1, 2, 3] and 17 * 5 <= 256
    plan.close()
    big = PlanTiled(None, 1023, 767, 3, 512, 512, TILED_ALLOW_HOLES)
    table = big.regions([(0, 0, 1023, 767), (5, 5, 1, 1)])[1]
    assert [int(table[8 * r + 6]) for r in range(3)] == [0, 576, 577] and -(-(767 * 192) // 256) == 576
    assert np.array_equal(table, region_table(1023, 767, 3, 512, 512, [(0, 0, 1023, 767), (5, 5, 1, 1)]))
    big.close()


def test_list_and_table_refusals_and_size_queries():
    w, h, c, tw, th = CASES[1]
    L, H = emit.load_library(), fa.load_library()
    plan = PlanTiled(None, w, h, c, tw, th)
    n = C.c_size_t(77)
    good = np.array([[0, 0, 1, 1], [w - 1, h - 1, 1, 1]], np.uint32)
    out = np.zeros(9, np.uint32)
    # the emitter: -3 with *n_list filled for list == NULL and for a capacity that is too small; 0 with the exact capacity
    assert L.fri_tiled_regions_tiles(w, h, tw, th, 2, P(good), None, 0, C.addressof(n)) == -3 and n.value == 2
    n.value = 77
    assert L.fri_tiled_regions_tiles(w, h, tw, th, 2, P(good), P(out), 1, C.addressof(n)) == -3 and n.value == 2 and not out.any()
    assert L.fri_tiled_regions_tiles(w, h, tw, th, 2, P(good), P(out), 2, C.addressof(n)) == 0 and out.tolist()[:3] == [0, 8, 0]
    # -1: no regions, null pointers, zero sizes, every region fri_tiled_region_tiles refuses - wherever it stands in the set
    assert L.fri_tiled_regions_tiles(w, h, tw, th, 0, P(good), P(out), 9, C.addressof(n)) == -1
    assert L.fri_tiled_regions_tiles(w, h, tw, th, 2, None, P(out), 9, C.addressof(n)) == -1
    assert L.fri_tiled_regions_tiles(w, h, tw, th, 2, P(good), P(out), 9, None) == -1
    assert L.fri_tiled_regions_tiles(w, h, 0, th, 2, P(good), P(out), 9, C.addressof(n)) == -1
    table = np.zeros(8 * 4 + 9, np.uint32)
    for bad in [(0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (0, 1, 1, h), (2**32 - 1, 0, 2, 1)]:
        for at in range(3):
            regs = [(0, 0, 1, 1), (5, 5, 2, 2)]
            regs.insert(at, bad)
            arr = np.array(regs, np.uint32)
            assert L.fri_tiled_regions_tiles(w, h, tw, th, 3, P(arr), P(out), 9, C.addressof(n)) == -1, (bad, at)
            assert H.fri_hip_plan_tiled_regions(plan._h, 3, P(arr), P(out), 9, C.addressof(n), P(table), table.size) == -1, (bad, at)
            with pytest.raises(emit.EmitError):
                tiled_regions_tiles(w, h, tw, th, regs)
            with pytest.raises(fa.FriHipError) as e:
                plan.regions(regs)
            assert e.value.code == -1
    for empty in ([], np.zeros((0, 4), np.uint32)):
        with pytest.raises(emit.EmitError):
            tiled_regions_tiles(w, h, tw, th, empty)
        with pytest.raises(fa.FriHipError) as e:
            plan.regions(empty)
        assert e.value.code == -1
    # the plan: R = 0 and R > 65535 are refused, R = 65535 is not; null pointers; the -3 size queries
    many = np.tile(np.array([[3, 3, 1, 1]], np.uint32), (65536, 1))
    big_table = np.zeros(8 * 65537 + 9, np.uint32)
    assert H.fri_hip_plan_tiled_regions(plan._h, 0, P(many), P(out), 9, C.addressof(n), P(big_table), big_table.size) == -1
    assert H.fri_hip_plan_tiled_regions(plan._h, 65536, P(many), P(out), 9, C.addressof(n), P(big_table), big_table.size) == -1
    assert H.fri_hip_plan_tiled_regions(plan._h, 65535, P(many), P(out), 9, C.addressof(n), P(big_table), big_table.size) == 0 and n.value == 1
    assert np.array_equal(big_table[: 8 * 65536 + 9], region_table(w, h, c, tw, th, [(3, 3, 1, 1)] * 65535))
    assert H.fri_hip_plan_tiled_regions(None, 2, P(good), P(out), 9, C.addressof(n), P(table), table.size) == -1
    assert H.fri_hip_plan_tiled_regions(plan._h, 2, None, P(out), 9, C.addressof(n), P(table), table.size) == -1
    assert H.fri_hip_plan_tiled_regions(plan._h, 2, P(good), P(out), 9, None, P(table), table.size) == -1
    need = 8 * 3 + 9
    for args in [(None, 0, P(table), need), (P(out), 1, P(table), need), (P(out), 2, None, 0), (P(out), 2, P(table), need - 1)]:
        n.value, out[:], table[:] = 77, 0, 0
        assert H.fri_hip_plan_tiled_regions(plan._h, 2, P(good), args[0], args[1], C.addressof(n), args[2], args[3]) == -3 and n.value == 2
        assert not out.any() and not table.any()  # nothing but *n_list is written
    assert H.fri_hip_plan_tiled_regions(plan._h, 2, P(good), P(out), 2, C.addressof(n), P(table), need) == 0
    assert np.array_equal(table[:need], region_table(w, h, c, tw, th, good.tolist()))
    plan.close()
    # n_groups >= 2^31 is refused. A row of 2^20 RGB pixels is 196608 strips: 42 rows are 32256 groups, 43 rows 33024, and 65535 such regions are
    # 2113929216 < 2^31 <= 2164227840 groups
    W2 = 1 << 20
    t2, o2 = np.zeros(8 * 65536 + 1024, np.uint32), np.zeros(1024, np.uint32)
    for rows, rc in ((42, 0), (43, -1)):
        wide = PlanTiled(None, W2, rows, 3, 1024, rows, TILED_ALLOW_HOLES)
        whole = np.tile(np.array([[0, 0, W2, rows]], np.uint32), (65535, 1))
        want = region_table(W2, rows, 3, 1024, rows, [(0, 0, W2, rows)] * 65535)
        assert H.fri_hip_plan_tiled_regions(wide._h, 65535, P(whole), P(o2), 1024, C.addressof(n), P(t2), t2.size) == rc, rows
        if rc == 0:
            assert np.array_equal(t2, want) and int(t2[8 * 65535 + 6]) == 65535 * 32256 and int(t2[8 * 65535 + 5]) > 0  # (the packed bytes pass 2^32)
        else:
            assert want is None
        wide.close()


# ---- the decode and the parse of a tile list ----------------------------------------------------------------------------------------------------------------

def _tiles_rc(data, tiles, cap=None, threads=2):
    """(rc, message, info, coefs) of fri_tiled_decode_tiles through the C ABI, into a buffer of `cap` elements (None: plenty)"""
    data = np.frombuffer(bytes(data), np.uint8)
    tl = np.asarray(tiles, np.uint32)
    info = np.zeros(8, np.uint32)
    err = C.create_string_buffer(256)
    buf = np.zeros(1 << 22 if cap is None else max(cap, 1), np.int32)
    rc = emit.load_library().fri_tiled_decode_tiles(P(data), data.size, threads, P(tl), tl.size, P(info), P(buf) if cap != 0 else None, buf.size if cap is None else cap, err, 256)
    return rc, err.value.decode(), [int(v) for v in info], buf


@pytest.mark.parametrize("case", CASES, ids=lambda s: "x".join(map(str, s)))
def test_decode_tiles_gives_the_listed_rows_of_the_whole_decode(case):
    w, h, c, tw, th = case
    assert grid(w, h, tw, th) == (3, 3)
    for mode, (frv, made_from) in files_of(case).items():
        whole_info, whole = emit.tiled_decode(frv, 2)
        assert np.array_equal(whole, made_from)
        F = whole.shape[2]
        for name, regs in region_sets(case).items():
            tiles = tile_list(w, h, tw, th, regs)
            want = whole[tiles]
            for threads in (1, 4):  # the same bytes for every thread count
                info, got = tiled_decode_tiles(frv, tiles, threads=threads)
                assert tuple(info) == tuple(whole_info) and got.shape == (len(tiles), c, F, 512) and np.array_equal(got, want), (mode, name, threads)
            if len(regs) == 1:  # the list of a single region is its sub-grid, row-major
                _, sub, part = emit.tiled_decode_region(frv, *regs[0])
                assert sub[2] * sub[3] == len(tiles) and np.array_equal(part, want), (mode, name)
        # the size query and a buffer one element short: -3 with info filled; the exact buffer: 0
        tiles = [2, 4, 5, 8]
        want = whole[tiles]
        for cap, rc in [(0, -3), (want.size - 1, -3), (want.size, 0)]:
            got_rc, msg, got_info, buf = _tiles_rc(frv, tiles, cap)
            assert got_rc == rc and got_info == [w, h, tw, th, 3, 3, c | (emit.QUALITY(50) if mode != "lossless" else 0), F], (mode, cap, msg)
        assert np.array_equal(buf[: want.size].reshape(want.shape), want)


def test_decode_tiles_of_a_tiled_420_file_is_in_plane_order():
    from tests.test_tiled420_host import H as H4, TH, TW, W as W4, _coefs_in_plane_order, _inputs as inputs420

    per, (streams, n_y, n_c, hist, vp, wp) = inputs420(60)
    frv = emit.tiled_encode_from_streams420(W4, H4, TW, TH, streams, n_y, n_c, hist, vp, wp, 60)
    assert len(per) == 4
    for tiles in ([0], [3], [1, 2], [0, 1, 3], [0, 1, 2, 3]):
        want = _coefs_in_plane_order([per[t] for t in tiles])  # the luma planes of the listed tiles, then their chroma planes: n = T
        for threads in (1, 4):
            info, got = tiled_decode_tiles(frv, tiles, threads=threads)
            assert info.s420 and got.shape == want.shape and np.array_equal(got, want), (tiles, threads)
        # ... and the coded planes in the same order
        whole = emit.tiled_parse_coded(frv)
        part = tiled_parse_coded_tiles(frv, tiles)
        rows = list(tiles) + [4 + 2 * t + k for t in tiles for k in (0, 1)]
        assert part[0].s420 and np.array_equal(part[2], whole[2][rows])
        for k in (3, 4, 5, 6):
            assert np.array_equal(part[k], whole[k][rows]), (tiles, k)
        for a, b, n in zip(part[1], whole[1][rows], part[2]):
            assert np.array_equal(a[:n], b[:n])
    assert np.array_equal(tiled_decode_tiles(frv, [0, 1, 2, 3])[1], emit.tiled_decode(frv)[1])
    _, sub, region = emit.tiled_decode_region(frv, 3, 55, 20, 10)  # the bottom left tile
    assert np.array_equal(tiled_decode_tiles(frv, emit.tiled_regions_tiles(W4, H4, TW, TH, [(3, 55, 20, 10)]))[1], region)


@pytest.mark.parametrize("case", CASES, ids=lambda s: "x".join(map(str, s)))
def test_parse_coded_tiles_gives_the_listed_rows_of_the_whole_parse(case):
    w, h, c, tw, th = case
    frv = files_of(case)["quality 50"][0]
    ti, words, n_words, models, off, vp, wp = emit.tiled_parse_coded(frv)
    for name, regs in region_sets(case).items():
        tiles = tile_list(w, h, tw, th, regs)
        rows = [t * c + ch for t in tiles for ch in range(c)]
        gi, gw, gn, gm, go, gvp, gwp = tiled_parse_coded_tiles(frv, tiles)
        assert tuple(gi) == tuple(ti) and gn.shape == (len(rows),) and np.array_equal(gn, n_words[rows]), name
        assert gw.shape == (len(rows), max(int(gn.max()), 1))
        for k, p in enumerate(rows):
            assert np.array_equal(gw[k, : gn[k]], words[p, : gn[k]]) and not gw[k, gn[k]:].any(), (name, p)
        assert np.array_equal(gm, models[rows]) and np.array_equal(go, off[rows]) and np.array_equal(gvp, vp[rows]) and np.array_equal(gwp, wp[rows]), name
    # the size queries: -3 without n_words or with too few planes, the counts alone with words == NULL, a stride that is too short names the plane of the list
    L = emit.load_library()
    data = np.frombuffer(frv, np.uint8)
    tl = np.array([2, 5], np.uint32)
    info, nw, err = np.zeros(8, np.uint32), np.zeros(2 * c, np.uint32), C.create_string_buffer(256)
    assert L.fri_tiled_parse_coded_tiles(P(data), data.size, P(tl), 2, P(info), 0, None, 0, None, None, None, None, None, err, 256) == -3 and int(info[4]) == 3
    assert L.fri_tiled_parse_coded_tiles(P(data), data.size, P(tl), 2, P(info), 2 * c - 1, None, 0, P(nw), None, None, None, None, err, 256) == -3 and not nw.any()
    assert L.fri_tiled_parse_coded_tiles(P(data), data.size, P(tl), 2, P(info), 2 * c, None, 0, P(nw), None, None, None, None, err, 256) == 0
    assert np.array_equal(nw, n_words[[t * c + ch for t in (2, 5) for ch in range(c)]])
    with pytest.raises(emit.EmitError, match="plane ") as e:
        tiled_parse_coded_tiles(frv, [2, 5], word_stride=int(nw.min()) - 1)
    assert e.value.code == -2 and np.array_equal(e.value.n_words, nw)


@pytest.mark.parametrize("case", CASES, ids=lambda s: "x".join(map(str, s)))
def test_damage_in_an_unlisted_payload_is_not_seen_and_damage_in_a_listed_one_names_the_files_tile(case):
    w, h, c, tw, th = case
    frv = frit_of(case)
    o = parse_frit(frv)["offsets"]
    tiles = [2, 4, 5, 8]
    want = tiled_decode_tiles(frv, tiles)[1]
    want_coded = tiled_parse_coded_tiles(frv, tiles)

    def flipped(tile, back, src=frv):  # a byte inside the body of a payload, `back` bytes before its end
        b = bytearray(src)
        b[o[tile + 1] - back] ^= 0xFF
        return bytes(b)

    for tile in (0, 1, 3, 6, 7):  # the end marker of an unlisted payload: the whole decode and the whole parse refuse the file, the tile-list forms do not look
        bad = flipped(tile, 1)
        for whole in (emit.tiled_decode, emit.tiled_parse_coded):
            with pytest.raises(emit.EmitError, match=f"tile {tile}:"):
                whole(bad)
        assert np.array_equal(tiled_decode_tiles(bad, tiles)[1], want), tile
        for a, b in zip(tiled_parse_coded_tiles(bad, tiles)[1:], want_coded[1:]):
            assert np.array_equal(a, b), tile
    b = bytearray(frv)  # ... nor at the middle of an unlisted payload's coded data
    for tile in (0, 1, 3, 6, 7):
        b[(o[tile] + o[tile + 1]) // 2] ^= 0xFF
    assert np.array_equal(tiled_decode_tiles(bytes(b), tiles)[1], want)
    # a listed payload: the error names the tile's index in the file's grid, not in the list - tile 5 is entry 2, tile 8 entry 3
    for tile in (5, 8):
        for call in (tiled_decode_tiles, tiled_parse_coded_tiles):
            with pytest.raises(emit.EmitError) as e:
                call(flipped(tile, 1), tiles)
            assert str(e.value).startswith(f"tile {tile}:") and e.value.code == -2, (tile, str(e.value))
    # the lowest failing tile of the list, whatever the thread count
    both = flipped(8, 1, flipped(5, 1))
    for threads in (1, 4):
        rc, msg, *_ = _tiles_rc(both, tiles, threads=threads)
        assert rc == -2 and msg.startswith("tile 5:"), msg


def test_bad_lists_files_and_null_pointers_are_refused():
    case = CASES[0]
    frv = frit_of(case)
    L = emit.load_library()
    data = np.frombuffer(frv, np.uint8)
    info, err = np.zeros(8, np.uint32), C.create_string_buffer(256)
    nw = np.zeros(64, np.uint32)
    for bad in ([], [1, 1], [2, 1], [0, 3, 3], [0, 9], [9], [2**32 - 1], [0, 1, 2, 3, 4, 5, 6, 7, 8, 8]):
        tl = np.array(bad, np.uint32)
        ptr = P(tl) if tl.size else P(np.zeros(1, np.uint32))
        assert L.fri_tiled_decode_tiles(P(data), data.size, 1, ptr, tl.size, P(info), None, 0, err, 256) == -1, bad
        assert L.fri_tiled_parse_coded_tiles(P(data), data.size, ptr, tl.size, P(info), 64, None, 0, P(nw), None, None, None, None, err, 256) == -1, bad
        for call in (tiled_decode_tiles, tiled_parse_coded_tiles):
            with pytest.raises(emit.EmitError) as e:
                call(frv, bad)
            assert e.value.code == -1, bad
    assert "invalid tile list" in err.value.decode()
    tl = np.array([4], np.uint32)
    assert L.fri_tiled_decode_tiles(None, data.size, 1, P(tl), 1, P(info), None, 0, err, 256) == -1
    assert L.fri_tiled_decode_tiles(P(data), data.size, 1, None, 1, P(info), None, 0, err, 256) == -1
    assert L.fri_tiled_decode_tiles(P(data), data.size, 1, P(tl), 1, None, None, 0, err, 256) == -1
    assert L.fri_tiled_parse_coded_tiles(P(data), data.size, None, 1, P(info), 0, None, 0, None, None, None, None, None, err, 256) == -1
    assert L.fri_tiled_parse_coded_tiles(P(data), data.size, P(tl), 1, P(info), 1, P(nw), 8, P(nw), None, None, None, None, err, 256) == -1  # words without the rest
    # a file that is not a well-formed `frit` file is refused whatever the list: a frif file, a truncation, a payload header that does not match
    f = parse_frit(frv)
    damaged = bytearray(frv)
    damaged[f["offsets"][7] + 4] ^= 1  # tile 7's height, in its 16-byte header: checked although tile 7 is not listed
    for bad in (f["payloads"][0], frv[:-1], b"frit", bytes(damaged)):
        for call in (tiled_decode_tiles, tiled_parse_coded_tiles):
            with pytest.raises(emit.EmitError, match="Malformed tiled image") as e:
                call(bad, [4])
            assert e.value.code == -2


# ---- the host-only tiled plan -------------------------------------------------------------------------------------------------------------------------------

def test_host_only_plan_gives_list_and_table_and_refuses_compute():
    case = CASES[1]
    w, h, c, tw, th = case
    p = PlanTiled(None, w, h, c, tw, th)
    regs = region_sets(case)["centre and last column"]
    tiles, table = p.regions(regs)
    assert tiles.tolist() == [2, 4, 5, 8] and np.array_equal(table, region_table(w, h, c, tw, th, regs))
    coefs = np.zeros((4, c, p.num_cells, 512), np.int32)
    coded = (np.zeros((4 * c, 32), np.uint32), np.full(4 * c, 20, np.uint32), np.zeros((4 * c, 10, 4), np.uint32), np.zeros((4 * c, 10, 1024), np.uint16),
             np.zeros((4 * c, 3, 6), np.float32), np.zeros((4 * c, 3, 6), np.float32))
    for call in (lambda: p.merge_tiles_regions_dev(16, 4, 2, 32, 48), lambda: p.decode_regions_tiled_dev(16, regs, 32), lambda: p.decode_regions_tiled(coefs, regs),
                 lambda: p.decode_regions_coded(coded, regs)):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -3
    # a bad region, a bad R and a null pointer are invalid arguments, with or without a device
    for call in (lambda: p.decode_regions_tiled_dev(16, [(w - 1, 0, 2, 1)], 32), lambda: p.decode_regions_tiled_dev(16, [], 32), lambda: p.decode_regions_tiled_dev(0, regs, 32),
                 lambda: p.decode_regions_tiled_dev(16, regs, 0), lambda: p.merge_tiles_regions_dev(0, 4, 2, 32, 48), lambda: p.merge_tiles_regions_dev(16, 4, 2, 0, 48),
                 lambda: p.merge_tiles_regions_dev(16, 4, 2, 32, 0), lambda: p.merge_tiles_regions_dev(16, 10, 2, 32, 48), lambda: p.merge_tiles_regions_dev(16, 0, 2, 32, 48),
                 lambda: p.merge_tiles_regions_dev(16, 4, 0, 32, 48), lambda: p.merge_tiles_regions_dev(16, 4, 65536, 32, 48),
                 lambda: p.decode_regions_tiled(coefs, [(0, 0, 0, 1)])):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -1
    p.close()
