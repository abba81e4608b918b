"""Preview of regions, host side (include/fri_emit.h and include/fri_hip.h, "Preview of regions"): the tile list and the preview-region table of
fri_tiled_preview_regions_tiles and fri_hip_plan_tiled_preview_regions against tests/preview_regions_ref.py, their size queries and refusals, the level-limited
decode of a tile list against both slices that define it, damage it must not see, the refusals that name the kind of file, the host-only plan, and a stand-alone
program that drives the two emitter functions under the sanitizers. CPU only. (That a call here leaves alone what fri_hip_merge_tiles_regions_dev accepts shows only
where that entry gets as far as its memory - with a device: tests/test_gpu_preview_regions.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd.api import TILED_ALLOW_HOLES, PlanTiled
from tests import preview_regions_ref as ref
from tests.coded_cases import tiled420_file, tiled_file
from tests.test_preview_host import FILES, _file, cut_stream_file
from tests.tiled_regions_ref import region_table, tile_list

preview_regions_tiles, decode_tiles_levels, plan_table = emit.tiled_preview_regions_tiles, emit.tiled_decode_tiles_levels, PlanTiled.preview_regions_table  # (without the feature the module fails here)

P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (W, H, C, tile_w, tile_h): the shapes of tests/test_gpu_preview.py, and one whose tiles are smaller than S = 16
SHAPES = [(41, 37, 3, 24, 20), (100, 70, 3, 36, 37), (150, 100, 1, 64, 64), (61, 45, 1, 7, 9)]


def region_set(w, h, shift):
    """regions of the thumbnail at `shift`: the whole thumbnail, the four 1 x 1 corners, the last column (the clamped sample where (W - 1) mod S < S / 2), a 17-wide
    region where the thumbnail has room for one, a repeat and an overlap"""
    tw, th = ref.thumbnail_size(w, h, shift)
    regs = [(0, 0, tw, th), (0, 0, 1, 1), (tw - 1, 0, 1, 1), (0, th - 1, 1, 1), (tw - 1, th - 1, 1, 1), (tw - 1, 0, 1, th)]
    if tw >= 19 and th >= 4:
        regs.append((2, 1, 17, 3))
    mid = (tw // 3, th // 3, max(1, tw // 2), max(1, th // 2))
    return regs + [mid, mid, (tw // 2, th // 2, tw - tw // 2, th - th // 2)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tile_list_and_table_equal_the_restatement(shape):
    w, h, c, tw, th = shape
    T = PlanTiled(None, w, h, c, tw, th, TILED_ALLOW_HOLES)
    clamped = 0
    for shift in range(5):
        s = 1 << shift
        clamped += (w - 1) % s < s // 2
        sets = [region_set(w, h, shift)] + [[r] for r in region_set(w, h, shift)[:6]]
        for regs in sets:
            want_list = ref.preview_tile_list(w, h, tw, th, shift, regs)
            want_table = ref.preview_region_table(w, h, c, tw, th, shift, regs)
            assert want_list == sorted(set(want_list)) and len(want_table) == 8 * (len(regs) + 1) + T.n_tiles
            assert preview_regions_tiles(w, h, tw, th, shift, regs).tolist() == want_list, (shift, regs)
            got_list, got_table = plan_table(T, shift, regs)
            assert got_list.tolist() == want_list and np.array_equal(got_table, want_table), (shift, regs)
            # every sample's tile is listed; a listed tile without a sample needs a tile side below S
            sampled = ref.sampled_tiles(w, h, tw, th, shift, regs)
            assert set(sampled) <= set(want_list)
            assert sampled == want_list or min(tw, th) < s, (shift, regs)
        if shift == 0:  # the thumbnail is the image: the list of "Several regions"; the table differs in its groups
            regs = sets[0]
            want_list, want_table = ref.preview_tile_list(w, h, tw, th, 0, regs), ref.preview_region_table(w, h, c, tw, th, 0, regs)
            assert want_list == tile_list(w, h, tw, th, regs)
            plain = region_table(w, h, c, tw, th, regs)
            assert np.array_equal(want_table[8 * (len(regs) + 1):], plain[8 * (len(regs) + 1):])
            assert np.array_equal(want_table.reshape(-1)[: 8 * len(regs)].reshape(-1, 8)[:, :6], plain[: 8 * len(regs)].reshape(-1, 8)[:, :6])
    assert clamped >= 2  # some shift's last column is the clamped sample
    T.close()


def test_a_tile_without_a_sample_is_listed():
    """61 x 45 in 7 x 9 tiles at S = 16: samples are 16 apart, so the whole thumbnail's source rectangle spans tiles that hold no sample - listed, never read"""
    w, h, c, tw, th = SHAPES[3]
    regs = [(0, 0, *ref.thumbnail_size(w, h, 4))]
    listed, sampled = ref.preview_tile_list(w, h, tw, th, 4, regs), ref.sampled_tiles(w, h, tw, th, 4, regs)
    assert set(sampled) < set(listed)
    assert preview_regions_tiles(w, h, tw, th, 4, regs).tolist() == listed


def test_size_queries_and_refusals():
    w, h, c, tw, th = SHAPES[1]
    L, H = emit.load_library(), fa.load_library()
    T = PlanTiled(None, w, h, c, tw, th, TILED_ALLOW_HOLES)
    shift = 2
    regs = np.array(region_set(w, h, shift), np.uint32)
    R = regs.shape[0]
    want_list, want_table = ref.preview_tile_list(w, h, tw, th, shift, regs.tolist()), ref.preview_region_table(w, h, c, tw, th, shift, regs.tolist())
    n = C.c_size_t(0)
    lst, table = np.full(len(want_list) + 1, 0xDEADBEEF, np.uint32), np.full(want_table.size + 1, 0xDEADBEEF, np.uint32)
    # the emitter: -3 with the count and nothing written, then the list
    for ptr, cap, rc in [(None, 0, -3), (P(lst), len(want_list) - 1, -3), (P(lst), len(want_list), 0)]:
        n.value = 0
        assert L.fri_tiled_preview_regions_tiles(w, h, tw, th, shift, R, P(regs), ptr, cap, C.addressof(n)) == rc and n.value == len(want_list)
        assert (lst == 0xDEADBEEF).all() if rc else (lst[:-1].tolist() == want_list and lst[-1] == 0xDEADBEEF)
    # the plan: -3 for a missing or short list or table, with the count and nothing written
    lst[:] = 0xDEADBEEF
    for lp, lc, tp, tc in [(None, 0, None, 0), (P(lst), len(want_list) - 1, P(table), want_table.size), (P(lst), len(want_list), P(table), want_table.size - 1),
                           (P(lst), len(want_list), None, want_table.size), (None, len(want_list), P(table), want_table.size)]:
        n.value = 0
        assert H.fri_hip_plan_tiled_preview_regions(T._h, shift, R, P(regs), lp, lc, C.addressof(n), tp, tc) == -3 and n.value == len(want_list)
        assert (lst == 0xDEADBEEF).all() and (table == 0xDEADBEEF).all()
    assert H.fri_hip_plan_tiled_preview_regions(T._h, shift, R, P(regs), P(lst), len(want_list), C.addressof(n), P(table), want_table.size) == 0
    assert lst[:-1].tolist() == want_list and np.array_equal(table[:-1], want_table) and lst[-1] == table[-1] == 0xDEADBEEF
    # refusals: shift > 4, a region that is empty or leaves the thumbnail (in 64 bits), R = 0, R > 65535, null pointers
    pw, ph = ref.thumbnail_size(w, h, shift)
    good = (0, 0, 2, 2)
    for bad in [(0, 0, 0, 1), (0, 0, 1, 0), (pw, 0, 1, 1), (0, ph, 1, 1), (1, 0, pw, 1), (0, 1, 1, ph), (2**32 - 1, 0, 2, 1), (0, 2**32 - 1, 1, 2)]:
        assert ref.preview_tile_list(w, h, tw, th, shift, [good, bad]) is None
        with pytest.raises(emit.EmitError):
            preview_regions_tiles(w, h, tw, th, shift, [good, bad])
        with pytest.raises(fa.FriHipError) as e:
            plan_table(T, shift, [bad, good])
        assert e.value.code == -1, bad
    assert (w - 1) // 4 + 1 == pw and ref.preview_tile_list(w, h, tw, th, 0, [(pw, 0, 1, 1)]) is not None  # (the same numbers are a region of the image itself)
    for s in (5, 6, 2**31):
        with pytest.raises(emit.EmitError):
            preview_regions_tiles(w, h, tw, th, s, [good])
        with pytest.raises(fa.FriHipError) as e:
            plan_table(T, s, [good])
        assert e.value.code == -1
    one = np.array([good], np.uint32)
    assert L.fri_tiled_preview_regions_tiles(w, h, tw, th, shift, 0, P(one), None, 0, C.addressof(n)) == -1
    assert L.fri_tiled_preview_regions_tiles(w, h, tw, th, shift, 1, None, None, 0, C.addressof(n)) == -1
    assert L.fri_tiled_preview_regions_tiles(w, h, tw, th, shift, 1, P(one), None, 0, None) == -1
    assert L.fri_tiled_preview_regions_tiles(w, h, 0, th, shift, 1, P(one), None, 0, C.addressof(n)) == -1
    assert H.fri_hip_plan_tiled_preview_regions(T._h, shift, 0, P(one), None, 0, C.addressof(n), None, 0) == -1
    assert H.fri_hip_plan_tiled_preview_regions(T._h, shift, 1, None, None, 0, C.addressof(n), None, 0) == -1
    assert H.fri_hip_plan_tiled_preview_regions(T._h, shift, 1, P(one), None, 0, None, None, 0) == -1
    assert H.fri_hip_plan_tiled_preview_regions(None, shift, 1, P(one), None, 0, C.addressof(n), None, 0) == -1
    many = np.tile(one, (65536, 1))
    assert ref.preview_region_table(w, h, c, tw, th, shift, many.tolist()) is None
    assert H.fri_hip_plan_tiled_preview_regions(T._h, shift, 65536, P(many), None, 0, C.addressof(n), None, 0) == -1
    assert H.fri_hip_plan_tiled_preview_regions(T._h, shift, 65535, P(many), None, 0, C.addressof(n), None, 0) == -3 and n.value == 1
    T.close()


def test_too_many_groups_are_refused():
    """the whole 4096 x 4096 image at m = 0 is 2^16 groups: 2^15 - 1 repeats of it fit, 2^15 make n_groups = 2^31 and are refused"""
    w = h = 4096
    T = PlanTiled(None, w, h, 1, 512, 512, TILED_ALLOW_HOLES)
    whole = np.tile(np.array([(0, 0, w, h)], np.uint32), (1 << 15, 1))
    assert ref.preview_region_table(w, h, 1, 512, 512, 0, whole.tolist()) is None
    with pytest.raises(fa.FriHipError) as e:
        plan_table(T, 0, whole)
    assert e.value.code == -1
    tiles, table = plan_table(T, 0, whole[:-1])
    assert tiles.size == 64 and int(table[8 * (whole.shape[0] - 1) + 6]) == 2**31 - 2**16
    assert int(table[8 * (whole.shape[0] - 1) + 4]) | int(table[8 * (whole.shape[0] - 1) + 5]) << 32 == (2**15 - 1) << 24  # the packed bytes pass 2^32
    T.close()


@pytest.mark.parametrize("case", FILES[:2] + FILES[3:], ids=lambda c: "%dx%dx%d_q%d" % (c[0], c[1], c[2], c[5]))
def test_level_limited_decode_of_a_tile_list_equals_both_slices(case):
    frv = _file(case)
    ti, full = emit.tiled_decode(frv)
    n = ti[4] * ti[5]
    lists = [[0], [n - 1], [0, n - 1], list(range(n))] if case == FILES[0] else [[1, n - 2]]
    for tiles in lists:
        _, part = emit.tiled_decode_tiles(frv, tiles)
        for levels in range(10) if case == FILES[0] else (0, 3, 7, 9):
            all_tiles = emit.tiled_decode_levels(frv, levels)[1]
            for threads in (1, 3):
                info, got = decode_tiles_levels(frv, tiles, levels, threads)
                assert tuple(info) == tuple(ti) and got.shape == (len(tiles),) + full.shape[1:3] + (1 << levels,)
                assert np.array_equal(got, all_tiles[tiles]), (tiles, levels, threads)
                assert np.array_equal(got, part[..., : 1 << levels]), (tiles, levels, threads)


def test_decode_refusals_and_the_size_query():
    frv = _file(FILES[0])
    L = emit.load_library()
    data = np.frombuffer(frv, np.uint8)
    ti, full = emit.tiled_decode(frv)
    tiles = np.array([1, 3], np.uint32)
    levels = 3
    buf = np.zeros(2 * full[0].size >> (9 - levels), np.int32)
    for cap, ptr, rc in [(0, None, -3), (buf.size - 1, P(buf), -3), (buf.size, P(buf), 0)]:
        info = np.zeros(8, np.uint32)
        assert L.fri_tiled_decode_tiles_levels(P(data), data.size, 2, P(tiles), 2, levels, P(info), ptr, cap, None, 0) == rc
        assert [int(x) for x in info] == [int(v) for v in ti[:8]]
    assert np.array_equal(buf.reshape((2,) + full.shape[1:3] + (8,)), full[[1, 3]][..., :8])
    info, err = np.zeros(8, np.uint32), C.create_string_buffer(256)
    args = (P(info), P(buf), buf.size, err, 256)
    assert L.fri_tiled_decode_tiles_levels(P(data), data.size, 2, P(tiles), 2, 10, *args) == -1
    assert L.fri_tiled_decode_tiles_levels(None, data.size, 2, P(tiles), 2, 3, *args) == -1
    assert L.fri_tiled_decode_tiles_levels(P(data), data.size, 2, None, 2, 3, *args) == -1
    assert L.fri_tiled_decode_tiles_levels(P(data), data.size, 2, P(tiles), 0, 3, *args) == -1
    assert L.fri_tiled_decode_tiles_levels(P(data), data.size, 2, P(tiles), 2, 3, None, P(buf), buf.size, err, 256) == -1
    for bad in ([3, 1], [1, 1], [4], []):
        with pytest.raises(emit.EmitError) as e:
            decode_tiles_levels(frv, bad, 3)
        assert e.value.code == -1 and (not bad or "invalid tile list" in str(e.value))
    with pytest.raises(emit.EmitError):
        decode_tiles_levels(frv, [0], 10)
    # what fri_tiled_decode refuses as malformed is malformed here too
    assert L.fri_tiled_decode_tiles_levels(P(data), data.size - 1, 2, P(tiles), 2, 3, *args) == -2 and b"Malformed tiled image" in err.value


def test_tiled_420_and_rgba_files_are_refused_by_name():
    from tests.test_tiled_rgba_host import GRIDS, _inputs
    from tests.tiled_rgba_ref import container

    L = emit.load_library()
    info, err = np.zeros(8, np.uint32), C.create_string_buffer(256)
    one = np.array([0], np.uint32)
    d420 = np.frombuffer(tiled420_file(100, 70, 52, 50, 50)[0], np.uint8)
    rgba = np.frombuffer(container(*GRIDS[0], _inputs("lossless", GRIDS[0])[1]), np.uint8)
    assert emit.tiled_info(rgba.tobytes()).alpha and emit.tiled_info(d420.tobytes()).s420
    for lv in (0, 4, 9):
        assert L.fri_tiled_decode_tiles_levels(P(d420), d420.size, 2, P(one), 1, lv, P(info), None, 0, err, 256) == -1
        assert b"4:2:0" in err.value
        assert L.fri_tiled_decode_tiles_levels(P(rgba), rgba.size, 2, P(one), 1, lv, P(info), None, 0, err, 256) == -1
        assert b"tiled RGBA" in err.value
    with pytest.raises(emit.EmitError, match="4:2:0"):
        decode_tiles_levels(d420.tobytes(), [0], 5)
    with pytest.raises(emit.EmitError, match="tiled RGBA"):
        decode_tiles_levels(rgba.tobytes(), [0], 5)


def test_damage_behind_the_prefix_or_in_an_unlisted_payload_is_not_seen():
    cut, plane, low = cut_stream_file()  # 250 x 250 x 1 in 2 x 2 tiles, lossless; tile 1's plane cut to half its words
    ti, full = emit.tiled_decode(_file(FILES[0]))
    assert plane == 1
    # listed, but the prefix ends before the cut
    got = decode_tiles_levels(cut, [1, 2], low)[1]
    assert np.array_equal(got, full[[1, 2]][..., : 1 << low])
    # all levels: seen when listed, by the tile's index in the file's grid; not seen when unlisted
    with pytest.raises(emit.EmitError, match="tile 1: channel 0: stream truncated") as e:
        decode_tiles_levels(cut, [0, 1], 9)
    assert e.value.code == -2
    got = decode_tiles_levels(cut, [0, 2, 3], 9)[1]
    assert np.array_equal(got, full[[0, 2, 3]])


def test_host_only_plan_refuses_what_computes():
    w, h, c, tw, th = SHAPES[1]
    T = PlanTiled(None, w, h, c, tw, th, TILED_ALLOW_HOLES)
    shift, levels = 2, 5
    regs = region_set(w, h, shift)
    tiles, table = plan_table(T, shift, regs)  # works without a device
    compact = np.zeros((tiles.size, c, T.num_cells, 1 << levels), np.int32)
    planes = tiles.size * c
    coded = (np.zeros((planes, 32), np.uint32), np.full(planes, 20, np.uint32), np.zeros((planes, 10, 4), np.uint32), np.zeros((planes, 10, 1024), np.uint16),
             np.zeros((planes, 3, 6), np.float32), np.zeros((planes, 3, 6), np.float32))
    calls = [lambda: T.preview_regions(compact, levels, shift, regs), lambda: T.preview_regions_coded(coded, levels, shift, regs),
             lambda: T.preview_tiles_regions_dev(16, T.num_cells << levels, 1 << levels, levels, shift, tiles.size, len(regs), 16, 16)]
    for call in calls:
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -3
    # what is refused as an argument is refused before the device is asked for
    for call in [lambda: T.preview_regions(compact, 10, shift, regs), lambda: T.preview_regions(compact, levels, 5, regs), lambda: T.preview_regions_coded(coded, levels, 5, regs),
                 lambda: T.preview_tiles_regions_dev(0, T.num_cells << levels, 1 << levels, levels, shift, tiles.size, len(regs), 16, 16),
                 lambda: T.preview_tiles_regions_dev(16, T.num_cells << levels, 64, levels, shift, tiles.size, len(regs), 16, 16)]:
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -1
    T.close()


def test_the_two_emitter_functions_under_the_sanitizers(tmp_path):
    """A stand-alone program with its own main: nothing loaded into python is run under a sanitizer."""
    exe, src = tmp_path / "preview_regions_host_check", tmp_path / "in.frv"
    host, csrc = os.path.join(ROOT, "frave_amd", "host"), os.path.join(ROOT, "frave_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "include"), "-I", host, "-I", csrc, "-o", str(exe), os.path.join(ROOT, "tests", "tools", "preview_regions_host_check.cpp"),
                           os.path.join(host, "emit.cpp"), os.path.join(host, "emit_abi.cpp"), os.path.join(csrc, "geometry.cpp")])
    src.write_bytes(tiled_file(100, 70, 1, 52, 50, 100)[0])
    out = subprocess.run([str(exe), str(src)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
