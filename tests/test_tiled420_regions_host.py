"""Several regions of a tiled 4:2:0 file, host side (include/fri_hip.h "Several regions of tiled 4:2:0 files"; fri_hip_plan_tiled420_regions): the tile list and the
4:2:0 region table against tests/tiled420_regions_ref.py on a host-only plan, the -3 size query, every refusal, and FRI_HIP_ERR_NO_DEVICE for everything that
computes. CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.emit as emit
from frave_amd.api import TILED_ALLOW_HOLES, PlanTiled420
from tests.test_gpu_tiled420 import REGION_SHAPES, regions_of
from tests.tiled420_regions_ref import region_table420
from tests.tiled_regions_ref import NOT_LISTED, grid_of, region_table, tile_list

plan_regions = PlanTiled420.regions  # (without the feature the module fails here)

P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (W, H, tile_w, tile_h): every strip crosses columns; a tile of one strip; odd tile width and height (chroma clamping); tiles below a strip; more than one group;
# the largest, 2 x 2 tiles with the last column and row partial
SHAPES = [(5, 3, 2, 2), (17, 9, 16, 4), (35, 23, 17, 9), (40, 33, 5, 3), (257, 130, 100, 50), (1023, 767, 512, 512)]


def region_sets(shape):
    """name -> [(x, y, w, h), ...]"""
    w, h, tw, th = shape
    sets = {
        "b: two pixels in opposite corners": [(0, 0, 1, 1), (w - 1, h - 1, 1, 1)],
        "w: the whole image, its last row and its last column": [(0, 0, w, h), (0, h - 1, w, 1), (w - 1, 0, 1, h)],
        "o: from pixel (1, 1)": [(1, 1, w - 1, h - 1)],  # its strips start on odd tile columns
    }
    if shape in REGION_SHAPES:
        every = list(regions_of(shape).values())
        sets["a: all regions of the region test and a repeat"] = every + [every[0]]
    return sets


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_list_and_table_are_the_restatements(shape):
    w, h, tw, th = shape
    nx, ny = grid_of(w, h, tw, th)
    plan = PlanTiled420(None, w, h, tw, th, TILED_ALLOW_HOLES)  # host only
    assert w > 1 and h > 1
    for name, regs in region_sets(shape).items():
        want_list, want_table = tile_list(w, h, tw, th, regs), region_table420(w, h, tw, th, regs)
        assert emit.tiled_regions_tiles(w, h, tw, th, regs).tolist() == want_list, name  # the "Several regions" list, unchanged
        tiles, table = plan.regions(regs)
        assert tiles.dtype == np.uint32 and tiles.tolist() == want_list and table.dtype == np.uint32 and np.array_equal(table, want_table), name
        assert table.size == 8 * (len(regs) + 1) + nx * ny
        slot = table[8 * (len(regs) + 1):]
        assert [int(slot[t]) for t in want_list] == list(range(len(want_list))) and (slot == NOT_LISTED).sum() == nx * ny - len(want_list)
        assert int(table[8 * len(regs) + 4]) == sum(3 * r[2] * r[3] for r in regs)
        if name.startswith("b") and nx * ny > 2:
            assert len(want_list) == 2 and want_list[1] - want_list[0] > 1  # not neighbours in the grid
        if name.startswith("w"):
            assert want_list == list(range(nx * ny)) and int(table[8 + 6]) == -(-(h * -(-w // 16)) // 256)
        if name.startswith("a"):
            assert len(regs) == 7 and any(int(table[8 * r + 4]) & 1 for r in range(len(regs)))  # some packed offsets are odd
    if shape == SHAPES[-1]:
        # strips of 16 pixels, not of 16 bytes: the whole image is 192 groups here and 576 in the C = 3 table of "Several regions"
        regs = region_sets(shape)["w: the whole image, its last row and its last column"]
        table = plan.regions(regs)[1]
        assert [int(table[8 * r + 6]) for r in range(4)] == [0, 192, 193, 196] and -(-(767 * 64) // 256) == 192
        assert int(region_table(w, h, 3, tw, th, regs)[8 + 6]) == 576
    plan.close()


def test_list_and_table_of_many_small_regions_on_a_small_grid():
    w, h, tw, th = 23, 17, 5, 4  # 5 x 5 tiles, the last column and row partial
    plan = PlanTiled420(None, w, h, tw, th, TILED_ALLOW_HOLES)
    rng = np.random.default_rng(18)
    for trial in range(40):
        regs = []
        for _ in range(int(rng.integers(1, 9))):
            x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
            regs.append((x, y, int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1))))
        tiles, table = plan.regions(regs)
        assert tiles.tolist() == tile_list(w, h, tw, th, regs), regs
        assert np.array_equal(table, region_table420(w, h, tw, th, regs)), regs
    plan.close()


def test_refusals_and_size_queries():
    w, h, tw, th = 257, 130, 100, 50  # 3 x 3 tiles
    H = fa.load_library()
    plan = PlanTiled420(None, w, h, tw, th, TILED_ALLOW_HOLES)
    n = C.c_size_t(77)
    good = np.array([[0, 0, 1, 1], [w - 1, h - 1, 1, 1]], np.uint32)
    out, table = np.zeros(9, np.uint32), np.zeros(8 * 4 + 9, np.uint32)
    # -1: every region "Region decode" refuses, wherever it stands in the set; no regions
    for bad in [(0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (0, 1, 1, h), (2**32 - 1, 0, 2, 1)]:
        for at in range(3):
            regs = [(0, 0, 1, 1), (5, 5, 2, 2)]
            regs.insert(at, bad)
            arr = np.array(regs, np.uint32)
            assert H.fri_hip_plan_tiled420_regions(plan._h, 3, P(arr), P(out), 9, C.addressof(n), P(table), table.size) == -1, (bad, at)
            assert region_table420(w, h, tw, th, regs) is None
            with pytest.raises(fa.FriHipError) as e:
                plan.regions(regs)
            assert e.value.code == -1
    for empty in ([], np.zeros((0, 4), np.uint32)):
        with pytest.raises(fa.FriHipError) as e:
            plan.regions(empty)
        assert e.value.code == -1
    # R = 0 and R > 65535 are refused, R = 65535 is not; null pointers; the -3 size queries
    many = np.tile(np.array([[3, 3, 1, 1]], np.uint32), (65536, 1))
    big_table = np.zeros(8 * 65537 + 9, np.uint32)
    assert H.fri_hip_plan_tiled420_regions(plan._h, 0, P(many), P(out), 9, C.addressof(n), P(big_table), big_table.size) == -1
    assert H.fri_hip_plan_tiled420_regions(plan._h, 65536, P(many), P(out), 9, C.addressof(n), P(big_table), big_table.size) == -1
    assert H.fri_hip_plan_tiled420_regions(plan._h, 65535, P(many), P(out), 9, C.addressof(n), P(big_table), big_table.size) == 0 and n.value == 1
    assert np.array_equal(big_table[: 8 * 65536 + 9], region_table420(w, h, tw, th, [(3, 3, 1, 1)] * 65535))
    assert H.fri_hip_plan_tiled420_regions(None, 2, P(good), P(out), 9, C.addressof(n), P(table), table.size) == -1
    assert H.fri_hip_plan_tiled420_regions(plan._h, 2, None, P(out), 9, C.addressof(n), P(table), table.size) == -1
    assert H.fri_hip_plan_tiled420_regions(plan._h, 2, P(good), P(out), 9, None, P(table), table.size) == -1
    need = 8 * 3 + 9
    for args in [(None, 0, P(table), need), (P(out), 1, P(table), need), (P(out), 2, None, 0), (P(out), 2, P(table), need - 1)]:
        n.value, out[:], table[:] = 77, 0, 0
        assert H.fri_hip_plan_tiled420_regions(plan._h, 2, P(good), args[0], args[1], C.addressof(n), args[2], args[3]) == -3 and n.value == 2
        assert not out.any() and not table.any()  # nothing but *n_list is written
    assert H.fri_hip_plan_tiled420_regions(plan._h, 2, P(good), P(out), 2, C.addressof(n), P(table), need) == 0 and out.tolist()[:3] == [0, 8, 0]
    assert np.array_equal(table[:need], region_table420(w, h, tw, th, good.tolist()))
    plan.close()
    # n_groups >= 2^31 is refused. A row of 2^20 pixels is 65536 strips, 256 groups: 65535 regions of 128 rows are 2147450880 < 2^31 <= 2164228096 groups of 129 rows
    W2 = 1 << 20
    t2, o2 = np.zeros(8 * 65536 + 1024, np.uint32), np.zeros(1024, np.uint32)
    for rows, rc in ((128, 0), (129, -1)):
        wide = PlanTiled420(None, W2, rows, 1024, rows, TILED_ALLOW_HOLES)
        whole = np.tile(np.array([[0, 0, W2, rows]], np.uint32), (65535, 1))
        want = region_table420(W2, rows, 1024, rows, [(0, 0, W2, rows)] * 65535)
        assert H.fri_hip_plan_tiled420_regions(wide._h, 65535, P(whole), P(o2), 1024, C.addressof(n), P(t2), t2.size) == rc, rows
        if rc == 0:
            assert np.array_equal(t2, want) and int(t2[8 * 65535 + 6]) == 65535 * 256 * 128 and int(t2[8 * 65535 + 5]) > 0  # (the packed bytes pass 2^32)
        else:
            assert want is None
        wide.close()
    # 3 W > 2^31 - 1 is refused: a region row's byte offsets are 32-bit
    for width, rc in ((715827882, 0), (715827883, -1)):
        assert (3 * width > 2**31 - 1) == (rc != 0)
        wide = PlanTiled420(None, width, 1, 32768, 1, TILED_ALLOW_HOLES)
        one = np.array([[5, 0, 1, 1]], np.uint32)
        t3 = np.zeros(16 + wide.n_tiles, np.uint32)
        assert H.fri_hip_plan_tiled420_regions(wide._h, 1, P(one), P(o2), 1024, C.addressof(n), P(t3), t3.size) == rc, width
        assert (region_table420(width, 1, 32768, 1, one.tolist()) is None) == (rc != 0)
        wide.close()


def test_host_only_plan_refuses_compute():
    w, h, tw, th = 257, 130, 100, 50
    p = PlanTiled420(None, w, h, tw, th, TILED_ALLOW_HOLES)
    regs = [(0, 0, 1, 1), (w - 1, h - 1, 1, 1)]
    tiles, table = p.regions(regs)
    assert tiles.tolist() == [0, 8] and np.array_equal(table, region_table420(w, h, tw, th, regs))
    coefs = np.zeros(2 * p.tile_coef_count, np.int32)
    coded = (np.zeros((6, 32), np.uint32), np.full(6, 20, np.uint32), np.zeros((6, 10, 4), np.uint32), np.zeros((6, 10, 1024), np.uint16),
             np.zeros((6, 3, 6), np.float32), np.zeros((6, 3, 6), np.float32))
    for call in (lambda: p.merge_tiles420_regions_dev(16, 16, 2, 2, 32, 48), lambda: p.decode_regions_tiled420_dev(16, 60, regs, 32), lambda: p.decode_regions_tiled420(coefs, 60, regs),
                 lambda: p.decode_regions_coded(coded, 60, regs)):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -3
    # a bad region, a bad R, a null pointer and a quality outside 1..99 are invalid arguments, with or without a device
    for call in (lambda: p.decode_regions_tiled420_dev(16, 60, [(w - 1, 0, 2, 1)], 32), lambda: p.decode_regions_tiled420_dev(16, 60, [], 32),
                 lambda: p.decode_regions_tiled420_dev(0, 60, regs, 32), lambda: p.decode_regions_tiled420_dev(16, 60, regs, 0),
                 lambda: p.decode_regions_tiled420_dev(16, 0, regs, 32), lambda: p.decode_regions_tiled420_dev(16, 100, regs, 32),
                 lambda: p.merge_tiles420_regions_dev(0, 16, 2, 2, 32, 48), lambda: p.merge_tiles420_regions_dev(16, 0, 2, 2, 32, 48),
                 lambda: p.merge_tiles420_regions_dev(16, 16, 2, 2, 0, 48), lambda: p.merge_tiles420_regions_dev(16, 16, 2, 2, 32, 0),
                 lambda: p.merge_tiles420_regions_dev(16, 16, 10, 2, 32, 48), lambda: p.merge_tiles420_regions_dev(16, 16, 0, 2, 32, 48),
                 lambda: p.merge_tiles420_regions_dev(16, 16, 2, 0, 32, 48), lambda: p.merge_tiles420_regions_dev(16, 16, 2, 65536, 32, 48),
                 lambda: p.decode_regions_tiled420(coefs, 60, [(0, 0, 0, 1)]), lambda: p.decode_regions_tiled420(coefs, 0, regs),
                 lambda: p.decode_regions_tiled420(coefs, 100, regs), lambda: p.decode_regions_coded(coded, 100, regs),
                 lambda: p.decode_regions_coded(coded, 60, [(0, 0, w + 1, 1)])):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -1
    p.close()


def test_the_builder_with_pixel_strips_under_the_sanitizers(tmp_path):
    """tests/tools/region_table420_check.cpp: csrc/region_table.hpp alone, build_region_table with StripUnit::Pixels against the definition restated in C++ and
    every refusal at its edge. A stand-alone program with its own main: nothing loaded into python is run under a sanitizer."""
    exe = tmp_path / "region_table420_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "frave_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "tools", "region_table420_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
