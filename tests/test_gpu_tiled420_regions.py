"""Several regions of a tiled 4:2:0 file on the device (K18's merge_tiles420_regions_kernel, fri_hip_decode_regions_tiled420*) against
tests/tiled420_regions_ref.py:

- K18 exactly equal to the restatement - the crops of the numpy merge of full-grid planes whose unlisted tiles hold poison - on shapes whose every strip crosses
  tile columns, with odd tile widths and heights, with more than one workgroup per region, for (b) two one-pixel regions in opposite corners (two tiles that are
  not neighbours: a lane that ignores the slot table shows), (w) the whole image with its last row and column, (o) the region from pixel (1, 1), whose strips start
  on odd tile columns and which is K12's region merge, and (a) all regions of the region test plus a repeat (odd packed offsets); random plane bytes, device
  pointers 0, 1 and 3 bytes off a 256-byte boundary, between guard bytes;
- a replay from a captured graph of the one kernel node on two inputs;
- end to end on a 3 x 2 file: fri_tiled_decode_tiles + fri_hip_decode_regions_tiled420 gives the crops of fri_tiled_decode + fri_hip_decode_image_tiled420, the _dev
  form on a stream of its own, a capturing stream refused, the coded route (K13) the same bytes, a truncated listed plane reported by its tile in the file's grid;
- fri_driver decode-regions --420, with and without --device-rans, and its refusals."""
import ctypes as C
import functools
import glob
import os
import subprocess

import numpy as np
import pytest

import frave_amd.emit as emit
from frave_amd.api import DECODE_TRUNCATED, TILED_ALLOW_HOLES, PlanTiled420
from tests.chroma420_ref import chroma_shape
from tests.coded_cases import tiled420_file
from tests.test_gpu_instances import Guarded
from tests.test_gpu_tiled420 import REGION_SHAPES
from tests.test_tiled420_regions_host import SHAPES, region_sets
from tests.tiled420_ref import sub_grid
from tests.tiled420_regions_ref import merge_regions420, region_table420
from tests.tiled_regions_ref import grid_of, tile_list

plan_regions = PlanTiled420.regions  # (without the feature the module fails here)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELAXED = 2  # hipStreamCaptureModeRelaxed
FILE = (150, 100, 52, 50, 60)  # W, H, tile_w, tile_h, quality: 3 x 2 tiles, the last column and row partial


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@functools.lru_cache(maxsize=None)
def _case(shape, name, seed=0):
    """(regions, tile list, 4:2:0 region table, random bytes for the tile-list planes y_tiles and c_tiles, the packed output the restatement makes of them)"""
    w, h, tw, th = shape
    cw, ch = chroma_shape(tw, th)
    regs = region_sets(shape)[name]
    tiles = tile_list(w, h, tw, th, regs)
    rng = np.random.default_rng([w, h, len(name), seed])
    y, c = rng.integers(0, 256, (len(tiles), th, tw), dtype=np.uint8), rng.integers(0, 256, (len(tiles), 2, ch, cw), dtype=np.uint8)
    want = merge_regions420(y, c, tiles, w, h, tw, th, regs)
    for a in (y, c, want):
        a.setflags(write=False)
    return regs, tiles, region_table420(w, h, tw, th, regs), y, c, want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_regions_kernel_equals_the_restatement(ctx, shape):
    import torch

    import frave_amd as fa

    w, h, tw, th = shape
    nx, ny = grid_of(w, h, tw, th)
    T = PlanTiled420(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    names = list(region_sets(shape))
    assert [n[0] for n in names] == (["b", "w", "o", "a"] if shape in REGION_SHAPES else ["b", "w", "o"])
    for name in names:
        regs, tiles, want_table, y, c, want = _case(shape, name)
        if name.startswith("b") and nx * ny > 2:
            assert len(tiles) == 2 and tiles[1] - tiles[0] > 1  # not neighbours in the grid, neighbours in the planes
        if name.startswith("w"):
            assert int(want_table[8 + 6]) == -(-(h * -(-w // 16)) // 256)
            assert shape != SHAPES[-1] or int(want_table[8 + 6]) == 192  # the whole image's groups: many at the largest shape
        if name.startswith("o"):
            assert regs == [(1, 1, w - 1, h - 1)] and tiles == list(range(nx * ny))
        if name.startswith("a"):
            assert any(int(want_table[8 * r + 4]) & 1 for r in range(len(regs)))  # some packed offsets are odd
        for offset in (0, 1, 3):
            got_list, table = T.regions(regs)  # (the plan launches for the table it wrote last)
            assert got_list.tolist() == tiles and np.array_equal(table, want_table)
            d_table = torch.from_numpy(table.view(np.int32).copy()).cuda()
            sy, sc = Guarded(torch, y.size, offset=offset, salt=4), Guarded(torch, c.size, offset=offset, salt=5)
            sy.put(torch, [y.reshape(-1)])
            sc.put(torch, [c.reshape(-1)])
            dst = Guarded(torch, want.size, offset=offset, salt=6)
            T.merge_tiles420_regions_dev(sy.ptr, sc.ptr, len(tiles), len(regs), d_table.data_ptr(), dst.ptr)
            (got,), intact = dst.get(torch)
            assert intact, ("K18 wrote outside the packed output", shape, name, offset)
            bad = got != want
            assert not bad.any(), (shape, name, offset, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
            (ay,), ok_y = sy.get(torch)  # the inputs come back intact
            (ac,), ok_c = sc.get(torch)
            assert ok_y and ok_c and np.array_equal(ay, y.reshape(-1)) and np.array_equal(ac, c.reshape(-1))
            if len(regs) == 1:  # one region: its list is its sub-grid, and the result K12's region merge
                i0, j0, ni, nj = T.region_tiles(*regs[0])
                assert np.array_equal(sub_grid(np.arange(nx * ny), nx, i0, j0, ni, nj), tiles)
                one = Guarded(torch, want.size, offset=offset, salt=7)
                T.merge_tiles420_region_dev(sy.ptr, sc.ptr, *regs[0], one.ptr)
                (merged,), ok = one.get(torch)
                assert ok and np.array_equal(got, merged)
    # a table of another call is refused, not launched
    T.regions([(0, 0, 1, 1)])
    before = dst.get(torch)[0][0]
    assert (len(tiles), len(regs)) != (1, 1)
    for n_list, n_regions in ((len(tiles), len(regs)), (2, 1), (1, 2)):  # the last launch's T and R, another T, another R
        with pytest.raises(fa.FriHipError) as e:
            T.merge_tiles420_regions_dev(sy.ptr, sc.ptr, n_list, n_regions, d_table.data_ptr(), dst.ptr)
        assert e.value.code == -1
    (after,), intact = dst.get(torch)
    assert intact and np.array_equal(before, after)
    T.close()


def test_regions_kernel_replays_from_a_graph_of_one_node_on_two_inputs(ctx, hip):
    import torch

    shape = (257, 130, 100, 50)
    name = "a: all regions of the region test and a repeat"
    T = PlanTiled420(ctx, *shape, TILED_ALLOW_HOLES)
    regs, tiles, want_table, y, c, want = _case(shape, name)
    _, table = T.regions(regs)
    d_table = torch.from_numpy(table.view(np.int32).copy()).cuda()
    d_y = torch.zeros(y.size, dtype=torch.uint8, device="cuda")
    d_c = torch.zeros(c.size, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    T.merge_tiles420_regions_dev(d_y.data_ptr(), d_c.data_ptr(), len(tiles), len(regs), d_table.data_ptr(), d_out.data_ptr(), stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    n_nodes = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 1
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    torch.cuda.synchronize()
    assert not d_out.cpu().numpy().any(), "capturing ran nothing"
    for seed in (0, 1):  # each replay works on what the buffers hold now
        _, _, _, y, c, want = _case(shape, name, seed)
        d_y.copy_(torch.from_numpy(y.reshape(-1).copy()))
        d_c.copy_(torch.from_numpy(c.reshape(-1).copy()))
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(ex, sp) == 0
        s.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), want), seed
    assert not np.array_equal(_case(shape, name, 0)[5], _case(shape, name, 1)[5])
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    T.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _file():
    return tiled420_file(*FILE)[0]


def file_regions():
    w, h, tw, th, _ = FILE
    across = (tw - 3, th - 2, 7, 5)
    return [(0, 0, 1, 1), (w - 1, h - 1, 1, 1), across, across]  # a corner pixel in tile 0, one in tile 5, across a tile corner, a repeat


def test_regions_decode_gives_the_crops_of_the_whole_decode(ctx, hip):
    import torch

    import frave_amd as fa

    w, h, tw, th, quality = FILE
    frv = _file()
    T = PlanTiled420(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    assert (T.nx, T.ny) == (3, 2)
    T.set_stream_order()
    regs = file_regions()
    tiles = tile_list(w, h, tw, th, regs)
    assert tiles == [0, 1, 3, 4, 5] and T.regions(regs)[0].tolist() == tiles
    total = sum(3 * r[2] * r[3] for r in regs)
    ti, coefs = emit.tiled_decode(frv)
    assert ti.s420 and ti.quality == quality
    whole = T.decode_image_tiled420(coefs, quality).reshape(h, w, 3)
    want = [whole[y:y + rh, x:x + rw] for x, y, rw, rh in regs]
    fresh = PlanTiled420(ctx, w, h, tw, th, TILED_ALLOW_HOLES)  # a fresh plan: its tile buffers hold the listed tiles and no more
    _, part = emit.tiled_decode_tiles(frv, tiles)
    got = fresh.decode_regions_tiled420(part, quality, regs)
    assert fresh.buffer_tiles() == (5, 5) and len(got) == len(regs)
    fresh.close()
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), k
    # the _dev form on a stream of its own: the same bytes, nothing outside the packed output
    s = torch.cuda.Stream()
    d_coefs = torch.from_numpy(part.reshape(-1).copy()).cuda()
    dst = Guarded(torch, total, offset=1, salt=7)
    torch.cuda.synchronize()
    T.decode_regions_tiled420_dev(d_coefs.data_ptr(), quality, regs, dst.ptr, stream=s.cuda_stream)
    s.synchronize()
    (packed,), intact = dst.get(torch)
    assert intact and np.array_equal(packed, np.concatenate([b.reshape(-1) for b in want]))
    # the coded route: K13 over the listed tiles' planes, the same bytes, every status 0
    coded = emit.tiled_parse_coded_tiles(frv, tiles)
    got, status = T.decode_regions_coded(coded, quality, regs)
    assert status.shape == (3 * len(tiles), 4) and not status[:, 0].any()
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), ("coded", k)
    # a capturing stream is refused with nothing enqueued
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    try:
        with pytest.raises(fa.FriHipError) as e:
            T.decode_regions_tiled420_dev(d_coefs.data_ptr(), quality, regs, d_out.data_ptr(), stream=s.cuda_stream)
        assert e.value.code == -1 and "graph" in str(e.value)
    finally:
        assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0
    n_nodes = C.c_size_t(12345)
    rc = hip.hipGraphGetNodes(graph, None, C.byref(n_nodes))
    hip.hipGraphDestroy(graph)
    assert rc == 0 and n_nodes.value == 0
    # bad regions, a bad R, a bad quality and null pointers are refused
    for bad in [(0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (0, 1, 1, h), (2**32 - 1, 0, 2, 1)]:
        for call in (lambda: T.regions([regs[0], bad]), lambda: T.decode_regions_tiled420_dev(d_coefs.data_ptr(), quality, [bad, regs[0]], d_out.data_ptr()),
                     lambda: T.decode_regions_tiled420(part, quality, [regs[0], bad]), lambda: T.decode_regions_coded(coded, quality, [bad])):
            with pytest.raises(fa.FriHipError) as e:
                call()
            assert e.value.code == -1, bad
    for call in (lambda: T.decode_regions_tiled420_dev(0, quality, regs, d_out.data_ptr()), lambda: T.decode_regions_tiled420_dev(d_coefs.data_ptr(), quality, regs, 0),
                 lambda: T.decode_regions_tiled420_dev(d_coefs.data_ptr(), quality, [], d_out.data_ptr()), lambda: T.decode_regions_tiled420_dev(d_coefs.data_ptr(), 0, regs, d_out.data_ptr()),
                 lambda: T.decode_regions_tiled420(part, 100, regs), lambda: T.decode_regions_coded(coded, 0, regs)):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -1
    T.close()


def test_a_truncated_listed_plane_is_reported_by_its_tile_in_the_files_grid(ctx):
    import frave_amd as fa
    from tests.test_gpu_decode import _with_plane_data

    w, h, tw, th, quality = FILE
    frv = _file()
    ti, words, n_words, models, off, vp, wp = emit.tiled_parse_coded(frv)
    plane = 6 + 2 * 5 + 1  # Cr of tile 5, in the plane order of the file's six tiles; its payload is tile 5's
    cut = _with_plane_data(frv, words[plane, : n_words[plane]], 1, 5, words[plane, : int(n_words[plane]) // 2])
    T = PlanTiled420(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    T.set_stream_order()
    whole = T.decode_image_tiled420(emit.tiled_decode(frv)[1], quality).reshape(h, w, 3)
    touching = file_regions()[:2]  # tiles 0 and 5: tile 5 is entry 1 of the list, its Cr plane T + 2 * 1 + 1 = 5 of the list's six
    tiles = T.regions(touching)[0].tolist()
    assert tiles == [0, 5]
    with pytest.raises(emit.EmitError, match="tile 5: channel 2: stream truncated"):
        emit.tiled_decode_tiles(cut, tiles)
    planes = emit.tiled_parse_coded_tiles(cut, tiles)
    words_k, n_k, models_k, off_k, vp_k, wp_k = (np.ascontiguousarray(a) for a in planes[1:])
    out = np.full(6, 0xA5, np.uint8)
    status = np.zeros((6, 4), np.uint32)
    rg = np.array(touching, np.uint32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = fa.load_library().fri_hip_decode_regions_tiled420_coded(T._h, 2, P(rg), P(words_k), words_k.shape[1], P(n_k), P(models_k), P(off_k), P(vp_k), P(wp_k), quality, P(out), P(status))
    assert rc == -1 and (out == 0xA5).all()  # the output is untouched
    assert status[5, 0] & DECODE_TRUNCATED and not status[:5, 0].any()
    with pytest.raises(fa.FriHipError) as e:
        T.decode_regions_coded(planes, quality, touching)
    assert e.value.code == -1 and e.value.tile == 5 and "tile 5: channel 2" in str(e.value)
    assert e.value.status[5, 0] & DECODE_TRUNCATED and not e.value.status[:5, 0].any()
    # regions that do not touch the damaged tile decode, on both routes
    beside = [(3, 3, 20, 20), (tw - 3, th - 2, 7, 5)]  # tiles 0, 1, 3, 4
    tiles = T.regions(beside)[0].tolist()
    assert tiles == [0, 1, 3, 4]
    want = [whole[y:y + rh, x:x + rw] for x, y, rw, rh in beside]
    got, status = T.decode_regions_coded(emit.tiled_parse_coded_tiles(cut, tiles), quality, beside)
    assert not status[:, 0].any() and all(np.array_equal(a, b) for a, b in zip(got, want))
    got = T.decode_regions_tiled420(emit.tiled_decode_tiles(cut, tiles)[1], quality, beside)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    T.close()


def test_driver_decodes_several_regions_of_a_tiled_420_file(ctx, tmp_path):
    """fri_driver decode-regions --420 (FRIDecoder::decode_regions420) writes the crops of decode-file's image, with and without --device-rans; a file that is not
    tiled 4:2:0, --preview and a bad region are refused with nothing written; without --420 the file is refused as before"""
    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h, tw, th, quality = FILE
    src, back = tmp_path / "s420.frv", tmp_path / "s420.ppm"
    src.write_bytes(_file())
    regs = file_regions() + [(10, 20, 120, 70)]  # ... and one across all six tiles, overlapping the others
    region_args = [a for r in regs for a in ("--region", ",".join(map(str, r)))]

    def run(*args):
        return subprocess.run([driver, *map(str, args)], capture_output=True, text=True, timeout=300)

    def written(prefix):
        return sorted(glob.glob(str(prefix) + "*"))

    out = run("decode-file", src, back)
    assert out.returncode == 0, out.stderr
    whole = np.frombuffer(back.read_bytes()[-3 * w * h:], np.uint8).reshape(h, w, 3)
    for route, extra in (("host", []), ("device", ["--device-rans"])):
        prefix = tmp_path / f"out_{route}"
        out = run("decode-regions", src, prefix, "--420", *region_args, *extra)
        assert out.returncode == 0, out.stdout + out.stderr
        assert written(prefix) == [f"{prefix}.{k}.ppm" for k in range(len(regs))] and "K18" in out.stdout
        for k, (x, y, rw, rh) in enumerate(regs):
            raw = open(f"{prefix}.{k}.ppm", "rb").read()
            assert raw.startswith(b"P6\n%d %d\n255\n" % (rw, rh)) and f"{rw}x{rh}x3" in out.stdout
            assert np.array_equal(np.frombuffer(raw[-3 * rw * rh:], np.uint8).reshape(rh, rw, 3), whole[y:y + rh, x:x + rw]), (route, k)
    # refusals write nothing: a bad region, no region, --preview with --420
    bad = tmp_path / "refused"
    for args in (["--region", f"{w - 1},0,2,1"], ["--region", "0,0,8,8", "--region", "0,0,0,5"], [], ["--device-rans"], ["--preview", "1", "--region", "0,0,8,8"],
                 ["--region", "0,0,8,8", "--preview", "2", "--device-rans"]):
        out = run("decode-regions", src, bad, "--420", *args)
        assert out.returncode != 0 and not written(bad), args
    out = run("decode-regions", src, bad, "--420", "--preview", "1", "--region", "0,0,8,8")
    assert "--preview" in out.stderr
    # without --420 the subcommand is what it was: the file is refused, and the message says what to use instead
    out = run("decode-regions", src, bad, "--region", "0,0,8,8")
    assert out.returncode != 0 and "4:2:0" in out.stderr and "decode-file --region" in out.stderr and not written(bad)
    # --420 on files that are not tiled 4:2:0: a 4:4:4 tiled file and an untiled file
    from tests.tiled_ref import mixed_image

    ppm = tmp_path / "in.ppm"
    ppm.write_bytes(b"P6\n%d %d\n255\n" % (334, 350) + mixed_image(334, 350, 3, 167, 8).tobytes())
    for name, flags, magic in (("frit444", ["--tile-size", "150", "--ycbcr", "--quality", "60"], b"frit"), ("frif", ["--ycbcr", "--quality", "60"], b"frif")):
        dst = tmp_path / f"{name}.frv"
        out = run("encode-file", ppm, dst, *flags)
        assert out.returncode == 0 and dst.read_bytes()[:4] == magic, out.stdout + out.stderr
        for extra in ([], ["--device-rans"]):
            out = run("decode-regions", dst, bad, "--420", "--region", "0,0,8,8", *extra)
            assert out.returncode != 0 and not written(bad), (name, extra)
        if name == "frit444":
            assert "4:2:0" in out.stderr
            out = run("decode-regions", dst, tmp_path / "ok444", "--region", "0,0,8,8")  # ... which the subcommand without --420 decodes
            assert out.returncode == 0 and written(tmp_path / "ok444") == [str(tmp_path / "ok444") + ".0.ppm"]
