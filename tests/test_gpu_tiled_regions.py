"""Several regions per call on the device (K15's merge_tiles_regions_kernel, fri_hip_decode_regions_tiled*) against tests/tiled_regions_ref.py:

- K15 exactly equal to the per-pixel restatement on the shapes of the region test - tile rows shorter than a 16-byte strip, more than one workgroup per region,
  several regions per launch - for (a) all regions of the region test in one call plus a repeat (overlapping, sizes differ, odd packed offsets), (b) two one-pixel
  regions in opposite corners (two tiles that are not neighbours: a lane that ignores the slot table shows), (c) one region, which is K10's region merge; random
  tile bytes, device pointers 0, 1 and 3 bytes off a 256-byte boundary, between guard bytes;
- a replay from a captured graph of the one kernel node;
- end to end: fri_tiled_decode_tiles + fri_hip_decode_regions_tiled gives the crops of fri_tiled_decode + fri_hip_decode_image_tiled, the _dev form on a stream of
  its own, a capturing stream refused, the coded route (K13) the same bytes, a truncated listed plane reported by its tile in the file's grid;
- fri_driver decode-regions, with and without --device-rans, and its refusals."""
import ctypes as C
import functools
import glob
import os
import subprocess

import numpy as np
import pytest

import frave_amd.emit as emit
from frave_amd.api import DECODE_TRUNCATED, TILED_ALLOW_HOLES, PlanTiled
from tests.oracle_ref import MIDPOINT, REFERENCE
from tests.test_gpu_instances import Guarded
from tests.test_gpu_tiled_region import kernel_regions
from tests.tiled_ref import mixed_image
from tests.tiled_regions_ref import merge_regions, merge_regions_fast, region_table, tile_list

plan_regions, tiled_decode_tiles, tiled_parse_coded_tiles = PlanTiled.regions, emit.tiled_decode_tiles, emit.tiled_parse_coded_tiles  # (without the feature the module fails here)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELAXED = 2  # hipStreamCaptureModeRelaxed
COLOUR_NONE, COLOUR_RCT, COLOUR_YCBCR = 0, 1, 3
# (W, H, C, tile_w, tile_h)
SHAPES = [(5, 3, 3, 2, 2), (17, 9, 1, 16, 4), (33, 20, 3, 16, 16), (257, 130, 3, 100, 50), (1023, 767, 3, 512, 512)]
IMAGES = [(375, 375, 1, 125, 125), (450, 330, 3, 167, 117)]  # 3 x 3 tiles (tests/test_tiled_region_host.py)


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


def region_sets(shape):
    w, h, c, tw, th = shape
    every = list(kernel_regions(shape).values())
    return {
        "a: all regions of the region test and a repeat": every + [every[0]],
        "b: two pixels in opposite corners": [(0, 0, 1, 1), (w - 1, h - 1, 1, 1)],
        "c: one region": [kernel_regions(shape)["interior, off the strip grid"]],
    }


@functools.lru_cache(maxsize=None)
def _case(shape, name):
    """(regions, tile list, region table, random bytes for the tile-list raster [T][tile_h][tile_w][C], the packed output the restatement makes of them)"""
    w, h, c, tw, th = shape
    regs = region_sets(shape)[name]
    tiles = tile_list(w, h, tw, th, regs)
    raster = np.random.default_rng([w, h, len(name)]).integers(0, 256, (len(tiles), th, tw, c), dtype=np.uint8)
    want = merge_regions_fast(raster, tiles, w, h, tw, th, regs)
    if w * h <= 257 * 130:  # the literal per-pixel definition wherever a Python loop over the pixels is affordable
        assert np.array_equal(want, merge_regions(raster, tiles, w, h, tw, th, regs))
    raster.setflags(write=False), want.setflags(write=False)
    return regs, tiles, region_table(w, h, c, tw, th, regs), raster, want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_regions_kernel_equals_the_restatement(ctx, shape):
    import torch

    w, h, c, tw, th = shape
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    for name in region_sets(shape):
        regs, tiles, want_table, raster, want = _case(shape, name)
        if name.startswith("a"):
            assert len(regs) == 10 and any(int(want_table[8 * r + 4]) & 1 for r in range(len(regs)))  # some packed offsets are odd
            assert int(want_table[8 + 6]) == -(-(h * -(-(w * c) // 16)) // 256)  # the whole image's groups: many at the largest shape
            assert shape != SHAPES[-1] or int(want_table[8 + 6]) == 576
        if name.startswith("b") and len(tiles) == 2:
            assert tiles[1] - tiles[0] > 1  # not neighbours in the grid, neighbours in the raster
        for offset in (0, 1, 3):
            got_list, table = T.regions(regs)  # (the plan launches for the table it wrote last)
            assert got_list.tolist() == tiles and np.array_equal(table, want_table)
            d_table = torch.from_numpy(table.view(np.int32).copy()).cuda()
            src = Guarded(torch, raster.size, offset=offset, salt=4)
            src.put(torch, [raster.reshape(-1)])
            dst = Guarded(torch, want.size, offset=offset, salt=5)
            T.merge_tiles_regions_dev(src.ptr, len(tiles), len(regs), d_table.data_ptr(), dst.ptr)
            (got,), intact = dst.get(torch)
            assert intact, ("K15 wrote outside the packed output", shape, name, offset)
            bad = got != want
            assert not bad.any(), (shape, name, offset, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
            (again,), ok = src.get(torch)  # the input comes back intact
            assert ok and np.array_equal(again, raster.reshape(-1))
            if name.startswith("c"):  # one region: its list is its sub-grid, and the result K10's region merge
                one = Guarded(torch, want.size, offset=offset, salt=6)
                T.merge_tiles_region_dev(src.ptr, *regs[0], one.ptr)
                (merged,), ok = one.get(torch)
                assert ok and np.array_equal(got, merged)
    # a table of another call is refused, not launched
    import frave_amd as fa

    T.regions([(0, 0, 1, 1)])
    with pytest.raises(fa.FriHipError) as e:
        T.merge_tiles_regions_dev(src.ptr, len(tiles), len(regs) + 1, d_table.data_ptr(), dst.ptr)
    assert e.value.code == -1
    T.close()


def test_regions_kernel_replays_from_a_graph_of_one_node(ctx, hip):
    import torch

    shape = (257, 130, 3, 100, 50)
    T = PlanTiled(ctx, *shape, TILED_ALLOW_HOLES)
    regs, tiles, want_table, raster, want = _case(shape, "a: all regions of the region test and a repeat")
    _, table = T.regions(regs)
    d_table = torch.from_numpy(table.view(np.int32).copy()).cuda()
    d_raster = torch.zeros(raster.size, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    T.merge_tiles_regions_dev(d_raster.data_ptr(), len(tiles), len(regs), d_table.data_ptr(), d_out.data_ptr(), stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    n_nodes = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 1
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    torch.cuda.synchronize()
    assert not d_out.cpu().numpy().any(), "capturing ran nothing"
    d_raster.copy_(torch.from_numpy(raster.reshape(-1).copy()))  # one replay, on what the buffer holds now
    torch.cuda.synchronize()
    assert hip.hipGraphLaunch(ex, sp) == 0
    s.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    T.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------

def image_regions(case):
    w, h, c, tw, th = case
    inside = (tw + 10, th + 7, tw - 31, th - 20)
    return [inside, (tw - 5, th - 3, 11, 9), (w - 1, h - 1, 1, 1), inside]  # inside the centre tile, across a tile corner, one pixel in the last tile, a repeat


def modes(c):
    """name -> (colour transform, quality, emitter flags, dequantiser)"""
    if c == 1:
        return {"lossless": (COLOUR_NONE, 0, {}, REFERENCE), "quality 60": (COLOUR_NONE, 60, dict(quality=60), MIDPOINT)}
    return {"lossless": (COLOUR_NONE, 0, {}, REFERENCE), "rct": (COLOUR_RCT, 0, dict(rct=True), REFERENCE), "ycbcr 60": (COLOUR_YCBCR, 60, dict(ycbcr=True, quality=60), MIDPOINT)}


@pytest.mark.parametrize("case", IMAGES, ids=lambda s: "x".join(map(str, s)))
def test_regions_decode_gives_the_crops_of_the_whole_decode(ctx, hip, case):
    import torch

    import frave_amd as fa

    w, h, c, tw, th = case
    img = mixed_image(w, h, c, tw, 3)
    T = PlanTiled(ctx, w, h, c, tw, th)
    assert (T.nx, T.ny) == (3, 3)
    T.set_stream_order()
    s = torch.cuda.Stream()
    regs = image_regions(case)
    tiles = tile_list(w, h, tw, th, regs)
    assert tiles == [0, 1, 3, 4, 8] and T.regions(regs)[0].tolist() == tiles
    total = sum(r[2] * r[3] * c for r in regs)
    for mode, (transform, quality, flags, dequantiser) in modes(c).items():
        T.tile.set_colour_transform(transform)
        T.tile.set_dequantiser(dequantiser)
        qm = fa.quality_matrix(quality) if quality else None
        sym, vp, wp, hist, oob = T.encode_image_tiled_symbols(img, qm)
        assert not oob.any()
        frv = emit.tiled_encode_from_streams(w, h, tw, th, sym, hist, vp, wp, **flags)
        ti, coefs = emit.tiled_decode(frv)
        whole = T.decode_image_tiled(coefs, qm).reshape(h, w, c)
        if not quality:
            assert np.array_equal(whole, img)
        want = [whole[y:y + rh, x:x + rw] for x, y, rw, rh in regs]
        _, part = tiled_decode_tiles(frv, tiles)
        got = T.decode_regions_tiled(part, regs, qm)
        assert len(got) == len(regs)
        for k, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and np.array_equal(a, b), (mode, k)
        # the _dev form on a stream of its own: the same bytes, nothing outside the packed output
        d_coefs = torch.from_numpy(part.reshape(-1).copy()).cuda()
        dst = Guarded(torch, total, offset=1, salt=7)
        torch.cuda.synchronize()
        T.decode_regions_tiled_dev(d_coefs.data_ptr(), regs, dst.ptr, qm, stream=s.cuda_stream)
        s.synchronize()
        (packed,), intact = dst.get(torch)
        assert intact and np.array_equal(packed, np.concatenate([b.reshape(-1) for b in want])), mode
        # the coded route: K13 over the listed tiles' planes, the same bytes, every status 0
        coded = tiled_parse_coded_tiles(frv, tiles)
        got, status = T.decode_regions_coded(coded, regs, qm)
        assert status.shape == (len(tiles) * c, 4) and not status[:, 0].any(), mode
        for k, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), (mode, "coded", k)
    # a capturing stream is refused with nothing enqueued
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    try:
        with pytest.raises(fa.FriHipError) as e:
            T.decode_regions_tiled_dev(d_coefs.data_ptr(), regs, d_out.data_ptr(), stream=s.cuda_stream)
        assert e.value.code == -1 and "graph" in str(e.value)
    finally:
        assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0
    n_nodes = C.c_size_t(12345)
    rc = hip.hipGraphGetNodes(graph, None, C.byref(n_nodes))
    hip.hipGraphDestroy(graph)
    assert rc == 0 and n_nodes.value == 0
    # bad regions, a bad R and null pointers are refused
    for bad in [(0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (0, 1, 1, h), (2**32 - 1, 0, 2, 1)]:
        for call in (lambda: T.regions([regs[0], bad]), lambda: T.decode_regions_tiled_dev(d_coefs.data_ptr(), [bad, regs[0]], d_out.data_ptr()),
                     lambda: T.decode_regions_tiled(part, [regs[0], bad]), lambda: T.decode_regions_coded(coded, [bad])):
            with pytest.raises(fa.FriHipError) as e:
                call()
            assert e.value.code == -1, bad
    for call in (lambda: T.decode_regions_tiled_dev(0, regs, d_out.data_ptr()), lambda: T.decode_regions_tiled_dev(d_coefs.data_ptr(), regs, 0),
                 lambda: T.decode_regions_tiled_dev(d_coefs.data_ptr(), [], d_out.data_ptr())):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -1
    T.close()


def test_a_truncated_listed_plane_is_reported_by_its_tile_in_the_files_grid(ctx):
    import frave_amd as fa
    from tests.test_preview_host import FILES, _file, cut_stream_file

    cut, plane, _ = cut_stream_file()  # 250 x 250 x 1 in 2 x 2 tiles, lossless; tile 1's plane cut to half its words
    w, h, c, tw, th = FILES[0][:5]
    assert (plane, c) == (1, 1)
    T = PlanTiled(ctx, w, h, c, tw, th)
    T.set_stream_order()
    T.tile.set_dequantiser(REFERENCE)
    whole = T.decode_image_tiled(emit.tiled_decode(_file(FILES[0]))[1]).reshape(h, w, c)
    touching = [(tw + 5, 5, 10, 10), (200, 200, 3, 3)]  # tiles 1 and 3: the cut plane is entry 0 of the list
    tiles = T.regions(touching)[0].tolist()
    assert tiles == [1, 3]
    with pytest.raises(emit.EmitError, match="tile 1: channel 0: stream truncated"):
        tiled_decode_tiles(cut, tiles)
    with pytest.raises(fa.FriHipError) as e:
        T.decode_regions_coded(tiled_parse_coded_tiles(cut, tiles), touching)
    assert e.value.code == -1 and e.value.tile == 1 and "tile 1: channel 0" in str(e.value)
    assert e.value.status[0, 0] & DECODE_TRUNCATED and not e.value.status[1, 0]
    # regions that do not touch the damaged tile decode, on both routes
    beside = [(3, 3, 20, 20), (5, th + 5, tw + 20, 30)]  # tiles 0, 2, 3
    tiles = T.regions(beside)[0].tolist()
    assert tiles == [0, 2, 3]
    want = [whole[y:y + rh, x:x + rw] for x, y, rw, rh in beside]
    got, status = T.decode_regions_coded(tiled_parse_coded_tiles(cut, tiles), beside)
    assert not status[:, 0].any() and all(np.array_equal(a, b) for a, b in zip(got, want))
    got = T.decode_regions_tiled(tiled_decode_tiles(cut, tiles)[1], beside)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    T.close()


def test_driver_decodes_several_regions_of_a_tiled_file(ctx, tmp_path):
    """fri_driver decode-regions (FRIDecoder::decode_regions) writes the crops of decode-file's image, with and without --device-rans; a `frif` file, a tiled 4:2:0
    file, a bad region and a missing --region are refused with nothing written"""
    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h = 334, 350
    img = mixed_image(w, h, 3, 167, 8)
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + img.tobytes())
    regs = [(100, 90, 150, 170), (0, 0, 1, 1), (w - 7, h - 5, 7, 5), (100, 90, 150, 170), (140, 140, 20, 20)]  # across tile boundaries, corners, a repeat, an overlap
    region_args = [a for r in regs for a in ("--region", ",".join(map(str, r)))]

    def run(*args):
        return subprocess.run([driver, *map(str, args)], capture_output=True, text=True, timeout=300)

    def written(prefix):
        return sorted(glob.glob(str(prefix) + "*"))

    for name, flags in (("frit", ["--tile-size", "150", "--ycbcr", "--quality", "60"]), ("frit_rct", ["--tile-size", "150", "--rct"])):
        dst, back = tmp_path / f"{name}.frv", tmp_path / f"{name}.ppm"
        out = run("encode-file", src, dst, *flags)
        assert out.returncode == 0, out.stdout + out.stderr
        assert dst.read_bytes()[:4] == b"frit"
        out = run("decode-file", dst, back)
        assert out.returncode == 0, out.stderr
        whole = np.frombuffer(back.read_bytes()[-3 * w * h:], np.uint8).reshape(h, w, 3)
        if name == "frit_rct":
            assert np.array_equal(whole, img)
        for route, extra in (("host", []), ("device", ["--device-rans"])):
            prefix = tmp_path / f"{name}_{route}"
            out = run("decode-regions", dst, prefix, *region_args, *extra)
            assert out.returncode == 0, out.stdout + out.stderr
            assert written(prefix) == [f"{prefix}.{k}.ppm" for k in range(len(regs))]
            for k, (x, y, rw, rh) in enumerate(regs):
                raw = open(f"{prefix}.{k}.ppm", "rb").read()
                assert raw.startswith(b"P6\n%d %d\n255\n" % (rw, rh)) and f"{rw}x{rh}x3" in out.stdout
                assert np.array_equal(np.frombuffer(raw[-3 * rw * rh:], np.uint8).reshape(rh, rw, 3), whole[y:y + rh, x:x + rw]), (name, route, k)
        bad = tmp_path / f"{name}_bad"
        for args in (["--region", f"{w - 1},0,2,1"], ["--region", "0,0,8,8", "--region", "0,0,0,5"], ["--region", "1,2,3"], ["--region", "1,2,3,4,5"], [], ["--device-rans"]):
            out = run("decode-regions", dst, bad, *args)
            assert out.returncode != 0 and not written(bad), (name, args)
        out = run("decode-regions", dst, bad)
        assert "--region" in out.stderr
    # a `frif` file and a tiled 4:2:0 file are refused, and the message says what to use instead
    bad = tmp_path / "refused"
    dst = tmp_path / "plain.frv"
    assert run("encode-file", src, dst, "--ycbcr", "--quality", "60").returncode == 0 and dst.read_bytes()[:4] == b"frif"
    out = run("decode-regions", dst, bad, "--region", "0,0,8,8")
    assert out.returncode != 0 and "decode-file --region" in out.stderr and not written(bad)
    dst = tmp_path / "s420.frv"
    assert run("encode-file", src, dst, "--tile-size-420", "150", "--quality", "60").returncode == 0 and dst.read_bytes()[:4] == b"frit"
    out = run("decode-regions", dst, bad, "--region", "0,0,8,8")
    assert out.returncode != 0 and "4:2:0" in out.stderr and "decode-file --region" in out.stderr and not written(bad)
