"""Region decode on the device (K10's merge_tiles_region_kernel, fri_hip_decode_region_tiled*) against tests/tiled_region_ref.py:

- the region kernel exactly equal to the per-pixel restatement on the shapes of the split and merge tests - tile rows shorter than a 16-byte strip, a tile larger
  than the image, more than one workgroup - for the whole image (which is the merge), single pixels in the corners, an interior rectangle off the 16-byte grid with
  a partial last strip, a region whose strips straddle every tile column, the last row and the last column; random tile bytes, so that a byte of the wrong tile or
  of a replicated row shows; device pointers 0, 1 and 3 bytes off a 256-byte boundary, between guard bytes;
- a replay from a captured graph of the one kernel node;
- end to end: fri_tiled_decode_region + fri_hip_decode_region_tiled is the crop of fri_tiled_decode + fri_hip_decode_image_tiled, the _dev form on a stream of
  its own, a capturing stream and bad regions refused;
- fri_driver decode-file --region on a `frit` and a `frif` file."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import frave_amd.emit as emit
from frave_amd.api import TILED_ALLOW_HOLES, PlanTiled
from tests.common import gen_image
from tests.oracle_ref import MIDPOINT, REFERENCE
from tests.test_gpu_instances import Guarded
from tests.tiled_ref import grid, merge_tiles, mixed_image
from tests.tiled_region_ref import merge_region, region_tiles

plan_region_tiles, tiled_decode_region = PlanTiled.region_tiles, emit.tiled_decode_region  # (without the feature the module fails here)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELAXED = 2  # hipStreamCaptureModeRelaxed
COLOUR_NONE, COLOUR_RCT, COLOUR_YCBCR = 0, 1, 3
# (W, H, C, tile_w, tile_h)
SHAPES = [(5, 3, 3, 2, 2), (17, 9, 1, 16, 4), (33, 20, 3, 16, 16), (50, 40, 1, 64, 64), (257, 130, 3, 100, 50), (1023, 767, 3, 512, 512)]
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


def kernel_regions(shape):
    """name -> (x, y, w, h): the regions of one shape, each with the property its name states (asserted here, not assumed)"""
    w, h, c, tw, th = shape
    nx, ny = grid(w, h, tw, th)
    out = {"whole image": (0, 0, w, h)}
    for name, x, y in (("top left", 0, 0), ("top right", w - 1, 0), ("bottom left", 0, h - 1), ("bottom right", w - 1, h - 1)):
        out["one pixel " + name] = (x, y, 1, 1)
    # an interior rectangle whose left byte offset is no multiple of 16 and whose rows end in a partial strip
    x, y = 1 + w // 7, min(1 + h // 7, h - 1)
    while x * c % 16 == 0:
        x += 1
    rw = max(1, (w - 1 - x) * 2 // 3)
    while rw * c % 16 == 0:
        rw -= 1
    rh = max(1, (h - y) // 2)
    assert 0 < x and x + rw < w and y + rh <= h and (x * c) % 16 and (rw * c) % 16
    out["interior, off the strip grid"] = (x, y, rw, rh)
    # full-width rows from an x at which no tile column starts on a strip boundary of the region: a strip straddles every tile column; three rows across the
    # first boundary between tile rows (or the image's last rows)
    x = next(x for x in range(1, 17) if all(((i * tw - x) * c) % 16 for i in range(1, nx)) and x < min(tw, w))
    y = max(0, min(th, h - 1) - 1)
    rh = min(3, h - y)
    assert region_tiles(w, h, tw, th, x, y, w - x, rh)[2] == nx
    out["straddles every tile column"] = (x, y, w - x, rh)
    out["last row"] = (0, h - 1, w, 1)
    out["last column"] = (w - 1, 0, 1, h)
    return out


@functools.lru_cache(maxsize=None)
def _sub_grid_bytes(shape, region):
    """random bytes for the sub-grid's tile raster [nj ni][tile_h][tile_w][C], and the region raster the restatement makes of them"""
    w, h, c, tw, th = shape
    i0, j0, ni, nj = region_tiles(w, h, tw, th, *region)
    sub = np.random.default_rng([w, h, *region]).integers(0, 256, (nj * ni, th, tw, c), dtype=np.uint8)
    want = merge_region(sub, tw, th, i0, j0, ni, *region)
    sub.setflags(write=False), want.setflags(write=False)
    return sub, want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_region_kernel_equals_the_restatement(ctx, shape):
    import torch

    w, h, c, tw, th = shape
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    for name, region in kernel_regions(shape).items():
        x, y, rw, rh = region
        assert T.region_tiles(*region) == region_tiles(w, h, tw, th, *region)
        sub, want = _sub_grid_bytes(shape, region)
        if name == "whole image":  # the sub-grid is the grid, and the region raster what the merge gives
            assert np.array_equal(want, merge_tiles(sub, w, h))
        for offset in (0, 1, 3):
            src = Guarded(torch, sub.size, offset=offset, salt=4)
            src.put(torch, [sub.reshape(-1)])
            dst = Guarded(torch, want.size, offset=offset, salt=5)
            T.merge_tiles_region_dev(src.ptr, x, y, rw, rh, dst.ptr)
            (got,), intact = dst.get(torch)
            assert intact, ("the region kernel wrote outside the region raster", shape, name, offset)
            bad = got != want.reshape(-1)
            assert not bad.any(), (shape, name, offset, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
            if name == "whole image":
                back = Guarded(torch, want.size, offset=offset, salt=6)
                T.merge_tiles_dev(src.ptr, back.ptr)
                (merged,), ok = back.get(torch)
                assert ok and np.array_equal(got, merged)
            (again,), ok = src.get(torch)  # the input comes back intact
            assert ok and np.array_equal(again, sub.reshape(-1))
    T.close()


def test_region_kernel_replays_from_a_graph_of_one_node(ctx, hip):
    import torch

    shape = (257, 130, 3, 100, 50)
    w, h, c, tw, th = shape
    region = kernel_regions(shape)["interior, off the strip grid"]
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    sub, want = _sub_grid_bytes(shape, region)
    d_sub = torch.zeros(sub.size, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    T.merge_tiles_region_dev(d_sub.data_ptr(), *region, d_out.data_ptr(), stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    n_nodes = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 1
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    torch.cuda.synchronize()
    assert not d_out.cpu().numpy().any(), "capturing ran nothing"
    d_sub.copy_(torch.from_numpy(sub.reshape(-1).copy()))  # one replay, on what the buffer holds now
    torch.cuda.synchronize()
    assert hip.hipGraphLaunch(ex, sp) == 0
    s.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want.reshape(-1))
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    T.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------

def image_regions(case):
    w, h, c, tw, th = case
    return {
        "centre tile": (tw, th, tw, th),
        "one pixel in a corner tile": (w - 1, h - 1, 1, 1),
        "across all nine": (tw - 3, th - 2, tw + 7, th + 5),
        "last partial column": (2 * tw, 0, w - 2 * tw, h),
        "whole image": (0, 0, w, h),
    }


def modes(c):
    """name -> (colour transform, quality, emitter flags, dequantiser)"""
    if c == 1:
        return {"lossless": (COLOUR_NONE, 0, {}, REFERENCE), "quality 50": (COLOUR_NONE, 50, dict(quality=50), MIDPOINT)}
    return {"lossless": (COLOUR_NONE, 0, {}, REFERENCE), "rct": (COLOUR_RCT, 0, dict(rct=True), REFERENCE), "ycbcr 50": (COLOUR_YCBCR, 50, dict(ycbcr=True, quality=50), MIDPOINT)}


@pytest.mark.parametrize("case", IMAGES, ids=lambda s: "x".join(map(str, s)))
def test_region_decode_is_the_crop_of_the_whole_decode(ctx, hip, case):
    import torch

    import frave_amd as fa

    w, h, c, tw, th = case
    img = mixed_image(w, h, c, tw, 3)
    T = PlanTiled(ctx, w, h, c, tw, th)
    assert (T.nx, T.ny) == (3, 3)
    T.set_stream_order()
    s = torch.cuda.Stream()
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
        for name, (x, y, rw, rh) in image_regions(case).items():
            want = whole[y:y + rh, x:x + rw].reshape(-1)
            info, tiles, part = tiled_decode_region(frv, x, y, rw, rh)
            assert tiles == region_tiles(w, h, tw, th, x, y, rw, rh) == T.region_tiles(x, y, rw, rh)
            got = T.decode_region_tiled(part, x, y, rw, rh, qm)
            assert np.array_equal(got, want), (mode, name)
            # the _dev form on a stream of its own: the same bytes, nothing outside the region raster
            d_coefs = torch.from_numpy(part.reshape(-1).copy()).cuda()
            dst = Guarded(torch, want.size, offset=1, salt=7)
            torch.cuda.synchronize()
            T.decode_region_tiled_dev(d_coefs.data_ptr(), x, y, rw, rh, dst.ptr, qm, stream=s.cuda_stream)
            s.synchronize()
            (got,), intact = dst.get(torch)
            assert intact and np.array_equal(got, want), (mode, name)
    # a capturing stream is refused with nothing enqueued
    x, y, rw, rh = image_regions(case)["centre tile"]
    d_out = torch.zeros(rw * rh * c, dtype=torch.uint8, device="cuda")
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    try:
        with pytest.raises(fa.FriHipError) as e:
            T.decode_region_tiled_dev(d_coefs.data_ptr(), x, y, rw, rh, d_out.data_ptr(), stream=s.cuda_stream)
        assert e.value.code == -1 and "graph" in str(e.value)
    finally:
        assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0
    n_nodes = C.c_size_t(12345)
    rc = hip.hipGraphGetNodes(graph, None, C.byref(n_nodes))
    hip.hipGraphDestroy(graph)
    assert rc == 0 and n_nodes.value == 0
    # bad regions and null pointers are refused
    one = np.zeros(c * T.num_cells * 512, np.int32)
    for bad in [(0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (0, 1, 1, h), (2**32 - 1, 0, 2, 1)]:
        for call in (lambda: T.region_tiles(*bad), lambda: T.decode_region_tiled_dev(d_coefs.data_ptr(), *bad, d_out.data_ptr()),
                     lambda: T.merge_tiles_region_dev(d_out.data_ptr(), *bad, d_out.data_ptr()),
                     lambda: fa.load_library().fri_hip_decode_region_tiled(T._h, one.ctypes.data, fa.quality_matrix(50).ctypes.data, *bad, one.ctypes.data)):
            try:
                rc = call()
            except fa.FriHipError as e:
                rc = e.code
            assert rc == -1, bad
    for call in (lambda: T.merge_tiles_region_dev(0, 0, 0, 1, 1, d_out.data_ptr()), lambda: T.merge_tiles_region_dev(d_out.data_ptr(), 0, 0, 1, 1, 0),
                 lambda: T.decode_region_tiled_dev(0, 0, 0, 1, 1, d_out.data_ptr()), lambda: T.decode_region_tiled_dev(d_coefs.data_ptr(), 0, 0, 1, 1, 0)):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -1
    T.close()


def test_driver_decodes_a_region_of_a_tiled_and_of_an_ordinary_file(ctx, tmp_path):
    """fri_driver decode-file --region (FRIDecoder::decode_region) writes the crop of decode-file's image: a `frit` file through the region route, a `frif` file
    decoded whole and cropped; a 4:2:0 file and a region that leaves the image are refused"""
    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h = 334, 350
    img = mixed_image(w, h, 3, 167, 8)
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + img.tobytes())
    x, y, rw, rh = 100, 90, 150, 170  # across tile boundaries in both directions

    def run(*args):
        return subprocess.run([driver, *map(str, args)], capture_output=True, text=True, timeout=300)

    for name, flags in (("frit", ["--tile-size", "150", "--ycbcr", "--quality", "60"]), ("frif", ["--ycbcr", "--quality", "60"]), ("frit_rct", ["--tile-size", "150", "--rct"])):
        dst, back, part = tmp_path / f"{name}.frv", tmp_path / f"{name}.ppm", tmp_path / f"{name}_part.ppm"
        out = run("encode-file", src, dst, *flags)
        assert out.returncode == 0, out.stdout + out.stderr
        assert dst.read_bytes()[:4] == (b"frit" if name.startswith("frit") else b"frif")
        out = run("decode-file", dst, back)
        assert out.returncode == 0, out.stderr
        whole = np.frombuffer(back.read_bytes()[-3 * w * h:], np.uint8).reshape(h, w, 3)
        out = run("decode-file", dst, part, "--region", f"{x},{y},{rw},{rh}")
        assert out.returncode == 0 and f"{rw}x{rh}x3" in out.stdout, out.stdout + out.stderr
        raw = part.read_bytes()
        assert raw.startswith(b"P6\n%d %d\n255\n" % (rw, rh))
        assert np.array_equal(np.frombuffer(raw[-3 * rw * rh:], np.uint8).reshape(rh, rw, 3), whole[y:y + rh, x:x + rw]), name
        if name == "frit_rct":
            assert np.array_equal(whole, img)
        for bad in (f"{w - 1},0,2,1", "0,0,0,5", "1,2,3", "1,2,3,4,5"):
            out = run("decode-file", dst, tmp_path / "bad.ppm", "--region", bad)
            assert out.returncode != 0 and not (tmp_path / "bad.ppm").exists(), (name, bad)
    dst = tmp_path / "s420.frv"
    assert run("encode-file", src, dst, "--420", "--quality", "60").returncode == 0
    out = run("decode-file", dst, tmp_path / "bad.ppm", "--region", "0,0,8,8")
    assert out.returncode != 0 and "4:2:0" in out.stderr and not (tmp_path / "bad.ppm").exists()
