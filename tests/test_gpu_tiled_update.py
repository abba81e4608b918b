"""Region update on the device (K10's split_tiles_region_kernel, fri_hip_split_tiles_region_dev, fri_hip_encode_symbols_region_tiled_dev,
fri_hip_encode_region_tiled_symbols) against tests/tiled_update_ref.py:

- the region split exactly equal to the per-pixel restatement on the shapes of the split and merge tests - tile rows shorter than a 16-byte strip, a tile larger
  than the image, a replicated right and bottom edge, more than one workgroup - for the regions of tests/test_gpu_tiled_region.py; both source forms, the whole
  raster and a staged copy of the covered rectangle alone (and that copy with a row pitch of its own); random image bytes; device pointers 0, 1 and 3 bytes off a
  256-byte boundary, between guard bytes; for the whole-image region the result is fri_hip_split_tiles_dev's;
- a replay from a captured graph of the one kernel node;
- the region encode against the sub-grid's rows of the whole-image encode, bit for bit: symbols, histograms, parameters, out-of-alphabet counts; the _dev form on
  a stream of its own; a capturing stream and a plan without its stream order refused;
- end to end: the device region encode + fri_tiled_update_from_streams on the file of A is the file of B; fri_driver update-file writes the same bytes."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import frave_amd.emit as emit
from frave_amd.api import TILED_ALLOW_HOLES, PlanTiled
from tests.test_gpu_instances import Guarded
from tests.test_gpu_tiled_region import COLOUR_NONE, COLOUR_YCBCR, IMAGES, RELAXED, SHAPES, kernel_regions
from tests.tiled_ref import grid, mixed_image, split_tiles
from tests.tiled_region_ref import region_tiles, sub_grid
from tests.tiled_update_ref import region_cover, split_region, split_region_fast, sub_tiles

# (without the feature the module fails here)
split_tiles_region_dev, encode_region_tiled_symbols, tiled_update_from_streams = PlanTiled.split_tiles_region_dev, PlanTiled.encode_region_tiled_symbols, emit.tiled_update_from_streams

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
def _raster(shape):
    """random image bytes [H][W][C] and the whole split of them, computed once"""
    w, h, c, tw, th = shape
    img = np.random.default_rng([w, h, c, tw, th]).integers(0, 256, (h, w, c), dtype=np.uint8)
    whole = split_tiles(img, tw, th)
    img.setflags(write=False), whole.setflags(write=False)
    return img, whole


@functools.lru_cache(maxsize=None)
def _want(shape, region):
    """the sub-grid's tile raster by the per-pixel restatement (by its index-array form on the one large shape, which tests/test_tiled_update_host.py holds to it)"""
    w, h, c, tw, th = shape
    img, whole = _raster(shape)
    want = (split_region if w * h <= 40000 else split_region_fast)(img, tw, th, *region)
    i0, j0, ni, nj = region_tiles(w, h, tw, th, *region)
    assert np.array_equal(want, sub_grid(whole, grid(w, h, tw, th)[0], i0, j0, ni, nj))  # by definition the sub-grid's rows of the split
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_region_split_equals_the_restatement(ctx, shape):
    import torch

    w, h, c, tw, th = shape
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    img, whole = _raster(shape)
    for offset in (0, 1, 3):
        raster = Guarded(torch, img.size, offset=offset, salt=4)  # the whole raster on the device: only read, by every region
        raster.put(torch, [img.reshape(-1)])
        for name, region in kernel_regions(shape).items():
            want = _want(shape, region)
            cx, cy, cw, ch = cover = region_cover(w, h, tw, th, *region)
            assert T.region_cover(*region) == cover
            crop = np.ascontiguousarray(img[cy:cy + ch, cx:cx + cw])
            staged = Guarded(torch, crop.size, offset=offset, salt=5)  # the covered rectangle alone: a read outside it meets guard bytes
            staged.put(torch, [crop.reshape(-1)])
            pitch = cw * c + 5
            pitched = Guarded(torch, cw * c, n_images=ch, stride=pitch, offset=offset, salt=6)  # ... and with a row pitch of its own
            pitched.put(torch, list(crop.reshape(ch, cw * c)))
            for form, src, source in (("whole raster", raster, (w * c, 0, 0, w, h)), ("staged cover", staged, (cw * c, cx, cy, cw, ch)), ("pitched cover", pitched, (pitch, cx, cy, cw, ch))):
                dst = Guarded(torch, want.size, offset=offset, salt=7)
                T.split_tiles_region_dev(src.ptr, *source, *region, dst.ptr)
                (got,), intact = dst.get(torch)
                assert intact, ("the region split wrote outside the sub-grid's tile raster", shape, name, form, offset)
                bad = got != want.reshape(-1)
                assert not bad.any(), (shape, name, form, offset, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
            for src, data in ((staged, [crop.reshape(-1)]), (pitched, list(crop.reshape(ch, cw * c)))):  # the sources come back intact
                back, ok = src.get(torch)
                assert ok and all(np.array_equal(a, b) for a, b in zip(back, data))
            if name == "whole image":  # the sub-grid is the grid: what the split gives
                assert np.array_equal(want, whole)
                full = Guarded(torch, whole.size, offset=offset, salt=8)
                T.split_tiles_dev(raster.ptr, full.ptr)
                (split,), ok = full.get(torch)
                assert ok and np.array_equal(split, got)
        (again,), ok = raster.get(torch)
        assert ok and np.array_equal(again, img.reshape(-1))
    T.close()


def test_region_split_replays_from_a_graph_of_one_node(ctx, hip):
    import torch

    shape = (257, 130, 3, 100, 50)
    w, h, c, tw, th = shape
    region = kernel_regions(shape)["interior, off the strip grid"]
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    img, _ = _raster(shape)
    want = _want(shape, region)
    d_img = torch.zeros(img.size, dtype=torch.uint8, device="cuda")
    d_out = torch.full((want.size,), 255, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    T.split_tiles_region_dev(d_img.data_ptr(), w * c, 0, 0, w, h, *region, d_out.data_ptr(), stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    n_nodes = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 1
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 255).all(), "capturing ran the kernel"
    d_img.copy_(torch.from_numpy(img.reshape(-1).copy()))  # one replay, on what the buffer holds now
    torch.cuda.synchronize()
    assert hip.hipGraphLaunch(ex, sp) == 0
    s.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want.reshape(-1))
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    T.close()


# ---- the region encode -------------------------------------------------------------------------------------------------------------------------------------

def encode_regions(case):
    """an interior tile, an edge sub-grid (the last, partial column: its right edge is replicated) and the whole grid"""
    w, h, c, tw, th = case
    return {"interior tile": (tw + 5, th + 7, 3, 2), "last column": (w - 2, 1, 2, h - 1), "bottom right 2 x 2": (2 * tw - 1, 2 * th - 1, 2, 2), "whole grid": (0, 0, w, h)}


def encode_modes(c):
    """name -> (colour transform, quality, emitter flags): lossless, and YCbCr at a quality"""
    if c == 1:
        return {"lossless": (COLOUR_NONE, 0, {})}
    return {"lossless": (COLOUR_NONE, 0, {}), "ycbcr 50": (COLOUR_YCBCR, 50, dict(ycbcr=True, quality=50))}


@pytest.mark.parametrize("case", IMAGES, ids=lambda s: "x".join(map(str, s)))
def test_region_encode_is_the_sub_grids_rows_of_the_whole_encode(ctx, hip, case):
    import torch

    import frave_amd as fa

    w, h, c, tw, th = case
    img = mixed_image(w, h, c, tw, 3)
    T = PlanTiled(ctx, w, h, c, tw, th)
    assert (T.nx, T.ny) == (3, 3)
    # without the stream order the encode is refused
    with pytest.raises(fa.FriHipError) as e:
        T.encode_region_tiled_symbols(img, 0, 0, 1, 1)
    assert e.value.code == -1
    T.set_stream_order()
    s = torch.cuda.Stream()
    n = T.num_some
    for mode, (transform, quality, flags) in encode_modes(c).items():
        T.tile.set_colour_transform(transform)
        qm = fa.quality_matrix(quality) if quality else None
        whole = T.encode_image_tiled_symbols(img, qm)  # (symbols, value_params, width_params, hist, oob), tile after tile
        assert not whole[4].any()
        for name, region in encode_regions(case).items():
            tiles = region_tiles(w, h, tw, th, *region)
            touched = sub_tiles(T.nx, *tiles)
            assert T.region_tiles(*region) == tiles and len(touched) == {"interior tile": 1, "last column": 3, "bottom right 2 x 2": 4, "whole grid": 9}[name]
            got = T.encode_region_tiled_symbols(img, *region, qm)
            for k, what in enumerate(("symbols", "value parameters", "width parameters", "histograms", "out-of-alphabet counts")):
                assert got[k].shape == whole[k][touched].shape and np.array_equal(got[k].view(np.uint8), np.ascontiguousarray(whole[k][touched]).view(np.uint8)), (mode, name, what)
            # the _dev form on a stream of its own, from the whole raster on the device: the same bits, nothing outside the outputs
            k_sub = len(touched)
            d_img = torch.from_numpy(img.reshape(-1).copy()).cuda()
            d_params = Guarded(torch, k_sub * c * 36 * 4, offset=0, salt=9)
            d_sym = Guarded(torch, k_sub * c * n * 2, offset=0, salt=10)
            d_hist = torch.zeros(k_sub * c * 10 * 1024, dtype=torch.int32, device="cuda")
            d_oob = torch.zeros(2 * k_sub * c, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            T.encode_symbols_region_tiled_dev(d_img.data_ptr(), w * c, 0, 0, w, h, *region, d_params.ptr, d_sym.ptr, d_hist.data_ptr(), d_oob.data_ptr(),
                                              d_oob.data_ptr() + 8 * k_sub * c, qm, stream=s.cuda_stream)
            s.synchronize()
            (params,), ok_p = d_params.get(torch)
            (sym,), ok_s = d_sym.get(torch)
            assert ok_p and ok_s, (mode, name)
            params = params.view(np.float32).reshape(k_sub, c, 2, 3, 6)
            assert np.array_equal(sym.view(np.uint16).reshape(k_sub, c, n), got[0]), (mode, name)
            assert np.array_equal(params[:, :, 0].view(np.uint32), got[1].view(np.uint32)) and np.array_equal(params[:, :, 1].view(np.uint32), got[2].view(np.uint32)), (mode, name)
            assert np.array_equal(d_hist.cpu().numpy().view(np.uint32).reshape(k_sub, c, 10, 1024), got[3]), (mode, name)
            assert not d_oob.cpu().numpy().any()
    # a capturing stream is refused with the graph left empty
    region = encode_regions(case)["interior tile"]
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    try:
        with pytest.raises(fa.FriHipError) as e:
            T.encode_symbols_region_tiled_dev(d_img.data_ptr(), w * c, 0, 0, w, h, *region, d_params.ptr, d_sym.ptr, d_hist.data_ptr(), d_oob.data_ptr(), None, stream=s.cuda_stream)
        assert e.value.code == -1 and "graph" in str(e.value)
    finally:
        assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0
    n_nodes = C.c_size_t(12345)
    rc = hip.hipGraphGetNodes(graph, None, C.byref(n_nodes))
    hip.hipGraphDestroy(graph)
    assert rc == 0 and n_nodes.value == 0
    T.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", IMAGES, ids=lambda s: "x".join(map(str, s)))
def test_region_update_of_the_file_of_a_gives_the_file_of_b(ctx, case):
    import frave_amd as fa

    w, h, c, tw, th = case
    img_a, other = mixed_image(w, h, c, tw, 3), mixed_image(w, h, c, tw, 11)
    T = PlanTiled(ctx, w, h, c, tw, th)
    T.set_stream_order()
    for mode, (transform, quality, flags) in encode_modes(c).items():
        T.tile.set_colour_transform(transform)
        qm = fa.quality_matrix(quality) if quality else None
        sym, vp, wp, hist, oob = T.encode_image_tiled_symbols(img_a, qm)
        file_a = emit.tiled_encode_from_streams(w, h, tw, th, sym, hist, vp, wp, **flags)
        for name, region in encode_regions(case).items():
            cx, cy, cw, ch = region_cover(w, h, tw, th, *region)
            img_b = img_a.copy()  # B differs from A inside the covered rectangle only - everywhere in it, the replicated edge's source pixels among it
            img_b[cy:cy + ch, cx:cx + cw] = other[cy:cy + ch, cx:cx + cw]
            sym, vp, wp, hist, oob = T.encode_image_tiled_symbols(img_b, qm)
            file_b = emit.tiled_encode_from_streams(w, h, tw, th, sym, hist, vp, wp, **flags)
            assert file_b != file_a
            sym, vp, wp, hist, oob = T.encode_region_tiled_symbols(img_b, *region, qm)
            assert not oob.any()
            got, tiles = tiled_update_from_streams(file_a, *region, sym, hist, vp, wp, **flags)
            assert tiles == region_tiles(w, h, tw, th, *region) and got == file_b, (mode, name)
    T.close()


def test_driver_updates_a_file_and_refuses_what_it_must(ctx, tmp_path):
    """fri_driver update-file writes the bytes encode-file writes for the new image, and the bytes of the Python route; a `frif` file, a tiled 4:2:0 file, an image of
    another size or channel count and a missing --region are refused, and the error says what to do instead"""
    import frave_amd as fa

    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h = 334, 350
    img_a, other = mixed_image(w, h, 3, 167, 8), mixed_image(w, h, 3, 167, 12)

    def ppm(name, img):
        path = tmp_path / name
        hh, ww, cc = img.shape
        path.write_bytes((b"P6\n%d %d\n255\n" if cc == 3 else b"P5\n%d %d\n255\n") % (ww, hh) + img.tobytes())
        return path

    def run(*args):
        return subprocess.run([driver, *map(str, args)], capture_output=True, text=True, timeout=300)

    src_a = ppm("a.ppm", img_a)
    for name, flags, transform, quality, emit_flags in (("ycbcr", ["--ycbcr", "--quality", "60"], COLOUR_YCBCR, 60, dict(ycbcr=True, quality=60)), ("lossless", [], COLOUR_NONE, 0, {})):
        file_a = tmp_path / f"{name}_a.frv"
        out = run("encode-file", src_a, file_a, "--tile-size", "150", *flags)
        assert out.returncode == 0, out.stdout + out.stderr
        ti = emit.tiled_info(file_a.read_bytes())
        tw, th = ti[2], ti[3]
        region = (tw - 7, 10, 20, 30)  # across the boundary between the first two tile columns, inside the first tile row
        cx, cy, cw, ch = region_cover(w, h, tw, th, *region)
        assert ti[4] * ti[5] > 2 and region_tiles(w, h, tw, th, *region) == (0, 0, 2, 1)
        img_b = img_a.copy()
        img_b[cy:cy + ch, cx:cx + cw] = other[cy:cy + ch, cx:cx + cw]
        src_b = ppm(f"{name}_b.ppm", img_b)
        file_b, updated = tmp_path / f"{name}_b.frv", tmp_path / f"{name}_updated.frv"
        assert run("encode-file", src_b, file_b, "--tile-size", "150", *flags).returncode == 0
        out = run("update-file", file_a, src_b, updated, "--region", "%d,%d,%d,%d" % region)
        assert out.returncode == 0 and "self-check" in out.stdout, out.stdout + out.stderr
        assert updated.read_bytes() == file_b.read_bytes() != file_a.read_bytes(), name
        # the Python route on the same file: the same bytes
        T = PlanTiled(ctx, w, h, 3, tw, th)
        T.set_stream_order()
        T.tile.set_colour_transform(transform)
        sym, vp, wp, hist, oob = T.encode_region_tiled_symbols(img_b, *region, fa.quality_matrix(quality) if quality else None)
        assert tiled_update_from_streams(file_a.read_bytes(), *region, sym, hist, vp, wp, **emit_flags)[0] == updated.read_bytes()
        T.close()
        # a whole-image region: the whole encode of the other image
        src_o, file_o = ppm("other.ppm", other), tmp_path / f"{name}_other.frv"
        assert run("encode-file", src_o, file_o, "--tile-size", "150", *flags).returncode == 0
        assert run("update-file", file_a, src_o, updated, "--region", f"0,0,{w},{h}").returncode == 0
        assert updated.read_bytes() == file_o.read_bytes()
    # the refusals: nothing is written, and the message says what to do instead
    bad = tmp_path / "bad.frv"
    frif, s420 = tmp_path / "plain.frv", tmp_path / "s420.frv"
    assert run("encode-file", src_a, frif, "--quality", "60").returncode == 0
    assert run("encode-file", src_a, s420, "--tile-size-420", "150", "--quality", "60").returncode == 0
    grey, small = ppm("grey.pgm", img_a[:, :, :1].copy()), ppm("small.ppm", img_a[:-1].copy())
    for args, words in (((frif, src_a, bad, "--region", "0,0,8,8"), ("frif", "encode-file")), ((s420, src_a, bad, "--region", "0,0,8,8"), ("4:2:0", "re-encoded whole")),
                        ((file_a, small, bad, "--region", "0,0,8,8"), ("size", "whole")), ((file_a, grey, bad, "--region", "0,0,8,8"), ("channel", "convert")),
                        ((file_a, src_a, bad), ("--region", "encode-file")), ((file_a, src_a, bad, "--region", f"{w - 1},0,2,1"), ("invalid region",)),
                        ((file_a, src_a, bad, "--region", "0,0,8,8", "--quality", "50"), ("no mode flags",))):
        out = run("update-file", *args)
        assert out.returncode != 0 and not bad.exists() and all(word in out.stderr for word in words), (args[3:], out.stderr)
