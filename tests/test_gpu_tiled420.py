"""Tiled 4:2:0 coding on the device (K12: split_tiles420_kernel, merge_tiles420_region_kernel; fri_hip_*_tiled420*) against tests/tiled420_ref.py:

- the split and the whole merge exactly equal to the numpy composition on the smallest shapes that reach every path, device pointers 0, 1 and 3 bytes off a
  256-byte boundary between guard bytes; the merge also on random planes, whose replicated pixels hold other values; the inputs come back intact;
- the region merge equal to the crop of the whole merge;
- split and merge replayed from a captured graph on two images;
- the encode equal, plane by plane, to Plan420.encode_image420_symbols of each numpy-split tile, and the `frit` file equal to the container of the per-tile files;
- the decode equal to the numpy merge of each tile's Plan420.decode_image420, the region decodes equal to its crops, the plan's buffers at the region's size;
- fri_driver encode-file --tile-size-420, decode-file and --region."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import frave_amd.emit as emit
from frave_amd.api import TILED_ALLOW_HOLES, Plan420, PlanTiled420, tile_shape420  # noqa: F401  (without the feature the module fails here)
from tests.chroma420_ref import chroma_shape
from tests.common import gen_image
from tests.test_gpu_instances import Guarded
from tests.tiled420_ref import grid, merge_tiles420, plane_index, split_tiles420
from tests.tiled_ref import merge_tiles, mixed_image, parse_frit, split_tiles

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELAXED = 2  # hipStreamCaptureModeRelaxed
# (W, H, tile_w, tile_h)
SHAPES = [(1, 1, 1, 1), (5, 3, 2, 2), (17, 9, 16, 4), (33, 20, 16, 16), (35, 23, 17, 9), (40, 33, 5, 3), (50, 40, 64, 64), (257, 130, 100, 50), (1023, 767, 512, 512)]
REGION_SHAPES = [(257, 130, 100, 50), (40, 33, 5, 3)]
IMAGE = (334, 350, 167, 175)  # 2 x 2 tiles of fri_hip_tile_shape420(334, 350, 150)
QUALITY = 60


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
def _reference(shape):
    """(image, y_tiles, c_tiles, merged image of those planes, random planes, their merged image) - computed once, read-only"""
    w, h, tw, th = shape
    img = gen_image("noise", w, h, 3, w + 7 * h)
    y, c = split_tiles420(img, tw, th)
    rng = np.random.default_rng([w, h, tw, th])
    ry, rc = rng.integers(0, 256, y.shape, dtype=np.uint8), rng.integers(0, 256, c.shape, dtype=np.uint8)
    out = (img, y, c, merge_tiles420(y, c, w, h), ry, rc, merge_tiles420(ry, rc, w, h))
    for a in out:
        a.setflags(write=False)
    return out


def regions_of(shape):
    """name -> (x, y, w, h), each with the property its name states (asserted here, not assumed)"""
    w, h, tw, th = shape
    nx, ny = grid(w, h, tw, th)
    out = {"one pixel": (w - 1, h - 1, 1, 1), "whole image": (0, 0, w, h), "last row": (0, h - 1, w, 1), "last column": (w - 1, 0, 1, h)}
    x, y = tw + 1 + 2 * (tw > 3), th + 1  # an odd tile column and row, inside tile (1, 1)
    rw, rh = min(tw - (x - tw), 21), min(th - (y - th), 5)
    assert (x - tw) % 2 == 1 and (y - th) % 2 == 1 and x // tw == (x + rw - 1) // tw == 1 and y // th == (y + rh - 1) // th == 1
    out["odd origin inside a tile"] = (x, y, rw, rh)
    x, y = tw - 3 if tw > 3 else tw - 1, th - 1
    rw, rh = min(w - x, tw + 40), min(h - y, th + 2)
    assert x // tw < (x + rw - 1) // tw and y // th < (y + rh - 1) // th
    out["across a tile column and a tile row"] = (x, y, rw, rh)
    return out


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_and_whole_merge_equal_the_numpy_composition(ctx, shape):
    import torch

    w, h, tw, th = shape
    img, y, c, merged, ry, rc, rmerged = _reference(shape)
    T = PlanTiled420(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    assert (T.y_tile_bytes, T.c_tile_bytes) == (y.size, c.size)
    for offset in (0, 1, 3):
        src = Guarded(torch, img.size, offset=offset, salt=1)
        src.put(torch, [img.reshape(-1)])
        dy, dc = Guarded(torch, y.size, offset=offset, salt=2), Guarded(torch, c.size, offset=offset, salt=3)
        T.split_tiles420_dev(src.ptr, dy.ptr, dc.ptr)
        (gy,), ok_y = dy.get(torch)
        (gc,), ok_c = dc.get(torch)
        assert ok_y and ok_c, ("the split wrote outside its planes", shape, offset)
        bad = gy != y.reshape(-1)
        assert not bad.any(), ("y_tiles", shape, offset, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
        bad = gc != c.reshape(-1)
        assert not bad.any(), ("c_tiles", shape, offset, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
        (again,), ok = src.get(torch)
        assert ok and np.array_equal(again, img.reshape(-1))
        # the merge of what the split wrote, and of random planes (replicated pixels hold other values: none of them may show)
        for planes_y, planes_c, want, salt in ((y, c, merged, 4), (ry, rc, rmerged, 7)):
            sy, sc = Guarded(torch, y.size, offset=offset, salt=salt), Guarded(torch, c.size, offset=offset, salt=salt + 1)
            sy.put(torch, [planes_y.reshape(-1)])
            sc.put(torch, [planes_c.reshape(-1)])
            dst = Guarded(torch, want.size, offset=offset, salt=salt + 2)
            T.merge_tiles420_dev(sy.ptr, sc.ptr, dst.ptr)
            (got,), intact = dst.get(torch)
            assert intact, ("the merge wrote outside the raster", shape, offset)
            bad = got != want.reshape(-1)
            assert not bad.any(), ("merge", shape, offset, salt, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
            (ay,), ok_y = sy.get(torch)
            (ac,), ok_c = sc.get(torch)
            assert ok_y and ok_c and np.array_equal(ay, planes_y.reshape(-1)) and np.array_equal(ac, planes_c.reshape(-1))
    T.close()


@pytest.mark.parametrize("shape", REGION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_region_merge_is_the_crop_of_the_whole_merge(ctx, shape):
    import torch

    from tests.tiled420_ref import sub_grid

    w, h, tw, th = shape
    img, y, c, merged, ry, rc, rmerged = _reference(shape)
    nx, ny = grid(w, h, tw, th)
    T = PlanTiled420(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    for name, (x, yy, rw, rh) in regions_of(shape).items():
        i0, j0, ni, nj = T.region_tiles(x, yy, rw, rh)
        assert (i0, j0, ni, nj) == emit.tiled_region_tiles(w, h, tw, th, x, yy, rw, rh)
        sub_y, sub_c = sub_grid(ry, nx, i0, j0, ni, nj), sub_grid(rc, nx, i0, j0, ni, nj)
        want = np.ascontiguousarray(rmerged[yy:yy + rh, x:x + rw]).reshape(-1)
        for offset in (0, 1, 3):
            sy, sc = Guarded(torch, sub_y.size, offset=offset, salt=1), Guarded(torch, sub_c.size, offset=offset, salt=2)
            sy.put(torch, [sub_y.reshape(-1)])
            sc.put(torch, [sub_c.reshape(-1)])
            dst = Guarded(torch, want.size, offset=offset, salt=3)
            T.merge_tiles420_region_dev(sy.ptr, sc.ptr, x, yy, rw, rh, dst.ptr)
            (got,), intact = dst.get(torch)
            assert intact, ("the region kernel wrote outside the region raster", shape, name, offset)
            bad = got != want
            assert not bad.any(), (shape, name, offset, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
    import frave_amd as fa

    for bad in [(0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (2**32 - 1, 0, 2, 1)]:
        with pytest.raises(fa.FriHipError) as e:
            T.merge_tiles420_region_dev(16, 16, *bad, 16)
        assert e.value.code == -1, bad
    T.close()


def test_split_and_merge_replay_from_a_graph_on_two_images(ctx, hip):
    import torch

    shape = (257, 130, 100, 50)
    w, h, tw, th = shape
    T = PlanTiled420(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    images = [_reference(shape)[0], gen_image("smooth", w, h, 3, 9)]
    d_img = torch.zeros(3 * w * h, dtype=torch.uint8, device="cuda")
    d_y = torch.zeros(T.y_tile_bytes, dtype=torch.uint8, device="cuda")
    d_c = torch.zeros(T.c_tile_bytes, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(3 * w * h, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    T.split_tiles420_dev(d_img.data_ptr(), d_y.data_ptr(), d_c.data_ptr(), stream=s.cuda_stream)
    T.merge_tiles420_dev(d_y.data_ptr(), d_c.data_ptr(), d_out.data_ptr(), stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    n_nodes = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 2
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    torch.cuda.synchronize()
    assert not d_out.cpu().numpy().any(), "capturing ran nothing"
    for img in images:
        y, c = split_tiles420(img, tw, th)
        d_img.copy_(torch.from_numpy(img.reshape(-1).copy()))
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(ex, sp) == 0
        s.synchronize()
        assert np.array_equal(d_y.cpu().numpy(), y.reshape(-1)) and np.array_equal(d_c.cpu().numpy(), c.reshape(-1))
        assert np.array_equal(d_out.cpu().numpy(), merge_tiles420(y, c, w, h).reshape(-1))
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    T.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _image():
    w, h, tw, th = IMAGE
    img = mixed_image(w, h, 3, tw, 3)
    img.setflags(write=False)
    return img


@pytest.fixture(scope="module")
def coded(ctx):
    """the tiled plan with its stream orders, the encode's outputs and the file - shared by the encode and the decode tests, unchanged by them"""
    w, h, tw, th = IMAGE
    assert tile_shape420(w, h, 150) == (tw, th)
    T = PlanTiled420(ctx, w, h, tw, th)
    T.set_stream_order()
    out = T.encode_image_tiled420_symbols(_image(), QUALITY)
    sym, vp, wp, hist, oob = out
    frv = emit.tiled_encode_from_streams420(w, h, tw, th, sym, T.n_luma, T.n_chroma, hist, vp, wp, QUALITY)
    yield T, out, frv
    T.close()


def test_encode_is_plan420_on_every_tile_in_plane_order(ctx, coded):
    import torch

    import frave_amd as fa

    w, h, tw, th = IMAGE
    T, (sym, vp, wp, hist, oob), frv = coded
    n, n_y, n_c = T.n_tiles, T.n_luma, T.n_chroma
    assert n == 4 and sym.size == n * (n_y + 2 * n_c) and vp.shape == wp.shape == (3 * n, 3, 6) and hist.shape == (3 * n, 10, 1024) and not oob.any()
    Q = Plan420(ctx, tw, th)
    Q.set_stream_order()
    assert (Q.luma.num_some, Q.chroma.num_some) == (n_y, n_c)
    tiles = split_tiles(_image(), tw, th)
    luma, chroma = sym[: n * n_y].reshape(n, n_y), sym[n * n_y:].reshape(n, 2, n_c)
    files = []
    for t in range(n):
        s1, v1, w1, h1, o1 = Q.encode_image420_symbols(tiles[t], QUALITY)
        assert not o1.any()
        for ch in range(3):
            k = plane_index(n, t, ch)
            got = luma[t] if ch == 0 else chroma[t, ch - 1]
            ref = s1[:n_y] if ch == 0 else s1[n_y + (ch - 1) * n_c: n_y + ch * n_c]
            assert np.array_equal(got, ref), (t, ch, "symbols")
            assert np.array_equal(hist[k], h1[ch]) and np.array_equal(vp[k], v1[ch]) and np.array_equal(wp[k], w1[ch]), (t, ch)
        files.append(emit.encode_image_from_streams(tw, th, s1, h1, v1, w1, quality=QUALITY, ycbcr=True, n_luma=n_y, empty_ok=True))
    f = parse_frit(frv)
    assert f["payloads"] == files and (f["W"], f["H"], f["tile_w"], f["tile_h"]) == (w, h, tw, th)
    Q.close()
    # the _dev form, fit on, on a stream of its own: the same arrays; the input intact
    s = torch.cuda.Stream()
    d_px = torch.from_numpy(_image().reshape(-1).copy()).cuda()
    d_params = torch.zeros(3 * n * 36, dtype=torch.float32, device="cuda")
    d_sym = torch.zeros(sym.size, dtype=torch.int16, device="cuda")
    d_hist = torch.zeros(3 * n * 10 * 1024, dtype=torch.int32, device="cuda")
    d_oob = torch.full((3 * n,), 5, dtype=torch.int64, device="cuda")
    d_oor = torch.full((3 * n,), 5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    T.encode_symbols_tiled420_dev(d_px.data_ptr(), QUALITY, d_params.data_ptr(), d_sym.data_ptr(), d_hist.data_ptr(), d_oob.data_ptr(), d_oor.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d_sym.cpu().numpy().view(np.uint16), sym) and np.array_equal(d_hist.cpu().numpy().view(np.uint32).reshape(hist.shape), hist)
    params = d_params.cpu().numpy().reshape(3 * n, 2, 3, 6)
    assert np.array_equal(params[:, 0], vp) and np.array_equal(params[:, 1], wp)
    assert not d_oob.cpu().numpy().any() and not d_oor.cpu().numpy().any() and np.array_equal(d_px.cpu().numpy(), _image().reshape(-1))
    # refusals: a quality outside 1..99, and inner plans without their stream order
    for q in (0, 100):
        with pytest.raises(fa.FriHipError) as e:
            T.encode_image_tiled420_symbols(_image(), q)
        assert e.value.code == -1
    bare = PlanTiled420(ctx, w, h, tw, th)
    with pytest.raises(fa.FriHipError) as e:
        bare.encode_image_tiled420_symbols(_image(), QUALITY)
    assert e.value.code == -1
    bare.close()


def test_decode_is_the_merge_of_plan420_decodes_and_regions_are_its_crops(ctx, hip, coded):
    import torch

    import frave_amd as fa

    w, h, tw, th = IMAGE
    T, _, frv = coded
    n = T.n_tiles
    ti, coefs = emit.tiled_decode(frv)
    assert ti.s420 and ti.quality == QUALITY and tuple(ti)[:7] == (w, h, tw, th, 2, 2, 3) and coefs.size == T.coef_count
    Q = Plan420(ctx, tw, th)
    fy, fc = Q.luma.num_cells * 512, Q.chroma.num_cells * 512
    per = []
    for t in range(n):
        planes = [coefs[t * fy:(t + 1) * fy]] + [coefs[n * fy + (2 * t + k) * fc: n * fy + (2 * t + k + 1) * fc] for k in range(2)]
        per.append(Q.decode_image420(np.concatenate(planes), QUALITY).reshape(th, tw, 3))
    Q.close()
    whole = merge_tiles(np.stack(per), w, h)
    got = T.decode_image_tiled420(coefs, QUALITY)
    assert np.array_equal(got, whole.reshape(-1))
    assert not np.array_equal(got, _image().reshape(-1))  # lossy (how far off colour noise comes back in 4:2:0 is the format's matter: the reference above is the check)
    s = torch.cuda.Stream()
    first = True
    for name, (x, y, rw, rh) in regions_of(IMAGE).items():
        want = np.ascontiguousarray(whole[y:y + rh, x:x + rw]).reshape(-1)
        info, tiles, part = emit.tiled_decode_region(frv, x, y, rw, rh)
        assert tiles == T.region_tiles(x, y, rw, rh)
        if first:  # a fresh plan: its tile buffers hold the region's tiles and no more
            fresh = PlanTiled420(ctx, w, h, tw, th)
            assert fresh.buffer_tiles() == (0, 0) and tiles[2] * tiles[3] == 1
            assert np.array_equal(fresh.decode_region_tiled420(part, QUALITY, x, y, rw, rh), want)
            assert fresh.buffer_tiles() == (1, 1)
            fresh.close()
            first = False
        assert np.array_equal(T.decode_region_tiled420(part, QUALITY, x, y, rw, rh), want), name
        d_coefs = torch.from_numpy(part.reshape(-1).copy()).cuda()
        dst = Guarded(torch, want.size, offset=1, salt=7)
        torch.cuda.synchronize()
        T.decode_region_tiled420_dev(d_coefs.data_ptr(), QUALITY, x, y, rw, rh, dst.ptr, stream=s.cuda_stream)
        s.synchronize()
        (got,), intact = dst.get(torch)
        assert intact and np.array_equal(got, want), name
    # a capturing stream is refused with nothing enqueued
    d_out = torch.zeros(3, dtype=torch.uint8, device="cuda")
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    try:
        with pytest.raises(fa.FriHipError) as e:
            T.decode_region_tiled420_dev(d_coefs.data_ptr(), QUALITY, 0, 0, 1, 1, d_out.data_ptr(), stream=s.cuda_stream)
        assert e.value.code == -1 and "graph" in str(e.value)
    finally:
        assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0
    n_nodes = C.c_size_t(12345)
    rc = hip.hipGraphGetNodes(graph, None, C.byref(n_nodes))
    hip.hipGraphDestroy(graph)
    assert rc == 0 and n_nodes.value == 0


def test_driver_tiled420_file(ctx, coded, tmp_path):
    """fri_driver encode-file --tile-size-420 passes its self-check; decode-file equals the Python route byte for byte; --region equals the crop; a target is
    refused and writes no file"""
    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h, tw, th = IMAGE
    T, _, frv = coded
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + _image().tobytes())

    def run(*args):
        return subprocess.run([driver, *map(str, args)], capture_output=True, text=True, timeout=300)

    dst, back, part = tmp_path / "t420.frv", tmp_path / "t420.ppm", tmp_path / "part.ppm"
    out = run("encode-file", src, dst, "--tile-size-420", "150", "--quality", QUALITY)
    assert out.returncode == 0 and "self-check" in out.stdout, out.stdout + out.stderr
    assert dst.read_bytes() == frv  # the C++ mirror writes the file of the Python route
    out = run("decode-file", dst, back)
    assert out.returncode == 0, out.stderr
    whole = T.decode_image_tiled420(emit.tiled_decode(frv)[1], QUALITY).reshape(h, w, 3)
    assert np.array_equal(np.frombuffer(back.read_bytes()[-3 * w * h:], np.uint8).reshape(h, w, 3), whole)
    x, y, rw, rh = regions_of(IMAGE)["across a tile column and a tile row"]
    out = run("decode-file", dst, part, "--region", f"{x},{y},{rw},{rh}")
    assert out.returncode == 0 and f"{rw}x{rh}x3" in out.stdout, out.stdout + out.stderr
    assert np.array_equal(np.frombuffer(part.read_bytes()[-3 * rw * rh:], np.uint8).reshape(rh, rw, 3), whole[y:y + rh, x:x + rw])
    for bad in (["--psnr", "35"], ["--quality", QUALITY, "--ssim", "0.9"], ["--size", "100000"], []):
        out = run("encode-file", src, tmp_path / "bad.frv", "--tile-size-420", "150", *bad)
        assert out.returncode != 0 and out.stderr and not (tmp_path / "bad.frv").exists(), bad
