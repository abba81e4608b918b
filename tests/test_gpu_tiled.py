"""Tiled coding on the device (fri_hip_plan_tiled, K10: k10_tiles.hip) against tests/tiled_ref.py and the existing plans:

- the split and the merge exactly equal to the restatement: one-pixel tiles, tiles narrower than a 16-byte strip, rows that are and are not a multiple of 16
  bytes, a tile larger than the image, a replicated edge in both directions, more than one workgroup; device pointers 0, 1 and 3 bytes off a 256-byte boundary,
  between guard bytes;
- graph capture of the raster kernels;
- fri_hip_encode_image_tiled_symbols against the existing route on an ordinary plan of the tile's shape, tile by tile, bit for bit; the _dev form with given
  parameters, whose `frit` payloads are the per-tile files;
- end to end through the container and fri_hip_decode_image_tiled: lossless files return the input, a YCbCr file the merge of the per-tile inverse transforms;
- fri_driver encode-file --tile-size and decode-file."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from frave_amd.api import TILED_ALLOW_HOLES, PlanTiled  # noqa: F401  (without the feature the module fails here)
from tests.common import KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS, gen_image
from tests.oracle_ref import MIDPOINT, REFERENCE
from tests.test_gpu_instances import Guarded
from tests.tiled_ref import grid, merge_tiles, mixed_image, parse_frit, split_tiles

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELAXED = 2  # hipStreamCaptureModeRelaxed
COLOUR_NONE, COLOUR_RCT, COLOUR_YCBCR = 0, 1, 3
# (W, H, C, tile_w, tile_h)
SHAPES = [(1, 1, 1, 1, 1), (5, 3, 3, 2, 2), (17, 9, 1, 16, 4), (33, 20, 3, 16, 16), (64, 48, 3, 64, 48), (50, 40, 1, 64, 64), (257, 130, 3, 100, 50), (1023, 767, 3, 512, 512)]
IMAGES = [(250, 250, 1, 125, 125), (334, 350, 3, 167, 117)]


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
    w, h, c, tw, th = shape
    img = gen_image("noise", w, h, c, w + h)
    return img.reshape(-1), split_tiles(img, tw, th).reshape(-1)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_and_merge_equal_the_restatement(ctx, shape):
    import torch

    w, h, c, tw, th = shape
    img, tiles = _reference(shape)
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    assert (T.nx, T.ny) == grid(w, h, tw, th) and T.tile_bytes == tiles.size and T.pixel_bytes == img.size
    for offset in (0, 1, 3):
        src = Guarded(torch, img.size, offset=offset, salt=1)
        src.put(torch, [img])
        cut = Guarded(torch, tiles.size, offset=offset, salt=2)
        T.split_tiles_dev(src.ptr, cut.ptr)
        (got,), intact = cut.get(torch)
        assert intact, "the split wrote outside its buffer"
        bad = got != tiles
        assert not bad.any(), (shape, offset, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
        back = Guarded(torch, img.size, offset=offset, salt=3)
        T.merge_tiles_dev(cut.ptr, back.ptr)
        (got,), intact = back.get(torch)
        assert intact, "the merge wrote outside its raster"
        bad = got != img  # split then merge gives the image back, every byte written
        assert not bad.any(), (shape, offset, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
        # the merge of tiles whose replicated pixels differ from the image's edge: only the in-image pixels are copied
        other = gen_image("noise", tw, th * T.n_tiles, c, 99).reshape(-1)
        cut.put(torch, [other])
        T.merge_tiles_dev(cut.ptr, back.ptr)
        (got,), intact = back.get(torch)
        assert intact and np.array_equal(got, merge_tiles(other.reshape(T.n_tiles, th, tw, c), w, h).reshape(-1)), (shape, offset)
        (again,), ok = src.get(torch)  # the input comes back intact
        assert ok and np.array_equal(again, img)
    T.close()


def test_raster_kernels_replay_from_a_graph(ctx, hip):
    import torch

    import frave_amd as fa

    shape = (257, 130, 3, 100, 50)
    w, h, c, tw, th = shape
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    imgs = [gen_image(kind, w, h, c, 5 + i) for i, kind in enumerate(("noise", "smooth"))]
    d_img = torch.from_numpy(imgs[0].reshape(-1).copy()).cuda()
    d_tiles = torch.empty(T.tile_bytes, dtype=torch.uint8, device="cuda")
    d_back = torch.empty(T.pixel_bytes, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    T.split_tiles_dev(d_img.data_ptr(), d_tiles.data_ptr(), stream=s.cuda_stream)
    T.merge_tiles_dev(d_tiles.data_ptr(), d_back.data_ptr(), stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    img = imgs[1]  # one replay, on what the pixel buffer holds now
    d_img.copy_(torch.from_numpy(img.reshape(-1).copy()))
    d_tiles.fill_(9), d_back.fill_(9)
    torch.cuda.synchronize()
    assert hip.hipGraphLaunch(ex, sp) == 0
    s.synchronize()
    assert np.array_equal(d_tiles.cpu().numpy(), split_tiles(img, tw, th).reshape(-1))
    assert np.array_equal(d_back.cpu().numpy(), img.reshape(-1))
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    # the encode chain refuses a capturing stream, as its inner call does
    T.set_stream_order()
    planes = T.n_tiles * c
    d_params = torch.zeros(planes * 36, dtype=torch.float32, device="cuda")
    d_sym = torch.zeros(planes * T.num_some, dtype=torch.int16, device="cuda")
    d_hist = torch.zeros(planes * 10 * 1024, dtype=torch.int32, device="cuda")
    d_oob = torch.zeros(2 * planes, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    try:
        with pytest.raises(fa.FriHipError) as e:
            T.encode_symbols_tiled_dev(d_img.data_ptr(), d_params.data_ptr(), d_sym.data_ptr(), d_hist.data_ptr(), d_oob.data_ptr(), stream=s.cuda_stream)
        assert e.value.code == -1 and "graph" in str(e.value)
    finally:
        assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0
    n_nodes = C.c_size_t(12345)
    rc = hip.hipGraphGetNodes(graph, None, C.byref(n_nodes))
    hip.hipGraphDestroy(graph)
    assert rc == 0 and n_nodes.value == 0
    T.close()


def _tiled(ctx, case, transform=COLOUR_NONE):
    w, h, c, tw, th = case
    T = PlanTiled(ctx, w, h, c, tw, th)
    T.set_stream_order()
    T.tile.set_colour_transform(transform)
    return T


def _tile_plan(ctx, case, transform=COLOUR_NONE):
    import frave_amd as fa

    w, h, c, tw, th = case
    Q = fa.Plan(ctx, tw, th, c)
    Q.set_stream_order()
    Q.set_colour_transform(transform)
    return Q


@pytest.mark.parametrize("case", IMAGES, ids=lambda s: "x".join(map(str, s)))
def test_encode_is_the_existing_route_on_every_tile(ctx, case):
    import torch

    import frave_amd.emit as emit

    w, h, c, tw, th = case
    img = mixed_image(w, h, c, tw, 3)
    tiles = split_tiles(img, tw, th)
    T, Q = _tiled(ctx, case), _tile_plan(ctx, case)
    n = T.n_tiles
    sym, vp, wp, hist, oob = T.encode_image_tiled_symbols(img)
    assert sym.shape == (n, c, T.num_some) and vp.shape == wp.shape == (n, c, 3, 6) and hist.shape == (n, c, 10, 1024) and oob.shape == (n, c)
    assert (hist.sum(axis=3) > 0).all(), "every tile fills all ten contexts"
    for t in range(n):  # with the fit on: bit for bit what an ordinary plan gives for the numpy-cut tile
        want = Q.encode_image_symbols(tiles[t], fit=True)
        for name, got, ref in zip(("symbols", "value_params", "width_params", "hist", "oob"), (sym[t], vp[t], wp[t], hist[t], oob[t]), want):
            assert np.array_equal(got, ref), (t, name)
    # fit = 0 with the known-answer parameters through the _dev form: the container's payloads are the per-tile files
    planes = n * c
    kat = np.tile(np.stack([KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS])[None], (planes, 1, 1, 1)).astype(np.float32)
    d_px = torch.from_numpy(img.reshape(-1).copy()).cuda()
    d_params = torch.from_numpy(kat.reshape(-1).copy()).cuda()
    d_sym = torch.zeros(planes * T.num_some, dtype=torch.int16, device="cuda")
    d_hist = torch.zeros(planes * 10 * 1024, dtype=torch.int32, device="cuda")
    d_oob = torch.full((planes,), 5, dtype=torch.int64, device="cuda")
    T.encode_symbols_tiled_dev(d_px.data_ptr(), d_params.data_ptr(), d_sym.data_ptr(), d_hist.data_ptr(), d_oob.data_ptr(), fit=False)
    torch.cuda.synchronize()
    assert np.array_equal(d_params.cpu().numpy().reshape(kat.shape), kat) and not d_oob.cpu().numpy().any()
    assert np.array_equal(d_px.cpu().numpy(), img.reshape(-1))
    ksym = d_sym.cpu().numpy().view(np.uint16).reshape(n, c, -1)
    khist = d_hist.cpu().numpy().view(np.uint32).reshape(n, c, 10, 1024)
    kvp, kwp = np.ascontiguousarray(kat[:, 0]).reshape(n, c, 3, 6), np.ascontiguousarray(kat[:, 1]).reshape(n, c, 3, 6)
    frit = emit.tiled_encode_from_streams(w, h, tw, th, ksym, khist, kvp, kwp)
    f = parse_frit(frit)
    for t in range(n):
        s1, v1, w1, h1, o1 = Q.encode_image_symbols(tiles[t], fit=False, value_params=np.stack([KAT_VALUE_PARAMS] * c), width_params=np.stack([KAT_WIDTH_PARAMS] * c))
        assert not o1.any() and f["payloads"][t] == emit.encode_image_from_streams(tw, th, s1, h1, v1, w1), t
    # lossless: the decoded planes give the source back
    ti, coefs = emit.tiled_decode(frit)
    assert tuple(ti) == (w, h, tw, th, T.nx, T.ny, c, T.num_cells)
    T.tile.set_dequantiser(REFERENCE)
    assert np.array_equal(T.decode_image_tiled(coefs), img.reshape(-1))
    # ... and so do those of the fitted encode
    ti, coefs = emit.tiled_decode(emit.tiled_encode_from_streams(w, h, tw, th, sym, hist, vp, wp, threads=3), threads=3)
    assert np.array_equal(T.decode_image_tiled(coefs), img.reshape(-1))
    Q.close()
    # without the stream order on the inner plan the encode is refused
    import frave_amd as fa

    bare = PlanTiled(ctx, w, h, c, tw, th)
    with pytest.raises(fa.FriHipError) as e:
        bare.encode_image_tiled_symbols(img)
    assert e.value.code == -1
    bare.close()
    T.close()


def test_ycbcr_decode_is_the_merge_of_the_tiles_inverse_transforms(ctx):
    import frave_amd as fa
    import frave_amd.emit as emit

    case = IMAGES[1]
    w, h, c, tw, th = case
    img = mixed_image(w, h, c, tw, 4)
    qm = fa.quality_matrix(50)
    T, Q = _tiled(ctx, case, COLOUR_YCBCR), _tile_plan(ctx, case, COLOUR_YCBCR)
    sym, vp, wp, hist, oob = T.encode_image_tiled_symbols(img, qm)
    assert not oob.any()
    frit = emit.tiled_encode_from_streams(w, h, tw, th, sym, hist, vp, wp, ycbcr=True, quality=50)
    ti, coefs = emit.tiled_decode(frit)
    assert (ti.ycbcr, ti.quality, ti.rct) == (True, 50, False)
    tiles = split_tiles(img, tw, th)
    T.tile.set_dequantiser(MIDPOINT)
    Q.set_dequantiser(MIDPOINT)
    per = []
    for t in range(T.n_tiles):
        assert np.array_equal(coefs[t], Q.transform_quant(tiles[t], qm)), t  # the file holds the tile's quantised planes
        per.append(Q.inverse_transform(coefs[t], qm).reshape(th, tw, c))
    want = merge_tiles(np.stack(per), w, h).reshape(-1)
    got = T.decode_image_tiled(coefs, qm)
    assert np.array_equal(got, want)
    err = np.abs(got.astype(np.int64) - img.reshape(-1).astype(np.int64))
    assert 0 < err.max() < 128  # lossy, and an image
    Q.close()
    T.close()


def test_driver_tiled_file(ctx, tmp_path):
    """fri_driver encode-file --tile-size (the C++ mirror: tile shape, device batch, threaded emitter) passes its self-check and decode-file recognises the
    container; what tiles do not take is refused"""
    import frave_amd as fa
    import frave_amd.emit as emit

    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h = 334, 350
    img = mixed_image(w, h, 3, 167, 8)
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + img.tobytes())
    tw, th = fa.tile_shape(w, h, 150)
    for name, flags in (("rct", ["--rct"]), ("ycc", ["--ycbcr", "--quality", "60"])):
        dst, back = tmp_path / f"{name}.frv", tmp_path / f"{name}.ppm"
        out = subprocess.run([driver, "encode-file", str(src), str(dst), "--tile-size", "150"] + flags, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "self-check" in out.stdout, out.stdout + out.stderr
        f = parse_frit(dst.read_bytes())
        assert (f["W"], f["H"], f["tile_w"], f["tile_h"]) == (w, h, tw, th)
        info = emit.tiled_info(dst.read_bytes())
        assert (info.rct, info.ycbcr, info.quality) == ((True, False, 0) if name == "rct" else (False, True, 60))
        out = subprocess.run([driver, "decode-file", str(dst), str(back)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        got = np.frombuffer(back.read_bytes()[-3 * w * h:], np.uint8)
        if name == "rct":
            assert np.array_equal(got, img.reshape(-1))
        else:
            assert np.abs(got.astype(np.int64) - img.reshape(-1)).max() < 128
    # the targets: the whole image's search picks the quality, the tiles are coded with it; a size budget holds for the tiled file
    for flags in (["--psnr", "30"], ["--ycbcr", "--ssim", "0.9"], ["--size", "250000"]):
        dst = tmp_path / "target.frv"
        out = subprocess.run([driver, "encode-file", str(src), str(dst), "--tile-size", "150"] + flags, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "self-check" in out.stdout, out.stdout + out.stderr
        q = emit.tiled_info(dst.read_bytes()).quality  # (0: the search found that only a lossless file reaches the target)
        assert 0 <= q <= 99 and (flags[0] != "--size" or q >= 1), flags
        assert flags[0] != "--size" or len(dst.read_bytes()) <= 250000
    for bad in (["--420", "--quality", "50"], ["--tile-size", "0"]):
        out = subprocess.run([driver, "encode-file", str(src), str(tmp_path / "bad.frv"), "--tile-size", "150"] + bad, capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and not (tmp_path / "bad.frv").exists(), bad
