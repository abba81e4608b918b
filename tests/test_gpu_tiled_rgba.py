"""Tiled RGBA coding on the device (K16: split_tiles_rgba_kernel, merge_tiles_rgba_region_kernel; fri_hip_*_tiled_rgba*) against tests/tiled_rgba_ref.py:

- the split, KEEP and CLEAN, and the whole merge exactly equal to the numpy composition on the smallest shapes that reach every path, device pointers 0, 1 and
  3 bytes off a 256-byte boundary between guard bytes; the merge also on random planes, whose replicated pixels hold other values; the inputs come back intact;
- the region merge equal to the crop of the whole merge;
- split and merge replayed from a captured graph on two images;
- the encode equal, plane by plane, to PlanRGBA.encode_image_rgba_symbols of each numpy-split tile, and the `frit` file equal to the container of the per-tile
  files;
- the decode equal to the numpy merge of each tile's PlanRGBA.decode_image_rgba, the region decodes equal to its crops, the plan's buffers at the region's size,
  the alpha plan's dequantiser setting intact;
- fri_driver encode-file in.pam --tile-size, decode-file and --region, and the combinations that stay refused."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import frave_amd.emit as emit
from frave_amd.api import ALPHA_CLEAN, ALPHA_KEEP, COLOUR_YCBCR, DEQUANT_MIDPOINT, DEQUANT_MULTIPLY, DEQUANT_REFERENCE, TILED_ALLOW_HOLES, PlanRGBA, tile_shape
from frave_amd.api import PlanTiledRgba  # noqa: F401  (without the feature the module fails here)
from tests.alpha_ref import alpha_plane, cleaned, rgba_image
from tests.common import gen_image
from tests.test_gpu_instances import Guarded
from tests.test_gpu_tiled420 import regions_of
from tests.tiled_rgba_ref import container, grid, merge_tiles_rgba, plane_index, split_tiles_rgba, sub_grid
from tests.tiled_ref import merge_tiles, mixed_image, parse_frit, split_tiles

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELAXED = 2  # hipStreamCaptureModeRelaxed
# (W, H, tile_w, tile_h): tile_w below, at and one over the 16-pixel strip; a clamped last column and row; a tile larger than the image; strips that cross tile
# columns in the region merge
SHAPES = [(1, 1, 1, 1), (5, 3, 2, 2), (17, 9, 16, 4), (33, 20, 16, 16), (35, 23, 17, 9), (40, 33, 5, 3), (50, 40, 64, 64), (257, 130, 100, 50), (1023, 767, 512, 512)]
REGION_SHAPES = [(257, 130, 100, 50), (40, 33, 5, 3)]
IMAGE = (334, 350, 167, 175)  # 2 x 2 tiles of fri_hip_tile_shape(334, 350, 150)
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


def _rgba(w, h, seed, kind="noise"):
    """colour without a zero byte under an alpha plane with about a quarter zeros, the last pixel - the one the edge tiles replicate - among them: CLEAN changes
    every transparent pixel, in full and partial strips and in replicated pixels"""
    rgb = np.maximum(gen_image(kind, w, h, 3, seed), 1).astype(np.uint8)
    a = alpha_plane("random", w, h, seed)
    a[h - 1, w - 1] = 0
    return rgba_image(rgb, a)


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """(image, {clean: (colour_tiles, alpha_tiles)}, random colour and alpha tiles, their merged image) - computed once, read-only"""
    w, h, tw, th = shape
    img = _rgba(w, h, w + 7 * h)
    assert img[h - 1, w - 1, 3] == 0 and img[:, :, :3].all()
    splits = {clean: split_tiles_rgba(img, w, h, tw, th, clean) for clean in (ALPHA_KEEP, ALPHA_CLEAN)}
    rng = np.random.default_rng([w, h, tw, th])
    rc, ra = rng.integers(0, 256, splits[0][0].shape, dtype=np.uint8), rng.integers(0, 256, splits[0][1].shape, dtype=np.uint8)
    out = (img, splits, rc, ra, merge_tiles_rgba(rc, ra, w, h))
    for a in (img, rc, ra, out[4], *splits[0], *splits[1]):
        a.setflags(write=False)
    return out


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_and_whole_merge_equal_the_numpy_composition(ctx, shape):
    import torch

    w, h, tw, th = shape
    img, splits, rc, ra, rmerged = _reference(shape)
    T = PlanTiledRgba(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    assert (T.colour_tile_bytes, T.alpha_tile_bytes) == (rc.size, ra.size)
    for offset in (0, 1, 3):
        src = Guarded(torch, img.size, offset=offset, salt=1)
        src.put(torch, [img.reshape(-1)])
        for clean in (ALPHA_KEEP, ALPHA_CLEAN):
            colour, alpha = splits[clean]
            dc, da = Guarded(torch, colour.size, offset=offset, salt=2), Guarded(torch, alpha.size, offset=offset, salt=3)
            T.split_tiles_rgba_dev(src.ptr, dc.ptr, da.ptr, clean=clean)
            (gc,), ok_c = dc.get(torch)
            (ga,), ok_a = da.get(torch)
            assert ok_c and ok_a, ("the split wrote outside its tile rasters", shape, offset, clean)
            bad = gc != colour.reshape(-1)
            assert not bad.any(), ("colour_tiles", shape, offset, clean, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
            bad = ga != alpha.reshape(-1)
            assert not bad.any(), ("alpha_tiles", shape, offset, clean, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
            (again,), ok = src.get(torch)
            assert ok and np.array_equal(again, img.reshape(-1))
        # the merge of what the split wrote, and of random planes (replicated pixels hold other values: none of them may show)
        for planes_c, planes_a, want, salt in ((*splits[ALPHA_KEEP], img, 4), (rc, ra, rmerged, 7)):
            sc, sa = Guarded(torch, planes_c.size, offset=offset, salt=salt), Guarded(torch, planes_a.size, offset=offset, salt=salt + 1)
            sc.put(torch, [planes_c.reshape(-1)])
            sa.put(torch, [planes_a.reshape(-1)])
            dst = Guarded(torch, want.size, offset=offset, salt=salt + 2)
            T.merge_tiles_rgba_dev(sc.ptr, sa.ptr, dst.ptr)
            (got,), intact = dst.get(torch)
            assert intact, ("the merge wrote outside the raster", shape, offset)
            bad = got != want.reshape(-1)
            assert not bad.any(), ("merge", shape, offset, salt, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
            (ac,), ok_c = sc.get(torch)
            (aa,), ok_a = sa.get(torch)
            assert ok_c and ok_a and np.array_equal(ac, planes_c.reshape(-1)) and np.array_equal(aa, planes_a.reshape(-1))
    import frave_amd as fa

    for bad_clean in (2, -1):
        with pytest.raises(fa.FriHipError) as e:
            T.split_tiles_rgba_dev(16, 16, 16, clean=bad_clean)
        assert e.value.code == -1
    T.close()


@pytest.mark.parametrize("shape", REGION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_region_merge_is_the_crop_of_the_whole_merge(ctx, shape):
    import torch

    import frave_amd as fa

    w, h, tw, th = shape
    img, splits, rc, ra, rmerged = _reference(shape)
    nx, ny = grid(w, h, tw, th)
    T = PlanTiledRgba(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    for name, (x, yy, rw, rh) in regions_of(shape).items():
        i0, j0, ni, nj = T.region(x, yy, rw, rh)
        assert (i0, j0, ni, nj) == emit.tiled_region_tiles(w, h, tw, th, x, yy, rw, rh)
        sub_c, sub_a = sub_grid(rc, nx, i0, j0, ni, nj), sub_grid(ra, nx, i0, j0, ni, nj)
        want = np.ascontiguousarray(rmerged[yy:yy + rh, x:x + rw]).reshape(-1)
        for offset in (0, 1, 3):
            sc, sa = Guarded(torch, sub_c.size, offset=offset, salt=1), Guarded(torch, sub_a.size, offset=offset, salt=2)
            sc.put(torch, [sub_c.reshape(-1)])
            sa.put(torch, [sub_a.reshape(-1)])
            dst = Guarded(torch, want.size, offset=offset, salt=3)
            T.merge_tiles_rgba_region_dev(sc.ptr, sa.ptr, x, yy, rw, rh, dst.ptr)
            (got,), intact = dst.get(torch)
            assert intact, ("the region kernel wrote outside the region raster", shape, name, offset)
            bad = got != want
            assert not bad.any(), (shape, name, offset, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())
    for bad in [(0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (2**32 - 1, 0, 2, 1)]:
        with pytest.raises(fa.FriHipError) as e:
            T.merge_tiles_rgba_region_dev(16, 16, *bad, 16)
        assert e.value.code == -1, bad
    T.close()


def test_split_and_merge_replay_from_a_graph_on_two_images(ctx, hip):
    import torch

    shape = (257, 130, 100, 50)
    w, h, tw, th = shape
    T = PlanTiledRgba(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    images = [_reference(shape)[0], _rgba(w, h, 9, "smooth")]
    d_img = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda")
    d_c = torch.zeros(T.colour_tile_bytes, dtype=torch.uint8, device="cuda")
    d_a = torch.zeros(T.alpha_tile_bytes, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    T.split_tiles_rgba_dev(d_img.data_ptr(), d_c.data_ptr(), d_a.data_ptr(), clean=ALPHA_CLEAN, stream=s.cuda_stream)
    T.merge_tiles_rgba_dev(d_c.data_ptr(), d_a.data_ptr(), d_out.data_ptr(), stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    n_nodes = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 2
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    torch.cuda.synchronize()
    assert not d_out.cpu().numpy().any(), "capturing ran nothing"
    for img in images:
        colour, alpha = split_tiles_rgba(img, w, h, tw, th, ALPHA_CLEAN)
        d_img.copy_(torch.from_numpy(img.reshape(-1).copy()))
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(ex, sp) == 0
        s.synchronize()
        assert np.array_equal(d_c.cpu().numpy(), colour.reshape(-1)) and np.array_equal(d_a.cpu().numpy(), alpha.reshape(-1))
        assert np.array_equal(d_out.cpu().numpy(), cleaned(img, w, h))
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    T.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _image():
    w, h, tw, th = IMAGE
    img = rgba_image(np.maximum(mixed_image(w, h, 3, tw, 3), 1).astype(np.uint8), alpha_plane("runs", w, h))
    img.setflags(write=False)
    return img


def _qm():
    import frave_amd as fa

    return fa.quality_matrix(QUALITY)


@pytest.fixture(scope="module")
def coded(ctx):
    """the tiled plan in YCbCr with its stream orders, the encode's outputs (quality 60, CLEAN) and the file - shared by the encode, the decode and the driver
    tests, unchanged by them"""
    w, h, tw, th = IMAGE
    assert tile_shape(w, h, 150) == (tw, th)
    T = PlanTiledRgba(ctx, w, h, tw, th)
    T.set_stream_order()
    T.colour.set_colour_transform(COLOUR_YCBCR)
    T.colour.set_dequantiser(DEQUANT_MIDPOINT)
    out = T.encode_image_tiled_rgba_symbols(_image(), _qm(), clean=ALPHA_CLEAN)
    sym, vp, wp, hist, oob = out
    frv = emit.tiled_encode_from_streams_rgba(w, h, tw, th, sym, hist, vp, wp, ycbcr=True, quality=QUALITY)
    yield T, out, frv
    T.close()


def _tile_plan(ctx):
    w, h, tw, th = IMAGE
    Q = PlanRGBA(ctx, tw, th)
    Q.set_stream_order()
    Q.colour.set_colour_transform(COLOUR_YCBCR)
    Q.colour.set_dequantiser(DEQUANT_MIDPOINT)
    return Q


def test_encode_is_plan_rgba_on_every_tile_in_plane_order(ctx, hip, coded):
    import torch

    import frave_amd as fa

    w, h, tw, th = IMAGE
    T, (sym, vp, wp, hist, oob), frv = coded
    n, n_some = T.n_tiles, T.num_some
    assert n == 4 and sym.shape == (4 * n, n_some) and vp.shape == wp.shape == (4 * n, 3, 6) and hist.shape == (4 * n, 10, 1024) and not oob.any()
    Q = _tile_plan(ctx)
    assert Q.num_some == n_some
    tiles = split_tiles(_image(), tw, th)  # the tile split of the R, G, B, A raster: every tile an RGBA image of its own
    files = []
    for t in range(n):
        s1, v1, w1, h1, o1 = Q.encode_image_rgba_symbols(tiles[t], _qm(), clean=ALPHA_CLEAN)
        assert not o1.any()
        for ch in range(4):
            k = plane_index(n, t, ch)
            assert np.array_equal(sym[k], s1[ch]), (t, ch, "symbols")
            assert np.array_equal(hist[k], h1[ch]) and np.array_equal(vp[k], v1[ch]) and np.array_equal(wp[k], w1[ch]) and oob[k] == o1[ch], (t, ch)
        files.append(emit.encode_image_from_streams(tw, th, s1, h1, v1, w1, quality=QUALITY, ycbcr=True, alpha=True, empty_ok=True))
    Q.close()
    f = parse_frit(frv)
    assert f["payloads"] == files and frv == container(w, h, tw, th, files)
    # the _dev form, fit on, on a stream of its own: the same arrays; the input intact
    s = torch.cuda.Stream()
    d_px = torch.from_numpy(_image().reshape(-1).copy()).cuda()
    d_params = torch.zeros(4 * n * 36, dtype=torch.float32, device="cuda")
    d_sym = torch.zeros(sym.size, dtype=torch.int16, device="cuda")
    d_hist = torch.zeros(4 * n * 10 * 1024, dtype=torch.int32, device="cuda")
    d_oob = torch.full((4 * n,), 5, dtype=torch.int64, device="cuda")
    d_oor = torch.full((4 * n,), 5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    T.encode_symbols_tiled_rgba_dev(d_px.data_ptr(), d_params.data_ptr(), d_sym.data_ptr(), d_hist.data_ptr(), d_oob.data_ptr(), d_oor.data_ptr(), clean=ALPHA_CLEAN, qmatrix=_qm(),
                                    stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d_sym.cpu().numpy().view(np.uint16).reshape(sym.shape), sym) and np.array_equal(d_hist.cpu().numpy().view(np.uint32).reshape(hist.shape), hist)
    params = d_params.cpu().numpy().reshape(4 * n, 2, 3, 6)
    assert np.array_equal(params[:, 0], vp) and np.array_equal(params[:, 1], wp)
    assert not d_oob.cpu().numpy().any() and not d_oor.cpu().numpy().any() and np.array_equal(d_px.cpu().numpy(), _image().reshape(-1))
    # a capturing stream is refused with nothing enqueued
    sp = C.c_void_p(s.cuda_stream)
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    try:
        with pytest.raises(fa.FriHipError) as e:
            T.encode_symbols_tiled_rgba_dev(d_px.data_ptr(), d_params.data_ptr(), d_sym.data_ptr(), d_hist.data_ptr(), d_oob.data_ptr(), stream=s.cuda_stream)
        assert e.value.code == -1 and "graph" in str(e.value)
    finally:
        assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0
    n_nodes = C.c_size_t(12345)
    rc = hip.hipGraphGetNodes(graph, None, C.byref(n_nodes))
    hip.hipGraphDestroy(graph)
    assert rc == 0 and n_nodes.value == 0
    # refusals: a bad `clean`, and inner plans without their stream order
    for bad_clean in (2, -1):
        with pytest.raises(fa.FriHipError) as e:
            T.encode_image_tiled_rgba_symbols(_image(), _qm(), clean=bad_clean)
        assert e.value.code == -1
    bare = PlanTiledRgba(ctx, w, h, tw, th)
    bare.colour.set_stream_order()
    with pytest.raises(fa.FriHipError) as e:
        bare.encode_image_tiled_rgba_symbols(_image(), _qm())
    assert e.value.code == -1
    bare.close()


def test_decode_is_the_merge_of_plan_rgba_decodes_and_regions_are_its_crops(ctx, hip, coded):
    import torch

    import frave_amd as fa

    w, h, tw, th = IMAGE
    T, _, frv = coded
    n = T.n_tiles
    ti, coefs = emit.tiled_decode(frv)
    assert ti.alpha and ti.ycbcr and ti.quality == QUALITY and tuple(ti)[:7] == (w, h, tw, th, 2, 2, 3) and coefs.size == T.coef_count
    Q = _tile_plan(ctx)
    per = [Q.decode_image_rgba(np.concatenate([coefs[3 * t:3 * t + 3], coefs[3 * n + t][None]]), _qm()).reshape(th, tw, 4) for t in range(n)]
    Q.close()
    whole = merge_tiles(np.stack(per), w, h)
    # the alpha planes decode with the reference dequantiser whatever is set on their plan, and the setting survives: an alpha plane quantised at quality 40
    # gives three different rasters under the three dequantisers, before and after
    lossy = gen_image("noise", tw, th, 1, 3)
    co_a = T.alpha.transform_quant(lossy, fa.quality_matrix(40))
    rasters = {}
    for mode in (DEQUANT_REFERENCE, DEQUANT_MULTIPLY, DEQUANT_MIDPOINT):
        T.alpha.set_dequantiser(mode)
        rasters[mode] = T.alpha.inverse_transform(co_a, fa.quality_matrix(40))
    assert not np.array_equal(rasters[DEQUANT_REFERENCE], rasters[DEQUANT_MULTIPLY]) and not np.array_equal(rasters[DEQUANT_MULTIPLY], rasters[DEQUANT_MIDPOINT])
    for mode in (DEQUANT_MULTIPLY, DEQUANT_MIDPOINT, DEQUANT_REFERENCE):
        T.alpha.set_dequantiser(mode)
        got = T.decode_image_tiled_rgba(coefs, _qm())
        assert np.array_equal(got, whole.reshape(-1)), mode
        assert np.array_equal(T.alpha.inverse_transform(co_a, fa.quality_matrix(40)), rasters[mode]), mode
    assert np.array_equal(got.reshape(h, w, 4)[:, :, 3], _image()[:, :, 3])  # alpha is lossless
    assert not np.array_equal(got, cleaned(_image(), w, h))  # the colour is lossy (how far off is the format's matter: the reference above is the check)
    s = torch.cuda.Stream()
    first = True
    for name, (x, y, rw, rh) in regions_of(IMAGE).items():
        want = np.ascontiguousarray(whole[y:y + rh, x:x + rw]).reshape(-1)
        info, tiles, part = emit.tiled_decode_region(frv, x, y, rw, rh)
        assert tiles == T.region(x, y, rw, rh) and info.alpha
        if first:  # a fresh plan: its tile buffers hold the region's tiles and no more
            fresh = PlanTiledRgba(ctx, w, h, tw, th)
            fresh.colour.set_colour_transform(COLOUR_YCBCR)
            fresh.colour.set_dequantiser(DEQUANT_MIDPOINT)
            assert fresh.buffer_tiles() == (0, 0) and tiles[2] * tiles[3] == 1
            assert np.array_equal(fresh.decode_region_tiled_rgba(part, x, y, rw, rh, _qm()), want)
            assert fresh.buffer_tiles() == (1, 1)
            fresh.close()
            first = False
        assert np.array_equal(T.decode_region_tiled_rgba(part, x, y, rw, rh, _qm()), want), name
        d_coefs = torch.from_numpy(part.reshape(-1).copy()).cuda()
        dst = Guarded(torch, want.size, offset=1, salt=7)
        torch.cuda.synchronize()
        T.decode_region_tiled_rgba_dev(d_coefs.data_ptr(), x, y, rw, rh, dst.ptr, qmatrix=_qm(), stream=s.cuda_stream)
        s.synchronize()
        (got,), intact = dst.get(torch)
        assert intact and np.array_equal(got, want), name
    # a tile list comes back in the same plane order: the first and the last tile are the region decodes of their pixels
    info, part = emit.tiled_decode_tiles(frv, [0, 3])
    assert info.alpha and np.array_equal(part[:3], coefs[:3]) and np.array_equal(part[3:6], coefs[9:12]) and np.array_equal(part[6], coefs[12]) and np.array_equal(part[7], coefs[15])
    # a capturing stream is refused with nothing enqueued
    d_out = torch.zeros(4, dtype=torch.uint8, device="cuda")
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    try:
        with pytest.raises(fa.FriHipError) as e:
            T.decode_region_tiled_rgba_dev(d_coefs.data_ptr(), 0, 0, 1, 1, d_out.data_ptr(), qmatrix=_qm(), stream=s.cuda_stream)
        assert e.value.code == -1 and "graph" in str(e.value)
    finally:
        assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0
    n_nodes = C.c_size_t(12345)
    rc = hip.hipGraphGetNodes(graph, None, C.byref(n_nodes))
    hip.hipGraphDestroy(graph)
    assert rc == 0 and n_nodes.value == 0
    # an empty or escaping region
    for bad in [(0, 0, 0, 1), (w, 0, 1, 1), (1, 0, w, 1)]:
        with pytest.raises(fa.FriHipError) as e:
            T.decode_region_tiled_rgba_dev(d_coefs.data_ptr(), *bad, d_out.data_ptr())
        assert e.value.code == -1, bad


def _pam(w, h, pixels):
    return b"P7\nWIDTH %d\nHEIGHT %d\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n" % (w, h) + np.ascontiguousarray(pixels, np.uint8).tobytes()


def test_driver_tiled_rgba_file(ctx, coded, tmp_path):
    """fri_driver encode-file in.pam --tile-size passes its self-check and writes the file of the Python route; a lossless file decodes to the input, and to the
    cleaned input with --clean-alpha; --region equals the crop; each combination that stays refused exits non-zero with nothing written"""
    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h, tw, th = IMAGE
    T, _, frv = coded
    img = _image()
    src = tmp_path / "in.pam"
    src.write_bytes(_pam(w, h, img))

    def run(*args):
        return subprocess.run([driver, *map(str, args)], capture_output=True, text=True, timeout=300)

    def pixels(path, rw=w, rh=h):
        data = path.read_bytes()
        assert data[: len(data) - 4 * rw * rh] == _pam(rw, rh, np.zeros((rh, rw, 4), np.uint8))[: -4 * rw * rh]  # the header of a PAM of that size
        return np.frombuffer(data[-4 * rw * rh:], np.uint8)

    # the lossy file of the fixture: the same bytes, the same pixels
    dst, back, part = tmp_path / "t.frv", tmp_path / "t.pam", tmp_path / "part.pam"
    out = run("encode-file", src, dst, "--tile-size", "150", "--ycbcr", "--quality", QUALITY, "--clean-alpha")
    assert out.returncode == 0 and "self-check" in out.stdout and "tiles" in out.stdout, out.stdout + out.stderr
    assert dst.read_bytes() == frv  # the C++ mirror writes the file of the Python route
    whole = T.decode_image_tiled_rgba(emit.tiled_decode(frv)[1], _qm()).reshape(h, w, 4)
    out = run("decode-file", dst, back)
    assert out.returncode == 0 and f"{w}x{h}x4" in out.stdout, out.stdout + out.stderr
    assert np.array_equal(pixels(back), whole.reshape(-1))
    x, y, rw, rh = regions_of(IMAGE)["across a tile column and a tile row"]
    out = run("decode-file", dst, part, "--region", f"{x},{y},{rw},{rh}")
    assert out.returncode == 0 and f"{rw}x{rh}x4" in out.stdout, out.stdout + out.stderr
    assert np.array_equal(pixels(part, rw, rh), np.ascontiguousarray(whole[y:y + rh, x:x + rw]).reshape(-1))
    # lossless round trips: the input, and the cleaned input
    for name, flags, want in (("keep", [], np.ascontiguousarray(img).reshape(-1)), ("clean", ["--rct", "--clean-alpha"], cleaned(img, w, h))):
        f, p = tmp_path / f"{name}.frv", tmp_path / f"{name}.pam"
        out = run("encode-file", src, f, "--tile-size", "150", *flags)
        assert out.returncode == 0 and "self-check" in out.stdout, out.stdout + out.stderr
        assert emit.tiled_info(f.read_bytes()).alpha
        out = run("decode-file", f, p)
        assert out.returncode == 0, out.stderr
        assert np.array_equal(pixels(p), want), name
    # a file with alpha goes to a PAM only
    out = run("decode-file", dst, tmp_path / "bad.ppm")
    assert out.returncode != 0 and "alpha" in out.stderr and not (tmp_path / "bad.ppm").exists()
    # what stays refused on tiled RGBA, each saying so and writing nothing
    for bad in (["--psnr", "35"], ["--ycbcr", "--ssim", "0.9"], ["--size", "100000"], ["--bpp", "2"], ["--target", "psnr=35"], ["--quality", QUALITY, "--device-rans"]):
        out = run("encode-file", src, tmp_path / "bad.frv", "--tile-size", "150", *bad)
        assert out.returncode != 0 and "tiled RGBA" in out.stderr and not (tmp_path / "bad.frv").exists(), (bad, out.stderr)
    for bad in (["--device-rans"], ["--preview", "1"], ["--preview", "2", "--device-rans"]):
        out = run("decode-file", dst, tmp_path / "bad.pam", *bad)
        assert out.returncode != 0 and "tiled RGBA" in out.stderr and not (tmp_path / "bad.pam").exists(), (bad, out.stderr)
    out = run("decode-regions", dst, tmp_path / "regions", "--region", "0,0,8,8", "--region", "100,100,90,90")
    assert out.returncode != 0 and "tiled RGBA" in out.stderr and not list(tmp_path.glob("regions*")), out.stderr
    ppm = tmp_path / "new.ppm"
    ppm.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(img[:, :, :3]).tobytes())
    for new in (ppm, src):
        out = run("update-file", dst, new, tmp_path / "updated.frv", "--region", "0,0,8,8")
        assert out.returncode != 0 and "tiled RGBA" in out.stderr and not (tmp_path / "updated.frv").exists(), (new, out.stderr)
