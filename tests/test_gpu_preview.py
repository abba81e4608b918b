"""Preview decode on the device (include/fri_hip.h "Preview decode"): K14 (k14_preview.hip), K13 with its step loop bounded by a level, and the two composed routes.

- K14 against the definition: the inverse kernel through decode_image_tiled on planes whose nodes at or above 2^L are 0, then a numpy subsample - every L with
  every shift on one small shape; shapes whose last sample clamps, whose image is no multiple of the tile and whose tile is no multiple of S, a 1 x 1 and a 3 x 2
  grid, C = 1 and 3, tiles with holes; both node strides, the three dequantisers, both colour transforms, outputs 1 and 3 bytes off alignment between guard bytes;
  the same bytes from a captured graph; one case against tests/preview_ref.py, which stands on the oracle's inverse;
- K13 bounded: its planes are the host's compact planes expanded, for a tile so small that DC, root and level 1 share one chunk and for prefixes that are no
  multiple of 64; damage behind the prefix is not seen; fri_hip_decode_planes_dev writes the bytes of the L = 9 launch, the host decoder's;
- end to end: the coded route, the host route and the definition agree on two files, and fri_driver decode-file --preview writes the same thumbnail."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.api as api
import frave_amd.emit as emit
from frave_amd.api import COLOUR_NONE, COLOUR_RCT, COLOUR_YCBCR, DECODE_TRUNCATED, DEQUANT_MIDPOINT, DEQUANT_MULTIPLY, DEQUANT_REFERENCE, TILED_ALLOW_HOLES, PlanTiled
from tests import preview_ref
from tests.coded_cases import file_of_image, tiled420_file, tiled_file
from tests.test_gpu_decode import Decode
from tests.test_gpu_instances import Guarded
from tests.test_preview_host import cut_stream_file
from tests.tiled_ref import mixed_image, parse_frit

preview_size = api.preview_size  # (without the feature the module fails here)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELAXED = 2  # hipStreamCaptureModeRelaxed
NONE = preview_ref.NONE


@pytest.fixture(scope="module")
def ctx():
    c = fa.Context(0)
    yield c
    c.close()


def _random_planes(T, seed):
    """full planes int32 [n_tiles][C][F][512]: None where the lattice has no node, small values with a few large ones (the clamp) elsewhere, a pixel-like DC"""
    rng = np.random.default_rng(seed)
    shape = (T.n_tiles, T.channels, T.num_cells, 512)
    co = rng.integers(-40, 41, shape).astype(np.int32)
    co[rng.random(shape) < 0.02] *= 9
    co[..., 0] = rng.integers(-20, 300, shape[:3])
    co[:, :, ~T.tile.valid_bits()] = NONE
    return co


def _definition(T, full, levels, shift, qm):
    """P_L through the inverse kernel and the merge, then the subsample"""
    image = T.decode_image_tiled(preview_ref.prefix_planes(full, levels), qm).reshape(T.height, T.width, T.channels)
    return preview_ref.subsample(image, shift)


def _k14(torch, T, full, levels, shift, qm, node_stride, offset=0, pad=8):
    """one fri_hip_preview_tiles_dev call: the planes at `node_stride` with a stride larger than needed, the output `offset` bytes off alignment between guard bytes"""
    w, h = preview_size(T.width, T.height, shift)
    planes = full[..., :node_stride].reshape(T.n_tiles * T.channels, -1)
    stride = planes.shape[1] + pad
    host = np.full((planes.shape[0], stride), 0x5A5A5A5, np.int32)
    host[:, : planes.shape[1]] = planes
    d_coefs = torch.from_numpy(host).cuda()
    out = Guarded(torch, w * h * T.channels, offset=offset, salt=7)
    T.preview_tiles_dev(d_coefs.data_ptr(), stride, node_stride, levels, shift, out.ptr, qm)
    regions, intact = out.get(torch)
    assert intact, "K14 wrote outside its output"
    return regions[0].reshape(h, w, T.channels)


def test_every_level_with_every_shift(ctx):
    import torch

    # 41 x 37 in 24 x 20 tiles: the image is no multiple of the tile, the tile no multiple of 8 or 16, and W = 41 clamps the last sample of S = 8 to column 40
    T = PlanTiled(ctx, 41, 37, 3, 24, 20, TILED_ALLOW_HOLES)
    full = _random_planes(T, 1)
    qm = api.quality_matrix(60)
    T.tile.set_dequantiser(DEQUANT_MIDPOINT)
    for levels in range(10):
        image = T.decode_image_tiled(preview_ref.prefix_planes(full, levels), qm).reshape(37, 41, 3)
        assert np.unique(image).size > 8, "the planes make no picture to compare"
        for shift in range(5):
            want = preview_ref.subsample(image, shift)
            for node_stride in (512, 1 << levels):
                got = _k14(torch, T, full, levels, shift, qm, node_stride, offset=(levels + shift) % 4)
                assert np.array_equal(got, want), (levels, shift, node_stride)
    assert preview_ref.subsample(image, 3).shape == (5, 6, 3) and np.array_equal(preview_ref.subsample(image, 3)[:, 5], image[np.minimum(np.arange(5) * 8 + 4, 36), 40])
    T.close()


# (W, H, C, tile_w, tile_h, flags): a 1 x 1 grid whose last sample clamps at S = 8; a 3 x 2 grid, tile sides no multiple of S; 64 x 64 tiles, which leave pixels to no cell
SHAPES = [(41, 30, 1, 41, 30, TILED_ALLOW_HOLES), (100, 70, 3, 36, 37, TILED_ALLOW_HOLES), (150, 100, 1, 64, 64, TILED_ALLOW_HOLES), (150, 100, 3, 64, 64, TILED_ALLOW_HOLES)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d_%dx%d" % s[:5])
def test_k14_is_the_definition(ctx, shape):
    import torch

    w, h, c, tw, th, flags = shape
    T = PlanTiled(ctx, w, h, c, tw, th, flags)
    full = _random_planes(T, w + h)
    if (tw, th) == (64, 64):
        assert T.tile.owned_pixels() < 64 * 64  # some samples have no owner and must read 0
    colours = (COLOUR_NONE, COLOUR_RCT, COLOUR_YCBCR) if c == 3 else (COLOUR_NONE,)
    k = 0
    for colour in colours:
        if c == 3:
            T.tile.set_colour_transform(colour)
        for dequant, quality in ((DEQUANT_REFERENCE, 100), (DEQUANT_REFERENCE, 35), (DEQUANT_MULTIPLY, 35), (DEQUANT_MIDPOINT, 35)):
            T.tile.set_dequantiser(dequant)
            qm = api.quality_matrix(quality)
            for levels, shift in ((9, 0), (7, 1), (5, 2), (3, 3), (1, 4), (0, 3), (8, 3)):
                want = _definition(T, full, levels, shift, qm)
                k += 1
                got = _k14(torch, T, full, levels, shift, qm, 512 if k % 2 else 1 << levels, offset=(0, 1, 3)[k % 3])
                assert np.array_equal(got, want), (colour, dequant, quality, levels, shift)
                if (tw, th) == (64, 64) and shift == 0:
                    assert (want.reshape(-1, c) == 0).all(axis=1).any()
    T.close()


def test_k14_against_the_oracles_inverse(ctx):
    import torch

    frv = tiled_file(334, 350, 3, 167, 117, 100, rct=True)[0]
    ti, full = emit.tiled_decode(frv)
    T = PlanTiled(ctx, 334, 350, 3, 167, 117)
    T.tile.set_colour_transform(COLOUR_RCT)
    for levels, shift in ((5, 2), (9, 0), (2, 3)):
        want = preview_ref.subsample(preview_ref.lossless_preview_image(full, 334, 350, 167, 117, levels, rct=True), shift)
        assert np.array_equal(_k14(torch, T, full, levels, shift, None, 1 << levels, offset=1), want), (levels, shift)
    T.close()


def test_k14_replays_from_a_graph_and_refuses_bad_arguments(ctx):
    import torch

    hip = C.CDLL("libamdhip64.so")
    T = PlanTiled(ctx, 100, 70, 3, 36, 37, TILED_ALLOW_HOLES)
    full = _random_planes(T, 5)
    levels, shift = 5, 2
    qm = api.quality_matrix(50)
    want = _definition(T, full, levels, shift, qm)
    w, h = preview_size(100, 70, shift)
    compact = np.ascontiguousarray(full[..., :32])
    d_coefs = torch.from_numpy(compact.reshape(-1)).cuda()
    out = Guarded(torch, w * h * 3, offset=3, salt=9)
    plane = T.num_cells * 32
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    T.preview_tiles_dev(d_coefs.data_ptr(), plane, 32, levels, shift, out.ptr, qm, stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    n_nodes = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 1
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    regions, intact = out.get(torch)
    assert intact and np.array_equal(regions[0], out.fill[out.start : out.start + out.size]), "capturing ran the kernel"
    for _ in range(2):
        out.raw.copy_(torch.from_numpy(out.fill))
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(ex, sp) == 0
        s.synchronize()
        regions, intact = out.get(torch)
        assert intact and np.array_equal(regions[0].reshape(h, w, 3), want)
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    # argument errors launch nothing
    out.raw.copy_(torch.from_numpy(out.fill))
    p = d_coefs.data_ptr()
    for args in ((p, plane, 64, levels, shift, out.ptr), (p, plane, 32, 10, shift, out.ptr), (p, plane, 32, levels, 5, out.ptr), (p, plane - 1, 32, levels, shift, out.ptr),
                 (0, plane, 32, levels, shift, out.ptr), (p, plane, 32, levels, shift, 0), (p, plane, 512, levels, shift, out.ptr)):
        with pytest.raises(fa.FriHipError) as e:
            T.preview_tiles_dev(*args, qm)
        assert e.value.code == -1, args
    with pytest.raises(fa.FriHipError) as e:
        T.preview(compact, 10, 0)
    assert e.value.code == -1
    regions, intact = out.get(torch)
    assert intact and np.array_equal(regions[0], out.fill[out.start : out.start + out.size])
    T.close()


# ---- K13 bounded ------------------------------------------------------------------------------------------------------------------------------------------------

class DecodeLevels(Decode):
    def launch_levels(self, levels, stream=0):
        i = {name: g for name, (g, rows) in self.inputs.items()}
        return api.decode_planes_dev(self.plan, self.planes, i["words"].ptr, self.word_stride, i["n_words"].ptr, i["models"].ptr, i["off"].ptr, i["vp"].ptr, i["wp"].ptr,
                                     self.coefs.ptr, self.coef_stride, self.status.ptr, self.scratch_ptr, stream, levels=levels)


def _small_tile_file():
    """40 x 20 in 20 x 20 tiles: so few cells that the DC scan, the root scan and level 1 share the first 64-entry chunk"""
    return file_of_image(mixed_image(40, 20, 1, 20, 5), 20, 20, 100)[0], 20, 20


@pytest.mark.parametrize("name", ["small", "100x70"])
def test_bounded_k13_is_the_hosts_compact_planes_expanded(ctx, name):
    frv, tw, th = _small_tile_file() if name == "small" else (tiled_file(100, 70, 1, 52, 50, 100)[0], 52, 50)
    d = DecodeLevels(ctx, tw, th, emit.tiled_parse_coded(frv))
    bits = d.plan.valid_bits()
    counts = [d.plan.num_some_levels(levels) for levels in range(10)]
    if name == "small":
        assert counts[2] < 64 < counts[9], "DC, root and level 1 share one chunk"
    assert any(n % 64 for n in counts)
    full = emit.tiled_decode(frv)[1].reshape(-1, d.F, 512)
    for levels in (0, 1, 2, 5, 8, 9):
        d.clear()
        d.launch_levels(levels)
        coefs, status = d.read()
        assert not status.any(), (levels, status)
        compact = emit.tiled_decode_levels(frv, levels)[1].reshape(-1, d.F, 1 << levels)
        assert np.array_equal(coefs, preview_ref.expand(compact, bits)), levels
    # fri_hip_decode_planes_dev is the L = 9 launch: the same bytes, the host decoder's planes
    nine = d.raw()
    d.clear()
    d.launch()
    assert all(np.array_equal(a, b) for a, b in zip(nine, d.raw()))
    coefs, status = d.read()
    assert not status.any() and np.array_equal(coefs, full)
    with pytest.raises(fa.FriHipError) as e:
        d.launch_levels(10)
    assert e.value.code == -1
    d.close()


def test_damage_beyond_the_prefix_is_not_seen_on_the_device(ctx):
    cut, plane, low = cut_stream_file()
    d = DecodeLevels(ctx, 125, 125, emit.tiled_parse_coded(cut))
    d.launch_levels(low)
    coefs, status = d.read()
    assert not status.any()
    compact = emit.tiled_decode_levels(cut, low)[1].reshape(-1, d.F, 1 << low)
    assert np.array_equal(coefs, preview_ref.expand(compact, d.plan.valid_bits()))
    d.clear()
    d.launch_levels(9)
    coefs, status = d.read()
    assert status[plane, 0] == DECODE_TRUNCATED and status[plane, 1] > d.plan.num_some_levels(low) and not np.delete(status, plane, axis=0).any()
    d.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------------

FILES = {"rct": (334, 350, 3, 167, 117, 100, dict(rct=True)), "ycbcr37": (334, 350, 3, 167, 117, 37, dict(ycbcr=True))}


def _decoder_plan(ctx, ti):
    """the tiled plan as FRIDecoder sets it up for a file"""
    T = PlanTiled(ctx, ti[0], ti[1], ti[6], ti[2], ti[3], TILED_ALLOW_HOLES)
    T.set_stream_order()
    if ti[6] == 3:
        T.tile.set_colour_transform(COLOUR_RCT if ti.rct else COLOUR_YCBCR if ti.ycbcr else COLOUR_NONE)
    T.tile.set_dequantiser(DEQUANT_MIDPOINT if ti.quality else DEQUANT_REFERENCE)
    return T, api.quality_matrix(ti.quality) if ti.quality else None


@pytest.mark.parametrize("name", sorted(FILES))
def test_coded_route_host_route_and_definition_agree(ctx, name):
    w, h, c, tw, th, quality, flags = FILES[name]
    frv = tiled_file(w, h, c, tw, th, quality, **flags)[0]
    ti, full = emit.tiled_decode(frv)
    coded = emit.tiled_parse_coded(frv)
    T, qm = _decoder_plan(ctx, ti)
    for levels, shift in ((7, 1), (5, 2), (3, 3), (9, 0), (0, 4)):
        want = _definition(T, full, levels, shift, qm)
        host = T.preview(emit.tiled_decode_levels(frv, levels)[1], levels, shift, qm)
        device, status = T.preview_coded(coded, levels, shift, qm)
        assert not status.any() and np.array_equal(host, want) and np.array_equal(device, want), (levels, shift)
    T.close()


def test_coded_route_reports_a_refused_plane(ctx):
    cut, plane, low = cut_stream_file()
    ti = emit.tiled_info(cut)
    T, qm = _decoder_plan(ctx, ti)
    coded = emit.tiled_parse_coded(cut)
    out, status = T.preview_coded(coded, low, 3, qm)  # the damage lies behind the prefix
    assert not status.any() and np.array_equal(out, T.preview(emit.tiled_decode_levels(cut, low)[1], low, 3, qm))
    with pytest.raises(fa.FriHipError) as e:
        T.preview_coded(coded, 9, 0, qm)
    assert e.value.code == -1 and e.value.status[plane, 0] == DECODE_TRUNCATED
    T.close()


def _read_pnm(path):
    data = path.read_bytes()
    magic, size, maxval, rest = data.split(b"\n", 3)
    w, h = (int(v) for v in size.split())
    return np.frombuffer(rest, np.uint8).reshape(h, w, 1 if magic == b"P5" else 3)


def test_driver_preview(ctx, tmp_path):
    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h, c, tw, th, quality, flags = FILES["ycbcr37"]
    frv = tiled_file(w, h, c, tw, th, quality, **flags)[0]
    src = tmp_path / "in.frv"
    src.write_bytes(frv)
    ti = emit.tiled_info(frv)
    T, qm = _decoder_plan(ctx, ti)
    for m in (1, 3):
        want = T.preview(emit.tiled_decode_levels(frv, 9 - 2 * m)[1], 9 - 2 * m, m, qm)
        for extra in ([], ["--device-rans"]):
            dst = tmp_path / ("m%d%s.ppm" % (m, "d" if extra else ""))
            out = subprocess.run([driver, "decode-file", str(src), str(dst), "--preview", str(m)] + extra, capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stdout + out.stderr
            assert np.array_equal(_read_pnm(dst), want), (m, extra)
    T.close()
    refused = tmp_path / "r.ppm"
    out = subprocess.run([driver, "decode-file", str(src), str(refused), "--preview", "2", "--region", "0,0,8,8"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "out of scope" in out.stderr and "--region" in out.stderr and not refused.exists()
    out = subprocess.run([driver, "decode-file", str(src), str(refused), "--preview", "5"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and not refused.exists()
    frif = tmp_path / "tile.frv"
    frif.write_bytes(parse_frit(frv)["payloads"][0])
    s420 = tmp_path / "420.frv"
    s420.write_bytes(tiled420_file(100, 70, 52, 50, 60)[0])
    for path, word in ((frif, "decode an untiled file whole"), (s420, "decode it whole")):
        for extra in ([], ["--device-rans"]):
            out = subprocess.run([driver, "decode-file", str(path), str(refused), "--preview", "2"] + extra, capture_output=True, text=True, timeout=120)
            assert out.returncode != 0 and word in out.stderr and not refused.exists(), (path, extra, out.stderr)
