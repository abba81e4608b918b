"""Preview of regions on the device (include/fri_hip.h, "Preview of regions"): K17 (k17_preview_regions.hip) and the routes composed around it.

- K17 is the definition: the crops of PlanTiled.preview's thumbnail - every (L, m) on the smallest shape, both node strides, regions that are the whole thumbnail,
  the four corners, 17 wide (two blocks, one partial), across a tile corner, a repeat and an overlap; on lossless files also against tests/preview_regions_ref.py
  on the oracle's inverse, plain and RCT; a plan whose tiles are smaller than S = 16, where a listed tile holds no sample;
- the three dequantisers with a quality matrix, YCbCr and RCT;
- the output at an odd byte offset between guard bytes, the input the listed tiles only, between planes of a value that would show;
- a replay from a captured graph of the one kernel node; refused arguments launch nothing; the memory of the last table is not the one K15's entry keeps;
- the coded route, the host route and the definition agree; a refused plane is reported by its tile in the file's grid and no pixel is written;
- the decode routes of a tiled plan one after another on ONE plan, a small call first, give what each gives on a fresh plan (they share the staging buffers);
- fri_driver decode-regions --preview M writes the crops of decode-file --preview M, with and without --device-rans, and its refusals write nothing.

The forms that grow buffers (fri_hip_preview_regions_tiled, ..._coded) take no stream argument, so there is no capturing stream to hand them: what can be
captured is K17's entry, and the graph test captures it."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.api as api
import frave_amd.emit as emit
from frave_amd.api import COLOUR_NONE, COLOUR_RCT, COLOUR_YCBCR, DECODE_TRUNCATED, DEQUANT_MIDPOINT, DEQUANT_MULTIPLY, DEQUANT_REFERENCE, TILED_ALLOW_HOLES, PlanTiled
from tests import preview_ref
from tests import preview_regions_ref as ref
from tests.coded_cases import tiled420_file, tiled_file
from tests.test_gpu_instances import Guarded
from tests.test_gpu_preview import _decoder_plan, _random_planes, _read_pnm
from tests.test_preview_host import cut_stream_file
from tests.tiled_ref import parse_frit

plan_table, decode_tiles_levels = PlanTiled.preview_regions_table, emit.tiled_decode_tiles_levels  # (without the feature the module fails here)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELAXED = 2  # hipStreamCaptureModeRelaxed
CANARY = 0x5A5A5A5  # between the planes K17 is given: a node read from there dequantises to something the clamp cannot hide in every sample
# (W, H, C, tile_w, tile_h): the small shapes of tests/test_gpu_preview.py
SMALL, MIDDLE, HOLES = (41, 37, 3, 24, 20), (100, 70, 3, 36, 37), (150, 100, 1, 64, 64)
TINY = (61, 45, 1, 7, 9)  # tile sides below 16: at m = 4 the source rectangles span tiles without a sample


@pytest.fixture(scope="module")
def ctx():
    c = fa.Context(0)
    yield c
    c.close()


def region_set(shape, shift):
    """regions of the thumbnail at `shift`: the whole thumbnail, the four 1 x 1 corners, a 17-wide region (two blocks, one partial) where there is room, a region
    across the corner of the first tile, a repeat of it, an overlap with it"""
    w, h, c, tile_w, tile_h = shape
    tw, th = ref.thumbnail_size(w, h, shift)
    regs = [(0, 0, tw, th), (0, 0, 1, 1), (tw - 1, 0, 1, 1), (0, th - 1, 1, 1), (tw - 1, th - 1, 1, 1)]
    if tw >= 17:
        regs.append((tw - 17, th // 3, 17, min(3, th - th // 3)))
    s = 1 << shift
    cx, cy = min(max(tile_w // s, 1), tw - 1), min(max(tile_h // s, 1), th - 1)  # the first sample right of, and below, the first tile - or the last sample
    corner = (cx - 1, cy - 1, min(3, tw - cx + 1), min(3, th - cy + 1))
    return regs + [corner, corner, (cx - 1, 0, tw - cx + 1, cy)]


def _k17(torch, T, full, levels, shift, qm, node_stride, regs, offset=1, pad=8):
    """one fri_hip_preview_tiles_regions_dev call on the planes `full` [n_tiles][C][F][512] of the whole file: the listed tiles' planes only, at `node_stride`, with a
    stride larger than needed and CANARY in the gaps and on both sides; the packed output `offset` bytes off alignment between guard bytes -> the regions' rasters"""
    tiles, table = plan_table(T, shift, regs)
    planes = full[tiles][..., :node_stride].reshape(tiles.size * T.channels, -1)
    stride = planes.shape[1] + pad
    host = np.full((planes.shape[0] + 2, stride), CANARY, np.int32)
    host[1:-1, : planes.shape[1]] = planes
    d_coefs = torch.from_numpy(host).cuda()
    d_table = torch.from_numpy(table.view(np.int32).copy()).cuda()
    total = int(table[8 * len(regs) + 4]) | int(table[8 * len(regs) + 5]) << 32
    assert total == ref.packed_offsets(T.channels, regs)[-1]
    out = Guarded(torch, total, offset=offset, salt=7)
    T.preview_tiles_regions_dev(d_coefs.data_ptr() + 4 * stride, stride, node_stride, levels, shift, tiles.size, len(regs), d_table.data_ptr(), out.ptr, qm)
    (packed,), intact = out.get(torch)
    assert intact, "K17 wrote outside the packed output"
    assert np.array_equal(d_coefs.cpu().numpy(), host)  # the input comes back intact
    return T._split_regions(packed, np.array(regs, np.uint32))


def _same(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, int((a != b).sum()))


def test_every_level_with_every_shift_is_the_crop_of_the_preview(ctx):
    import torch

    w, h, c, tw, th = SMALL
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    full = _random_planes(T, 1)
    qm = api.quality_matrix(60)
    T.tile.set_dequantiser(DEQUANT_MIDPOINT)
    for shift in range(5):
        regs = region_set(SMALL, shift)
        want_list, want_table = ref.preview_tile_list(w, h, tw, th, shift, regs), ref.preview_region_table(w, h, c, tw, th, shift, regs)
        got_list, got_table = plan_table(T, shift, regs)
        assert got_list.tolist() == want_list and np.array_equal(got_table, want_table)
        assert shift > 1 or int(want_table[8 * 5 + 7]) == 2  # the 17-wide region: two blocks in a row
        for levels in range(10):
            thumbnail = T.preview(full[..., : 1 << levels], levels, shift, qm)
            assert levels < 3 or shift > 2 or np.unique(thumbnail).size > 8, "the planes make no picture to compare"
            want = ref.crops(thumbnail, regs)
            for node_stride in (512, 1 << levels):
                _same(_k17(torch, T, full, levels, shift, qm, node_stride, regs, offset=1 + 2 * ((levels + shift) % 2)), want, (levels, shift, node_stride))
    T.close()


@pytest.mark.parametrize("shape", [MIDDLE, HOLES], ids=lambda s: "x".join(map(str, s)))
def test_dequantisers_and_colour_transforms(ctx, shape):
    import torch

    w, h, c, tw, th = shape
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    full = _random_planes(T, w + h)
    if shape == HOLES:
        assert T.tile.owned_pixels() < tw * th  # some samples have no owner and must read 0
    k = 0
    for colour in (COLOUR_NONE, COLOUR_RCT, COLOUR_YCBCR) if c == 3 else (COLOUR_NONE,):
        if c == 3:
            T.tile.set_colour_transform(colour)
        for dequant, quality in ((DEQUANT_REFERENCE, 100), (DEQUANT_REFERENCE, 35), (DEQUANT_MULTIPLY, 35), (DEQUANT_MIDPOINT, 35)):
            T.tile.set_dequantiser(dequant)
            qm = api.quality_matrix(quality)
            for levels, shift in ((9, 0), (7, 1), (5, 2), (3, 3), (1, 4)):
                regs = region_set(shape, shift)
                thumbnail = T.preview(full[..., : 1 << levels], levels, shift, qm)
                k += 1
                got = _k17(torch, T, full, levels, shift, qm, 512 if k % 2 else 1 << levels, regs, offset=(1, 3, 5)[k % 3])
                _same(got, ref.crops(thumbnail, regs), (colour, dequant, quality, levels, shift))
                if shape == HOLES and shift == 0:
                    assert (got[0].reshape(-1, c) == 0).all(axis=1).any()
    T.close()


def test_a_listed_tile_without_a_sample_is_never_read(ctx):
    """61 x 45 in 7 x 9 tiles at m = 4: samples are 16 apart, the source rectangles span tiles that hold none. Such a tile's planes are CANARY here: read, they show."""
    import torch

    w, h, c, tw, th = TINY
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)  # (a plan with tile sides below 16 can be created: tests/test_preview_regions_host.py has its table)
    full = _random_planes(T, 9)
    shift, levels = 4, 3
    regs = region_set(TINY, shift)
    listed, sampled = ref.preview_tile_list(w, h, tw, th, shift, regs), ref.sampled_tiles(w, h, tw, th, shift, regs)
    assert set(sampled) < set(listed)
    thumbnail = T.preview(full[..., : 1 << levels], levels, shift)
    spoiled = full.copy()
    spoiled[sorted(set(listed) - set(sampled))] = CANARY
    for node_stride in (512, 1 << levels):
        _same(_k17(torch, T, spoiled, levels, shift, None, node_stride, regs), ref.crops(thumbnail, regs), node_stride)
    T.close()


@pytest.mark.parametrize("name", ["plain", "rct"])
def test_k17_against_the_oracles_inverse(ctx, name):
    import torch

    w, h, c, tw, th, quality, flags = (250, 250, 1, 125, 125, 100, {}) if name == "plain" else (334, 350, 3, 167, 117, 100, dict(rct=True))
    frv = tiled_file(w, h, c, tw, th, quality, **flags)[0]
    ti, full = emit.tiled_decode(frv)
    T = PlanTiled(ctx, w, h, c, tw, th)
    if name == "rct":
        T.tile.set_colour_transform(COLOUR_RCT)
    shape = (w, h, c, tw, th)
    for levels, shift in ((5, 2), (9, 0), (2, 3)):
        regs = region_set(shape, shift)
        image = preview_ref.lossless_preview_image(full, w, h, tw, th, levels, rct=name == "rct")
        _same(_k17(torch, T, full, levels, shift, None, 1 << levels, regs), ref.region_pixels(image, shift, regs), (levels, shift))
    # at m = 0, L = 9 the result is that of fri_hip_decode_regions_tiled
    regs = region_set(shape, 0)
    tiles = plan_table(T, 0, regs)[0]
    assert tiles.tolist() == T.regions(regs)[0].tolist()
    _same(T.preview_regions(full[tiles], 9, 0, regs), T.decode_regions_tiled(full[tiles], regs), "m = 0, L = 9")
    T.close()


def test_graph_replay_argument_checks_and_the_two_memories(ctx):
    import torch

    hip = C.CDLL("libamdhip64.so")
    w, h, c, tw, th = MIDDLE
    T = PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    full = _random_planes(T, 5)
    levels, shift = 5, 2
    qm = api.quality_matrix(50)
    regs = region_set(MIDDLE, shift)
    want = np.concatenate([r.reshape(-1) for r in ref.crops(T.preview(full[..., :32], levels, shift, qm), regs)])
    tiles, table = plan_table(T, shift, regs)
    d_coefs = torch.from_numpy(np.ascontiguousarray(full[tiles][..., :32]).reshape(-1)).cuda()
    d_table = torch.from_numpy(table.view(np.int32).copy()).cuda()
    out = Guarded(torch, want.size, offset=3, salt=9)
    plane = T.num_cells * 32
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    T.preview_tiles_regions_dev(d_coefs.data_ptr(), plane, 32, levels, shift, tiles.size, len(regs), d_table.data_ptr(), out.ptr, qm, stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    n_nodes = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 1
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    (packed,), intact = out.get(torch)
    assert intact and np.array_equal(packed, out.fill[out.start : out.start + out.size]), "capturing ran the kernel"
    for _ in range(2):
        out.raw.copy_(torch.from_numpy(out.fill))
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(ex, sp) == 0
        s.synchronize()
        (packed,), intact = out.get(torch)
        assert intact and np.array_equal(packed, want)
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    # argument errors launch nothing
    out.raw.copy_(torch.from_numpy(out.fill))
    p, t, n, r = d_coefs.data_ptr(), d_table.data_ptr(), tiles.size, len(regs)
    good = (p, plane, 32, levels, shift, n, r, t, out.ptr)
    T.preview_tiles_regions_dev(*good, qm)
    (packed,), intact = out.get(torch)
    assert intact and np.array_equal(packed, want)
    out.raw.copy_(torch.from_numpy(out.fill))
    for args in ((p, plane, 32, levels, shift, n, r + 1, t, out.ptr), (p, plane, 32, levels, shift, n - 1, r, t, out.ptr), (p, plane, 32, levels, shift + 1, n, r, t, out.ptr),
                 (p, plane, 32, levels, shift, 0, r, t, out.ptr), (p, plane, 32, levels, shift, n, 0, t, out.ptr), (p, plane, 32, levels, shift, T.n_tiles + 1, r, t, out.ptr),
                 (0, plane, 32, levels, shift, n, r, t, out.ptr), (p, plane, 32, levels, shift, n, r, 0, out.ptr), (p, plane, 32, levels, shift, n, r, t, 0),
                 (p, plane, 32, 10, shift, n, r, t, out.ptr), (p, plane, 32, levels, 5, n, r, t, out.ptr), (p, plane, 64, levels, shift, n, r, t, out.ptr),
                 (p, plane, 512, levels, shift, n, r, t, out.ptr), (p, plane - 1, 32, levels, shift, n, r, t, out.ptr)):
        with pytest.raises(fa.FriHipError) as e:
            T.preview_tiles_regions_dev(*args, qm)
        assert e.value.code == -1, args
    compact = np.ascontiguousarray(full[tiles][..., :32])
    for call in (lambda: T.preview_regions(compact, 10, shift, regs), lambda: T.preview_regions(compact, levels, 5, regs), lambda: T.preview_regions(compact, levels, shift, []),
                 lambda: T.preview_regions(compact, levels, shift, [(0, 0, 26, 1)]), lambda: T.preview_regions(compact, levels, shift, [(0, 0, 0, 1)])):
        with pytest.raises(fa.FriHipError) as e:
            call()
        assert e.value.code == -1
    L = fa.load_library()
    rg, qq, px = np.array(regs, np.uint32), api.quality_matrix(50), np.zeros(want.size, np.uint8)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for a in ((None, P(qq), P(rg), P(px)), (P(compact), None, P(rg), P(px)), (P(compact), P(qq), None, P(px)), (P(compact), P(qq), P(rg), None)):
        assert L.fri_hip_preview_regions_tiled(T._h, a[0], levels, shift, a[1], len(regs), a[2], a[3]) == -1
    (packed,), intact = out.get(torch)
    assert intact and np.array_equal(packed, out.fill[out.start : out.start + out.size])
    # two memories: a table of "Several regions" does not change what K17's entry accepts, and a preview table does not change what K15's accepts
    image_regs = [(0, 0, w, h), (3, 3, 5, 5), (50, 40, 20, 20)]
    list15, table15 = T.regions(image_regs)
    assert len(image_regs) != r and table15.size != table.size
    T.preview_tiles_regions_dev(*good, qm)
    (packed,), intact = out.get(torch)
    assert intact and np.array_equal(packed, want)
    raster = np.random.default_rng(3).integers(0, 256, (list15.size, th, tw, c), dtype=np.uint8)
    d_raster, d_table15 = torch.from_numpy(raster.reshape(-1)).cuda(), torch.from_numpy(table15.view(np.int32).copy()).cuda()
    total15 = sum(rw * rh * c for _, _, rw, rh in image_regs)
    d_out15 = torch.zeros(total15, dtype=torch.uint8, device="cuda")
    plan_table(T, shift, regs[:2])  # a preview table in between
    T.merge_tiles_regions_dev(d_raster.data_ptr(), list15.size, len(image_regs), d_table15.data_ptr(), d_out15.data_ptr())
    torch.cuda.synchronize()
    from tests.tiled_regions_ref import merge_regions_fast

    assert np.array_equal(d_out15.cpu().numpy(), merge_regions_fast(raster, list15.tolist(), w, h, tw, th, image_regs))
    with pytest.raises(fa.FriHipError) as e:  # ... and K17's entry now wants the table of two regions
        T.preview_tiles_regions_dev(*good, qm)
    assert e.value.code == -1 and "fri_hip_plan_tiled_preview_regions" in str(e.value)
    T.close()


FILES = {"rct": (334, 350, 3, 167, 117, 100, dict(rct=True)), "ycbcr37": (334, 350, 3, 167, 117, 37, dict(ycbcr=True))}


@pytest.mark.parametrize("name", sorted(FILES))
def test_coded_route_host_route_and_definition_agree(ctx, name):
    w, h, c, tw, th, quality, flags = FILES[name]
    frv = tiled_file(w, h, c, tw, th, quality, **flags)[0]
    ti = emit.tiled_info(frv)
    T, qm = _decoder_plan(ctx, ti)
    for levels, shift in ((7, 1), (5, 2), (3, 3), (9, 0), (0, 4)):
        regs = region_set((w, h, c, tw, th), shift)[5:]  # without the whole thumbnail and the corners: the last row of tiles is not listed
        tiles = plan_table(T, shift, regs)[0]
        assert 1 < tiles.size < T.n_tiles
        want = ref.crops(T.preview(emit.tiled_decode_levels(frv, levels)[1], levels, shift, qm), regs)
        _same(T.preview_regions(decode_tiles_levels(frv, tiles, levels)[1], levels, shift, regs, qm), want, ("host", levels, shift))
        got, status = T.preview_regions_coded(emit.tiled_parse_coded_tiles(frv, tiles), levels, shift, regs, qm)
        assert status.shape == (tiles.size * c, 4) and not status.any()
        _same(got, want, ("coded", levels, shift))
    T.close()


def test_routes_in_turn_on_one_plan_equal_fresh_plans(ctx):
    """The decode routes share the plan's staging buffers (coefs, rans_words, region_table, regions_out, preview) and each grows what it needs: on ONE plan a
    small call first and larger ones behind it - regions coded in one tile, the whole image coded, a preview of two regions coded, the preview coded, every tile
    as one region from host planes - each give the bytes of the same call on a fresh plan. The lossless RGB file of this module (2 x 3 tiles, the smallest
    lossless RGB file the GPU tests build)."""
    w, h, c, tw, th, quality, flags = FILES["rct"]
    frv = tiled_file(w, h, c, tw, th, quality, **flags)[0]
    ti = emit.tiled_info(frv)
    whole, one, two, every = emit.tiled_parse_coded(frv), [(5, 7, 20, 10)], [(3, 3, 20, 20), (100, 120, 40, 30)], [(0, 0, w, h)]
    routes = [
        lambda T, qm: T.decode_regions_coded(emit.tiled_parse_coded_tiles(frv, T.regions(one)[0]), one, qm),
        lambda T, qm: T.decode_coded(whole, qm),
        lambda T, qm: T.preview_regions_coded(emit.tiled_parse_coded_tiles(frv, plan_table(T, 1, two)[0]), 7, 1, two, qm),
        lambda T, qm: T.preview_coded(whole, 5, 2, qm),
        lambda T, qm: (T.decode_regions_tiled(emit.tiled_decode_tiles(frv, T.regions(every)[0])[1], every, qm), None),
    ]

    def parts(result):
        pixels, status = result
        return list(pixels) if isinstance(pixels, list) else [pixels], status

    T, qm = _decoder_plan(ctx, ti)
    assert (T.nx, T.ny) == (2, 3) and T.regions(one)[0].tolist() == [0] and plan_table(T, 1, two)[0].tolist() == [0, 5] and T.regions(every)[0].size == 6
    seen = []
    for k, route in enumerate(routes):
        got, status = parts(route(T, qm))
        F, _ = _decoder_plan(ctx, ti)
        want, want_status = parts(route(F, qm))
        F.close()
        assert len(got) == len(want) and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want)), k
        assert status is None or (np.array_equal(status, want_status) and not status.any()), k
        seen.append(got)
    assert np.array_equal(seen[4][0].reshape(-1), seen[1][0])  # the last route's one region is the whole image
    T.close()


def test_coded_route_reports_a_refused_plane_by_its_tile(ctx):
    cut, plane, low = cut_stream_file()  # 250 x 250 x 1 in 2 x 2 tiles, lossless; tile 1's plane cut to half its words
    ti = emit.tiled_info(cut)
    T, qm = _decoder_plan(ctx, ti)
    shift = 1
    touching = [(70, 5, 10, 10), (110, 110, 3, 3)]  # thumbnail coordinates at m = 1: tiles 1 and 3, the cut plane is entry 0 of the list
    tiles = plan_table(T, shift, touching)[0].tolist()
    assert tiles == [1, 3]
    coded = emit.tiled_parse_coded_tiles(cut, tiles)
    got, status = T.preview_regions_coded(coded, low, shift, touching, qm)  # the damage lies behind the prefix
    assert not status.any()
    _same(got, T.preview_regions(decode_tiles_levels(cut, tiles, low)[1], low, shift, touching, qm), "behind the prefix")
    L = fa.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    words, n_words, models, off, vp, wp = api._coded_planes(coded, 2)
    rg, qq = np.array(touching, np.uint32), np.ones(32, np.int32)
    pixels, st = np.full(sum(r[2] * r[3] for r in touching), 0xA5, np.uint8), np.zeros((2, 4), np.uint32)
    rc = L.fri_hip_preview_regions_tiled_coded(T._h, 2, P(rg), P(words), words.shape[1], P(n_words), P(models), P(off), P(vp), P(wp), 9, shift, P(qq), P(pixels), P(st))
    assert rc == -1 and (pixels == 0xA5).all() and st[0, 0] & DECODE_TRUNCATED and not st[1, 0]
    with pytest.raises(fa.FriHipError) as e:
        T.preview_regions_coded(coded, 9, shift, touching, qm)
    assert e.value.code == -1 and e.value.tile == 1 and "tile 1: channel 0" in str(e.value)
    assert e.value.status[0, 0] & DECODE_TRUNCATED and not e.value.status[1, 0]
    # regions that do not touch the damaged tile decode at every level
    beside = [(3, 3, 20, 20), (5, 70, 80, 30)]  # tiles 0, 2, 3
    tiles = plan_table(T, shift, beside)[0].tolist()
    assert tiles == [0, 2, 3]
    got, status = T.preview_regions_coded(emit.tiled_parse_coded_tiles(cut, tiles), 9, shift, beside, qm)
    assert not status.any()
    _same(got, T.preview_regions(decode_tiles_levels(cut, tiles, 9)[1], 9, shift, beside, qm), "beside the damage")
    T.close()


def test_driver_decodes_regions_of_the_preview(ctx, tmp_path):
    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h, c, tw, th, quality, flags = FILES["ycbcr37"]
    frv = tiled_file(w, h, c, tw, th, quality, **flags)[0]
    src = tmp_path / "in.frv"
    src.write_bytes(frv)

    def run(*args):
        return subprocess.run([driver, *map(str, args)], capture_output=True, text=True, timeout=300)

    def written(prefix):
        return sorted(glob.glob(str(prefix) + "*"))

    for m in (1, 3):
        whole = tmp_path / f"whole{m}.ppm"
        out = run("decode-file", src, whole, "--preview", m)
        assert out.returncode == 0, out.stdout + out.stderr
        thumbnail = _read_pnm(whole)
        regs = region_set((w, h, c, tw, th), m)
        region_args = [a for r in regs for a in ("--region", ",".join(map(str, r)))]
        for route, extra in (("host", []), ("device", ["--device-rans"])):
            prefix = tmp_path / f"m{m}_{route}"
            out = run("decode-regions", src, prefix, "--preview", m, *region_args, *extra)
            assert out.returncode == 0, out.stdout + out.stderr
            assert written(prefix) == sorted(f"{prefix}.{k}.ppm" for k in range(len(regs)))
            for k, (x, y, rw, rh) in enumerate(regs):
                assert np.array_equal(_read_pnm(tmp_path / f"m{m}_{route}.{k}.ppm"), thumbnail[y:y + rh, x:x + rw]), (m, route, k)
    # refused with nothing written: M outside 1..4, a region that leaves the thumbnail, no --region, a `frif` file, a tiled 4:2:0 file, a tiled RGBA file
    bad = tmp_path / "refused"
    pw, ph = ref.thumbnail_size(w, h, 2)
    for args in (["--preview", 0, "--region", "0,0,4,4"], ["--preview", 5, "--region", "0,0,4,4"], ["--preview", 2, "--region", f"{pw - 1},0,2,1"],
                 ["--preview", 2, "--region", f"0,{ph},1,1"], ["--preview", 2, "--region", "0,0,4,4", "--region", "0,0,0,4"], ["--preview", 2], ["--preview", 2, "--device-rans"],
                 ["--preview", "--region", "0,0,4,4"]):
        out = run("decode-regions", src, bad, *args)
        assert out.returncode != 0 and not written(bad), args
    assert run("decode-regions", src, bad, "--region", f"{pw - 1},0,2,1").returncode == 0 and written(bad)  # (the same numbers are a region of the image itself)
    for path in written(bad):
        os.remove(path)
    frif = tmp_path / "tile.frv"
    frif.write_bytes(parse_frit(frv)["payloads"][0])
    s420 = tmp_path / "420.frv"
    s420.write_bytes(tiled420_file(100, 70, 52, 50, 60)[0])
    from tests.test_tiled_rgba_host import GRIDS, _inputs
    from tests.tiled_rgba_ref import container

    rgba = tmp_path / "rgba.frv"
    rgba.write_bytes(container(*GRIDS[0], _inputs("lossless", GRIDS[0])[1]))
    for path, word in ((frif, "tiled"), (s420, "4:2:0"), (rgba, "tiled RGBA")):
        for extra in ([], ["--device-rans"]):
            out = run("decode-regions", path, bad, "--preview", 1, "--region", "0,0,4,4", *extra)
            assert out.returncode != 0 and word in out.stderr and not written(bad), (path, extra, out.stderr)
