"""What the preview of several regions of a tiled image in one call (fri_tiled_preview_regions_tiles, fri_tiled_decode_tiles_levels / fri_tiled_parse_coded_tiles,
fri_hip_preview_regions_tiled[_coded], K17's preview_regions_kernel) costs against the two routes the parent commit offers to the same pixels. Steps, each a
process of its own that appends its section to the report; run them under a time limit each and chained, so that trouble in one ends the run:

    timeout -k 10 300 python3 tools/preview_regions_time.py kernels && timeout -k 10 500 python3 tools/preview_regions_time.py host 512 && \
        timeout -k 10 500 python3 tools/preview_regions_time.py host 256

The image and the method are those of tools/regions_time.py: 4096^2 RGB, half smooth and half noise, lossless, in tiles of 512^2 (64 tiles) and of 256^2 (256
tiles). The region sets are 16 and 256 random 224^2 regions of the thumbnail from one seed, at m = 1 (L = 7, a thumbnail of 2048^2) and m = 3 (L = 3, 512^2).

kernels: K17 on a region set in one launch against ONE K14 launch for the whole thumbnail, timed with events around `launches` back-to-back repetitions; medians of
         interleaved rounds. Compact planes of random values (node stride 2^L); every repetition reads another copy of the planes and writes another copy of the
         output, out of pools of more bytes than the 256 MB cache. K17 reads the first T tiles' planes of a copy: the bytes differ from the listed tiles', their
         number and pattern do not. K17's regions are checked against the crops of K14's thumbnail on the listed tiles once, before the timing. The calls are
         made from Python through ctypes: where a kernel is shorter than such a call the figure is the host's rate of launching, for both kernels alike.
host:    the image through the device into a `frit` file; then, host to host, wall clock, medians of three, buffers allocated beforehand, the emitter on 16 threads:
           new call     fri_tiled_preview_regions_tiles + fri_tiled_decode_tiles_levels + fri_hip_preview_regions_tiled
           new, coded   fri_tiled_preview_regions_tiles + fri_tiled_parse_coded_tiles (the count query, then the planes) + fri_hip_preview_regions_tiled_coded
           whole + crop fri_tiled_decode_levels + fri_hip_preview_image_tiled for the whole thumbnail, then numpy crops into the packed output
           full + subsample  the source rectangles through fri_tiled_regions_tiles + fri_tiled_decode_tiles + fri_hip_decode_regions_tiled, then every S-th pixel
                        of every S-th row of each region's raster into the packed output
         Every region of the first three routes is checked against the crop of the whole thumbnail. The fourth reads the same places of the full-resolution image:
         point samples, not the node means of P_L, so its bytes are not the thumbnail's - it is what a caller without a preview of regions would show.

usage: python3 tools/preview_regions_time.py kernels | host TILE [--out profiles/preview_regions_time.txt] [--launches 20] [--rounds 5]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.region_time import Report, _mixed_image, _wall  # noqa: E402

SIZE, CHANNELS, SIDE = 4096, 3, 224
SETS = (16, 256)
TILES = (512, 256)
SHIFTS = (1, 3)  # m; L = 9 - 2 m
POOL = 512 << 20  # bytes a pool holds at least: twice the cache


def _args():
    a = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "preview_regions_time.txt"), "--launches": "20", "--rounds": "5"}
    pos = []
    i = 0
    while i < len(a):
        if a[i] in opt:
            opt[a[i]] = a[i + 1]
            i += 2
        else:
            pos.append(a[i])
            i += 1
    return pos, opt["--out"], int(opt["--launches"]), int(opt["--rounds"])


def region_set(np, n, shift):
    """n random SIDE x SIDE regions of the thumbnail at `shift`; the first 16 of the 256 are the set of 16"""
    side = SIZE >> shift
    rng = np.random.default_rng(224 + shift)
    xy = rng.integers(0, side - SIDE + 1, (max(SETS), 2))
    return [(int(x), int(y), SIDE, SIDE) for x, y in xy[:n]]


def source_rectangles(regs, shift):
    """(the image is a multiple of S: no sample is clamped) region (X, Y, w, h) reads every S-th pixel from (X S + S / 2, Y S + S / 2)"""
    s = 1 << shift
    return [(x * s + s // 2, y * s + s // 2, (w - 1) * s + 1, (h - 1) * s + 1) for x, y, w, h in regs]


def step_kernels(rep, n, rounds):
    import numpy as np
    import torch

    import frave_amd
    from frave_amd.api import TILED_ALLOW_HOLES

    ctx = frave_amd.Context(0)
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    L = frave_amd.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ones = np.ones(32, np.int32)
    rep.line(f"python3 tools/preview_regions_time.py kernels --launches {n} --rounds {rounds} (one process; medians of {rounds} interleaved rounds; us per repetition = one K17 "
             f"launch for the region set, or one K14 launch for the whole thumbnail; {SIZE}x{SIZE}x{CHANNELS}, thumbnail regions of {SIDE}x{SIDE}; calls from Python through ctypes)")

    def events(fn, count, at):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for i in range(at, at + count):
            fn(i)
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / count

    for tile in TILES:
        T = frave_amd.PlanTiled(ctx, SIZE, SIZE, CHANNELS, tile, tile, TILED_ALLOW_HOLES)
        h = T._h
        for shift in SHIFTS:
            levels = 9 - 2 * shift
            side = SIZE >> shift
            plane = T.num_cells << levels  # elements of one compact plane
            tile_elems = CHANNELS * plane
            all_elems = T.n_tiles * tile_elems
            thumb = side * side * CHANNELS
            slots = max(2, -(-POOL // (4 * all_elems)))
            d_coefs = torch.randint(-40, 41, (slots * all_elems,), dtype=torch.int32, device="cuda")
            d_thumb = torch.zeros(max(2, -(-POOL // thumb)) * thumb, dtype=torch.uint8, device="cuda")
            thumb_slots = d_thumb.numel() // thumb
            src = [d_coefs.data_ptr() + 4 * k * all_elems for k in range(slots)]
            dst14 = [d_thumb.data_ptr() + k * thumb for k in range(thumb_slots)]

            def k14(i):
                return L.fri_hip_preview_tiles_dev(h, src[i % slots], plane, 1 << levels, levels, shift, P(ones), dst14[i % thumb_slots], sp)

            for count in SETS:
                regs = region_set(np, count, shift)
                tiles, table = T.preview_regions_table(shift, regs)
                n_list, total, groups = int(tiles.size), int(table[8 * count + 4]) | int(table[8 * count + 5]) << 32, int(table[8 * count + 6])
                d_table = torch.from_numpy(table.view(np.int32).copy()).cuda()
                out_slots = max(2, -(-POOL // total))
                d_out = torch.zeros(out_slots * total, dtype=torch.uint8, device="cuda")
                dst17 = [d_out.data_ptr() + k * total for k in range(out_slots)]
                tp = d_table.data_ptr()
                # once, before the timing: K17 on the listed tiles of copy 0 against the crops of K14's thumbnail of copy 0
                listed = d_coefs[:all_elems].view(T.n_tiles, tile_elems)[torch.from_numpy(tiles.astype(np.int64)).cuda()].contiguous()
                assert L.fri_hip_preview_tiles_regions_dev(h, listed.data_ptr(), plane, 1 << levels, levels, shift, P(ones), n_list, count, tp, dst17[0], sp) == 0
                assert k14(0) == 0
                s.synchronize()
                whole = d_thumb[:thumb].view(side, side, CHANNELS)
                want = torch.cat([whole[y:y + rh, x:x + rw].reshape(-1) for x, y, rw, rh in regs])
                assert torch.equal(d_out[:total], want), (tile, shift, count)
                del listed, want

                def k17(i):
                    return L.fri_hip_preview_tiles_regions_dev(h, src[i % slots], plane, 1 << levels, levels, shift, P(ones), n_list, count, tp, dst17[i % out_slots], sp)

                res = {"K17": [], "K14": []}
                at = 0
                for fn in (k17, k14):
                    events(fn, max(slots, out_slots if fn is k17 else thumb_slots), 0)  # spin-up, and every copy touched once
                for _ in range(rounds):
                    for name, fn in (("K17", k17), ("K14", k14)):
                        res[name].append(events(fn, n, at))
                    at += n
                a, b = statistics.median(res["K17"]), statistics.median(res["K14"])
                rep.line(f"tiles of {tile}x{tile}, m = {shift} (L = {levels}), {count} regions, {n_list} of {T.n_tiles} tiles listed, {total / 1e6:.2f} MB of samples against "
                         f"{thumb / 1e6:.2f} MB for the whole thumbnail: K17, one launch of {groups} workgroups {a:.2f} us; K14, one launch for the whole thumbnail {b:.2f} us; "
                         f"K14 / K17 = {b / a:.2f}; rounds K17 " + " ".join(f"{v:.2f}" for v in res["K17"]) + "; K14 " + " ".join(f"{v:.2f}" for v in res["K14"]))
                del d_out
            del d_coefs, d_thumb
            torch.cuda.empty_cache()
        T.close()


def step_host(rep, tile):
    import numpy as np

    import frave_amd
    import frave_amd.emit as emit
    from frave_amd.api import TILED_ALLOW_HOLES

    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ctx = frave_amd.Context(0)
    E, L = emit.load_library(), frave_amd.load_library()
    rep.line(f"python3 tools/preview_regions_time.py host {tile} ({SIZE}x{SIZE}x{CHANNELS} half smooth / half noise in {tile}x{tile} tiles, lossless, fitted parameters; host to "
             f"host, wall clock, medians of 3, buffers allocated beforehand, the emitter on 16 threads; {os.cpu_count()} CPUs visible, "
             f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', '-')})")
    ones = np.ones(32, np.int32)
    img = _mixed_image(np, SIZE, CHANNELS, 7)
    T = frave_amd.PlanTiled(ctx, SIZE, SIZE, CHANNELS, tile, tile, TILED_ALLOW_HOLES)
    T.set_stream_order()
    sym, vp, wp, hist, oob = T.encode_image_tiled_symbols(img)
    assert not oob.any()
    frv = np.frombuffer(emit.tiled_encode_from_streams(SIZE, SIZE, tile, tile, sym, hist, vp, wp, threads=16), np.uint8)
    del sym, hist, img
    rep.line(f"file {frv.size} bytes, {T.n_tiles} tiles")
    info = np.zeros(8, np.uint32)
    err = C.create_string_buffer(256)
    h = T._h
    F = T.num_cells
    for shift in SHIFTS:
        levels, s, side = 9 - 2 * shift, 1 << shift, SIZE >> shift
        whole_coefs = np.empty(T.n_tiles * CHANNELS * F << levels, np.int32)
        thumbnail = np.zeros((side, side, CHANNELS), np.uint8)
        for count in SETS:
            regs = region_set(np, count, shift)
            rg = np.array(regs, np.uint32)
            src = source_rectangles(regs, shift)
            sg = np.array(src, np.uint32)
            offs = np.concatenate([[0], np.cumsum([rw * rh * CHANNELS for _, _, rw, rh in regs])]).astype(np.int64)
            out = np.zeros(int(offs[-1]), np.uint8)
            views = [out[offs[r]:offs[r + 1]].reshape(rh, rw, CHANNELS) for r, (_, _, rw, rh) in enumerate(regs)]
            n_list = C.c_size_t(0)
            tiles = np.zeros(T.n_tiles, np.uint32)
            assert E.fri_tiled_preview_regions_tiles(SIZE, SIZE, tile, tile, shift, count, P(rg), P(tiles), tiles.size, C.addressof(n_list)) == 0
            listed_tiles = n_list.value
            compact = np.empty(listed_tiles * CHANNELS * F << levels, np.int32)
            full = np.empty(listed_tiles * CHANNELS * F * 512, np.int32)
            src_offs = np.concatenate([[0], np.cumsum([rw * rh * CHANNELS for _, _, rw, rh in src])]).astype(np.int64)
            big = np.empty(int(src_offs[-1]), np.uint8)
            planes_cap = listed_tiles * CHANNELS
            stride = T.num_some + 20
            words, nw = np.zeros((planes_cap, stride), np.uint32), np.zeros(planes_cap, np.uint32)
            models, off = np.zeros((planes_cap, 10, 4), np.uint32), np.zeros((planes_cap, 10, 1024), np.uint16)
            cvp, cwp, status = np.zeros((planes_cap, 3, 6), np.float32), np.zeros((planes_cap, 3, 6), np.float32), np.zeros((planes_cap, 4), np.uint32)

            def new_call():
                t0 = time.perf_counter()
                rc = E.fri_tiled_preview_regions_tiles(SIZE, SIZE, tile, tile, shift, count, P(rg), P(tiles), tiles.size, C.addressof(n_list))
                rc |= E.fri_tiled_decode_tiles_levels(P(frv), frv.size, 16, P(tiles), n_list.value, levels, P(info), P(compact), compact.size, err, 256)
                t1 = time.perf_counter()
                rc |= L.fri_hip_preview_regions_tiled(h, P(compact), levels, shift, P(ones), count, P(rg), P(out))
                assert rc == 0, err.value
                return {"host": t1 - t0, "dev": time.perf_counter() - t1, "after": 0.0}

            def new_coded():
                t0 = time.perf_counter()
                rc = E.fri_tiled_preview_regions_tiles(SIZE, SIZE, tile, tile, shift, count, P(rg), P(tiles), tiles.size, C.addressof(n_list))
                planes = n_list.value * CHANNELS
                rc |= E.fri_tiled_parse_coded_tiles(P(frv), frv.size, P(tiles), n_list.value, P(info), planes, None, 0, P(nw), None, None, None, None, err, 256)
                rc |= E.fri_tiled_parse_coded_tiles(P(frv), frv.size, P(tiles), n_list.value, P(info), planes, P(words), stride, P(nw), P(models), P(off), P(cvp), P(cwp), err, 256)
                t1 = time.perf_counter()
                rc |= L.fri_hip_preview_regions_tiled_coded(h, count, P(rg), P(words), stride, P(nw), P(models), P(off), P(cvp), P(cwp), levels, shift, P(ones), P(out), P(status))
                assert rc == 0 and not status[:planes, 0].any(), err.value
                return {"host": t1 - t0, "dev": time.perf_counter() - t1, "after": 0.0}

            def whole_and_crop():
                t0 = time.perf_counter()
                rc = E.fri_tiled_decode_levels(P(frv), frv.size, 16, levels, P(info), P(whole_coefs), whole_coefs.size, err, 256)
                t1 = time.perf_counter()
                rc |= L.fri_hip_preview_image_tiled(h, P(whole_coefs), levels, shift, P(ones), P(thumbnail))
                t2 = time.perf_counter()
                for v, (x, y, rw, rh) in zip(views, regs):
                    v[:] = thumbnail[y:y + rh, x:x + rw]
                assert rc == 0, err.value
                return {"host": t1 - t0, "dev": t2 - t1, "after": time.perf_counter() - t2}

            def full_and_subsample():
                t0 = time.perf_counter()
                rc = E.fri_tiled_regions_tiles(SIZE, SIZE, tile, tile, count, P(sg), P(tiles), tiles.size, C.addressof(n_list))
                assert n_list.value == listed_tiles
                rc |= E.fri_tiled_decode_tiles(P(frv), frv.size, 16, P(tiles), n_list.value, P(info), P(full), full.size, err, 256)
                t1 = time.perf_counter()
                rc |= L.fri_hip_decode_regions_tiled(h, P(full), P(ones), count, P(sg), P(big))
                t2 = time.perf_counter()
                for r, (v, (_, _, rw, rh)) in enumerate(zip(views, src)):
                    v[:] = big[src_offs[r]:src_offs[r + 1]].reshape(rh, rw, CHANNELS)[::s, ::s]
                assert rc == 0, err.value
                return {"host": t1 - t0, "dev": t2 - t1, "after": time.perf_counter() - t2}

            res = {}
            want = None
            for name, fn in (("whole preview + crop", whole_and_crop), ("new call", new_call), ("new call, coded", new_coded), ("full regions + subsample", full_and_subsample)):
                out[:] = 0
                parts, total = _wall(fn)
                if want is None:
                    want = out.copy()  # the crops of the whole thumbnail: what every route must give
                    assert want.any()
                # (the last route's pixels are point samples of the full-resolution image, not the node means of P_L: the same places, other bytes - compared with
                # the full-resolution regions it was cut from, not with the thumbnail)
                assert np.array_equal(out, want) or name.startswith("full"), name
                res[name] = (total, parts)
            new = res["new call"][0]
            for name, (total, parts) in res.items():
                rep.line(f"m = {shift} (L = {levels}), {count} regions, {listed_tiles} of {T.n_tiles} tiles listed, {want.size / 1e6:.2f} MB of samples"
                         f"{f', {big.size / 1e6:.0f} MB of source pixels' if name.startswith('full') else ''}: {name}: emitter {parts['host'] * 1e3:.1f} ms + device call "
                         f"{parts['dev'] * 1e3:.1f} ms + host crop or subsample {parts['after'] * 1e3:.1f} ms = {total * 1e3:.1f} ms, {total / new:.2f} x the new call's time; "
                         + ("point samples of the full-resolution image at the samples' places: not the thumbnail's bytes" if name.startswith("full") else
                            "every region is the crop of the whole thumbnail"))
            del big, full, compact, words, off
    T.close()


def main():
    pos, out, n, rounds = _args()
    if not pos or pos[0] not in ("kernels", "host") or (pos[0] == "host" and (len(pos) < 2 or int(pos[1]) not in TILES)):
        print(__doc__)
        return 2
    rep = Report(out, fresh=pos[0] == "kernels")
    if pos[0] == "kernels":
        step_kernels(rep, n, rounds)
    else:
        step_host(rep, int(pos[1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
