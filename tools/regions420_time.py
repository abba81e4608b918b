"""What decoding several regions of a tiled 4:2:0 image in one call (fri_tiled_decode_tiles / fri_tiled_parse_coded_tiles, fri_hip_decode_regions_tiled420[_coded],
K18's merge_tiles420_regions_kernel) costs against one call per region (fri_tiled_decode_region, fri_hip_decode_region_tiled420, K12's merge_tiles420_region_kernel).
tools/regions_time.py for the tiled 4:2:0 plan. Three steps, each a process of its own that appends its section to the report; run them under a time limit each and
chained, so that trouble in one ends the run:

    timeout -k 10 300 python3 tools/regions420_time.py kernels && timeout -k 10 500 python3 tools/regions420_time.py host 512 && timeout -k 10 500 python3 tools/regions420_time.py host 256

The image is 4096^2 RGB, half smooth and half noise as in tools/tiled_time.py, at quality 60 in 4:2:0 tiles of 512^2 (64 tiles) and of 256^2 (256 tiles). The region
sets are tools/regions_time.py's: 16 and 256 random 224^2 regions from one seed, the same ones for every tile size and every route.

kernels: K18 on a region set in one launch against K12's region kernel launched once per region of the set, timed with events around `launches` back-to-back
         repetitions; medians of interleaved rounds. Every repetition reads another copy of the tile-list planes and writes another copy of the packed output, out
         of pools of more bytes than the 256 MB cache. The calls are made from Python through ctypes with every pointer worked out beforehand: where a kernel is
         shorter than such a call the figure is the host's rate of launching, for both kernels alike. K12's launches read ni nj consecutive tiles from the place of
         the region's first tile in the pool - the bytes differ from a real sub-grid's, their number and pattern do not; K18's output is checked against K12's on
         real sub-grids once, before the timing.
host:    the image through the device (quality 60, fitted parameters) into a tiled 4:2:0 `frit` file; then, host to host, wall clock, medians of three, buffers
         allocated beforehand, the emitter on 16 threads:
           per region  for every region fri_tiled_decode_region + fri_hip_decode_region_tiled420 - what the parent commit offers
           one call    fri_tiled_regions_tiles + fri_tiled_decode_tiles + fri_hip_decode_regions_tiled420
           coded       fri_tiled_regions_tiles + fri_tiled_parse_coded_tiles (the count query, then the planes) + fri_hip_decode_regions_tiled420_coded (K13, K3, K18)
         Every region of every route is checked against the crop of the whole decode.

usage: python3 tools/regions420_time.py kernels | host TILE [--out profiles/regions420_time.txt] [--launches 20] [--rounds 5]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.region_time import Report, _mixed_image, _wall  # noqa: E402
from tools.regions_time import POOL, SETS, SIDE, SIZE, TILES, region_set  # noqa: E402

QUALITY = 60


def _args():
    a = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "regions420_time.txt"), "--launches": "20", "--rounds": "5"}
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


def step_kernels(rep, n, rounds):
    import numpy as np
    import torch

    import frave_amd
    from frave_amd.api import TILED_ALLOW_HOLES

    ctx = frave_amd.Context(0)
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    L = frave_amd.load_library()
    rep.line(f"python3 tools/regions420_time.py kernels --launches {n} --rounds {rounds} (one process; medians of {rounds} interleaved rounds; us per repetition = one K18 launch, or "
             f"one K12 region launch per region; {SIZE}x{SIZE}x3 in 4:2:0 tiles, regions of {SIDE}x{SIDE}; calls from Python through ctypes)")

    def events(fn, count, at):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for i in range(at, at + count):
            fn(i)
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / count

    for tile in TILES:
        T = frave_amd.PlanTiled420(ctx, SIZE, SIZE, tile, tile, TILED_ALLOW_HOLES)
        y_bytes, c_bytes = tile * tile, 2 * T.cw * T.ch
        for count in SETS:
            regs = region_set(np, count)
            tiles, table = T.regions(regs)
            n_list, total = int(tiles.size), int(table[8 * count + 4]) | int(table[8 * count + 5]) << 32
            slot = table[8 * (count + 1):]
            planes_bytes = n_list * (y_bytes + c_bytes)  # what a repetition reads at most
            slots = max(2, -(-POOL // planes_bytes))
            d_y = torch.randint(0, 256, ((slots * n_list + 4) * y_bytes,), dtype=torch.uint8, device="cuda")  # (room behind the last copy for a K12 launch's tiles)
            d_c = torch.randint(0, 256, ((slots * n_list + 4) * c_bytes,), dtype=torch.uint8, device="cuda")
            d_out = torch.zeros(slots * total, dtype=torch.uint8, device="cuda")
            d_one = torch.zeros(total, dtype=torch.uint8, device="cuda")
            d_table = torch.from_numpy(table.view(np.int32).copy()).cuda()
            src_y = [d_y.data_ptr() + k * n_list * y_bytes for k in range(slots)]
            src_c = [d_c.data_ptr() + k * n_list * c_bytes for k in range(slots)]
            dst = [d_out.data_ptr() + k * total for k in range(slots)]
            offs = [int(table[8 * r + 4]) | int(table[8 * r + 5]) << 32 for r in range(count)]
            first = [int(slot[(y // tile) * T.nx + x // tile]) for x, y, _, _ in regs]
            # once, before the timing: K18's regions against K12's on the real sub-grids, gathered from copy 0
            assert L.fri_hip_merge_tiles420_regions_dev(T._h, src_y[0], src_c[0], n_list, count, d_table.data_ptr(), dst[0], sp) == 0
            y0, c0 = d_y[:n_list * y_bytes].view(n_list, y_bytes), d_c[:n_list * c_bytes].view(n_list, c_bytes)
            for r, (x, y, w, h) in enumerate(regs):
                i0, j0, ni, nj = T.region_tiles(x, y, w, h)
                idx = torch.tensor([int(slot[(j0 + b) * T.nx + i0 + a]) for b in range(nj) for a in range(ni)], device="cuda")
                sub_y, sub_c = y0[idx].contiguous(), c0[idx].contiguous()
                T.merge_tiles420_region_dev(sub_y.data_ptr(), sub_c.data_ptr(), x, y, w, h, d_one.data_ptr() + offs[r], stream=sp)
            s.synchronize()
            assert torch.equal(d_one, d_out[:total]), (tile, count)
            h = T._h
            tp = d_table.data_ptr()

            def k18(i):
                return L.fri_hip_merge_tiles420_regions_dev(h, src_y[i % slots], src_c[i % slots], n_list, count, tp, dst[i % slots], sp)

            def k12(i):
                a, c, b = src_y[i % slots], src_c[i % slots], dst[i % slots]
                for r in range(count):
                    L.fri_hip_merge_tiles420_region_dev(h, a + first[r] * y_bytes, c + first[r] * c_bytes, *regs[r], b + offs[r], sp)

            res = {"K18": [], "K12": []}
            at = 0
            for fn in (k18, k12):
                events(fn, slots, 0)  # spin-up, and every copy touched once
            for _ in range(rounds):
                for name, fn in (("K18", k18), ("K12", k12)):
                    res[name].append(events(fn, n, at))
                at += n
            a, b = statistics.median(res["K18"]), statistics.median(res["K12"])
            moved = 1.5 * total  # a pixel's 3 output bytes, its Y byte and half a byte of chroma
            rep.line(f"tiles of {tile}x{tile}, {count} regions, {n_list} of {T.n_tiles} tiles listed, {moved / 1e6:.2f} MB algorithmic (read + written): K18, one launch of "
                     f"{int(table[8 * count + 6])} workgroups {a:.2f} us = {moved / a / 1e6:.3f} TB/s; K12, {count} launches {b:.2f} us ({b / count:.2f} us each) = "
                     f"{moved / b / 1e6:.3f} TB/s; K12 / K18 = {b / a:.2f}; rounds K18 " + " ".join(f"{v:.2f}" for v in res["K18"]) + "; K12 " + " ".join(f"{v:.2f}" for v in res["K12"]))
            del d_y, d_c, d_out, d_one
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
    rep.line(f"python3 tools/regions420_time.py host {tile} ({SIZE}x{SIZE}x3 half smooth / half noise in {tile}x{tile} 4:2:0 tiles, quality {QUALITY}, fitted parameters; host to host, "
             f"wall clock, medians of 3, buffers allocated beforehand, the emitter on 16 threads; {os.cpu_count()} CPUs visible, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', '-')})")
    img = _mixed_image(np, SIZE, 3, 7)
    T = frave_amd.PlanTiled420(ctx, SIZE, SIZE, tile, tile, TILED_ALLOW_HOLES)
    T.set_stream_order()
    sym, vp, wp, hist, oob = T.encode_image_tiled420_symbols(img, QUALITY)
    assert not oob.any()
    frv = np.frombuffer(emit.tiled_encode_from_streams420(SIZE, SIZE, tile, tile, sym, T.n_luma, T.n_chroma, hist, vp, wp, QUALITY, threads=16), np.uint8)
    del sym, hist
    whole = T.decode_image_tiled420(emit.tiled_decode(frv.tobytes(), 16)[1], QUALITY).reshape(SIZE, SIZE, 3)  # the crops are of this
    rep.line(f"file {frv.size} bytes, {T.n_tiles} tiles")
    per_tile = T.tile_coef_count
    info, sub = np.zeros(8, np.uint32), np.zeros(4, np.uint32)
    err = C.create_string_buffer(256)
    h = T._h
    for count in SETS:
        regs = region_set(np, count)
        rg = np.array(regs, np.uint32)
        want = np.concatenate([whole[y:y + rh, x:x + rw].reshape(-1) for x, y, rw, rh in regs])
        out = np.zeros(want.size, np.uint8)
        offs = np.concatenate([[0], np.cumsum([rw * rh * 3 for _, _, rw, rh in regs])]).astype(np.int64)
        part = np.empty(4 * per_tile, np.int32)  # a 224^2 region touches at most 2 x 2 tiles of either size
        n_list = C.c_size_t(0)
        tiles = np.zeros(T.n_tiles, np.uint32)
        listed = np.empty(min(T.n_tiles, 4 * count) * per_tile, np.int32)
        t = {}

        def per_region():
            t["host"] = t["dev"] = 0.0
            for r, (x, y, rw, rh) in enumerate(regs):
                t0 = time.perf_counter()
                rc = E.fri_tiled_decode_region(P(frv), frv.size, 16, x, y, rw, rh, P(info), P(sub), P(part), part.size, err, 256)
                t1 = time.perf_counter()
                rc |= L.fri_hip_decode_region_tiled420(h, P(part), QUALITY, x, y, rw, rh, P(out[offs[r]:]))
                t["host"], t["dev"] = t["host"] + t1 - t0, t["dev"] + time.perf_counter() - t1
                assert rc == 0, err.value
            return dict(t)

        def one_call():
            t0 = time.perf_counter()
            rc = E.fri_tiled_regions_tiles(SIZE, SIZE, tile, tile, count, P(rg), P(tiles), tiles.size, C.addressof(n_list))
            rc |= E.fri_tiled_decode_tiles(P(frv), frv.size, 16, P(tiles), n_list.value, P(info), P(listed), listed.size, err, 256)
            t1 = time.perf_counter()
            rc |= L.fri_hip_decode_regions_tiled420(h, P(listed), QUALITY, count, P(rg), P(out))
            assert rc == 0, err.value
            return {"host": t1 - t0, "dev": time.perf_counter() - t1}

        planes_cap = min(T.n_tiles, 4 * count) * 3
        stride = max(T.n_luma, T.n_chroma) + 20
        words, nw = np.zeros((planes_cap, stride), np.uint32), np.zeros(planes_cap, np.uint32)
        models, off = np.zeros((planes_cap, 10, 4), np.uint32), np.zeros((planes_cap, 10, 1024), np.uint16)
        cvp, cwp, status = np.zeros((planes_cap, 3, 6), np.float32), np.zeros((planes_cap, 3, 6), np.float32), np.zeros((planes_cap, 4), np.uint32)

        def coded():
            t0 = time.perf_counter()
            rc = E.fri_tiled_regions_tiles(SIZE, SIZE, tile, tile, count, P(rg), P(tiles), tiles.size, C.addressof(n_list))
            planes = n_list.value * 3
            rc |= E.fri_tiled_parse_coded_tiles(P(frv), frv.size, P(tiles), n_list.value, P(info), planes, None, 0, P(nw), None, None, None, None, err, 256)
            rc |= E.fri_tiled_parse_coded_tiles(P(frv), frv.size, P(tiles), n_list.value, P(info), planes, P(words), stride, P(nw), P(models), P(off), P(cvp), P(cwp), err, 256)
            t1 = time.perf_counter()
            rc |= L.fri_hip_decode_regions_tiled420_coded(h, count, P(rg), P(words), stride, P(nw), P(models), P(off), P(cvp), P(cwp), QUALITY, P(out), P(status))
            assert rc == 0 and not status[:planes, 0].any(), err.value
            return {"host": t1 - t0, "dev": time.perf_counter() - t1}

        res = {}
        for name, fn in (("per region", per_region), ("one call", one_call), ("coded", coded)):
            out[:] = 0
            parts, total = _wall(fn)
            assert np.array_equal(out, want), name
            res[name] = (total, parts)
        base = res["per region"][0]
        for name, (total, parts) in res.items():
            rep.line(f"{count} regions, {n_list.value} of {T.n_tiles} tiles listed, {want.size / 1e6:.2f} MB of pixels: {name}: emitter {parts['host'] * 1e3:.1f} ms + device call(s) "
                     f"{parts['dev'] * 1e3:.1f} ms = {total * 1e3:.1f} ms, {base / total:.2f} x the per-region loop's speed; every region is the crop")
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
