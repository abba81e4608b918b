"""What region decode (fri_tiled_decode_region, fri_hip_decode_region_tiled, K10's merge_tiles_region_kernel) costs against decoding the whole tiled image. Two
steps, each a process of its own that appends its section to the report; run them under a time limit each and chained, so that trouble in one ends the run:

    timeout -k 10 300 python3 tools/region_time.py kernels && timeout -k 10 600 python3 tools/region_time.py host

The image is 4096^2 (C = 1 and C = 3) in 64 tiles of 512^2, half smooth and half noise as in tools/tiled_time.py. The regions: a tile-aligned 1024^2 (4 tiles), the
same size at (300, 300) (9 tiles), and 256^2 inside one tile.

kernels: merge_tiles_kernel on the whole image and merge_tiles_region_kernel on each region, timed with events around `launches` back-to-back launches; medians of
         interleaved rounds. Every launch reads and writes another place of two pools of more bytes than the 256 MB cache (rotating slots for the merge; for a
         region the next ni nj tiles of the tile pool and the next w h C bytes of the output pool), and the merge's rounds in between move gigabytes, so no launch
         finds its lines cached. The 2 w h C algorithmic bytes of each and their rate. A region's launch moves so little that the figure is mostly the launch.
host:    the image through the device (lossless, fitted parameters) into a `frit` file; then, wall clock, medians of three, each C call on its own with its
         buffers allocated beforehand: fri_tiled_decode on 16 threads + fri_hip_decode_image_tiled against fri_tiled_decode_region (16 threads, and 1) +
         fri_hip_decode_region_tiled for each region. The device calls are the synchronous host forms: staging copies included. Every region raster is checked
         against the crop of the whole decode.

usage: python3 tools/region_time.py kernels|host [--out profiles/region_time.txt] [--launches 200] [--rounds 5]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12  # bytes per second
SIZE, TILE = 4096, 512
REGIONS = [("tile-aligned 1024x1024", (1024, 1024, 1024, 1024)), ("1024x1024 at (300, 300)", (300, 300, 1024, 1024)), ("256x256 inside one tile", (640, 640, 256, 256))]


def _args():
    a = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "region_time.txt"), "--launches": "200", "--rounds": "5"}
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


class Report:
    def __init__(self, path, fresh):
        self.path = path
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if fresh and os.path.exists(path):
            os.remove(path)

    def line(self, text):
        print(text, flush=True)
        with open(self.path, "a") as f:
            f.write(text + "\n")


def _mixed_image(np, size, channels, seed):
    """every plane: left half smooth, right half noise (tools/tiled_time.py's plane)"""
    planes = []
    for c in range(channels):
        rng = np.random.default_rng(seed + c)
        y, x = np.mgrid[0:size, 0:size]
        smooth = (((x + 2 * y) >> 3) + rng.integers(0, 8, (size, size))) & 0xFF
        noise = rng.integers(0, 256, (size, size))
        planes.append(np.where(x < size // 2, smooth, noise).astype(np.uint8))
    return np.ascontiguousarray(np.stack(planes, axis=2))


def step_kernels(rep, n, rounds):
    import torch

    import frave_amd

    ctx = frave_amd.Context(0)
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    at = [0]  # launches so far: every launch of a kind goes on from where the last one stopped

    def events(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for i in range(at[0], at[0] + launches):
            fn(i)
        e1.record(s)
        e1.synchronize()
        at[0] += launches
        return e0.elapsed_time(e1) * 1e3 / launches

    rep.line(f"python3 tools/region_time.py kernels --launches {n} --rounds {rounds} (one process; medians of {rounds} interleaved rounds, us per launch, back to back)")
    for channels, slots in ((1, 32), (3, 32)):
        T = frave_amd.PlanTiled(ctx, SIZE, SIZE, channels, TILE, TILE)
        nbytes = SIZE * SIZE * channels
        tile_bytes = TILE * TILE * channels
        d_tiles = torch.randint(0, 256, (slots, nbytes), dtype=torch.uint8, device="cuda")
        d_back = torch.empty_like(d_tiles)
        L, h = frave_amd.load_library(), T._h
        tiles, back = ([t[k].data_ptr() for k in range(slots)] for t in (d_tiles, d_back))
        # (the library's entry points called directly with pointers worked out beforehand: a short launch must not wait for the interpreter)
        fns = {"merge, whole image": lambda i: L.fri_hip_merge_tiles_dev(h, tiles[i % slots], back[i % slots], sp)}
        moved = {"merge, whole image": 2 * nbytes}
        pool_tiles = slots * T.n_tiles
        for name, (x, y, w, hh) in REGIONS:
            i0, j0, ni, nj = T.region_tiles(x, y, w, hh)
            # the region raster against the crop of the merge, once: the sub-grid gathered from slot 0's tiles
            grid = d_tiles[0].view(T.ny, T.nx, tile_bytes)
            sub = grid[j0:j0 + nj, i0:i0 + ni].contiguous()
            out = torch.zeros(w * hh * channels, dtype=torch.uint8, device="cuda")
            T.merge_tiles_dev(tiles[0], back[0], stream=sp)
            T.merge_tiles_region_dev(sub.data_ptr(), x, y, w, hh, out.data_ptr(), stream=sp)
            s.synchronize()
            assert torch.equal(out.view(hh, w, channels), d_back[0].view(SIZE, SIZE, channels)[y:y + hh, x:x + w]), name
            src = [tiles[0] + k * ni * nj * tile_bytes for k in range(pool_tiles // (ni * nj))]
            dst = [back[0] + k * w * hh * channels for k in range(slots * nbytes // (w * hh * channels))]
            assert n <= len(src) and n <= len(dst), "a round must not come back to a place it has been"
            fns[name] = lambda i, src=src, dst=dst, r=(x, y, w, hh): L.fri_hip_merge_tiles_region_dev(h, src[i % len(src)], *r, dst[i % len(dst)], sp)
            moved[name] = 2 * w * hh * channels
        res = {k: [] for k in fns}
        for k, fn in fns.items():
            assert fn(0) == 0, k
            events(fn, 2 * slots)  # spin-up
        for _ in range(rounds):
            for k, fn in fns.items():
                events(fn, slots)
                res[k].append(events(fn, n))
        whole = statistics.median(res["merge, whole image"])
        for k in fns:
            us = statistics.median(res[k])
            rep.line(f"{k}, {SIZE}x{SIZE}x{channels} in {T.n_tiles} tiles of {TILE}x{TILE}, {n} launches: {us:.2f} us, {moved[k] / 1e6:.2f} MB algorithmic = "
                     f"{moved[k] / us / 1e6:.3f} TB/s ({100 * moved[k] / us * 1e6 / PEAK:.1f} % of 8 TB/s), {us / whole:.3f} x the whole merge; rounds "
                     + " ".join(f"{v:.2f}" for v in res[k]))
        del d_tiles, d_back
        torch.cuda.empty_cache()
        T.close()


def _wall(fn, repeats=3):
    out, times = None, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, statistics.median(times)


def step_host(rep, n, rounds):
    import numpy as np

    import frave_amd
    import frave_amd.emit as emit

    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ctx = frave_amd.Context(0)
    E, L = emit.load_library(), frave_amd.load_library()
    rep.line(f"python3 tools/region_time.py host ({SIZE}x{SIZE} half smooth / half noise in {TILE}x{TILE} tiles, lossless, fitted parameters; wall clock, medians of 3, every C call "
             f"alone with its buffers allocated beforehand; {os.cpu_count()} CPUs visible, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', '-')})")
    ones = np.ones(32, np.int32)
    for channels in (1, 3):
        img = _mixed_image(np, SIZE, channels, 7)
        T = frave_amd.PlanTiled(ctx, SIZE, SIZE, channels, TILE, TILE)
        T.set_stream_order()
        sym, vp, wp, hist, oob = T.encode_image_tiled_symbols(img)
        assert not oob.any()
        frv = np.frombuffer(emit.tiled_encode_from_streams(SIZE, SIZE, TILE, TILE, sym, hist, vp, wp, threads=16), np.uint8)
        del sym, hist
        info, tiles = np.zeros(8, np.uint32), np.zeros(4, np.uint32)
        err = C.create_string_buffer(256)
        coefs = np.empty(T.coef_count, np.int32)
        pixels = np.empty(T.pixel_bytes, np.uint8)
        rc, t_host = _wall(lambda: E.fri_tiled_decode(P(frv), frv.size, 16, P(info), P(coefs), coefs.size, err, 256))
        assert rc == 0, err.value
        rc, t_dev = _wall(lambda: L.fri_hip_decode_image_tiled(T._h, P(coefs), P(ones), P(pixels)))
        assert rc == 0 and np.array_equal(pixels, img.reshape(-1))
        rep.line(f"C = {channels}: file {frv.size} bytes; whole image ({T.n_tiles} tiles): fri_tiled_decode on 16 threads {t_host * 1e3:.1f} ms + fri_hip_decode_image_tiled "
                 f"{t_dev * 1e3:.1f} ms = {(t_host + t_dev) * 1e3:.1f} ms")
        whole = t_host + t_dev
        per_tile = T.coef_count // T.n_tiles
        for name, (x, y, w, h) in REGIONS:
            i0, j0, ni, nj = T.region_tiles(x, y, w, h)
            part = np.empty(ni * nj * per_tile, np.int32)
            out = np.empty(w * h * channels, np.uint8)
            t_threads = {}
            for threads in (16, 1):
                rc, t_threads[threads] = _wall(lambda: E.fri_tiled_decode_region(P(frv), frv.size, threads, x, y, w, h, P(info), P(tiles), P(part), part.size, err, 256))
                assert rc == 0 and tuple(int(v) for v in tiles) == (i0, j0, ni, nj), err.value
            rc, t_d = _wall(lambda: L.fri_hip_decode_region_tiled(T._h, P(part), P(ones), x, y, w, h, P(out)))
            assert rc == 0 and np.array_equal(out.reshape(h, w, channels), img[y:y + h, x:x + w]), name
            total = t_threads[16] + t_d
            rep.line(f"C = {channels}: {name} ({ni * nj} tiles): fri_tiled_decode_region on 16 threads {t_threads[16] * 1e3:.1f} ms (on 1 thread {t_threads[1] * 1e3:.1f} ms) + "
                     f"fri_hip_decode_region_tiled {t_d * 1e3:.2f} ms = {total * 1e3:.1f} ms, {whole / total:.1f} x faster than the whole image; the raster is the crop")
        T.close()


def main():
    pos, out, n, rounds = _args()
    steps = {"kernels": step_kernels, "host": step_host}
    if not pos or pos[0] not in steps:
        print(__doc__)
        return 2
    rep = Report(out, fresh=pos[0] == "kernels")
    steps[pos[0]](rep, n, rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
