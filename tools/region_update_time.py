"""What a region update of a tiled file (fri_hip_encode_region_tiled_symbols, fri_tiled_update_from_streams, K10's split_tiles_region_kernel) costs against coding
the whole image again. Three steps, each a process of its own that appends its section to the report; run them under a time limit each and chained, so that
trouble in one ends the run:

    timeout -k 10 300 python3 tools/region_update_time.py kernel && timeout -k 10 600 python3 tools/region_update_time.py host && \
    timeout -k 10 600 python3 tools/region_update_time.py plan

kernel: split_tiles_kernel and split_tiles_region_kernel on the whole-image region of the same raster - the same bytes - timed with events around `launches`
        back-to-back launches; medians of interleaved rounds after a spin-up. Every launch reads and writes another slot of two pools of more bytes than the
        256 MB cache, so no launch finds its lines cached. The 2 W H C algorithmic bytes of each and their rate.
host:   case A, 4096^2 RGB in 512^2 tiles, YCbCr at quality 60 and lossless, host memory to host memory, wall clock, medians of `repeats` after one warm-up call,
        every C call alone with its buffers allocated beforehand. The baseline is the whole encode, fri_hip_encode_image_tiled_symbols +
        fri_tiled_encode_from_streams on 16 threads; against it fri_hip_encode_region_tiled_symbols + fri_tiled_update_from_streams (16 threads; the call that
        writes, its size known) for a region inside one tile, a 2 x 2 sub-grid and the whole grid. Every updated file is checked against the whole encode of the
        changed image.
plan:   case B, a 16384^2 plane in 512^2 tiles (1024 tiles), lossless: one tile updated on a fresh plan, then the whole image coded on another; the device bytes
        each plan came to hold (the fall of hipMemGetInfo's free bytes around the plan's life), and the wall clock of the calls.

usage: python3 tools/region_update_time.py kernel|host|plan [--out profiles/region_update_time.txt] [--launches 100] [--rounds 5] [--repeats 5]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12  # bytes per second
SIZE, TILE = 4096, 512
REGIONS = [("200x200 inside one tile", (700, 650, 200, 200)), ("200x200 across a tile corner (2 x 2 tiles)", (924, 924, 200, 200)), ("the whole grid", (0, 0, SIZE, SIZE))]


def _args():
    a = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "region_update_time.txt"), "--launches": "100", "--rounds": "5", "--repeats": "5"}
    pos = []
    i = 0
    while i < len(a):
        if a[i] in opt:
            opt[a[i]] = a[i + 1]
            i += 2
        else:
            pos.append(a[i])
            i += 1
    return pos, opt["--out"], int(opt["--launches"]), int(opt["--rounds"]), int(opt["--repeats"])


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


def step_kernel(rep, n, rounds, repeats):
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

    rep.line(f"python3 tools/region_update_time.py kernel --launches {n} --rounds {rounds} (one process; device events around {n} back-to-back launches, medians of {rounds} "
             f"interleaved rounds after a spin-up, us per launch; every launch on another slot of pools larger than the 256 MB cache)")
    for channels, slots in ((1, 24), (3, 8)):
        T = frave_amd.PlanTiled(ctx, SIZE, SIZE, channels, TILE, TILE)
        nbytes = SIZE * SIZE * channels
        d_img = torch.randint(0, 256, (slots, nbytes), dtype=torch.uint8, device="cuda")
        d_tiles = torch.empty_like(d_img)
        L, h = frave_amd.load_library(), T._h
        img, tiles = ([t[k].data_ptr() for k in range(slots)] for t in (d_img, d_tiles))
        # (the library's entry points called directly with pointers worked out beforehand: a short launch must not wait for the interpreter)
        fns = {
            "split_tiles_kernel": lambda i: L.fri_hip_split_tiles_dev(h, img[i % slots], tiles[i % slots], sp),
            "split_tiles_region_kernel, whole-image region": lambda i: L.fri_hip_split_tiles_region_dev(h, img[i % slots], SIZE * channels, 0, 0, SIZE, SIZE, 0, 0, SIZE, SIZE,
                                                                                                        tiles[i % slots], sp),
        }
        # the two give the same bytes, once
        check = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        assert fns["split_tiles_kernel"](0) == 0
        T.split_tiles_region_dev(img[0], SIZE * channels, 0, 0, SIZE, SIZE, 0, 0, SIZE, SIZE, check.data_ptr(), stream=sp)
        s.synchronize()
        assert torch.equal(check, d_tiles[0])
        res = {k: [] for k in fns}
        for k, fn in fns.items():
            assert fn(0) == 0, k
            events(fn, 2 * slots)  # spin-up
        for _ in range(rounds):
            for k, fn in fns.items():
                events(fn, slots)
                res[k].append(events(fn, n))
        base = statistics.median(res["split_tiles_kernel"])
        for k in fns:
            us = statistics.median(res[k])
            rep.line(f"{k}, {SIZE}x{SIZE}x{channels} in {T.n_tiles} tiles of {TILE}x{TILE}: {us:.2f} us, {2 * nbytes / 1e6:.1f} MB algorithmic = {2 * nbytes / us / 1e6:.3f} TB/s "
                     f"({100 * 2 * nbytes / us * 1e6 / PEAK:.1f} % of 8 TB/s), {us / base:.3f} x split_tiles_kernel; rounds " + " ".join(f"{v:.2f}" for v in res[k]))
        del d_img, d_tiles, check
        torch.cuda.empty_cache()
        T.close()


def _wall(fn, repeats):
    fn()  # warm-up: buffers grown, pages touched
    out, times = None, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, statistics.median(times)


class _Update:
    """the C calls of one image shape with their buffers allocated beforehand"""

    def __init__(self, np, frave_amd, emit, T, width, height, channels, word):
        self.np, self.T, self.word = np, T, word
        self.E, self.L = emit.load_library(), frave_amd.load_library()
        self.w, self.h, self.c = width, height, channels
        self.P = lambda a: a.ctypes.data_as(C.c_void_p)
        self.err = C.create_string_buffer(256)

    def arrays(self, n_tiles):
        np, planes, n = self.np, n_tiles * self.c, self.T.num_some
        return dict(sym=np.empty(planes * n, np.uint16), hist=np.empty(planes * 10240, np.uint32), vp=np.zeros(planes * 18, np.float32), wp=np.zeros(planes * 18, np.float32),
                    oob=np.zeros(planes, np.uint64))

    def encode_whole(self, img, qm, a):
        P = self.P
        return self.L.fri_hip_encode_image_tiled_symbols(self.T._h, P(img), P(qm), P(a["vp"]), P(a["wp"]), P(a["sym"]), P(a["hist"]), P(a["oob"]))

    def emit_whole(self, a, out):
        P, n = self.P, C.c_size_t(0)
        rc = self.E.fri_tiled_encode_from_streams(self.w, self.h, self.T.tile_w, self.T.tile_h, self.word, P(a["sym"]), self.T.num_some, P(a["hist"]), P(a["vp"]), P(a["wp"]), 16,
                                                  P(out), out.size, C.addressof(n), self.err, 256)
        assert rc == 0, (rc, self.err.value)
        return n.value

    def encode_region(self, img, qm, region, a):
        P = self.P
        return self.L.fri_hip_encode_region_tiled_symbols(self.T._h, P(img), *region, P(qm), P(a["vp"]), P(a["wp"]), P(a["sym"]), P(a["hist"]), P(a["oob"]))

    def emit_update(self, frv, region, a, out):
        P, n, tiles = self.P, C.c_size_t(0), self.np.zeros(4, self.np.uint32)
        rc = self.E.fri_tiled_update_from_streams(P(frv), frv.size, *region, self.word, P(a["sym"]), self.T.num_some, P(a["hist"]), P(a["vp"]), P(a["wp"]), 16, P(tiles), P(out),
                                                  out.size, C.addressof(n), self.err, 256)
        assert rc == 0, (rc, self.err.value)
        return n.value


def step_host(rep, n, rounds, repeats):
    import numpy as np

    import frave_amd
    import frave_amd.emit as emit

    ctx = frave_amd.Context(0)
    rep.line(f"python3 tools/region_update_time.py host --repeats {repeats} (case A: {SIZE}x{SIZE} RGB, half smooth / half noise, in {TILE}x{TILE} tiles, fitted parameters; host "
             f"memory to host memory; time.perf_counter around each synchronous C call alone, buffers allocated beforehand, medians of {repeats} after one warm-up call; "
             f"{os.cpu_count()} CPUs visible, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', '-')})")
    img_a, other = _mixed_image(np, SIZE, 3, 7), _mixed_image(np, SIZE, 3, 19)
    T = frave_amd.PlanTiled(ctx, SIZE, SIZE, 3, TILE, TILE)
    T.set_stream_order()
    for mode, transform, quality, word in (("YCbCr, quality 60", 3, 60, 3 | emit.YCBCR | emit.QUALITY(60)), ("lossless", 0, 100, 3)):
        T.tile.set_colour_transform(transform)
        qm = frave_amd.quality_matrix(quality)
        U = _Update(np, frave_amd, emit, T, SIZE, SIZE, 3, word)
        whole = U.arrays(T.n_tiles)
        out = np.empty(whole["sym"].size * 4 + (1 << 24), np.uint8)
        assert U.encode_whole(img_a, qm, whole) == 0 and not whole["oob"].any()
        file_a = out[: U.emit_whole(whole, out)].copy()
        rc, t_dev = _wall(lambda: U.encode_whole(img_a, qm, whole), repeats)
        assert rc == 0
        _, t_emit = _wall(lambda: U.emit_whole(whole, out), repeats)
        base = t_dev + t_emit
        rep.line(f"{mode}: file {file_a.size} bytes; the whole encode ({T.n_tiles} tiles): fri_hip_encode_image_tiled_symbols {t_dev * 1e3:.1f} ms + "
                 f"fri_tiled_encode_from_streams on 16 threads {t_emit * 1e3:.1f} ms = {base * 1e3:.1f} ms")
        for name, region in REGIONS:
            i0, j0, ni, nj = T.region_tiles(*region)
            cx, cy, cw, ch = T.region_cover(*region)
            img_b = img_a.copy()
            img_b[cy:cy + ch, cx:cx + cw] = other[cy:cy + ch, cx:cx + cw]
            part = U.arrays(ni * nj)
            rc, t_r = _wall(lambda: U.encode_region(img_b, qm, region, part), repeats)
            assert rc == 0 and not part["oob"].any()
            size, t_u = _wall(lambda: U.emit_update(file_a, region, part, out), repeats)
            updated = out[:size].copy()
            assert U.encode_whole(img_b, qm, whole) == 0  # the whole encode of the changed image: the same file
            assert np.array_equal(updated, out[: U.emit_whole(whole, out)]), (mode, name)
            total = t_r + t_u
            rep.line(f"{mode}: {name} ({ni * nj} of {T.n_tiles} tiles, {cw}x{ch} pixels up): fri_hip_encode_region_tiled_symbols {t_r * 1e3:.2f} ms + fri_tiled_update_from_streams "
                     f"on 16 threads {t_u * 1e3:.2f} ms = {total * 1e3:.2f} ms, {base / total:.2f} x the whole encode's speed ({total / base:.3f} x its time); byte for byte the whole "
                     f"encode of the changed image")
    T.close()


def step_plan(rep, n, rounds, repeats):
    import numpy as np
    import torch

    import frave_amd
    import frave_amd.emit as emit

    big = 16384
    ctx = frave_amd.Context(0)
    torch.zeros(1, device="cuda")
    free = lambda: torch.cuda.mem_get_info()[0]  # noqa: E731
    rep.line(f"python3 tools/region_update_time.py plan (case B: a {big}x{big} plane, half smooth / half noise, in {TILE}x{TILE} tiles, lossless; device bytes = the fall of "
             f"hipMemGetInfo's free bytes from before the plan to after its first call; wall clock of single calls, the first on a fresh plan and the one after it)")
    img = _mixed_image(np, big, 1, 5)
    qm = frave_amd.quality_matrix(100)
    region = (5200, 7200, 200, 200)  # inside tile (10, 14)
    before = free()
    T = frave_amd.PlanTiled(ctx, big, big, 1, TILE, TILE)
    T.set_stream_order()
    U = _Update(np, frave_amd, emit, T, big, big, 1, 1)
    i0, j0, ni, nj = T.region_tiles(*region)
    part = U.arrays(ni * nj)
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        assert U.encode_region(img, qm, region, part) == 0
        times.append(time.perf_counter() - t0)
    region_bytes = before - free()
    assert ni * nj == 1
    rep.line(f"one tile ({ni * nj} of {T.n_tiles}, region {region}): the plan holds {region_bytes / 1e6:.1f} MB on the device; fri_hip_encode_region_tiled_symbols {times[0] * 1e3:.1f} ms "
             f"the first time, {times[1] * 1e3:.2f} ms the second")
    T.close()
    torch.cuda.synchronize()
    before = free()
    T = frave_amd.PlanTiled(ctx, big, big, 1, TILE, TILE)
    T.set_stream_order()
    U = _Update(np, frave_amd, emit, T, big, big, 1, 1)
    whole = U.arrays(T.n_tiles)
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        assert U.encode_whole(img, qm, whole) == 0
        times.append(time.perf_counter() - t0)
    whole_bytes = before - free()
    rep.line(f"the whole image ({T.n_tiles} tiles): the plan holds {whole_bytes / 1e6:.1f} MB on the device, {whole_bytes / max(region_bytes, 1):.1f} x the one-tile plan's; "
             f"fri_hip_encode_image_tiled_symbols {times[0] * 1e3:.1f} ms the first time, {times[1] * 1e3:.1f} ms the second")
    # the update of the one tile on the whole file, and the whole emit it replaces
    n_oob = int(np.count_nonzero(whole["oob"]))
    if n_oob:  # (the host library refuses such an image: "symbol outside the 1024-entry alphabet")
        rep.line(f"{n_oob} of the {T.n_tiles} tiles have symbols outside the alphabet: no file of this image, the emitter's part of case B is not measured")
        T.close()
        return
    out = np.empty(whole["sym"].size * 4 + (1 << 24), np.uint8)
    t0 = time.perf_counter()
    size = U.emit_whole(whole, out)
    t_emit = time.perf_counter() - t0
    file_a = out[:size].copy()
    img[region[1]:region[1] + region[3], region[0]:region[0] + region[2], 0] ^= 0x55
    assert U.encode_region(img, qm, region, part) == 0 and not part["oob"].any()
    t0 = time.perf_counter()
    size = U.emit_update(file_a, region, part, out)
    t_update = time.perf_counter() - t0
    rep.line(f"file {file_a.size} bytes: fri_tiled_encode_from_streams on 16 threads {t_emit * 1e3:.1f} ms; fri_tiled_update_from_streams of the one tile {t_update * 1e3:.1f} ms "
             f"(the copy of the other {T.n_tiles - 1} payloads), the updated file {size} bytes")
    T.close()


def main():
    pos, out, n, rounds, repeats = _args()
    steps = {"kernel": step_kernel, "host": step_host, "plan": step_plan}
    if not pos or pos[0] not in steps:
        print(__doc__)
        return 2
    rep = Report(out, fresh=pos[0] == "kernel")
    steps[pos[0]](rep, n, rounds, repeats)
    return 0


if __name__ == "__main__":
    sys.exit(main())
