"""What tiled coding (fri_hip_plan_tiled, K10: k10_tiles.hip, the `frit` container) costs against coding the whole plane. Three steps, each a process of its own that
appends its section to the report; run them under a time limit each and chained, so that trouble in one ends the run:

    timeout -k 10 300 python3 tools/tiled_time.py kernels && timeout -k 10 300 python3 tools/tiled_time.py chain && timeout -k 10 600 python3 tools/tiled_time.py host

kernels: the split and the merge of a 4096^2 plane in 64 tiles of 512^2 (C = 1, and C = 3) over rotating HBM-resident slots (more bytes than the 256 MB cache),
         timed with events around `launches` launches; next to each a device-to-device hipMemcpyAsync that moves the same total bytes. Medians of interleaved
         rounds; the 2 W H C algorithmic bytes and their fraction of 8 TB/s.
chain:   the tiled encode chain with the fit on (fri_hip_encode_symbols_tiled_dev: split + one direct stream chain over 64 tiles of 512^2) against the whole-plane
         chain (fri_hip_encode_symbols_batch_dev in its direct form with n = 1 on a 4096^2 plan), and the 64-tile batch chain without the split (fed the tile
         raster): where the difference goes. Lossless, half smooth / half noise planes, interleaved rounds, medians.
host:    one half smooth / half noise 4096^2 plane through the device with fitted parameters, whole and in tiles of 512 and 256; then the host stages alone, wall
         clock, medians of three: fri_emit_encode_image_from_streams and fri_emit_decode_image on the whole plane, fri_tiled_encode_from_streams and
         fri_tiled_decode at 1, 4 and 16 threads on the 512 tiles; the file sizes.

usage: python3 tools/tiled_time.py kernels|chain|host [--out profiles/tiled_time.txt] [--launches 200] [--rounds 5]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12  # bytes per second
SIZE, TILE = 4096, 512


def _args():
    a = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "tiled_time.txt"), "--launches": "200", "--rounds": "5"}
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


def _events(torch, s, fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for i in range(launches):
        fn(i)
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def _mixed_plane(np, size, seed):
    """left half smooth, right half noise (tests/test_emit.py's image): small and large prediction widths"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:size, 0:size]
    smooth = (((x + 2 * y) >> 3) + rng.integers(0, 8, (size, size))) & 0xFF
    noise = rng.integers(0, 256, (size, size))
    return np.where(x < size // 2, smooth, noise).astype(np.uint8)


def step_kernels(rep, n, rounds):
    import torch

    import frave_amd

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    ctx = frave_amd.Context(0)
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    rep.line(f"python3 tools/tiled_time.py kernels --launches {n} --rounds {rounds} (one process; medians of {rounds} interleaved rounds, us per launch)")
    for channels, slots in ((1, 24), (3, 8)):
        T = frave_amd.PlanTiled(ctx, SIZE, SIZE, channels, TILE, TILE)
        nbytes = SIZE * SIZE * channels
        d_img = torch.randint(0, 256, (slots, nbytes), dtype=torch.uint8, device="cuda")
        d_tiles = torch.randint(0, 256, (slots, nbytes), dtype=torch.uint8, device="cuda")
        d_back = torch.empty_like(d_img)
        total = 2 * nbytes  # every byte is read once and written once
        L, h = frave_amd.load_library(), T._h
        img, tiles, back = ([t[k].data_ptr() for k in range(slots)] for t in (d_img, d_tiles, d_back))
        # (the library's entry points called directly with pointers worked out beforehand: a short launch must not wait for the interpreter)
        fns = {
            "split": lambda i: L.fri_hip_split_tiles_dev(h, img[i % slots], tiles[i % slots], sp),
            "merge": lambda i: L.fri_hip_merge_tiles_dev(h, tiles[i % slots], back[i % slots], sp),
            "hipMemcpyAsync D2D": lambda i: hip.hipMemcpyAsync(back[i % slots], img[(i + 1) % slots], nbytes, 3, sp),  # hipMemcpyDeviceToDevice
        }
        res = {k: [] for k in fns}
        for k, fn in fns.items():
            assert fn(0) == 0, k
            _events(torch, s, fn, 2 * slots)  # spin-up
        for _ in range(rounds):
            for k, fn in fns.items():
                _events(torch, s, fn, slots)
                res[k].append(_events(torch, s, fn, n))
        cp = statistics.median(res["hipMemcpyAsync D2D"])
        for k in ("split", "merge"):
            us = statistics.median(res[k])
            rep.line(f"{k} {SIZE}x{SIZE}x{channels} in {T.n_tiles} tiles of {TILE}x{TILE}, {slots} slots, {n} launches: {us:.2f} us, {total / 1e6:.1f} MB algorithmic = "
                     f"{total / us / 1e6:.2f} TB/s ({100 * total / us * 1e6 / PEAK:.1f} % of 8 TB/s); D2D copy of the same bytes {cp:.2f} us ({us / cp:.2f} x the copy); rounds "
                     + " ".join(f"{x:.2f}" for x in res[k]) + " / copy " + " ".join(f"{x:.2f}" for x in res["hipMemcpyAsync D2D"]))
        del d_img, d_tiles, d_back
        torch.cuda.empty_cache()
        T.close()


def step_chain(rep, n, rounds):
    import numpy as np
    import torch

    import frave_amd

    ctx = frave_amd.Context(0)
    slots = 16
    px = SIZE * SIZE
    launches = max(slots, n // 4)
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    rep.line(f"python3 tools/tiled_time.py chain --launches {n} --rounds {rounds} ({SIZE}x{SIZE}x1, lossless, the fit on, half smooth / half noise planes, {slots} slots, "
             f"{launches} launches per round; us per plane, medians of {rounds} interleaved rounds)")
    T = frave_amd.PlanTiled(ctx, SIZE, SIZE, 1, TILE, TILE)
    T.set_stream_order()
    Q = frave_amd.Plan(ctx, SIZE, SIZE, 1)
    Q.set_stream_order()
    nt = T.n_tiles
    host = np.stack([_mixed_plane(np, SIZE, 100 + k).reshape(-1) for k in range(slots)])
    d_img = torch.from_numpy(host).cuda()
    d_tiles = torch.empty_like(d_img)
    for k in range(slots):
        T.split_tiles_dev(d_img[k].data_ptr(), d_tiles[k].data_ptr(), stream=sp)
    n_sym = max(nt * T.num_some, Q.num_some)
    d_sym = torch.empty((slots, n_sym), dtype=torch.int16, device="cuda")
    d_hist = torch.empty((slots, nt * 10 * 1024), dtype=torch.int32, device="cuda")
    d_par = torch.zeros((slots, nt * 36), dtype=torch.float32, device="cuda")
    d_oob = torch.zeros((slots, 2 * nt), dtype=torch.int64, device="cuda")
    ones = np.ones(32, np.int32)

    def tiled(i):
        k = i % slots
        T.encode_symbols_tiled_dev(d_img[k].data_ptr(), d_par[k].data_ptr(), d_sym[k].data_ptr(), d_hist[k].data_ptr(), d_oob[k].data_ptr(), d_oob[k].data_ptr() + 8 * nt,
                                   qmatrix=ones, fit=True, stream=sp)

    def batch(i):  # the same without the split: the inner plan on the tile raster
        k = i % slots
        T.tile.encode_symbols_batch_dev(nt, d_tiles[k].data_ptr(), TILE * TILE, ones, True, d_par[k].data_ptr(), None, 0, None, 0, d_sym[k].data_ptr(), T.num_some,
                                        d_hist[k].data_ptr(), d_oob[k].data_ptr(), d_oob[k].data_ptr() + 8 * nt, stream=sp)

    def whole(i):
        k = i % slots
        Q.encode_symbols_batch_dev(1, d_img[k].data_ptr(), 0, ones, True, d_par[k].data_ptr(), None, 0, None, 0, d_sym[k].data_ptr(), Q.num_some, d_hist[k].data_ptr(),
                                   d_oob[k].data_ptr(), d_oob[k].data_ptr() + 8 * nt, stream=sp)

    fns = {"tiled chain": tiled, "64-tile batch chain, no split": batch, "whole-plane chain": whole}
    res = {k: [] for k in fns}
    for fn in fns.values():
        _events(torch, s, fn, 2 * slots)  # spin-up: everything the chains allocate exists
    for _ in range(rounds):
        for k, fn in fns.items():
            _events(torch, s, fn, slots)
            res[k].append(_events(torch, s, fn, launches))
    a, b, c = (statistics.median(res[k]) for k in fns)
    rep.line(f"tiled chain (split + {nt} tiles of {TILE}x{TILE} as one batch) {a:.2f} us; the batch alone {b:.2f} us (the split adds {a - b:.2f} us); whole-plane chain {c:.2f} us; "
             f"tiled / whole {a / c:.3f}; symbols per plane: tiles {nt * T.num_some}, whole {Q.num_some}; rounds tiled " + " ".join(f"{x:.2f}" for x in res["tiled chain"])
             + " / batch " + " ".join(f"{x:.2f}" for x in res["64-tile batch chain, no split"]) + " / whole " + " ".join(f"{x:.2f}" for x in res["whole-plane chain"]))
    T.close(), Q.close()


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

    ctx = frave_amd.Context(0)
    img = _mixed_plane(np, SIZE, 7).reshape(SIZE, SIZE, 1)
    rep.line(f"python3 tools/tiled_time.py host ({SIZE}x{SIZE}x1 half smooth / half noise, lossless, fitted parameters; host stages alone, wall clock, medians of 3; "
             f"{os.cpu_count()} CPUs visible, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', '-')})")
    Q = frave_amd.Plan(ctx, SIZE, SIZE, 1)
    Q.set_stream_order()
    sym, vp, wp, hist, oob = Q.encode_image_symbols(img, fit=True)
    assert not oob.any()
    whole, t_enc = _wall(lambda: emit.encode_image_from_streams(SIZE, SIZE, sym, hist, vp, wp))
    dec, t_dec = _wall(lambda: emit.decode_image(whole))
    assert np.array_equal(Q.inverse_transform(dec[4]), img.reshape(-1))
    Q.close()
    rep.line(f"whole plane: file {len(whole)} bytes; fri_emit_encode_image_from_streams {t_enc * 1e3:.1f} ms; fri_emit_decode_image {t_dec * 1e3:.1f} ms")
    for tile in (512, 256):
        T = frave_amd.PlanTiled(ctx, SIZE, SIZE, 1, tile, tile)
        T.set_stream_order()
        tsym, tvp, twp, thist, toob = T.encode_image_tiled_symbols(img)
        assert not toob.any()
        empty = int((thist.sum(axis=3) == 0).sum())
        files = {}
        for threads in (1, 4, 16):
            files[threads], t_e = _wall(lambda: emit.tiled_encode_from_streams(SIZE, SIZE, tile, tile, tsym, thist, tvp, twp, threads=threads))
            (ti, coefs), t_d = _wall(lambda: emit.tiled_decode(files[threads], threads))
            rep.line(f"{tile}x{tile} tiles ({T.n_tiles}), {threads:2d} threads: fri_tiled_encode_from_streams {t_e * 1e3:.1f} ms ({t_enc / t_e:.2f} x the whole plane's emit); "
                     f"fri_tiled_decode {t_d * 1e3:.1f} ms ({t_dec / t_d:.2f} x the whole plane's decode)")
        assert files[1] == files[4] == files[16]
        assert np.array_equal(T.decode_image_tiled(coefs), img.reshape(-1))
        rep.line(f"{tile}x{tile} tiles: file {len(files[1])} bytes = {100.0 * (len(files[1]) / len(whole) - 1):+.2f} % against the whole plane's {len(whole)}; "
                 f"{empty} of {T.n_tiles * 10} contexts without symbols; the file decodes to the input")
        T.close()


def main():
    pos, out, n, rounds = _args()
    steps = {"kernels": step_kernels, "chain": step_chain, "host": step_host}
    if not pos or pos[0] not in steps:
        print(__doc__)
        return 2
    rep = Report(out, fresh=pos[0] == "kernels")
    steps[pos[0]](rep, n, rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
