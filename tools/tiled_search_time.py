"""What the quality searches and the size estimate over tiles cost, and what they change (fri_hip_search_quality*_tiled, fri_hip_estimate_size_tiled_dev, K10's
measuring kernel). Three steps, each a process of its own that appends its section to the report; run them under a time limit each and chained, so that trouble
in one ends the run:

    timeout -k 10 300 python3 tools/tiled_search_time.py kernels && timeout -k 10 420 python3 tools/tiled_search_time.py searches && \\
        timeout -k 10 420 python3 tools/tiled_search_time.py choice

kernels:  the measuring kernel on a 4096^2 plane in 64 tiles of 512^2 (C = 1, and C = 3) over rotating HBM-resident slots (more bytes than the 256 MB cache), timed
          with events around `launches` launches, next to merge_tiles_kernel and to a device-to-device hipMemcpyAsync of the same bytes; then
          fri_hip_estimate_size_tiled_dev on the histograms of 64 tiles. Medians of interleaved rounds.
searches: wall clock per call of the three tiled searches (the _dev forms, pixels resident) beside the whole-image searches on a 4096^2 plan, on the same half
          smooth / half noise image, C = 1 and C = 3. Medians of interleaved rounds after one round that is not counted.
choice:   on one image (C = 1): the quality, PSNR and size estimate the whole-image searches choose, with what the tiled file of that quality really measures (the
          tiled round trip's PSNR, the emitted file's size); the same for the tiled searches.

usage: python3 tools/tiled_search_time.py kernels|searches|choice [--out profiles/tiled_search_time.txt] [--launches 200] [--rounds 5]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12  # bytes per second
SIZE, TILE = 4096, 512
MIDPOINT = 2  # FRI_HIP_DEQUANT_MIDPOINT
TARGET_DB, TARGET_SSIM = 40.0, 0.95


def _args():
    a = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "tiled_search_time.txt"), "--launches": "200", "--rounds": "5"}
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


def _mixed_image(np, size, channels, seed):
    """left half smooth, right half noise (tools/tiled_time.py's plane), the channels decorrelated a little"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:size, 0:size]
    out = np.empty((size, size, channels), np.uint8)
    for c in range(channels):
        smooth = (((x + 2 * y + 40 * c) >> 3) + rng.integers(0, 8, (size, size))) & 0xFF
        noise = rng.integers(0, 256, (size, size))
        out[:, :, c] = np.where(x < size // 2, smooth, noise)
    return out


def _fmt(xs):
    return " ".join(f"{x:.2f}" for x in xs)


def step_kernels(rep, n, rounds):
    import torch

    import frave_amd

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    ctx = frave_amd.Context(0)
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    rep.line(f"python3 tools/tiled_search_time.py kernels --launches {n} --rounds {rounds} (one process; medians of {rounds} interleaved rounds, us per launch)")
    L = frave_amd.load_library()
    for channels, slots in ((1, 24), (3, 8)):
        T = frave_amd.PlanTiled(ctx, SIZE, SIZE, channels, TILE, TILE)
        h = T._h
        nbytes = SIZE * SIZE * channels
        d_ref = torch.randint(0, 256, (slots, nbytes), dtype=torch.uint8, device="cuda")
        d_tiles = torch.randint(0, 256, (slots, nbytes), dtype=torch.uint8, device="cuda")
        d_back = torch.empty_like(d_ref)
        d_out = torch.zeros((slots, 8), dtype=torch.int64, device="cuda")
        total = 2 * nbytes  # the measure reads two rasters; the merge and the copy read one and write one
        ref, tiles, back, out = ([t[k].data_ptr() for k in range(slots)] for t in (d_ref, d_tiles, d_back, d_out))
        fns = {
            "measure": lambda i: L.fri_hip_measure_distortion_tiled_dev(h, tiles[i % slots], ref[i % slots], out[i % slots], sp),
            "merge": lambda i: L.fri_hip_merge_tiles_dev(h, tiles[i % slots], back[i % slots], sp),
            "hipMemcpyAsync D2D": lambda i: hip.hipMemcpyAsync(back[i % slots], ref[(i + 1) % slots], nbytes, 3, sp),  # hipMemcpyDeviceToDevice
        }
        res = {k: [] for k in fns}
        for k, fn in fns.items():
            assert fn(0) == 0, k
            _events(torch, s, fn, 2 * slots)  # spin-up
        for _ in range(rounds):
            for k, fn in fns.items():
                _events(torch, s, fn, slots)
                res[k].append(_events(torch, s, fn, n))
        me, mg, cp = (statistics.median(res[k]) for k in fns)
        rep.line(f"measure {SIZE}x{SIZE}x{channels} in {T.n_tiles} tiles of {TILE}x{TILE}, {slots} slots, {n} launches (the clearing kernel included): {me:.2f} us, "
                 f"{total / 1e6:.1f} MB read = {total / me / 1e6:.2f} TB/s ({100 * total / me * 1e6 / PEAK:.1f} % of 8 TB/s); merge {mg:.2f} us ({me / mg:.2f} x the merge); "
                 f"D2D copy of the same bytes {cp:.2f} us ({me / cp:.2f} x the copy); rounds measure {_fmt(res['measure'])} / merge {_fmt(res['merge'])} / copy "
                 f"{_fmt(res['hipMemcpyAsync D2D'])}")
        del d_ref, d_tiles, d_back
        torch.cuda.empty_cache()
        # the estimate: the histograms of 64 tiles, every context filled alike
        nt, eslots = T.n_tiles, 8
        words = nt * channels * 10 * 1024
        import numpy as np

        shape = (20000.0 * np.exp(-np.arange(1024) / 8.0)).astype(np.int32)  # a context as images fill it: a peak and a tail that runs out (a few listed values)
        host = np.stack([np.tile(shape // (1 + k), nt * channels * 10) for k in range(eslots)])
        d_hist = torch.from_numpy(host).cuda()
        d_file = torch.zeros((eslots, 1), dtype=torch.int64, device="cuda")
        d_tb = torch.zeros((eslots, nt), dtype=torch.int64, device="cuda")
        hist, fb, tb = ([t[k].data_ptr() for k in range(eslots)] for t in (d_hist, d_file, d_tb))

        def est(i):
            return L.fri_hip_estimate_size_tiled_dev(h, hist[i % eslots], None, fb[i % eslots], tb[i % eslots], None, sp)

        assert est(0) == 0
        _events(torch, s, est, 2 * eslots)
        times = []
        for _ in range(rounds):
            _events(torch, s, est, eslots)
            times.append(_events(torch, s, est, n))
        torch.cuda.synchronize()
        assert int(d_file[0, 0]) > 0
        rep.line(f"fri_hip_estimate_size_tiled_dev, {nt} tiles x {channels} channels ({nt * channels * 10} contexts, {4 * words / 1e6:.1f} MB of histograms), {eslots} slots, "
                 f"{n} launches: {statistics.median(times):.2f} us per call (a memset and three kernels); rounds {_fmt(times)}")
        T.close()


def _plans(frave_amd, ctx, channels):
    T = frave_amd.PlanTiled(ctx, SIZE, SIZE, channels, TILE, TILE)
    T.set_stream_order()
    Q = frave_amd.Plan(ctx, SIZE, SIZE, channels)
    Q.set_stream_order()
    return T, Q


def step_searches(rep, n, rounds):
    import numpy as np
    import torch

    import frave_amd

    ctx = frave_amd.Context(0)
    rep.line(f"python3 tools/tiled_search_time.py searches --rounds {rounds} ({SIZE}x{SIZE}, half smooth / half noise; tiled: {TILE}x{TILE} tiles; the _dev forms on resident "
             f"pixels; wall clock per call in ms, medians of {rounds} interleaved rounds after one uncounted round)")
    for channels in (1, 3):
        img = _mixed_image(np, SIZE, channels, 7)
        d_img = torch.from_numpy(img.reshape(-1).copy()).cuda()
        p = d_img.data_ptr()
        T, Q = _plans(frave_amd, ctx, channels)
        budget = 3 * Q.search_quality_for_size(p, 1 << 40)[1] // 4  # three quarters of the lossless file's estimate
        calls = {
            "psnr tiled": lambda: T.search_quality(p, TARGET_DB), "psnr whole": lambda: Q.search_quality(p, TARGET_DB),
            "ssim tiled": lambda: T.search_quality_ssim(p, TARGET_SSIM), "ssim whole": lambda: Q.search_quality_ssim(p, TARGET_SSIM),
            "size tiled": lambda: T.search_quality_for_size(p, budget), "size whole": lambda: Q.search_quality_for_size(p, budget),
        }
        res = {k: [] for k in calls}
        got = {}
        for r in range(rounds + 1):
            for k, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got[k] = fn()
                if r:
                    res[k].append((time.perf_counter() - t0) * 1e3)
        for kind, target in (("psnr", f"{TARGET_DB} dB"), ("ssim", f"SSIM {TARGET_SSIM}"), ("size", f"{budget} bytes")):
            a, b = statistics.median(res[kind + " tiled"]), statistics.median(res[kind + " whole"])
            rep.line(f"C = {channels}, {kind} search to {target}: tiled {a:.2f} ms -> {got[kind + ' tiled']}; whole image {b:.2f} ms -> {got[kind + ' whole']}; tiled / whole "
                     f"{a / b:.2f}; rounds tiled {_fmt(res[kind + ' tiled'])} / whole {_fmt(res[kind + ' whole'])}")
        T.close(), Q.close()
        del d_img
        torch.cuda.empty_cache()


def _tiled_psnr_at(frave_amd, np, torch, T, d_img, quality):
    """the PSNR of the tiled round trip at `quality`, from the pieces: split, forward and inverse kernels over all tiles (midpoint dequantiser), the measuring kernel"""
    qm = frave_amd.quality_matrix(quality)
    nt, c = T.n_tiles, T.channels
    per_tile, per_coefs = T.tile_bytes // nt, T.tile.coef_count
    d_tiles = torch.empty(T.tile_bytes, dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros(T.tile_bytes, dtype=torch.uint8, device="cuda")
    d_coefs = torch.empty(nt * per_coefs, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(2 * c + 1, dtype=torch.int64, device="cuda")
    T.split_tiles_dev(d_img.data_ptr(), d_tiles.data_ptr())
    T.tile.transform_quant_dev(d_tiles.data_ptr(), d_coefs.data_ptr(), qm, n_images=nt, pixel_stride=per_tile, coef_stride=per_coefs)
    T.tile.set_dequantiser(MIDPOINT)
    T.tile.inverse_transform_batch_dev(nt, d_coefs.data_ptr(), per_coefs, d_rec.data_ptr(), per_tile, qm)
    T.tile.set_dequantiser(0)
    T.measure_distortion_tiled_dev(d_rec.data_ptr(), d_img.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    return float(frave_amd.api.distortion_psnr(d_out.cpu().numpy().view(np.uint64), c))


def _tiled_file_bytes(frave_amd, emit, T, img, quality):
    sym, vp, wp, hist, oob = T.encode_image_tiled_symbols(img, frave_amd.quality_matrix(quality))
    assert not oob.any()
    return len(emit.tiled_encode_from_streams(SIZE, SIZE, TILE, TILE, sym, hist, vp, wp, quality=quality if quality < 100 else 0, threads=16))


def step_choice(rep, n, rounds):
    import numpy as np
    import torch

    import frave_amd
    import frave_amd.emit as emit

    ctx = frave_amd.Context(0)
    channels = 1
    img = _mixed_image(np, SIZE, channels, 7)
    d_img = torch.from_numpy(img.reshape(-1).copy()).cuda()
    T, Q = _plans(frave_amd, ctx, channels)
    budget = 3 * Q.search_quality_for_size(d_img.data_ptr(), 1 << 40)[1] // 4  # three quarters of the lossless file's estimate
    rep.line(f"python3 tools/tiled_search_time.py choice ({SIZE}x{SIZE}x{channels}, half smooth / half noise, {TILE}x{TILE} tiles: what each search chooses, and what the tiled file of "
             f"that quality measures - the tiled round trip's PSNR from the kernels, the size of the file the emitter writes)")
    for name, plan in (("whole-image", Q), ("tiled", T)):
        q, db = plan.search_quality(d_img.data_ptr(), TARGET_DB)
        real = _tiled_psnr_at(frave_amd, np, torch, T, d_img, q) if q < 100 else float("inf")
        rep.line(f"{name} PSNR search to {TARGET_DB} dB: quality {q}, its own measure {db:.4f} dB; the tiled round trip at quality {q} measures {real:.4f} dB "
                 f"({'reaches' if real >= TARGET_DB else 'MISSES'} the target)")
        q, est = plan.search_quality_for_size(d_img.data_ptr(), budget)
        size = _tiled_file_bytes(frave_amd, emit, T, img, q)
        rep.line(f"{name} size search to {budget} bytes: quality {q}, its own estimate {est} bytes; the tiled file of quality {q} is {size} bytes "
                 f"(estimate {100.0 * (est / size - 1):+.3f} %; {'within' if size <= budget else 'OVER'} the budget)")
    T.close(), Q.close()


def main():
    pos, out, n, rounds = _args()
    steps = {"kernels": step_kernels, "searches": step_searches, "choice": step_choice}
    if not pos or pos[0] not in steps:
        print(__doc__)
        return 2
    rep = Report(out, fresh=pos[0] == "kernels")
    steps[pos[0]](rep, n, rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
