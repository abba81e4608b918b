"""What the quality searches, the measuring kernel and the device coder of tiled 4:2:0 cost (fri_hip_search_quality*_tiled420, K12's measure_tiles420_kernel,
fri_hip_encode_image_tiled420_coded). Three steps, each a process of its own that appends its section to the report; run them under a time limit each and
chained, so that trouble in one ends the run:

    timeout -k 10 300 python3 tools/tiled420_search_time.py kernels && timeout -k 10 420 python3 tools/tiled420_search_time.py searches && \\
        timeout -k 10 420 python3 tools/tiled420_search_time.py coder

All on a 4096^2 RGB image, left half smooth and right half noise, in 4:2:0 tiles of about 512^2 and about 256^2 (fri_hip_tile_shape420).

kernels:  the measuring kernel over rotating HBM-resident slots (more bytes than the 256 MB cache), timed with events around `launches` launches, next to the
          whole-image merge on the same planes: they read the same planes; the measure loads the reference raster where the merge stores its raster.
searches: wall clock per call of the three tiled 4:2:0 searches (the _dev forms, pixels resident) beside the tiled 4:4:4 YCbCr searches on the same tile grid
          and the untiled 4:2:0 searches. Medians of interleaved rounds after one round that is not counted.
coder:    quality 60: fri_hip_encode_image_tiled420_coded + fri_tiled_encode_from_coded420 against fri_hip_encode_image_tiled420_symbols +
          fri_tiled_encode_from_streams420, both on 16 emitter threads, by wall clock, with the bytes each route reads back; the two files are compared.

usage: python3 tools/tiled420_search_time.py kernels|searches|coder [--out profiles/tiled420_search_time.txt] [--launches 200] [--rounds 5]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12  # bytes per second
SIZE, TARGETS = 4096, (512, 256)
COLOUR_YCBCR = 3
TARGET_DB, TARGET_SSIM, QUALITY = 30.0, 0.9, 60


def _args():
    a = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "tiled420_search_time.txt"), "--launches": "200", "--rounds": "5"}
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


def _mixed_image(np, size, seed):
    """left half smooth, right half noise (tools/tiled_search_time.py's image), the channels decorrelated a little"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:size, 0:size]
    out = np.empty((size, size, 3), np.uint8)
    for c in range(3):
        smooth = (((x + 2 * y + 40 * c) >> 3) + rng.integers(0, 8, (size, size))) & 0xFF
        noise = rng.integers(0, 256, (size, size))
        out[:, :, c] = np.where(x < size // 2, smooth, noise)
    return out


def _fmt(xs):
    return " ".join(f"{x:.2f}" for x in xs)


def step_kernels(rep, n, rounds):
    import torch

    import frave_amd

    ctx = frave_amd.Context(0)
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    rep.line(f"python3 tools/tiled420_search_time.py kernels --launches {n} --rounds {rounds} (one process; medians of {rounds} interleaved rounds, us per launch)")
    L = frave_amd.load_library()
    slots = 8
    for target in TARGETS:
        tw, th = frave_amd.api.tile_shape420(SIZE, SIZE, target)
        T = frave_amd.PlanTiled420(ctx, SIZE, SIZE, tw, th)
        h = T._h
        d_ref = torch.randint(0, 256, (slots, T.pixel_bytes), dtype=torch.uint8, device="cuda")
        d_y = torch.randint(0, 256, (slots, T.y_tile_bytes), dtype=torch.uint8, device="cuda")
        d_c = torch.randint(0, 256, (slots, T.c_tile_bytes), dtype=torch.uint8, device="cuda")
        d_back = torch.empty_like(d_ref)
        d_out = torch.zeros((slots, 8), dtype=torch.int64, device="cuda")
        total = T.pixel_bytes + T.y_tile_bytes + T.c_tile_bytes  # the measure reads the planes and the reference; the merge reads the planes and writes the raster
        ref, ys, cs, back, out = ([t[k].data_ptr() for k in range(slots)] for t in (d_ref, d_y, d_c, d_back, d_out))
        fns = {
            "measure": lambda i: L.fri_hip_measure_distortion_tiled420_dev(h, ys[i % slots], cs[i % slots], ref[i % slots], out[i % slots], sp),
            "merge": lambda i: L.fri_hip_merge_tiles420_dev(h, ys[i % slots], cs[i % slots], back[i % slots], sp),
        }
        res = {k: [] for k in fns}
        for k, fn in fns.items():
            assert fn(0) == 0, k
            _events(torch, s, fn, 2 * slots)  # spin-up
        for _ in range(rounds):
            for k, fn in fns.items():
                _events(torch, s, fn, slots)
                res[k].append(_events(torch, s, fn, n))
        me, mg = (statistics.median(res[k]) for k in fns)
        rep.line(f"measure {SIZE}x{SIZE}x3 in {T.n_tiles} 4:2:0 tiles of {tw}x{th}, {slots} slots of {total / 1e6:.1f} MB, {n} launches (the clearing kernel included): {me:.2f} us, "
                 f"{total / 1e6:.1f} MB read = {total / me / 1e6:.2f} TB/s ({100 * total / me * 1e6 / PEAK:.1f} % of 8 TB/s); merge of the same planes {mg:.2f} us = "
                 f"{total / mg / 1e6:.2f} TB/s read and written ({me / mg:.2f} x the merge); rounds measure {_fmt(res['measure'])} / merge {_fmt(res['merge'])}")
        T.close()
        del d_ref, d_y, d_c, d_back
        torch.cuda.empty_cache()


def step_searches(rep, n, rounds):
    import numpy as np
    import torch

    import frave_amd

    ctx = frave_amd.Context(0)
    rep.line(f"python3 tools/tiled420_search_time.py searches --rounds {rounds} ({SIZE}x{SIZE}x3, half smooth / half noise; the _dev forms on resident pixels; wall clock "
             f"per call in ms, medians of {rounds} interleaved rounds after one uncounted round)")
    img = _mixed_image(np, SIZE, 7)
    d_img = torch.from_numpy(img.reshape(-1).copy()).cuda()
    p = d_img.data_ptr()
    Q = frave_amd.Plan420(ctx, SIZE, SIZE)
    Q.set_stream_order()
    for target in TARGETS:
        tw, th = frave_amd.api.tile_shape420(SIZE, SIZE, target)
        T = frave_amd.PlanTiled420(ctx, SIZE, SIZE, tw, th)
        T.set_stream_order()
        F = frave_amd.PlanTiled(ctx, SIZE, SIZE, 3, tw, th)  # the same grid in 4:4:4 YCbCr
        F.set_stream_order()
        F.tile.set_colour_transform(COLOUR_YCBCR)
        budget = 3 * F.search_quality_for_size(p, 1 << 40)[1] // 4  # three quarters of the 4:4:4 file's estimate at quality 99: a budget every kind can meet
        calls = {}
        for name, plan in (("tiled 4:2:0", T), ("tiled 4:4:4", F), ("untiled 4:2:0", Q)):
            calls["psnr " + name] = lambda plan=plan: plan.search_quality(p, TARGET_DB)
            calls["ssim " + name] = lambda plan=plan: plan.search_quality_ssim(p, TARGET_SSIM)
            calls["size " + name] = lambda plan=plan: plan.search_quality_for_size(p, budget)
        res = {k: [] for k in calls}
        got = {}
        for r in range(rounds + 1):
            for k, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    got[k] = fn()
                except frave_amd.FriHipError as e:  # (a budget below a kind's quality 1: the search still ran its probes)
                    got[k] = f"refused ({e.code})"
                if r:
                    res[k].append((time.perf_counter() - t0) * 1e3)
        for kind, what in (("psnr", f"{TARGET_DB} dB"), ("ssim", f"SSIM {TARGET_SSIM}"), ("size", f"{budget} bytes")):
            a, b, c = (statistics.median(res[f"{kind} {name}"]) for name in ("tiled 4:2:0", "tiled 4:4:4", "untiled 4:2:0"))
            rep.line(f"{tw}x{th} tiles, {kind} search to {what}: tiled 4:2:0 {a:.2f} ms -> {got[kind + ' tiled 4:2:0']}; tiled 4:4:4 YCbCr {b:.2f} ms -> "
                     f"{got[kind + ' tiled 4:4:4']} (4:2:0 / 4:4:4 {a / b:.2f}); untiled 4:2:0 {c:.2f} ms -> {got[kind + ' untiled 4:2:0']} (tiled / untiled {a / c:.2f}); rounds "
                     f"{_fmt(res[kind + ' tiled 4:2:0'])} / {_fmt(res[kind + ' tiled 4:4:4'])} / {_fmt(res[kind + ' untiled 4:2:0'])}")
        T.close(), F.close()
    Q.close()


def step_coder(rep, n, rounds):
    import numpy as np

    import frave_amd
    import frave_amd.emit as emit

    ctx = frave_amd.Context(0)
    rep.line(f"python3 tools/tiled420_search_time.py coder --rounds {rounds} ({SIZE}x{SIZE}x3, half smooth / half noise, quality {QUALITY}; host pixels in, the file out; 16 emitter "
             f"threads; wall clock in ms, medians of {rounds} interleaved rounds after one uncounted round)")
    img = _mixed_image(np, SIZE, 7)
    for target in TARGETS:
        tw, th = frave_amd.api.tile_shape420(SIZE, SIZE, target)
        T = frave_amd.PlanTiled420(ctx, SIZE, SIZE, tw, th)
        T.set_stream_order()
        res = {k: [] for k in ("device chain", "device emit", "host chain", "host emit")}
        files, down = {}, {}
        for r in range(rounds + 1):
            t0 = time.perf_counter()
            words, n_words, models, off, status, vp, wp = T.encode_image_tiled420_coded(img, QUALITY)
            t1 = time.perf_counter()
            files["device"] = emit.tiled_encode_from_coded420(SIZE, SIZE, tw, th, words, n_words, models, off, vp, wp, QUALITY, threads=16)
            t2 = time.perf_counter()
            sym, hvp, hwp, hist, oob = T.encode_image_tiled420_symbols(img, QUALITY)
            t3 = time.perf_counter()
            files["host"] = emit.tiled_encode_from_streams420(SIZE, SIZE, tw, th, sym, T.n_luma, T.n_chroma, hist, hvp, hwp, QUALITY, threads=16)
            t4 = time.perf_counter()
            if r:
                for k, v in zip(res, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                    res[k].append(v * 1e3)
            # what each route copies down: the counts, status and models, the coded rows and the lists as hipMemcpy2D takes them; against streams and histograms
            planes = 3 * T.n_tiles
            most_off = int(models[:, :, 1].max())
            down["device"] = planes * 45 * 4 + 4 * (T.n_tiles * int(n_words[: T.n_tiles].max()) + 2 * T.n_tiles * int(n_words[T.n_tiles:].max())) + 2 * most_off * planes * 10
            down["host"] = sym.nbytes + hist.nbytes
        assert files["device"] == files["host"] and not status.any()
        dc, de, hc, he = (statistics.median(res[k]) for k in res)
        rep.line(f"{T.n_tiles} 4:2:0 tiles of {tw}x{th}: device coder route {dc + de:.1f} ms (chain, K11 and read-back {dc:.1f}, container {de:.1f}) with {down['device'] / 1e6:.2f} MB down; "
                 f"host coder route {hc + he:.1f} ms (chain and read-back {hc:.1f}, coder and container on 16 threads {he:.1f}) with {down['host'] / 1e6:.2f} MB down; "
                 f"device / host {(dc + de) / (hc + he):.2f}, bytes down {100 * down['device'] / down['host']:.1f} %; the files are equal ({len(files['host'])} bytes); rounds "
                 f"{_fmt(res['device chain'])} + {_fmt(res['device emit'])} / {_fmt(res['host chain'])} + {_fmt(res['host emit'])}")
        T.close()


def main():
    pos, out, n, rounds = _args()
    steps = {"kernels": step_kernels, "searches": step_searches, "coder": step_coder}
    if not pos or pos[0] not in steps:
        print(__doc__)
        return 2
    rep = Report(out, fresh=pos[0] == "kernels")
    steps[pos[0]](rep, n, rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
