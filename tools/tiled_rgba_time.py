"""What the fused raster kernels of tiled RGBA coding (K16, k16_tiles_rgba.hip) cost against the composition of K9 and K10 they replace, and what a tiled RGBA
encode and decode cost against the untiled RGBA ones. Two steps, each a process of its own that appends its section to the report; run them under a time limit
each and chained, so that trouble in one ends the run:

    timeout -k 10 300 python3 tools/tiled_rgba_time.py kernel && timeout -k 10 900 python3 tools/tiled_rgba_time.py host

kernel: a 4096^2 R, G, B, A raster in 512^2 and in 256^2 tiles. The split: split_tiles_rgba_kernel (one launch) against split_rgba_kernel, then
        split_tiles_kernel<3> and split_tiles_kernel<1> (three launches) into the same tile rasters. The whole merge: merge_tiles_rgba_region_kernel on the
        region (0, 0, W, H) against merge_tiles_kernel<3>, merge_tiles_kernel<1>, then merge_rgba_kernel. Device events around `launches` back-to-back
        repetitions; medians of interleaved rounds after a spin-up, and the rounds themselves, whose spread is the run-to-run noise. Every repetition works on
        another slot of pools of more bytes than the 256 MB cache, so none finds its lines cached. Algorithmic bytes: 8 W H for the fused kernels, 16 W H for the
        compositions. Both routes give the same bytes, checked once.
host:   the same raster (half smooth, half noise, alpha in runs), YCbCr at quality 60, host memory to host memory through the Python bindings (the output arrays
        are allocated inside the timed call), wall clock, medians of `repeats` after one warm-up call. Encode: fri_hip_encode_image_tiled_rgba_symbols +
        fri_tiled_encode_from_streams_rgba on 16 threads against fri_hip_encode_image_rgba_symbols + fri_emit_encode_image_from_streams. Decode: fri_tiled_decode
        on 16 threads + fri_hip_decode_image_tiled_rgba against fri_emit_decode_image + fri_hip_decode_image_rgba.

usage: python3 tools/tiled_rgba_time.py kernel|host [--out profiles/tiled_rgba_time.txt] [--launches 50] [--rounds 5] [--repeats 3]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12  # bytes per second
SIZE, TILES = 4096, (512, 256)
QUALITY = 60


def _args():
    a = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "tiled_rgba_time.txt"), "--launches": "50", "--rounds": "5", "--repeats": "3"}
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


def step_kernel(rep, n, rounds, repeats):
    import torch

    import frave_amd
    from frave_amd.api import TILED_ALLOW_HOLES

    ctx = frave_amd.Context(0)
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    L = frave_amd.load_library()
    at = [0]  # repetitions so far: every repetition of a kind goes on from where the last one stopped

    def events(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for i in range(at[0], at[0] + launches):
            fn(i)
        e1.record(s)
        e1.synchronize()
        at[0] += launches
        return e0.elapsed_time(e1) * 1e3 / launches

    slots, N = 6, SIZE * SIZE
    rep.line(f"python3 tools/tiled_rgba_time.py kernel --launches {n} --rounds {rounds} (one process; device events around {n} back-to-back repetitions, medians of {rounds} "
             f"interleaved rounds after a spin-up, us per repetition; every repetition on another of {slots} slots of pools larger than the 256 MB cache)")
    R = frave_amd.PlanRGBA(ctx, SIZE, SIZE)  # (K9's launchers go through a plan of the image's shape)
    d_rgba = torch.randint(0, 256, (slots, 4 * N), dtype=torch.uint8, device="cuda")
    d_back = torch.empty_like(d_rgba)
    d_rgb = torch.empty((slots, 3 * N), dtype=torch.uint8, device="cuda")
    d_a = torch.empty((slots, N), dtype=torch.uint8, device="cuda")
    d_ct = torch.empty((slots, 3 * N), dtype=torch.uint8, device="cuda")  # (4096 is a multiple of both tile sizes: the tile rasters hold N pixels)
    d_at = torch.empty((slots, N), dtype=torch.uint8, device="cuda")
    rgba, back, rgb, a, ct, al = ([t[k].data_ptr() for k in range(slots)] for t in (d_rgba, d_back, d_rgb, d_a, d_ct, d_at))
    for tile in TILES:
        T = frave_amd.PlanTiledRgba(ctx, SIZE, SIZE, tile, tile, TILED_ALLOW_HOLES)
        T3 = frave_amd.PlanTiled(ctx, SIZE, SIZE, 3, tile, tile, TILED_ALLOW_HOLES)
        T1 = frave_amd.PlanTiled(ctx, SIZE, SIZE, 1, tile, tile, TILED_ALLOW_HOLES)
        h, h3, h1, hr = T._h, T3._h, T1._h, R._h
        # (the library's entry points called directly with pointers worked out beforehand: a short launch must not wait for the interpreter)

        def split_composed(i):
            k = i % slots
            return L.fri_hip_split_rgba_dev(hr, rgba[k], 0, rgb[k], a[k], sp) | L.fri_hip_split_tiles_dev(h3, rgb[k], ct[k], sp) | L.fri_hip_split_tiles_dev(h1, a[k], al[k], sp)

        def merge_composed(i):
            k = i % slots
            return L.fri_hip_merge_tiles_dev(h3, ct[k], rgb[k], sp) | L.fri_hip_merge_tiles_dev(h1, al[k], a[k], sp) | L.fri_hip_merge_rgba_dev(hr, rgb[k], a[k], back[k], sp)

        groups = {
            "split": {"split_tiles_rgba_kernel (K16)": lambda i: L.fri_hip_split_tiles_rgba_dev(h, rgba[i % slots], 0, ct[i % slots], al[i % slots], sp),
                      "split_rgba_kernel + split_tiles_kernel<3> + <1> (K9, K10)": split_composed},
            "merge": {"merge_tiles_rgba_region_kernel, whole image (K16)": lambda i: L.fri_hip_merge_tiles_rgba_dev(h, ct[i % slots], al[i % slots], back[i % slots], sp),
                      "merge_tiles_kernel<3> + <1> + merge_rgba_kernel (K10, K9)": merge_composed},
        }
        # both routes give the same bytes, once: the tile rasters of slot 0 by K16 against the composition's, and both merges give the raster back
        assert split_composed(0) == 0
        s.synchronize()
        want_ct, want_at = d_ct[0].clone(), d_at[0].clone()
        d_ct[0].zero_(), d_at[0].zero_()
        assert groups["split"]["split_tiles_rgba_kernel (K16)"](0) == 0
        s.synchronize()
        assert torch.equal(d_ct[0], want_ct) and torch.equal(d_at[0], want_at)
        for fn in groups["merge"].values():
            d_back[0].zero_()
            assert fn(0) == 0
            s.synchronize()
            assert torch.equal(d_back[0], d_rgba[0])
        del want_ct, want_at
        for what, fns in groups.items():
            res = {k: [] for k in fns}
            for k, fn in fns.items():
                events(fn, 2 * slots)  # spin-up
            for _ in range(rounds):
                for k, fn in fns.items():
                    events(fn, slots)
                    res[k].append(events(fn, n))
            names = list(fns)
            base = statistics.median(res[names[1]])
            for k, nbytes in zip(names, (8 * N, 16 * N)):
                us = statistics.median(res[k])
                rep.line(f"{what}, {SIZE}x{SIZE} RGBA in {T.n_tiles} tiles of {tile}x{tile}: {k}: {us:.2f} us, {nbytes / 1e6:.1f} MB algorithmic = {nbytes / us / 1e6:.3f} TB/s "
                         f"({100 * nbytes / us * 1e6 / PEAK:.1f} % of 8 TB/s), {us / base:.3f} x the composition's time; rounds " + " ".join(f"{v:.2f}" for v in res[k]))
            lo, hi = min(res[names[1]]), max(res[names[1]])
            fused = statistics.median(res[names[0]])
            rep.line(f"{what}, {tile}x{tile} tiles: the composition's rounds span {lo:.2f} .. {hi:.2f} us ({100 * (hi - lo) / base:.1f} % of their median); K16 is "
                     f"{'not slower than the composition beyond that spread: it stays' if fused <= hi else 'SLOWER than the composition beyond that spread: it loses'}")
        T.close(), T3.close(), T1.close()
    R.close()


def _mixed_rgba(np, size, seed):
    """colour: every plane left half smooth, right half noise (tools/tiled_time.py's plane); alpha: runs of 0 and 255 and a ramp"""
    planes = []
    y, x = np.mgrid[0:size, 0:size]
    for c in range(3):
        rng = np.random.default_rng(seed + c)
        smooth = (((x + 2 * y) >> 3) + rng.integers(0, 8, (size, size))) & 0xFF
        noise = rng.integers(0, 256, (size, size))
        planes.append(np.where(x < size // 2, smooth, noise).astype(np.uint8))
    a = np.zeros((size, size), np.uint8)
    a[:, size // 4: size // 2] = 255
    a[size // 3: 2 * size // 3, : size // 4] = 255
    a[:, size // 2:] = (np.arange(size - size // 2) * 255 // (size - size // 2 - 1)).astype(np.uint8)[None, :]
    return np.ascontiguousarray(np.stack(planes + [a], axis=2))


def _wall(fn, repeats):
    fn()  # warm-up: buffers grown, pages touched
    out, times = None, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, statistics.median(times)


def step_host(rep, n, rounds, repeats):
    import numpy as np

    import frave_amd
    import frave_amd.emit as emit
    from frave_amd.api import COLOUR_YCBCR, DEQUANT_MIDPOINT, TILED_ALLOW_HOLES

    ctx = frave_amd.Context(0)
    rep.line(f"python3 tools/tiled_rgba_time.py host --repeats {repeats} ({SIZE}x{SIZE} RGBA, colour half smooth / half noise, alpha in runs; YCbCr at quality {QUALITY}, fitted "
             f"parameters; host memory to host memory through the Python bindings, output arrays allocated inside the call; time.perf_counter around each synchronous "
             f"call, medians of {repeats} after one warm-up call; {os.cpu_count()} CPUs visible, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', '-')})")
    img = _mixed_rgba(np, SIZE, 7)
    qm = frave_amd.quality_matrix(QUALITY)
    R = frave_amd.PlanRGBA(ctx, SIZE, SIZE)
    R.set_stream_order()
    R.colour.set_colour_transform(COLOUR_YCBCR)
    R.colour.set_dequantiser(DEQUANT_MIDPOINT)
    (sym, vp, wp, hist, oob), t_dev = _wall(lambda: R.encode_image_rgba_symbols(img, qm), repeats)
    assert not oob.any()
    frv, t_emit = _wall(lambda: emit.encode_image_from_streams(SIZE, SIZE, sym, hist, vp, wp, quality=QUALITY, ycbcr=True, alpha=True), repeats)
    d, t_host = _wall(lambda: emit.decode_image(frv), repeats)
    flat, t_inv = _wall(lambda: R.decode_image_rgba(d[4], qm), repeats)
    enc, dec = t_dev + t_emit, t_host + t_inv
    rep.line(f"untiled: file {len(frv)} bytes; encode: fri_hip_encode_image_rgba_symbols {t_dev * 1e3:.1f} ms + fri_emit_encode_image_from_streams {t_emit * 1e3:.1f} ms = "
             f"{enc * 1e3:.1f} ms; decode: fri_emit_decode_image {t_host * 1e3:.1f} ms + fri_hip_decode_image_rgba {t_inv * 1e3:.1f} ms = {dec * 1e3:.1f} ms")
    assert np.array_equal(flat.reshape(SIZE, SIZE, 4)[:, :, 3], img[:, :, 3])
    del sym, hist, d, flat
    R.close()
    for tile in TILES:
        T = frave_amd.PlanTiledRgba(ctx, SIZE, SIZE, tile, tile, TILED_ALLOW_HOLES)
        T.set_stream_order()
        T.colour.set_colour_transform(COLOUR_YCBCR)
        T.colour.set_dequantiser(DEQUANT_MIDPOINT)
        (sym, vp, wp, hist, oob), t_dev = _wall(lambda: T.encode_image_tiled_rgba_symbols(img, qm), repeats)
        assert not oob.any()
        frt, t_emit = _wall(lambda: emit.tiled_encode_from_streams_rgba(SIZE, SIZE, tile, tile, sym, hist, vp, wp, ycbcr=True, quality=QUALITY, threads=16), repeats)
        (ti, coefs), t_host = _wall(lambda: emit.tiled_decode(frt, 16), repeats)
        flat, t_inv = _wall(lambda: T.decode_image_tiled_rgba(coefs, qm), repeats)
        assert ti.alpha and np.array_equal(flat.reshape(SIZE, SIZE, 4)[:, :, 3], img[:, :, 3])
        te, td = t_dev + t_emit, t_host + t_inv
        rep.line(f"{T.n_tiles} tiles of {tile}x{tile}: file {len(frt)} bytes ({len(frt) / len(frv):.4f} x the untiled file); encode: fri_hip_encode_image_tiled_rgba_symbols "
                 f"{t_dev * 1e3:.1f} ms + fri_tiled_encode_from_streams_rgba on 16 threads {t_emit * 1e3:.1f} ms = {te * 1e3:.1f} ms, {enc / te:.2f} x the untiled encode's speed; "
                 f"decode: fri_tiled_decode on 16 threads {t_host * 1e3:.1f} ms + fri_hip_decode_image_tiled_rgba {t_inv * 1e3:.1f} ms = {td * 1e3:.1f} ms, {dec / td:.2f} x the "
                 f"untiled decode's speed")
        del sym, hist, coefs, flat
        T.close()


def main():
    pos, out, n, rounds, repeats = _args()
    steps = {"kernel": step_kernel, "host": step_host}
    if len(pos) != 1 or pos[0] not in steps:
        sys.exit(__doc__)
    steps[pos[0]](Report(out, fresh=pos[0] == "kernel"), n, rounds, repeats)


if __name__ == "__main__":
    main()
