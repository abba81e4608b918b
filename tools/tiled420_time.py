"""What tiled 4:2:0 coding (K12, fri_hip_*_tiled420*, fri_tiled_encode_from_streams420) costs, on one MI355X in one process:

    timeout -k 10 900 python3 tools/tiled420_time.py [--out profiles/tiled420_time.txt] [--launches 40] [--rounds 5]

The image is 4096^2 RGB, every plane half smooth and half noise as in tools/tiled_time.py and tools/region_time.py: synthetic content - natural photographs are
not measured here.

split:   K12's fused split_tiles420_kernel against the only route the library offered before it: fri_hip_split_tiles_dev (K10), then one fri_hip_split420_dev (K8)
         per tile - 1 + n launches. 512^2 and 256^2 tiles. Events around `launches` back-to-back runs of each route, medians of interleaved rounds; every run
         reads and writes another of `slots` rotating buffer sets that together exceed the 256 MB cache. The two routes' planes are compared once.
merge:   merge_tiles420_region_kernel on the whole image and on a 1024^2 region (tile-aligned, and at (300, 300)), the same way.
end to end (wall clock, medians of 3, quality 60): pixels -> file and file -> pixels for tiled 4:2:0, tiled 4:4:4 YCbCr (512^2 tiles both) and untiled 4:2:0;
         the emitter and the host decoder on 16 threads where they take threads; file sizes and the R, G, B PSNR of each; and a 1024^2 region decode of the
         tiled 4:2:0 file against its whole decode."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZE, QUALITY = 4096, 60
REGIONS = [("tile-aligned 1024x1024", (1024, 1024, 1024, 1024)), ("1024x1024 at (300, 300)", (300, 300, 1024, 1024))]


def _args():
    a = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "tiled420_time.txt"), "--launches": "40", "--rounds": "5"}
    for i in range(0, len(a) - 1, 2):
        if a[i] in opt:
            opt[a[i]] = a[i + 1]
    return opt["--out"], int(opt["--launches"]), int(opt["--rounds"])


class Report:
    def __init__(self, path):
        self.path = path
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if os.path.exists(path):
            os.remove(path)

    def line(self, text):
        print(text, flush=True)
        with open(self.path, "a") as f:
            f.write(text + "\n")


def _mixed_image(np, size, seed):
    """every plane: left half smooth, right half noise (tools/tiled_time.py's plane)"""
    planes = []
    for c in range(3):
        rng = np.random.default_rng(seed + c)
        y, x = np.mgrid[0:size, 0:size]
        smooth = (((x + 2 * y) >> 3) + rng.integers(0, 8, (size, size))) & 0xFF
        noise = rng.integers(0, 256, (size, size))
        planes.append(np.where(x < size // 2, smooth, noise).astype(np.uint8))
    return np.ascontiguousarray(np.stack(planes, axis=2))


def _psnr(np, a, b):
    sse = float(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())
    return float("inf") if sse == 0 else 10 * np.log10(255.0 ** 2 * a.size / sse)


def _wall(fn, repeats=3):
    out, times = None, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, statistics.median(times)


def step_kernels(rep, ctx, n, rounds):
    import torch

    import frave_amd

    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    L = frave_amd.load_library()
    at = [0]

    def events(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for i in range(at[0], at[0] + launches):
            fn(i)
        e1.record(s)
        e1.synchronize()
        at[0] += launches
        return e0.elapsed_time(e1) * 1e3 / launches

    def measure(fns):
        res = {k: [] for k in fns}
        for fn in fns.values():
            events(fn, 4)  # spin-up
        for _ in range(rounds):
            for k, fn in fns.items():
                events(fn, 2)
                res[k].append(events(fn, n))
        return res

    slots = 8
    nbytes = SIZE * SIZE * 3
    d_img = torch.randint(0, 256, (slots, nbytes), dtype=torch.uint8, device="cuda")
    img = [d_img[k].data_ptr() for k in range(slots)]
    rep.line(f"python3 tools/tiled420_time.py --launches {n} --rounds {rounds} (one process; kernels: medians of {rounds} interleaved rounds, us per run, back to back, "
             f"{slots} rotating buffer sets of {nbytes / 1e6:.0f} MB of pixels each)")
    for tile in (512, 256):
        T = frave_amd.PlanTiled420(ctx, SIZE, SIZE, tile, tile, frave_amd.TILED_ALLOW_HOLES)
        K10 = frave_amd.PlanTiled(ctx, SIZE, SIZE, 3, tile, tile, frave_amd.TILED_ALLOW_HOLES)
        K8 = frave_amd.Plan420(ctx, tile, tile)
        nt, yb, cb = T.n_tiles, tile * tile, 2 * T.cw * T.ch
        d_y, d_c = (torch.zeros((slots, nt * b), dtype=torch.uint8, device="cuda") for b in (yb, cb))
        d_y2, d_c2 = torch.zeros_like(d_y), torch.zeros_like(d_c)
        d_tiles = torch.zeros((slots, nt * tile * tile * 3), dtype=torch.uint8, device="cuda")
        y, c, y2, c2, tl = ([t[k].data_ptr() for k in range(slots)] for t in (d_y, d_c, d_y2, d_c2, d_tiles))
        h12, h10, h8 = T._h, K10._h, K8._h

        def fused(i):
            k = i % slots
            return L.fri_hip_split_tiles420_dev(h12, img[k], y[k], c[k], sp)

        def parent(i):
            k = i % slots
            rc = L.fri_hip_split_tiles_dev(h10, img[k], tl[k], sp)
            for t in range(nt):
                rc |= L.fri_hip_split420_dev(h8, tl[k] + t * 3 * yb, y2[k] + t * yb, c2[k] + t * cb, sp)
            return rc

        assert fused(0) == 0 and parent(0) == 0
        s.synchronize()
        assert torch.equal(d_y[0], d_y2[0]) and torch.equal(d_c[0], d_c2[0]), "the two routes write the same planes"
        res = measure({"fused": fused, "parent": parent})
        f, p = statistics.median(res["fused"]), statistics.median(res["parent"])
        moved = nbytes + nt * (yb + cb)  # the pixels in, the planes out (the parent route also writes and reads the tile raster)
        rep.line(f"split, {SIZE}x{SIZE} RGB in {nt} tiles of {tile}x{tile}: fused split_tiles420_kernel {f:.1f} us ({moved / f / 1e6:.2f} TB/s of its {moved / 1e6:.0f} MB); "
                 f"split_tiles + {nt} x split420 ({nt + 1} launches) {p:.1f} us; fused is {p / f:.2f} x faster; rounds fused " + " ".join(f"{v:.1f}" for v in res["fused"])
                 + "; parent " + " ".join(f"{v:.1f}" for v in res["parent"]))
        if tile == 512:
            d_out = torch.zeros((slots, nbytes), dtype=torch.uint8, device="cuda")
            out = [d_out[k].data_ptr() for k in range(slots)]
            fns = {"whole image": lambda i: L.fri_hip_merge_tiles420_dev(h12, y[i % slots], c[i % slots], out[i % slots], sp)}
            moved = {"whole image": nbytes + nt * (yb + cb)}
            for name, (rx, ry, rw, rh) in REGIONS:
                i0, j0, ni, nj = T.region_tiles(rx, ry, rw, rh)
                sub = ni * nj
                # (any ni nj consecutive tiles of a slot serve as the sub-grid's planes: the kernel's work does not depend on what they hold)
                fns[name] = (lambda i, r=(rx, ry, rw, rh), sub=sub: L.fri_hip_merge_tiles420_region_dev(
                    h12, y[i % slots] + (i // slots % (nt // sub)) * sub * yb, c[i % slots] + (i // slots % (nt // sub)) * sub * cb, *r, out[i % slots], sp))
                moved[name] = rw * rh * 3 + rw * rh * 3 // 2
            for k, fn in fns.items():
                assert fn(0) == 0, k
            res = measure(fns)
            whole = statistics.median(res["whole image"])
            for k in fns:
                us = statistics.median(res[k])
                rep.line(f"merge_tiles420_region_kernel, {k}: {us:.2f} us, {moved[k] / 1e6:.2f} MB algorithmic = {moved[k] / us / 1e6:.3f} TB/s, {us / whole:.3f} x the whole "
                         "merge; rounds " + " ".join(f"{v:.2f}" for v in res[k]))
            del d_out
        del d_y, d_c, d_y2, d_c2, d_tiles
        torch.cuda.empty_cache()
        T.close(), K10.close(), K8.close()
    del d_img
    torch.cuda.empty_cache()


def step_end_to_end(rep, ctx):
    import numpy as np

    import frave_amd
    import frave_amd.emit as emit

    img = _mixed_image(np, SIZE, 7)
    qm = frave_amd.quality_matrix(QUALITY)
    tile = 512
    rep.line(f"end to end, {SIZE}x{SIZE} RGB, every plane half smooth / half noise (synthetic: natural photographs are not measured), quality {QUALITY}; wall clock, "
             f"medians of 3; host coder and decoder on 16 threads where they take threads; {os.cpu_count()} CPUs visible")
    # tiled 4:2:0
    T = frave_amd.PlanTiled420(ctx, SIZE, SIZE, tile, tile)
    T.set_stream_order()

    def enc_t420():
        sym, vp, wp, hist, oob = T.encode_image_tiled420_symbols(img, QUALITY)
        return emit.tiled_encode_from_streams420(SIZE, SIZE, tile, tile, sym, T.n_luma, T.n_chroma, hist, vp, wp, QUALITY, threads=16)

    def dec_t420(frv):
        return T.decode_image_tiled420(emit.tiled_decode(frv, 16)[1], QUALITY)

    f_t420, t_e = _wall(enc_t420)
    px, t_d = _wall(lambda: dec_t420(f_t420))
    rep.line(f"tiled 4:2:0 ({T.n_tiles} tiles of {tile}x{tile}): file {len(f_t420)} bytes; encode (pixels to file) {t_e * 1e3:.0f} ms; decode (file to pixels) {t_d * 1e3:.0f} ms; "
             f"PSNR {_psnr(np, px, img.reshape(-1)):.2f} dB")
    whole = px.reshape(SIZE, SIZE, 3)
    for name, (x, y, w, h) in REGIONS:
        got, t_r = _wall(lambda: T.decode_region_tiled420(emit.tiled_decode_region(f_t420, x, y, w, h, 16)[2], QUALITY, x, y, w, h))
        assert np.array_equal(got.reshape(h, w, 3), whole[y:y + h, x:x + w]), name
        rep.line(f"tiled 4:2:0, region {name}: {t_r * 1e3:.1f} ms, {t_d / t_r:.1f} x faster than the whole decode; the raster is the crop")
    T.close()
    # tiled 4:4:4 YCbCr at the same quality
    P = frave_amd.PlanTiled(ctx, SIZE, SIZE, 3, tile, tile)
    P.set_stream_order()
    P.tile.set_colour_transform(frave_amd.api.COLOUR_YCBCR)
    P.tile.set_dequantiser(frave_amd.api.DEQUANT_MIDPOINT)

    def enc_t444():
        sym, vp, wp, hist, oob = P.encode_image_tiled_symbols(img, qm)
        return emit.tiled_encode_from_streams(SIZE, SIZE, tile, tile, sym, hist, vp, wp, ycbcr=True, quality=QUALITY, threads=16)

    f_t444, t_e = _wall(enc_t444)
    px, t_d = _wall(lambda: P.decode_image_tiled(emit.tiled_decode(f_t444, 16)[1], qm))
    rep.line(f"tiled 4:4:4 YCbCr ({P.n_tiles} tiles of {tile}x{tile}): file {len(f_t444)} bytes; encode {t_e * 1e3:.0f} ms; decode {t_d * 1e3:.0f} ms; "
             f"PSNR {_psnr(np, px, img.reshape(-1)):.2f} dB")
    P.close()
    # untiled 4:2:0
    U = frave_amd.Plan420(ctx, SIZE, SIZE)
    U.set_stream_order()

    def enc_u420():
        sym, vp, wp, hist, oob = U.encode_image420_symbols(img, QUALITY)
        return emit.encode_image_from_streams(SIZE, SIZE, sym, hist, vp, wp, quality=QUALITY, ycbcr=True, n_luma=U.luma.num_some)

    f_u420, t_e = _wall(enc_u420)
    px, t_d = _wall(lambda: U.decode_image420(np.concatenate([p.reshape(-1) for p in emit.decode_image(f_u420)[4]]), QUALITY))
    rep.line(f"untiled 4:2:0: file {len(f_u420)} bytes; encode {t_e * 1e3:.0f} ms; decode {t_d * 1e3:.0f} ms; PSNR {_psnr(np, px, img.reshape(-1)):.2f} dB")
    U.close()


def main():
    import frave_amd

    out, n, rounds = _args()
    rep = Report(out)
    ctx = frave_amd.Context(0)
    step_kernels(rep, ctx, n, rounds)
    step_end_to_end(rep, ctx)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
