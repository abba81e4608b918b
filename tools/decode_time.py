"""What decoding a tiled file costs with the entropy decoder on the host (the existing route) and on the device (K13, k13_decode.hip), from the same file bytes.
One process; each shape appends its section to the report:

    timeout -k 10 900 python3 tools/decode_time.py [rgb512 rgb256 plane16k rgb512_420]

rgb512      a 4096^2 RGB image in 512^2 tiles (192 planes), lossless
rgb256      the same image in 256^2 tiles (768 planes), lossless
plane16k    a 16384^2 plane in 512^2 tiles (1024 planes), lossless
rgb512_420  the tiled 4:2:0 form of the first at quality 50 (64 luma planes on the 512^2 lattice, 128 chroma planes on the 256^2 lattice)

Every image is half smooth, half noise per tile column (tests/test_emit.py's image, per channel). The file is written by the device coder (K11) and the host
container. Per file, wall clock around calls that end synchronised, one warm-up and the median of `--repeats`:

existing route   fri_tiled_decode on 16 threads, then fri_hip_decode_image_tiled[420] (upload of the int32 planes, inverse kernel, merge, download)
new route        fri_tiled_parse_coded (the Python binding: size queries and the copy), then fri_hip_decode_image_tiled[420]_coded (upload of the coded planes, K13,
                 inverse kernel, merge, download)
K13 alone        fri_hip_decode_time_planes_dev on device-resident planes: the model and the decode kernel between events, and the decode kernel's time per step of
                 a plane (every plane of a lattice has the same number of steps)

and the bytes each route uploads. The two routes' pixels are compared.

usage: python3 tools/decode_time.py [shape ...] [--out profiles/rans_decode_time.txt] [--repeats 3]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THREADS = 16


def _args():
    a = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "rans_decode_time.txt"), "--repeats": "3"}
    pos, i = [], 0
    while i < len(a):
        if a[i] in opt:
            opt[a[i]] = a[i + 1]
            i += 2
        else:
            pos.append(a[i])
            i += 1
    return pos, opt["--out"], int(opt["--repeats"])


class Report:
    def __init__(self, path):
        self.path = path
        os.makedirs(os.path.dirname(path), exist_ok=True)

    def line(self, text):
        print(text, flush=True)
        with open(self.path, "a") as f:
            f.write(text + "\n")


def _mixed(np, size, channels, tile, seed):
    """smooth where x % tile < tile / 2 and noise elsewhere, per channel: every tile gets both"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:size, 0:size]
    planes = []
    for c in range(channels):
        smooth = (((x + 2 * y) >> 3) + 40 * c + rng.integers(0, 8, (size, size))) & 0xFF
        noise = rng.integers(0, 256, (size, size))
        planes.append(np.where((x % tile) < tile // 2, smooth, noise).astype(np.uint8))
    return np.ascontiguousarray(np.stack(planes, axis=2))


def _wall(fn, repeats):
    fn()  # warm-up: buffers grown, code objects loaded, pages touched
    out, times = None, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, statistics.median(times), times


def _coded_upload_bytes(np, coded):
    """what fri_hip_decode_image_tiled[420]_coded copies to the device: every row to the longest plane, every list to the longest list"""
    words, n_words, models, off, vp, wp = coded[-6:]
    planes = n_words.size
    longest = max(1, int(np.minimum(n_words, words.shape[1]).max()))
    most_off = int(np.minimum(models[:, :, 1], 1024).max())
    return planes * (4 * longest + 4 + 160 + 10 * 2 * most_off + 144)


def _k13_alone(np, torch, api, plan, coded, first, count, repeats):
    """(model us, decode us) medians of fri_hip_decode_time_planes_dev over the planes first .. first + count - 1 on device-resident arrays; the status must be 0"""
    words, n_words, models, off, vp, wp = (np.ascontiguousarray(a[first : first + count]) for a in coded[-6:])

    def dev(a):
        return torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).cuda()

    d = [dev(a) for a in (words, n_words, models, off, vp, wp)]
    F = plan.num_cells
    d_coefs = torch.empty(count * F * 512, dtype=torch.int32, device="cuda")
    d_status = torch.empty(count * 4, dtype=torch.int32, device="cuda")
    d_scratch = torch.empty(api.decode_scratch_bytes(count) + 256, dtype=torch.uint8, device="cuda")
    scratch = (d_scratch.data_ptr() + 255) & ~255
    runs = []
    for _ in range(repeats + 1):
        runs.append(api.decode_planes_dev(plan, count, d[0].data_ptr(), words.shape[1], d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(),
                                          d_coefs.data_ptr(), F * 512, d_status.data_ptr(), scratch, torch.cuda.current_stream().cuda_stream, timed=True))
    assert not d_status.cpu().numpy().any()
    runs = runs[1:]
    return statistics.median(r[0] for r in runs), statistics.median(r[1] for r in runs)


def measure(rep, name, repeats):
    import numpy as np
    import torch

    import frave_amd
    import frave_amd.api as api
    import frave_amd.emit as emit

    size, channels, tile, s420 = {"rgb512": (4096, 3, 512, False), "rgb256": (4096, 3, 256, False), "plane16k": (16384, 1, 512, False), "rgb512_420": (4096, 3, 512, True)}[name]
    ctx = frave_amd.Context(0)
    img = _mixed(np, size, channels, tile, 7)
    quality = 50 if s420 else 0
    if s420:
        tw, th = api.tile_shape420(size, size, tile)
        T = frave_amd.PlanTiled420(ctx, size, size, tw, th)
        T.set_stream_order()
        words, n_words, models, off, status, vp, wp = T.encode_image_tiled420_coded(img, quality, word_stride=max(T.n_luma, T.n_chroma) // 2 + 20)
        assert not status.any()
        frv = emit.tiled_encode_from_coded420(size, size, tw, th, words, n_words, models, off, vp, wp, quality)
        lattices = [("luma", T.luma, 0, T.n_tiles), ("chroma", T.chroma, T.n_tiles, 2 * T.n_tiles)]
        old_dev, new_dev = (lambda coefs: T.decode_image_tiled420(coefs, quality)), (lambda coded: T.decode_coded(coded, quality)[0])
    else:
        tw, th = api.tile_shape(size, size, tile)
        T = frave_amd.PlanTiled(ctx, size, size, channels, tw, th)
        T.set_stream_order()
        words, n_words, models, off, status, vp, wp = T.encode_image_tiled_coded(img, word_stride=T.num_some // 2 + 20)
        assert not status.any()
        frv = emit.tiled_encode_from_coded(size, size, tw, th, words, n_words, models, off, vp, wp)
        lattices = [("tile", T.tile, 0, T.n_tiles * channels)]
        old_dev, new_dev = (lambda coefs: T.decode_image_tiled(coefs)), (lambda coded: T.decode_coded(coded)[0])
    del words, off
    planes = n_words.size
    rep.line(f"{name}: {size}x{size}x{channels} in {T.n_tiles} tiles of {tw}x{th}{' 4:2:0, quality 50' if s420 else ', lossless'}: {planes} planes, file {len(frv)} bytes, "
             f"longest plane {int(n_words.max())} words; wall clock, 1 warm-up + median of {repeats}; {os.cpu_count()} CPUs visible")
    (ti, coefs), t_host, _ = _wall(lambda: emit.tiled_decode(frv, THREADS), repeats)
    old_px, t_old_dev, _ = _wall(lambda: old_dev(coefs), repeats)
    coded, t_parse, _ = _wall(lambda: emit.tiled_parse_coded(frv), repeats)
    new_px, t_new_dev, _ = _wall(lambda: new_dev(coded), repeats)
    assert np.array_equal(old_px, new_px), "the two routes' pixels differ"
    if not s420:
        assert np.array_equal(new_px, img.reshape(-1)), "the lossless file does not decode to the image"
    up_old, up_new = coefs.nbytes, _coded_upload_bytes(np, coded)
    rep.line(f"  existing route: fri_tiled_decode on {THREADS} threads {t_host * 1e3:.1f} ms + fri_hip_decode_image_tiled{'420' if s420 else ''} {t_old_dev * 1e3:.1f} ms = "
             f"{(t_host + t_old_dev) * 1e3:.1f} ms; uploads {up_old / 1e6:.1f} MB")
    rep.line(f"  new route:      fri_tiled_parse_coded {t_parse * 1e3:.1f} ms + fri_hip_decode_image_tiled{'420' if s420 else ''}_coded {t_new_dev * 1e3:.1f} ms = "
             f"{(t_parse + t_new_dev) * 1e3:.1f} ms; uploads {up_new / 1e6:.1f} MB ({up_old / up_new:.1f} x fewer bytes); new / existing "
             f"{(t_parse + t_new_dev) / (t_host + t_old_dev):.2f}; same pixels")
    del coefs
    for label, plan, first, count in lattices:
        model_us, decode_us = _k13_alone(np, torch, api, plan, coded, first, count, repeats)
        rep.line(f"  K13 alone, {label} lattice: {count} planes of {plan.num_some} steps: model kernel {model_us:.1f} us, decode kernel {decode_us / 1e3:.2f} ms = "
                 f"{1e3 * decode_us / plan.num_some:.0f} ns per step of a plane ({1e3 * decode_us / (plan.num_some * count):.2f} ns per symbol of the batch)")
    T.close()
    ctx.close()


def main():
    pos, out, repeats = _args()
    shapes = pos or ["rgb512", "rgb256", "plane16k", "rgb512_420"]
    rep = Report(out)
    rep.line("python3 tools/decode_time.py " + " ".join(shapes) + f" --repeats {repeats}")
    for name in shapes:
        measure(rep, name, repeats)
    return 0


if __name__ == "__main__":
    sys.exit(main())
