"""What a thumbnail of a tiled file costs through the preview decode (fri_tiled_decode_levels, K13 bounded by a level, K14: k14_preview.hip) against the full
decode the parent needs for the same thumbnail, from the same file bytes. One process; each shape appends its section to the report:

    timeout -k 10 900 python3 tools/preview_time.py [rgb512 rgb256]

rgb512   a 4096^2 RGB image in 512^2 tiles (192 planes), lossless
rgb256   the same image in 256^2 tiles (768 planes), lossless

Every image is half smooth, half noise per tile column (tools/decode_time.py's image). The file is written by the device coder (K11) and the host container. Per
file and per M = 1..4 (thumbnail of ceil(4096 / 2^M)^2, L = 9 - 2 M), wall clock around calls that end synchronised, one warm-up and the median of `--repeats`:

host route    fri_tiled_decode_levels on 16 threads, then fri_hip_preview_image_tiled (upload of the compact planes, K14, download)
device route  fri_tiled_parse_coded once per file (the Python binding: size queries and the copy; timed once, it does not depend on M), then
              fri_hip_preview_image_tiled_coded (upload of the coded planes, K13 bounded by L, K14, download)
baseline      what the same thumbnail costs without the preview decode: fri_tiled_decode on 16 threads, fri_hip_decode_image_tiled (upload of the int32 planes,
              inverse kernel, merge, download), then the subsample of the definition on the host (numpy)

and, on device-resident planes between events: K14 alone at each (L, M), the inverse kernel plus the merge (the full-size route K14's M = 0 does not replace), and the
steps per plane at each L (fri_hip_plan_num_some_levels). The three routes' thumbnails are compared.

usage: python3 tools/preview_time.py [shape ...] [--out profiles/preview_time.txt] [--repeats 3]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from decode_time import THREADS, Report, _mixed, _wall  # noqa: E402


def _args():
    a = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "preview_time.txt"), "--repeats": "3"}
    pos, i = [], 0
    while i < len(a):
        if a[i] in opt:
            opt[a[i]] = a[i + 1]
            i += 2
        else:
            pos.append(a[i])
            i += 1
    return pos, opt["--out"], int(opt["--repeats"])


def _subsample(np, image, shift):
    h, w = image.shape[:2]
    s = 1 << shift
    rows = np.minimum(np.arange(-(-h // s)) * s + s // 2, h - 1)
    cols = np.minimum(np.arange(-(-w // s)) * s + s // 2, w - 1)
    return np.ascontiguousarray(image[rows][:, cols])


def _events_us(torch, fn, repeats):
    """median microseconds of fn() between two events on the current stream, after one warm-up"""
    fn()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(1e3 * e0.elapsed_time(e1))
    return statistics.median(times)


def measure(rep, name, repeats):
    import numpy as np
    import torch

    import frave_amd
    import frave_amd.api as api
    import frave_amd.emit as emit

    size, channels, tile = {"rgb512": (4096, 3, 512), "rgb256": (4096, 3, 256)}[name]
    ctx = frave_amd.Context(0)
    img = _mixed(np, size, channels, tile, 7)
    tw, th = api.tile_shape(size, size, tile)
    T = frave_amd.PlanTiled(ctx, size, size, channels, tw, th)
    T.set_stream_order()
    words, n_words, models, off, status, vp, wp = T.encode_image_tiled_coded(img, word_stride=T.num_some // 2 + 20)
    assert not status.any()
    frv = emit.tiled_encode_from_coded(size, size, tw, th, words, n_words, models, off, vp, wp)
    del words, off
    F = T.num_cells
    steps = [T.tile.num_some_levels(levels) for levels in range(10)]
    rep.line(f"{name}: {size}x{size}x{channels} in {T.n_tiles} tiles of {tw}x{th}, lossless: {n_words.size} planes of {F} cells, file {len(frv)} bytes; wall clock, 1 warm-up + "
             f"median of {repeats}; {os.cpu_count()} CPUs visible")
    rep.line("  steps per plane at L = 0..9: " + " ".join(str(n) for n in steps) + f" (L = 7, 5, 3, 1: {steps[7] / steps[9]:.3f}, {steps[5] / steps[9]:.3f}, {steps[3] / steps[9]:.4f}, "
             f"{steps[1] / steps[9]:.4f} of the whole plane)")
    (ti, full), t_full, _ = _wall(lambda: emit.tiled_decode(frv, THREADS), repeats)
    full_px, t_full_dev, _ = _wall(lambda: T.decode_image_tiled(full), repeats)
    assert np.array_equal(full_px, img.reshape(-1)), "the lossless file does not decode to the image"
    image = full_px.reshape(size, size, channels)
    coded, t_parse, _ = _wall(lambda: emit.tiled_parse_coded(frv), repeats)
    rep.line(f"  full decode: fri_tiled_decode on {THREADS} threads {t_full * 1e3:.1f} ms + fri_hip_decode_image_tiled {t_full_dev * 1e3:.1f} ms (uploads {full.nbytes / 1e6:.1f} MB); "
             f"fri_tiled_parse_coded {t_parse * 1e3:.1f} ms")
    d_full = torch.from_numpy(full.reshape(-1)).cuda()
    d_tiles = torch.empty(T.tile_bytes, dtype=torch.uint8, device="cuda")
    d_raster = torch.empty(T.pixel_bytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    image_coefs = channels * F * 512

    def k3_merge():
        T.tile.inverse_transform_batch_dev(T.n_tiles, d_full.data_ptr(), image_coefs, d_tiles.data_ptr(), tw * th * channels, stream=stream)
        T.merge_tiles_dev(d_tiles.data_ptr(), d_raster.data_ptr(), stream)

    us_k3 = _events_us(torch, k3_merge, repeats)
    rep.line(f"  the inverse kernel + the merge on device-resident planes: {us_k3:.1f} us")
    for m in (1, 2, 3, 4):
        levels = 9 - 2 * m
        want, t_sub, _ = _wall(lambda: _subsample(np, image, m), repeats)
        (_, compact), t_host, _ = _wall(lambda: emit.tiled_decode_levels(frv, levels, THREADS), repeats)
        host_px, t_host_dev, _ = _wall(lambda: T.preview(compact, levels, m), repeats)
        (dev_px, st), t_dev, _ = _wall(lambda: T.preview_coded(coded, levels, m), repeats)
        assert not st.any() and np.array_equal(host_px, dev_px), "the two routes' thumbnails differ"
        definition = _subsample(np, T.decode_image_tiled(np.where((np.arange(512) < (1 << levels)) | (full == -(2 ** 31)), full, 0)).reshape(size, size, channels), m)
        assert np.array_equal(host_px, definition), "the thumbnail is not the definition's"
        w, h = api.preview_size(size, size, m)
        d_out = torch.empty(w * h * channels + 3, dtype=torch.uint8, device="cuda")
        us_full = _events_us(torch, lambda: T.preview_tiles_dev(d_full.data_ptr(), F * 512, 512, levels, m, d_out.data_ptr(), stream=stream), repeats)
        d_compact = torch.from_numpy(compact.reshape(-1)).cuda()
        us_compact = _events_us(torch, lambda: T.preview_tiles_dev(d_compact.data_ptr(), F << levels, 1 << levels, levels, m, d_out.data_ptr(), stream=stream), repeats)
        base = t_full + t_full_dev + t_sub
        rep.line(f"  M = {m} (L = {levels}, {w}x{h}): host route fri_tiled_decode_levels {t_host * 1e3:.1f} ms + fri_hip_preview_image_tiled {t_host_dev * 1e3:.2f} ms = "
                 f"{(t_host + t_host_dev) * 1e3:.1f} ms (uploads {compact.nbytes / 1e6:.2f} MB); device route parse {t_parse * 1e3:.1f} ms + fri_hip_preview_image_tiled_coded "
                 f"{t_dev * 1e3:.1f} ms = {(t_parse + t_dev) * 1e3:.1f} ms; baseline {t_full * 1e3:.1f} + {t_full_dev * 1e3:.1f} + subsample {t_sub * 1e3:.2f} ms = {base * 1e3:.1f} ms; "
                 f"host route {base / (t_host + t_host_dev):.1f} x, device route {base / (t_parse + t_dev):.1f} x the baseline's speed; same thumbnail, and the definition's")
        rep.line(f"           K14 alone: {us_full:.1f} us on full-stride planes, {us_compact:.1f} us on compact planes (the inverse kernel + the merge: {us_k3:.1f} us)")
        del d_compact, d_out
    us_m0 = _events_us(torch, lambda: T.preview_tiles_dev(d_full.data_ptr(), F * 512, 512, 9, 0, d_raster.data_ptr(), stream=stream), repeats)
    assert np.array_equal(d_raster.cpu().numpy(), img.reshape(-1))
    rep.line(f"  M = 0, L = 9 (the definition's full-size case, not a route): K14 {us_m0:.1f} us against {us_k3:.1f} us of the inverse kernel + the merge; the image")
    T.close()
    ctx.close()


def main():
    pos, out, repeats = _args()
    shapes = pos or ["rgb512", "rgb256"]
    rep = Report(out)
    rep.line("python3 tools/preview_time.py " + " ".join(shapes) + f" --repeats {repeats}")
    for name in shapes:
        measure(rep, name, repeats)
    return 0


if __name__ == "__main__":
    sys.exit(main())
