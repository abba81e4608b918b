"""What the device rANS coder (K11, k11_rans.hip) costs against the host coder it replaces, on one box, in one process, in interleaved rounds:

    timeout -k 10 900 python3 tools/rans_time.py [--out profiles/rans_time.txt] [--rounds 3] [--shapes 4096x3x512,4096x3x256,16384x1x512]

Per shape (a square image of C channels in square tiles; half smooth / half noise per tile column, lossless, the fit on), over rotating input slots so that
nothing a route reads still sits in the 256 MB cache from its previous round:

device   K11's three kernels, each between HIP events (fri_hip_rans_time_planes_dev on a slot's device-resident streams and histograms); the whole
         fri_hip_encode_image_tiled_coded call by wall clock (upload, chain, K11, the read-back of the coded planes); fri_tiled_encode_from_coded, the container.
baseline today's route: fri_hip_encode_image_tiled_symbols by wall clock (upload, chain, the read-back of streams and histograms), then
         fri_tiled_encode_from_streams on 16 threads.
Both routes write into host buffers allocated once; the two files are compared; the bytes each route reads back per image are worked out from what it returned.
Also: the share of a plane's symbols in its largest context, which bounds the coder kernel (one sequential chain per context)."""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _args():
    opt = {"--out": os.path.join(ROOT, "profiles", "rans_time.txt"), "--rounds": "3", "--shapes": "4096x3x512,4096x3x256,16384x1x512"}
    a = sys.argv[1:]
    for i in range(0, len(a) - 1, 2):
        opt[a[i]] = a[i + 1]
    return opt["--out"], int(opt["--rounds"]), [tuple(int(v) for v in s.split("x")) for s in opt["--shapes"].split(",")]


def _image(np, size, channels, tile, seed):
    """every tile column half smooth, half noise (tests/tiled_ref.py's mixed image): every tile fills its contexts"""
    rng = np.random.default_rng(seed)
    x = np.arange(size, dtype=np.int32)[None, :, None]
    y = np.arange(size, dtype=np.int32)[:, None, None]
    smooth = (((x + 2 * y) >> 3) + rng.integers(0, 8, (size, size, channels), dtype=np.int32)) & 0xFF
    noise = rng.integers(0, 256, (size, size, channels), dtype=np.int32)
    return np.where(x % tile < tile // 2, smooth, noise).astype(np.uint8)


def main():
    import numpy as np
    import torch

    import frave_amd
    import frave_amd.emit as emit
    from frave_amd import api

    out_path, rounds, shapes = _args()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    log = open(out_path, "w")

    def line(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ctx = frave_amd.Context(0)
    L, E = frave_amd.load_library(), emit.load_library()
    line(f"python3 tools/rans_time.py --rounds {rounds} (one process, interleaved rounds, medians; {os.cpu_count()} CPUs visible, the host coder on 16 threads)")
    ones = np.ones(32, np.int32)
    for size, c, tile in shapes:
        slots = 3 if size <= 4096 else 2
        T = frave_amd.PlanTiled(ctx, size, size, c, tile, tile)
        T.set_stream_order()
        planes, n = T.n_tiles * c, T.num_some
        imgs = [_image(np, size, c, tile, 11 + k).reshape(-1) for k in range(slots)]
        # host buffers of both routes, allocated and touched once
        sym, hist = np.zeros((planes, n), np.uint16), np.zeros((planes, 10, 1024), np.uint32)
        vp, wp, oob = np.zeros((planes, 18), np.float32), np.zeros((planes, 18), np.float32), np.zeros(planes, np.uint64)
        stride = n + 20
        words, n_words = np.zeros((planes, stride), np.uint32), np.zeros(planes, np.uint32)
        models, off, status = np.zeros((planes, 10, 4), np.uint32), np.zeros((planes, 10, 1024), np.uint16), np.zeros((planes, 4), np.uint32)
        file_a, file_b = np.zeros(planes * n * 2 + (1 << 24), np.uint8), np.zeros(planes * n * 2 + (1 << 24), np.uint8)
        len_a, len_b, err = C.c_size_t(0), C.c_size_t(0), C.create_string_buffer(256)
        # device-resident streams and histograms per slot, for the kernels alone
        d_px = [torch.from_numpy(im).cuda() for im in imgs]
        d_sym = torch.zeros((slots, planes * n), dtype=torch.int16, device="cuda")
        d_hist = torch.zeros((slots, planes * 10240), dtype=torch.int32, device="cuda")
        d_par = torch.zeros((slots, planes * 36), dtype=torch.float32, device="cuda")
        d_oob = torch.zeros((slots, 2 * planes), dtype=torch.int64, device="cuda")
        for k in range(slots):
            T.encode_symbols_tiled_dev(d_px[k].data_ptr(), d_par[k].data_ptr(), d_sym[k].data_ptr(), d_hist[k].data_ptr(), d_oob[k].data_ptr(), d_oob[k].data_ptr() + 8 * planes,
                                       qmatrix=ones, fit=True)
        torch.cuda.synchronize()
        d_words = torch.zeros(planes * stride, dtype=torch.int32, device="cuda")
        d_small = torch.zeros(planes * 45, dtype=torch.int32, device="cuda")
        d_off = torch.zeros(planes * 10240, dtype=torch.int16, device="cuda")
        d_scratch = torch.zeros(api.rans_scratch_bytes(planes, n) + 256, dtype=torch.uint8, device="cuda")
        scratch = (d_scratch.data_ptr() + 255) & ~255

        def kernels(k):
            return api.rans_encode_planes_dev(ctx, planes, d_sym[k].data_ptr(), n, n, d_hist[k].data_ptr(), api.RANS_EMPTY_OK, d_words.data_ptr(), stride, d_small.data_ptr(),
                                              d_small.data_ptr() + 20 * planes, d_off.data_ptr(), d_small.data_ptr() + 4 * planes, scratch, 0, timed=True)

        def device_route(k):
            t0 = time.perf_counter()
            rc = L.fri_hip_encode_image_tiled_coded(T._h, P(imgs[k]), P(ones), P(vp), P(wp), P(words), stride, P(n_words), P(models), P(off), P(status))
            t1 = time.perf_counter()
            assert rc == 0 and not status.any(), rc
            rc = E.fri_tiled_encode_from_coded(size, size, tile, tile, c, P(words), stride, P(n_words), P(models), P(off), P(vp), P(wp), 16, P(file_a), file_a.size, C.addressof(len_a),
                                               err, 256)
            t2 = time.perf_counter()
            assert rc == 0, err.value
            return t1 - t0, t2 - t1

        def baseline_route(k):
            t0 = time.perf_counter()
            rc = L.fri_hip_encode_image_tiled_symbols(T._h, P(imgs[k]), P(ones), P(vp), P(wp), P(sym), P(hist), P(oob))
            t1 = time.perf_counter()
            assert rc == 0 and not oob.any(), rc
            rc = E.fri_tiled_encode_from_streams(size, size, tile, tile, c, P(sym), n, P(hist), P(vp), P(wp), 16, P(file_b), file_b.size, C.addressof(len_b), err, 256)
            t2 = time.perf_counter()
            assert rc == 0, err.value
            return t1 - t0, t2 - t1

        kernels(0), device_route(0), baseline_route(0)  # spin-up: every buffer the routes grow exists, every page is touched
        assert len_a.value == len_b.value and np.array_equal(file_a[: len_a.value], file_b[: len_b.value]), "the two routes' files differ"
        res = {"model": [], "coder": [], "stitch": [], "coded call": [], "assembly": [], "symbols call": [], "host coder": []}
        for r in range(rounds):
            k = (r + 1) % slots
            us = kernels(k)
            for name, v in zip(("model", "coder", "stitch"), us):
                res[name].append(v / 1e3)
            a, b = device_route(k)
            res["coded call"].append(a * 1e3), res["assembly"].append(b * 1e3)
            a, b = baseline_route(k)
            res["symbols call"].append(a * 1e3), res["host coder"].append(b * 1e3)
            assert np.array_equal(file_a[: len_a.value], file_b[: len_b.value])
        m = {k: statistics.median(v) for k, v in res.items()}
        # bytes each route reads back per image (fri_hip.cpp): streams, histograms, parameters and counts / the coded rows up to the longest, the lists up to the longest, the counts
        back_base = planes * (n * 2 + 10240 * 4 + 36 * 4 + 16)
        back_dev = planes * (int(n_words.max()) * 4 + 10 * int(models[:, :, 1].max()) * 2 + 45 * 4 + 36 * 4 + 16)
        share = (hist.sum(axis=2).max(axis=1) / hist.sum(axis=(1, 2))).astype(np.float64)  # per plane: its largest context
        line(f"{size}x{size}x{c} in {T.n_tiles} tiles of {tile}x{tile}: {planes} planes of {n} symbols, {planes * 10} chains; file {len_a.value} bytes, identical on both routes")
        line(f"  K11 kernels (events): model {m['model']:.3f} ms, coder {m['coder']:.3f} ms, stitch {m['stitch']:.3f} ms; rounds coder " + " ".join(f"{v:.3f}" for v in res["coder"]))
        line(f"  device route: fri_hip_encode_image_tiled_coded {m['coded call']:.1f} ms + fri_tiled_encode_from_coded {m['assembly']:.1f} ms = {m['coded call'] + m['assembly']:.1f} ms; "
             f"read back {back_dev / 1e6:.1f} MB")
        line(f"  baseline:     fri_hip_encode_image_tiled_symbols {m['symbols call']:.1f} ms + fri_tiled_encode_from_streams on 16 threads {m['host coder']:.1f} ms = "
             f"{m['symbols call'] + m['host coder']:.1f} ms; read back {back_base / 1e6:.1f} MB")
        line(f"  largest context's share of a plane's symbols: median {100 * statistics.median(share):.1f} %, largest {100 * share.max():.1f} % "
             f"= a chain of {int(hist.sum(axis=2).max())} steps; the coder kernel's {m['coder']:.3f} ms are {1e6 * m['coder'] / max(1, int(hist.sum(axis=2).max())):.1f} ns per step of it")
        del d_px, d_sym, d_hist, d_par, d_oob, d_words, d_small, d_off, d_scratch
        torch.cuda.empty_cache()
        T.close()
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
