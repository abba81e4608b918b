"""What 4:2:0 chroma subsampling (fri_hip_plan420, K8: k8_chroma420.hip) costs and gives. Three steps, each a process of its own that appends its section to the
report; run them under a time limit each and chained, so that trouble in one ends the run:

    timeout -k 10 600 python3 tools/chroma420_time.py kernels && timeout -k 10 900 python3 tools/chroma420_time.py paths PARENT_LIB && \\
    timeout -k 10 600 python3 tools/chroma420_time.py table

kernels: the split, the merge and the measuring merge at 4096^2 and 16384^2 over rotating HBM-resident slots (more bytes than the 256 MB cache), timed with
         events around `launches` launches; next to each a device-to-device hipMemcpyAsync that moves the same total bytes (it copies half of them: every byte
         is read once and written once). Medians of five interleaved rounds; algorithmic bytes and their fraction of 8 TB/s.
paths:   the 4:2:0 forward path (split + K1 on Y + K1 on Cb, Cr) and inverse path (K3 on Y + K3 on Cb, Cr + merge) at 4096^2 RGB against the 4:4:4 YCbCr K1 and
         K3 of PARENT_LIB (a build of the parent commit's library, loaded through FRI_HIP_LIBRARY): one child process per library and round, alternating, each
         replaying a captured graph of its launches over the slots. Medians of five rounds.
table:   bits per pixel / PSNR in R, G, B against quality for three 1024 x 768 images, 4:4:4 YCbCr and 4:2:0 rows.

usage: python3 tools/chroma420_time.py kernels|paths|table [PARENT_LIB] [--out profiles/chroma420_time.txt] [--launches 200] [--rounds 5]"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12  # bytes per second
RELAXED = 2  # hipStreamCaptureModeRelaxed


def _args():
    a = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "chroma420_time.txt"), "--launches": "200", "--rounds": "5"}
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


def step_kernels(rep, n, rounds):
    import torch

    import frave_amd

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    ctx = frave_amd.Context(0)
    s = torch.cuda.current_stream()
    rep.line(f"python3 tools/chroma420_time.py kernels --launches {n} --rounds {rounds} (one process; medians of {rounds} interleaved rounds, us per launch)")
    for size, slots in ((4096, 8), (16384, 2)):
        P = frave_amd.Plan420(ctx, size, size)
        n_y = size * size
        d_rgb = torch.randint(0, 256, (slots, P.pixel_bytes), dtype=torch.uint8, device="cuda")
        d_pl = torch.randint(0, 256, (slots, P.plane_bytes), dtype=torch.uint8, device="cuda")
        d_back = torch.empty_like(d_rgb)
        d_m = torch.zeros(8, dtype=torch.int64, device="cuda")
        launches = max(slots, n if size == 4096 else n // 8)
        total = {"split": P.pixel_bytes + P.plane_bytes, "merge": P.pixel_bytes + P.plane_bytes, "measuring merge": P.pixel_bytes + P.plane_bytes}
        sp = s.cuda_stream
        L, h420 = frave_amd.load_library(), P._h
        rgb, pl, back, m = [d_rgb[k].data_ptr() for k in range(slots)], [d_pl[k].data_ptr() for k in range(slots)], [d_back[k].data_ptr() for k in range(slots)], d_m.data_ptr()
        # (the library's entry points called directly with pointers worked out beforehand: a launch of 15 us must not wait for the interpreter)
        fns = {
            "split": lambda i: L.fri_hip_split420_dev(h420, rgb[i % slots], pl[i % slots], pl[i % slots] + n_y, sp),
            "merge": lambda i: L.fri_hip_merge420_dev(h420, pl[i % slots], pl[i % slots] + n_y, back[i % slots], sp),
            "measuring merge": lambda i: L.fri_hip_measure_distortion420_dev(h420, pl[i % slots], pl[i % slots] + n_y, rgb[i % slots], m, sp),
        }
        half = (P.pixel_bytes + P.plane_bytes) // 2  # the copy reads and writes `half` bytes: the kernels' total

        def copy(i):
            k = i % slots
            return hip.hipMemcpyAsync(back[k], rgb[(k + 1) % slots], half, 3, sp)  # hipMemcpyDeviceToDevice

        fns["hipMemcpyAsync D2D"] = copy
        res = {k: [] for k in fns}
        for k, fn in fns.items():
            assert fn(0) == 0, k
            _events(torch, s, fn, 2 * slots)  # spin-up
        for _ in range(rounds):
            for k, fn in fns.items():
                _events(torch, s, fn, slots)
                res[k].append(_events(torch, s, fn, launches))
        cp = statistics.median(res["hipMemcpyAsync D2D"])
        for k in ("split", "merge", "measuring merge"):
            us = statistics.median(res[k])
            rep.line(f"{k} {size}x{size}, {slots} slots, {launches} launches: {us:.2f} us, {total[k] / 1e6:.1f} MB algorithmic = {total[k] / us / 1e6:.2f} TB/s "
                     f"({100 * total[k] / us * 1e6 / PEAK:.1f} % of 8 TB/s); D2D copy of the same total bytes {cp:.2f} us ({us / cp:.2f} x the copy); rounds "
                     + " ".join(f"{x:.2f}" for x in res[k]) + " / copy " + " ".join(f"{x:.2f}" for x in res["hipMemcpyAsync D2D"]))
        del d_rgb, d_pl, d_back
        torch.cuda.empty_cache()
        P.close()


def child_paths(which, launches):
    """one library, one round: us per image of the forward and the inverse path, as JSON on the last line. which = 420 | 444"""
    import torch

    import frave_amd
    from frave_amd.api import COLOUR_YCBCR, DEQUANT_MIDPOINT

    hip = C.CDLL("libamdhip64.so")
    ctx = frave_amd.Context(0)
    size, slots = 4096, 6
    s = torch.cuda.Stream()
    sp, spp = s.cuda_stream, C.c_void_p(s.cuda_stream)
    qm = frave_amd.quality_matrix(75)
    d_rgb = torch.randint(0, 256, (slots, size * size * 3), dtype=torch.uint8, device="cuda")
    d_back = torch.empty_like(d_rgb)
    if which == "420":
        P = frave_amd.Plan420(ctx, size, size)
        P.luma.set_dequantiser(DEQUANT_MIDPOINT), P.chroma.set_dequantiser(DEQUANT_MIDPOINT)
        n_y, n_c, fy, fc = size * size, P.cw * P.ch, P.luma.num_cells * 512, P.chroma.num_cells * 512
        d_pl = torch.empty((slots, P.plane_bytes), dtype=torch.uint8, device="cuda")
        d_co = torch.empty((slots, P.coef_count), dtype=torch.int32, device="cuda")

        def forward(k):
            pl, co = d_pl[k].data_ptr(), d_co[k].data_ptr()
            P.split420_dev(d_rgb[k].data_ptr(), pl, pl + n_y, stream=sp)
            P.luma.transform_quant_dev(pl, co, qm, stream=sp)
            P.chroma.transform_quant_dev(pl + n_y, co + 4 * fy, qm, stream=sp, n_images=2, pixel_stride=n_c, coef_stride=fc)

        def inverse(k):
            pl, co = d_pl[k].data_ptr(), d_co[k].data_ptr()
            P.luma.inverse_transform_dev(co, pl, qm, stream=sp)
            P.chroma.inverse_transform_batch_dev(2, co + 4 * fy, fc, pl + n_y, n_c, qm, stream=sp)
            P.merge420_dev(pl, pl + n_y, d_back[k].data_ptr(), stream=sp)
    else:
        P = frave_amd.Plan(ctx, size, size, 3)
        P.set_colour_transform(COLOUR_YCBCR)
        P.set_dequantiser(DEQUANT_MIDPOINT)
        d_co = torch.empty((slots, P.coef_count), dtype=torch.int32, device="cuda")

        def forward(k):
            P.transform_quant_dev(d_rgb[k].data_ptr(), d_co[k].data_ptr(), qm, stream=sp)

        def inverse(k):
            P.inverse_transform_dev(d_co[k].data_ptr(), d_back[k].data_ptr(), qm, stream=sp)

    out = {}
    for name, fn in (("forward", forward), ("inverse", inverse)):
        for k in range(slots):  # outside any capture first: everything the launches allocate exists
            fn(k)
        s.synchronize()
        assert hip.hipStreamBeginCapture(spp, RELAXED) == 0
        for k in range(slots):
            fn(k)
        graph, ex = C.c_void_p(), C.c_void_p()
        assert hip.hipStreamEndCapture(spp, C.byref(graph)) == 0 and graph.value
        assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
        replays = max(2, launches // slots)
        with torch.cuda.stream(s):
            for _ in range(2):
                assert hip.hipGraphLaunch(ex, spp) == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(replays):
                assert hip.hipGraphLaunch(ex, spp) == 0
            e1.record(s)
            e1.synchronize()
        out[name] = e0.elapsed_time(e1) * 1e3 / (replays * slots)
        hip.hipGraphExecDestroy(ex)
        hip.hipGraphDestroy(graph)
    print(json.dumps(out), flush=True)


def step_paths(rep, parent_lib, n, rounds):
    rep.line(f"python3 tools/chroma420_time.py paths PARENT_LIB --launches {n} --rounds {rounds} (4096x4096 RGB, quality 75's matrix, K3 with the midpoint dequantiser; "
             f"one child process per library and round, alternating; each replays a captured graph of its launches over 6 slots; us per image, medians of {rounds})")
    res = {("420", "forward"): [], ("420", "inverse"): [], ("444", "forward"): [], ("444", "inverse"): []}
    for _ in range(rounds):
        for which in ("420", "444"):
            env = dict(os.environ)
            if which == "444":
                env["FRI_HIP_LIBRARY"] = parent_lib
            else:
                env.pop("FRI_HIP_LIBRARY", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", which, "--launches", str(n)], env=env, capture_output=True, text=True, timeout=240)
            if p.returncode != 0:  # nothing more is started on the GPU after a failure
                rep.line(f"child {which} failed with {p.returncode}: {p.stderr[-400:]}")
                sys.exit(1)
            got = json.loads(p.stdout.strip().splitlines()[-1])
            for k, v in got.items():
                res[which, k].append(v)
    for k, parts in (("forward", "split + K1 on Y + K1 on Cb, Cr"), ("inverse", "K3 on Y + K3 on Cb, Cr + merge")):
        a, b = statistics.median(res["420", k]), statistics.median(res["444", k])
        rep.line(f"{k} path: 4:2:0 ({parts}) {a:.2f} us, 4:4:4 YCbCr {'K1' if k == 'forward' else 'K3'} of the parent commit's library {b:.2f} us, ratio {a / b:.3f}; rounds 4:2:0 "
                 + " ".join(f"{x:.2f}" for x in res["420", k]) + " / 4:4:4 " + " ".join(f"{x:.2f}" for x in res["444", k]))


def step_table(rep):
    import numpy as np

    import frave_amd
    import frave_amd.emit as emit
    from frave_amd.api import COLOUR_YCBCR, DEQUANT_MIDPOINT
    from tests.common import gen_image
    from tests.test_rct_host import correlated_image

    ctx = frave_amd.Context(0)
    qualities = (25, 50, 75, 90, 99)
    w, h = 1024, 768
    rep.line(f"bits per pixel (.frv, device chain + host emitter) / PSNR dB in R, G, B (midpoint dequantiser) against quality, {w}x{h}")
    rep.line("| image | mode | " + " | ".join(f"q={q}" for q in qualities) + " |")
    rep.line("|---|---|" + "---|" * len(qualities))

    def db_of(back, img):
        e = back.astype(np.float64) - img.reshape(-1)
        return 10 * np.log10(255.0 ** 2 / max(float((e * e).mean()), 1e-30))

    images = {"correlated": correlated_image(w, h, 7), "smooth": gen_image("smooth", w, h, 3, 1), "noise": gen_image("noise", w, h, 3, 1)}
    for name, img in images.items():
        Q = frave_amd.Plan(ctx, w, h, 3)
        Q.set_colour_transform(COLOUR_YCBCR)
        Q.set_dequantiser(DEQUANT_MIDPOINT)
        Q.set_stream_order()
        P = frave_amd.Plan420(ctx, w, h)
        P.set_stream_order()
        full, sub = [], []
        for q in qualities:
            qm = frave_amd.quality_matrix(q)
            sym, vp, wp, hist, oob = Q.encode_image_symbols(img, qm, fit=True)
            frv = emit.encode_image_from_streams(w, h, sym, hist, vp, wp, quality=q, ycbcr=True)
            full.append(f"{8.0 * len(frv) / (w * h):.3f} / {db_of(Q.inverse_transform(Q.transform_quant(img, qm), qm), img):.1f}")
            sym, vp, wp, hist, oob = P.encode_image420_symbols(img, q)
            frv = emit.encode_image_from_streams(w, h, sym, hist, vp, wp, quality=q, ycbcr=True, n_luma=P.luma.num_some)
            d = emit.decode_image(frv)
            sub.append(f"{8.0 * len(frv) / (w * h):.3f} / {db_of(P.decode_image420(np.concatenate([c.reshape(-1) for c in d[4]]), q), img):.1f}")
        Q.close(), P.close()
        rep.line(f"| {name} | YCbCr 4:4:4 | " + " | ".join(full) + " |")
        rep.line(f"| {name} | YCbCr 4:2:0 | " + " | ".join(sub) + " |")


def main():
    pos, out, n, rounds = _args()
    if not pos or pos[0] not in ("kernels", "paths", "table", "child"):
        print(__doc__)
        return 2
    if pos[0] == "child":
        child_paths(pos[1], n)
        return 0
    rep = Report(out, fresh=pos[0] == "kernels")
    if pos[0] == "kernels":
        step_kernels(rep, n, rounds)
    elif pos[0] == "paths":
        if len(pos) < 2 or not os.path.exists(pos[1]):
            print("paths needs PARENT_LIB: a build of the parent commit's libfri_hip.so")
            return 2
        step_paths(rep, os.path.abspath(pos[1]), n, rounds)
    else:
        step_table(rep)
    return 0


if __name__ == "__main__":
    sys.exit(main())
