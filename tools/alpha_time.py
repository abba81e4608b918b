"""What RGBA coding (fri_hip_plan_rgba, K9: k9_alpha.hip) costs. Two steps, each a process of its own that appends its section to the report; run them under a
time limit each and chained, so that trouble in one ends the run:

    timeout -k 10 600 python3 tools/alpha_time.py kernels && timeout -k 10 600 python3 tools/alpha_time.py chain

kernels: the split (KEEP and CLEAN) and the merge at 4096^2 and 16384^2 over rotating HBM-resident slots (more bytes than the 256 MB cache), timed with events
         around `launches` launches; next to each a device-to-device hipMemcpyAsync that moves the same total bytes (it copies half of them: every byte is read
         once and written once). Medians of five interleaved rounds; the 8 W H algorithmic bytes and their fraction of 8 TB/s.
chain:   the RGBA encode chain (fri_hip_encode_symbols_rgba_dev: split, the direct stream chain on the colour plan, the same on the alpha plan; the fit on) at
         4096^2 against the plain RGB chain plus a luma chain on ordinary plans (fri_hip_encode_symbols_batch_dev in its direct form on a C = 3 and a C = 1 plan,
         fed the already split rasters): what the split and the second plan's buffers add. Lossless, interleaved rounds, medians.

usage: python3 tools/alpha_time.py kernels|chain [--out profiles/alpha_time.txt] [--launches 200] [--rounds 5]"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12  # bytes per second


def _args():
    a = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "alpha_time.txt"), "--launches": "200", "--rounds": "5"}
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
    rep.line(f"python3 tools/alpha_time.py kernels --launches {n} --rounds {rounds} (one process; medians of {rounds} interleaved rounds, us per launch)")
    for size, slots in ((4096, 8), (16384, 2)):
        R = frave_amd.PlanRGBA(ctx, size, size)
        px = size * size
        d_rgba = torch.randint(0, 256, (slots, 4 * px), dtype=torch.uint8, device="cuda")
        d_rgb = torch.randint(0, 256, (slots, 3 * px), dtype=torch.uint8, device="cuda")
        d_a = torch.randint(0, 256, (slots, px), dtype=torch.uint8, device="cuda")
        d_back = torch.empty_like(d_rgba)
        launches = max(slots, n if size == 4096 else n // 8)
        total = 8 * px  # every kernel reads 4 W H bytes and writes 4 W H
        sp = s.cuda_stream
        L, h = frave_amd.load_library(), R._h
        rgba, rgb, a, back = ([t[k].data_ptr() for k in range(slots)] for t in (d_rgba, d_rgb, d_a, d_back))
        # (the library's entry points called directly with pointers worked out beforehand: a short launch must not wait for the interpreter)
        fns = {
            "split KEEP": lambda i: L.fri_hip_split_rgba_dev(h, rgba[i % slots], 0, rgb[i % slots], a[i % slots], sp),
            "split CLEAN": lambda i: L.fri_hip_split_rgba_dev(h, rgba[i % slots], 1, rgb[i % slots], a[i % slots], sp),
            "merge": lambda i: L.fri_hip_merge_rgba_dev(h, rgb[i % slots], a[i % slots], back[i % slots], sp),
        }

        def copy(i):
            k = i % slots
            return hip.hipMemcpyAsync(back[k], rgba[(k + 1) % slots], total // 2, 3, sp)  # hipMemcpyDeviceToDevice

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
        for k in ("split KEEP", "split CLEAN", "merge"):
            us = statistics.median(res[k])
            rep.line(f"{k} {size}x{size}, {slots} slots, {launches} launches: {us:.2f} us, {total / 1e6:.1f} MB algorithmic = {total / us / 1e6:.2f} TB/s "
                     f"({100 * total / us * 1e6 / PEAK:.1f} % of 8 TB/s); D2D copy of the same total bytes {cp:.2f} us ({us / cp:.2f} x the copy); rounds "
                     + " ".join(f"{x:.2f}" for x in res[k]) + " / copy " + " ".join(f"{x:.2f}" for x in res["hipMemcpyAsync D2D"]))
        del d_rgba, d_rgb, d_a, d_back
        torch.cuda.empty_cache()
        R.close()


def step_chain(rep, n, rounds):
    import numpy as np
    import torch

    import frave_amd

    ctx = frave_amd.Context(0)
    size, slots = 4096, 4
    px = size * size
    launches = max(slots, n // 4)
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    rep.line(f"python3 tools/alpha_time.py chain --launches {n} --rounds {rounds} ({size}x{size}, lossless, the fit on, {slots} slots, {launches} launches per round; "
             f"us per image, medians of {rounds} interleaved rounds)")
    R = frave_amd.PlanRGBA(ctx, size, size)
    R.set_stream_order()
    Q3, Q1 = frave_amd.Plan(ctx, size, size, 3), frave_amd.Plan(ctx, size, size, 1)
    Q3.set_stream_order(), Q1.set_stream_order()
    n_some = R.num_some
    d_rgba = torch.randint(0, 256, (slots, 4 * px), dtype=torch.uint8, device="cuda")
    d_rgb = torch.randint(0, 256, (slots, 3 * px), dtype=torch.uint8, device="cuda")
    d_a = torch.randint(0, 256, (slots, px), dtype=torch.uint8, device="cuda")
    d_sym = torch.empty((slots, 4 * n_some), dtype=torch.int16, device="cuda")
    d_hist = torch.empty((slots, 4 * 10 * 1024), dtype=torch.int32, device="cuda")
    d_par = torch.zeros((slots, 4 * 36), dtype=torch.float32, device="cuda")
    d_oob = torch.zeros((slots, 8), dtype=torch.int64, device="cuda")
    ones = np.ones(32, np.int32)

    def rgba_chain(i):
        k = i % slots
        R.encode_symbols_rgba_dev(d_rgba[k].data_ptr(), d_par[k].data_ptr(), d_sym[k].data_ptr(), d_hist[k].data_ptr(), d_oob[k].data_ptr(), d_oob[k].data_ptr() + 32,
                                  qmatrix=ones, fit=True, stream=sp)

    def plain_chains(i):
        k = i % slots
        Q3.encode_symbols_batch_dev(1, d_rgb[k].data_ptr(), 0, ones, True, d_par[k].data_ptr(), None, 0, None, 0, d_sym[k].data_ptr(), 3 * n_some, d_hist[k].data_ptr(),
                                    d_oob[k].data_ptr(), d_oob[k].data_ptr() + 32, stream=sp)
        Q1.encode_symbols_batch_dev(1, d_a[k].data_ptr(), 0, ones, True, d_par[k].data_ptr() + 4 * 108, None, 0, None, 0, d_sym[k].data_ptr() + 2 * 3 * n_some, n_some,
                                    d_hist[k].data_ptr() + 4 * 3 * 10240, d_oob[k].data_ptr() + 24, d_oob[k].data_ptr() + 56, stream=sp)

    fns = {"RGBA chain": rgba_chain, "RGB chain + luma chain": plain_chains}
    res = {k: [] for k in fns}
    for fn in fns.values():
        _events(torch, s, fn, 2 * slots)  # spin-up: everything the chains allocate exists
    for _ in range(rounds):
        for k, fn in fns.items():
            _events(torch, s, fn, slots)
            res[k].append(_events(torch, s, fn, launches))
    a, b = statistics.median(res["RGBA chain"]), statistics.median(res["RGB chain + luma chain"])
    rep.line(f"RGBA chain (split + colour chain + alpha chain) {a:.2f} us, RGB chain + luma chain on ordinary plans {b:.2f} us, ratio {a / b:.3f}, difference {a - b:.2f} us; "
             "rounds RGBA " + " ".join(f"{x:.2f}" for x in res["RGBA chain"]) + " / plain " + " ".join(f"{x:.2f}" for x in res["RGB chain + luma chain"]))
    R.close(), Q3.close(), Q1.close()


def main():
    pos, out, n, rounds = _args()
    if not pos or pos[0] not in ("kernels", "chain"):
        print(__doc__)
        return 2
    rep = Report(out, fresh=pos[0] == "kernels")
    if pos[0] == "kernels":
        step_kernels(rep, n, rounds)
    else:
        step_chain(rep, n, rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
