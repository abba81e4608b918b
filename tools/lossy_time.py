"""What lossy coding by quality costs on the device: K3 with the midpoint dequantiser and K3's measuring instance against plain K3 (the reference
dequantiser), all with the matrix of quality 50, and fri_hip_search_quality_dev; at 4096^2 and 16384^2, C = 1 and 3.

K3: the inverse entry point over rotating slots - 24 at 4096^2 (far beyond the 256 MiB Infinity Cache), 3 at 16384^2 (one RGB image alone is 805 MB of
pixels and 3.2 GB of coefficients) - timed with events around n launches; the three modes in interleaved rounds in one process, medians in microseconds
per launch. The search is synchronous (one read-back per probe): wall-clock time per call on a smooth + noise image, target 40 dB.

usage: python3 tools/lossy_time.py [launches per measurement = 200] [rounds = 5] [out = profiles/lossy_time.txt]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import frave_amd  # noqa: E402
from frave_amd.api import DEQUANT_MIDPOINT, DEQUANT_REFERENCE  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "lossy_time.txt")
ctx = frave_amd.Context(0)
s = torch.cuda.current_stream()
lines = [f"# tools/lossy_time.py {n} {rounds}: medians over {rounds} interleaved rounds, microseconds per launch (K3) / per call (search)"]


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for i in range(launches):
        fn(i)
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def smooth_noise(size, c):
    """a smooth gradient with noise on top (+-8), on the device"""
    y = torch.arange(size, device="cuda", dtype=torch.float32).view(-1, 1, 1)
    x = torch.arange(size, device="cuda", dtype=torch.float32).view(1, -1, 1)
    ch = torch.arange(c, device="cuda", dtype=torch.float32).view(1, 1, -1)
    base = 128 + 90 * torch.sin(x / 97.0 + ch) * torch.cos(y / 131.0)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    noise = torch.randint(-8, 9, (size, size, c), device="cuda", generator=g, dtype=torch.int32).to(torch.float32)
    return (base + noise).clamp(0, 255).to(torch.uint8).view(-1)


for size, slots in ((4096, 24), (16384, 3)):
    for c in (1, 3):
        plan = frave_amd.Plan(ctx, size, size, c)
        qm = frave_amd.quality_matrix(50)
        d_px = torch.randint(0, 256, (slots, plan.pixel_bytes), dtype=torch.uint8, device="cuda")
        d_co = torch.empty((slots, plan.coef_count), dtype=torch.int32, device="cuda")
        d_back = torch.empty_like(d_px)
        d_out = torch.zeros(slots * 8, dtype=torch.int64, device="cuda")
        for k in range(slots):
            plan.transform_quant_dev(d_px[k].data_ptr(), d_co[k].data_ptr(), qm, stream=s.cuda_stream)
        launches = max(slots, n if size == 4096 else n // 8)

        def inv(i):
            plan.inverse_transform_dev(d_co[i % slots].data_ptr(), d_back[i % slots].data_ptr(), qm, stream=s.cuda_stream)

        def meas(i):
            plan.measure_distortion_dev(d_co[i % slots].data_ptr(), d_px[i % slots].data_ptr(), d_out[8 * (i % slots)].data_ptr(), qm, stream=s.cuda_stream)

        res = {"K3 reference": [], "K3 midpoint": [], "K3 measure (midpoint)": []}
        timed(inv, launches)  # spin-up
        for r in range(rounds):
            plan.set_dequantiser(DEQUANT_REFERENCE)
            res["K3 reference"].append(timed(inv, launches))
            plan.set_dequantiser(DEQUANT_MIDPOINT)
            res["K3 midpoint"].append(timed(inv, launches))
            res["K3 measure (midpoint)"].append(timed(meas, launches))
        del d_co, d_back
        torch.cuda.empty_cache()
        img = smooth_noise(size, c)
        plan.search_quality(img.data_ptr(), 40.0, stream=s.cuda_stream)  # spin-up
        ts = []
        for r in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q, db = plan.search_quality(img.data_ptr(), 40.0, stream=s.cuda_stream)
            ts.append((time.perf_counter() - t0) * 1e6)
        base = statistics.median(res["K3 reference"])
        for k, v in res.items():
            m = statistics.median(v)
            lines.append(f"{size}^2 C={c}  {k:24s} {m:9.2f} us  ({m / base - 1:+.1%} vs reference; runs {min(v):.2f}-{max(v):.2f})")
        lines.append(f"{size}^2 C={c}  search to 40 dB           {statistics.median(ts):9.1f} us  (quality {q}, {db:.2f} dB; runs {min(ts):.1f}-{max(ts):.1f})")
        print("\n".join(lines[-4:]), flush=True)
        del plan, d_px, d_out, img
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
